"""Writes tests/golden/conv_routes.json: the C entry points, in order, of every convolution route that tests/conv_routes.py
lists (GPU only).  The fixture records what the code at hand does -- regenerate it only with a change that is MEANT to move a
layer to another route, and read the diff of names:

    python tools/gen_conv_routes.py [output.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_routes as CR  # noqa: E402
from u2pl_amd import nn as Kn  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_routes.json")
    routes = CR.record_all(Kn)
    with open(out, "w") as f:
        json.dump(routes, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, sum(len(v) for c in routes.values() for s in c.values() for v in s.values()), "calls")


if __name__ == "__main__":
    main()
