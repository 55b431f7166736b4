"""CPU checks of the inference surface: colour maps against the reference's tables (tests/golden/colormaps.npz, written
by tools/gen_infer_golden.py), the float64 normalisation table, infer.py's command line, and the C-ABI call sites of
the new files."""
import ast
import importlib.util
import os

import numpy as np

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]      # tools/city_semi_template.yaml


def _cli():
    spec = importlib.util.spec_from_file_location("infer_cli", os.path.join(ROOT, "infer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_colormaps_equal_the_reference_tables():
    from u2pl_amd.infer import colormap
    g = golden("colormaps")
    for name in ("pascal", "cityscapes"):
        cm = colormap(name)
        assert cm.dtype == np.uint8 and cm.shape == (256, 3)
        assert np.array_equal(cm, g[name]), name


def test_normalise_lut_is_the_float64_expression_rounded_once():
    from u2pl_amd.infer import normalise_lut
    lut = normalise_lut(MEAN, STD)
    assert lut.dtype == np.float32 and lut.shape == (3, 256) and lut.flags["C_CONTIGUOUS"]
    v = np.arange(256, dtype=np.float32).reshape(256, 1, 1).repeat(3, axis=2)      # an "image" that holds every byte value
    ref = (v - MEAN) / STD                                                           # infer.py:119-121 (lists: float64)
    assert ref.dtype == np.float64
    assert np.array_equal(lut, ref.astype(np.float32)[:, 0].T)
    all32 = ((v - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32))[:, 0].T
    assert all32.dtype == np.float32
    ndiff = int((all32 != lut).sum())
    print("entries where the all-fp32 expression differs:", ndiff, "of", lut.size)
    assert ndiff >= 1


def test_infer_cli_has_the_reference_options_and_defaults():
    p = _cli().get_parser()
    a = p.parse_args([])
    assert (a.config, a.model_path, a.save_folder) == ("config.yaml", "checkpoints/psp_best.pth", "viewer")
    assert a.input_scale is None                                    # the 769 / 513 rule unless given
    a = p.parse_args(["--config", "c.yaml", "--model_path", "m.pth", "--save_folder", "out", "--input_scale", "97", "65"])
    assert (a.config, a.model_path, a.save_folder, a.input_scale) == ("c.yaml", "m.pth", "out", [97, 65])
    opts = {s for act in p._actions for s in act.option_strings}
    assert opts == {"-h", "--help", "--config", "--model_path", "--save_folder", "--input_scale"}


def test_new_call_sites_match_the_c_header():
    """the walk of test_static_cpu.py::test_call_sites_match_the_c_header over infer.py and u2pl_amd/infer.py, and over
    the two hipops wrappers they go through"""
    from u2pl_amd._lib import parse_header
    decls = parse_header()
    for name in ("u2pl_predict_map_f32", "u2pl_infer_input_u8_f32"):
        assert name in decls and decls[name][2][-1] == "stream"
    bad, seen = [], set()
    for rel in ("infer.py", os.path.join("u2pl_amd", "infer.py"), os.path.join("u2pl_amd", "hipops.py"),
                os.path.join("u2pl_amd", "evaluate.py")):
        tree = ast.parse(open(os.path.join(ROOT, rel)).read())
        for n in ast.walk(tree):
            if not (isinstance(n, ast.Call) and n.args and isinstance(n.args[0], ast.Constant)
                    and isinstance(n.args[0].value, str) and n.args[0].value.startswith("u2pl_")):
                continue
            fn = n.func.attr if isinstance(n.func, ast.Attribute) else getattr(n.func, "id", "")
            if fn not in ("call", "query"):
                continue
            name = n.args[0].value
            if name not in decls:
                bad.append((rel, n.lineno, name, "not declared in the header"))
                continue
            seen.add(name)
            want = len(decls[name][1]) - (1 if fn == "call" else 0)      # call() appends hipStream_t
            star = [a for a in n.args if isinstance(a, ast.Starred)]
            if star:
                # the only starred argument of the new wrappers is *_strides_nchw(x): four values
                if not all(isinstance(a.value, ast.Call) and getattr(a.value.func, "id", "") == "_strides_nchw" for a in star):
                    continue
                got = len(n.args) - 1 + 3 * len(star)
            else:
                got = len(n.args) - 1
            if got != want:
                bad.append((rel, n.lineno, name, f"passes {got} args, header wants {want}"))
    assert not bad, bad
    assert {"u2pl_predict_map_f32", "u2pl_infer_input_u8_f32"} <= seen
