"""Every decoder's parameter layout and seeded initial values against tests/golden/decoder_layout.json.

ParamArena lays parameters out in registration order, checkpoints are keyed by state_dict names, and every constructed layer
draws from the RNG: a decoder whose submodules are built in another order trains from other weights and loads no old checkpoint.
For each constructor call of CASES the fixture holds the children's names, the ordered (key, shape) list of state_dict() and a
sha256 over the key names and the tensors' bytes after torch.manual_seed(0).  `python tests/test_decoder_layout_cpu.py` writes the
fixture anew: only when a layout changes on purpose."""
import hashlib
import json
import os

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_layout.json")
CASES = {
    "deeplabv3": ("dec_deeplabv3", {}),
    "deeplabv3_separable": ("dec_deeplabv3", dict(separable=True)),
    "deeplabv3_plus": ("dec_deeplabv3_plus", {}),
    "deeplabv3_plus_separable_no_rep": ("dec_deeplabv3_plus", dict(separable=True, rep_head=False)),
    "pspnet_rep": ("dec_pspnet", dict(rep_head=True)),
    "pspnet": ("dec_pspnet", dict(rep_head=False)),
    "pspnet_two_bins": ("dec_pspnet", dict(rep_head=True, bins=(2, 3), inner_planes=64)),
    "ocrnet_rep": ("dec_ocrnet", dict(rep_head=True)),
    "ocrnet": ("dec_ocrnet", dict(rep_head=False, inner_planes=64, key_planes=32)),
    "ccnet_shared": ("dec_ccnet", dict(rep_head=True, shared=True)),
    "ccnet_three_blocks": ("dec_ccnet", dict(rep_head=True, shared=False, recurrence=3)),
    "ccnet": ("dec_ccnet", dict(rep_head=False, inner_planes=64, key_planes=32)),
    "nonlocal_two_heads_stride_2": ("dec_nonlocal", dict(rep_head=True, heads=2, kv_stride=2)),
    "nonlocal": ("dec_nonlocal", dict(rep_head=False, inner_planes=64, key_planes=32, value_planes=48)),
    "aux": ("Aux_Module", {}),
}


def layout(name):
    from u2pl_amd.models import decoder
    cls, kwargs = CASES[name]
    torch.manual_seed(0)
    m = getattr(decoder, cls)(128, **kwargs)
    sd = m.state_dict()
    assert [k for k in sd if k in dict(m.named_parameters())] == [k for k, _ in m.named_parameters()]
    h = hashlib.sha256()
    for k, t in sd.items():
        h.update(k.encode())
        h.update(t.detach().contiguous().numpy().tobytes())
    return dict(children=[k for k, _ in m.named_children()], state=[[k, list(t.shape)] for k, t in sd.items()], sha256=h.hexdigest())


def write_fixture(cases):
    """one line per constructor call"""
    with open(FIXTURE, "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join("%s: %s" % (json.dumps(name), json.dumps(cases[name], sort_keys=True)) for name in sorted(cases)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_decoder_layout_and_seeded_values_are_the_recorded_ones(name):
    want = json.load(open(FIXTURE))[name]
    got = layout(name)
    assert got["children"] == want["children"]
    assert got["state"] == want["state"]
    assert got["sha256"] == want["sha256"]


def test_fixture_holds_exactly_the_cases():
    assert sorted(json.load(open(FIXTURE))) == sorted(CASES)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_fixture({name: layout(name) for name in CASES})
    print("wrote", FIXTURE)
