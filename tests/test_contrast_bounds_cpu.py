"""The InfoNCE bound of tests/contrast_bounds.py on the CPU: the fp32 emulation of k_infonce in its own order (rows in batches of
four, the fixed shift 1 / temp while 2 / temp <= 80 and the batch-wise rescaled running maximum above, max(vn, 1e-16) under the
rsqrt) and the fp32 torch form of the reference (torch.cosine_similarity + F.cross_entropy) meet it on every operand family at
every temperature; the bound rejects each mutant of that arithmetic by name; hipops.group_entries keeps its properties on random
draws.  (The GPU kernels are held to the same bound in tests/test_gpu_contrast_bounds.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrast_bounds as CB  # noqa: E402
from oracle import restate as R  # noqa: E402

KD = ((50, 256), (3, 64))
Q = 8
WORST = {}


def _cases():
    return [(fam, temp, K, D) for fam in CB.FAMILIES for temp in CB.TEMPS for (K, D) in KD]


_CACHE = {}


def _ref(fam, temp, K, D):
    """case and float64 reference, computed once and shared (never modified)"""
    key = (fam, temp, K, D)
    if key not in _CACHE:
        case = _CACHE.get((fam, K, D)) or CB.make_case(fam, 1, D, K, Q)
        _CACHE[(fam, K, D)] = case
        _CACHE[key] = (case,) + CB.case_ref(case, temp)
    return _CACHE[key]


def _excesses(form, fam, temp, K, D, mutant=None):
    case, l64, g64, _, anchors = _ref(fam, temp, K, D)
    if form == "emulation":
        l, g = CB.emulate_case(case, temp, mutant)
    else:
        out = [CB.torch_fp32(*CB.job_operands(case, j)[1:], temp) for j in range(len(case["jobs"]))]
        l, g = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    return CB.loss_excess(l, l64, D, K, temp), CB.grad_excess(g, g64, anchors, D, K, temp)


def test_reference_is_the_oracles_info_nce():
    """nce_ref is restate.info_nce per anchor: its mean is the oracle's loss, its gradient / Q the oracle's gradient"""
    case = CB.make_case("random", 3, 128, 7, Q)
    _, a, f = CB.job_operands(case, 2)
    for temp in (0.5, 0.024):
        l, g = CB.nce_ref(a, f, temp)
        lo, go = R.info_nce(a, f[0, 0], f[:, 1:], CB.temp32(temp))
        assert abs(l.mean() - lo) <= 1e-12 * max(1.0, abs(lo)) and np.abs(g / Q - go).max() <= 1e-12 * np.abs(go).max()


def test_ring_addressing_and_case_geometry():
    case = CB.make_case("zero", 0, 64, 3, Q)
    J = case["jobs"][1]
    ring = J["ring"]
    assert ring["head"] == ring["cap"] - 2 and np.array_equal(CB.ring_rows(ring, [0, 1, 2]), ring["storage"][[62, 63, 0]])
    assert [len(j["cand"]) for j in case["jobs"]] == [1, 5, 11] and [j["ring"]["cap"] for j in case["jobs"]] == [7, 64, 300]
    shared = np.intersect1d(case["jobs"][1]["cand"], case["jobs"][2]["cand"])
    assert shared.size == 1 and all(j["cand"][j["ia"][0]] == shared[0] for j in case["jobs"][1:])
    assert not J["proto"].any() and not case["rep"][case["jobs"][2]["cand"][case["jobs"][2]["ia"][-1]]].any()
    for j in range(3):      # no draw reaches an unfilled slot, no row has a norm in (0, 1e-8)
        _, a, f = CB.job_operands(case, j)
        assert np.isfinite(f).all()
        for x in (a, f):
            nrm = np.linalg.norm(x.astype(np.float64), axis=-1)
            assert not ((nrm > 0) & (nrm < 1e-8)).any()


@pytest.mark.parametrize("form", ["emulation", "torch_fp32"])
@pytest.mark.parametrize("fam", CB.FAMILIES)
def test_fp32_forms_meet_the_bound(form, fam):
    for temp in CB.TEMPS:
        for K, D in KD:
            el, eg = _excesses(form, fam, temp, K, D)
            w = WORST.setdefault((form, fam), [0.0, 0.0, 0.0])
            w[0], w[1] = max(w[0], el), max(w[1], eg)
            w[2] = max(w[2], el * CB.E_loss(D, K, temp) / (CB.CAL_LOSS * CB.cal_unit(temp)))
            assert el <= 1.0 and eg <= 1.0, (form, fam, temp, K, D, el, eg)
    print(f"\n{form:10s} {fam:8s} worst excess: loss {WORST[(form, fam)][0]:.4f} grad {WORST[(form, fam)][1]:.4f}"
          f"  (loss error / 1.2 EPS (2/temp + 8): {WORST[(form, fam)][2]:.3f})")


def test_bound_against_the_contract_ceilings():
    """E_loss never exceeds the parity contract; where the derived count does (small temperatures) the contract is the bound"""
    over = [t for t in CB.TEMPS for K, D in KD if CB.E_loss_derived(D, K, t) > CB.CONTRACT_LOSS]
    assert all(CB.E_loss(D, K, t) <= CB.CONTRACT_LOSS for t in CB.TEMPS for K, D in KD)
    assert set(over) == {0.025, 0.024, 0.01}      # the finding of the module docstring
    # nothing asserted is more than ten times what the reference's fp32 arithmetic reaches (the calibration of the module docstring)
    for t in CB.TEMPS:
        for K, D in KD + ((100, 512),):
            assert CB.E_loss(D, K, t) <= 10 * 1.2 * CB.EPS * (2 / CB.temp32(t) + 8)
            assert CB.E_grad_comp(D, K, t) <= 10 * 0.12 * CB.EPS * (2 / CB.temp32(t) + 8)
    assert CB.loss_AB(256, 50, 0.5)[0] == 67 and CB.grad_AB(256, 50, 0.5)[0] == 68 and CB.grad_AB(256, 50, 0.5)[1] == 280
    assert CB.is_online(0.024) and not CB.is_online(0.025)


@pytest.mark.parametrize("mutant", CB.MUTANTS)
def test_bound_rejects_mutant(mutant):
    """every mutant of the emulation exceeds the bound on at least one family (a mutant that survives fails here)"""
    hits = []
    for fam, temp, K, D in _cases():
        if mutant.startswith("no_rescale") and not CB.is_online(temp):
            continue
        el, eg = _excesses("emulation", fam, temp, K, D, mutant)
        if max(el, eg) > 1.0:
            hits.append((fam, temp, K, D))
    assert hits, mutant
    print(f"\n{mutant}: rejected on {len(hits)} cases, e.g. {hits[0]}")


def test_group_entries_properties():
    """every entry once in `order`; the leaders' (seg_pos, seg_len) tile [jQ, (j + 1) Q); a group's members share one candidate
    and ascend; seg_len is zero for non-leaders"""
    from u2pl_amd.hipops import group_entries as ge
    rng = np.random.default_rng(0)
    for trial in range(60):
        Qn = int(rng.choice([1, 4, 6, 8, 33]))
        ncs = [1] + [int(rng.integers(1, 2 * Qn + 2)) for _ in range(int(rng.integers(0, 4)))]
        ia = [rng.integers(0, nc, Qn) for nc in ncs]
        order, pos, ln = ge(ia, Qn)
        n = len(ncs) * Qn
        assert sorted(order.tolist()) == list(range(n))
        for j in range(len(ncs)):
            lead = [e for e in range(j * Qn, (j + 1) * Qn) if ln[e] > 0]
            segs = sorted((int(pos[e]), int(ln[e]), e) for e in lead)
            assert segs[0][0] == j * Qn and all(a[0] + a[1] == b[0] for a, b in zip(segs, segs[1:])) and segs[-1][0] + segs[-1][1] == (j + 1) * Qn
            for p0, l0, e in segs:
                mem = order[p0:p0 + l0]
                assert mem[0] == e and (np.diff(mem) > 0).all() and len(set(ia[j][mem - j * Qn].tolist())) == 1
            assert len({int(ia[j][e - j * Qn]) for e in lead}) == len(lead) == len(set(ia[j].tolist()))
            if ncs[j] == 1:
                assert len(lead) == 1 and ln[lead[0]] == Qn
