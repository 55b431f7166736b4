"""Sorted reference of the exact selection (u2pl_amd/csrc/select.hip), value families, edge descriptors and the case
tuples shared by tests/test_select_cpu.py (conditions on the reference alone) and tests/test_gpu_select_exact.py.  numpy only.

Nothing here has a tolerance: the selection is integer bookkeeping on the order-preserving key of a float32, followed by
one float32 lerp without FMA.  The reference sorts BY KEY (so -0 < +0, every NaN above +inf on one key), derives the two ranks of a
percentile with the arithmetic of resolve_chain (select.hip: virtual index float32(n - 1) * (float32(q) / float32(100))),
and lerps like k_sel_finish.  chain() restates resolve_chain level by level and yields the descriptors that prove that a
case stands on the edge it is named for, together with the expected histogram words."""
import functools
from collections import namedtuple

import numpy as np

f32, u32 = np.float32, np.uint32

# workspace words of select.hip's header
SEL_VAL, SEL_THR, SEL_GAMMA, SEL_H0 = 40, 56, 64, 128
MAXS = 8                                   # U2PL_SEL_MAX_SLOTS: two rank slots per spec, four specs at the most
SEL_H1 = SEL_H0 + 2048
SEL_H2 = SEL_H1 + MAXS * 2048
SEL_WORDS = SEL_H2 + MAXS * 1024
SHIFTS = (21, 10, 0)                       # 11 + 11 + 10 key bits
NBINS = (2048, 2048, 1024)
GROUP = 4                                  # distinct prefixes that k_sel_pass histograms per sweep
EINVAL = 1001                              # U2PL_EINVAL
QNAN = 0x7FC00000                          # what the project's producers write on invalid pixels
NAN_PATTERNS = (0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC54321, 0x7F800001, 0xFFFFFFFF)
RF_CAP = 12288                             # relfused.hip: candidate keys selected in LDS


# ---- keys ------------------------------------------------------------------------------------------------------------------
def bits(v):
    return np.ascontiguousarray(v, dtype=f32).view(u32)


def bits1(x):
    """the uint32 word of one float32 scalar (no conversion on the way: a NaN keeps its sign and payload)"""
    return int(bits(x).reshape(-1)[0])


def key(v):
    """f32_key (common.h) of float32 values: unsigned order == float order, -0 below +0"""
    u = bits(v)
    return np.where(u & u32(0x80000000), ~u, u | u32(0x80000000)).astype(u32)


def unkey(k):
    """key_f32 (common.h)"""
    k = np.asarray(k, dtype=u32)
    return np.where(k & u32(0x80000000), k & u32(0x7FFFFFFF), ~k).astype(u32).view(f32)


def sel_key(v):
    """sel_key of select.hip's plain-array passes: f32_key, but every NaN, of any sign and payload, gets the key of
    0x7fc00000 (above +inf; what f32_key gives the producers' NaN)"""
    return np.where(np.isnan(np.asarray(v, dtype=f32)), u32(0xFFC00000), key(v)).astype(u32)


def rf_bin(e, scale):
    """rf_bin (relfused.hip), for choosing two entropies that land in different bins: nothing else uses it"""
    e = f32(e)
    if not e >= f32(2.384185791015625e-07):
        return 0
    if e < f32(0.015625):
        return 1 + ((bits1(e) - 0x34800000) >> 17)
    b = int(f32(f32(e - f32(0.015625)) * f32(scale)))
    return 1025 + min(b, 1022)


def rf_bin_scale(C):
    return f32(f32(1022.0) / f32(f32(f32(np.log(f32(C))) + f32(0.02)) - f32(0.015625)))


# ---- ranks and thresholds ----------------------------------------------------------------------------------------------------
def q32_of(q):
    """numpy's q / 100 with a python-float q against float32 data (hipops.percentile_q32)"""
    return f32(q) / f32(100)


def vindex(n, q):
    """-> (lo, hi, gamma): resolve_chain's ranks of a percentile over n valid values and k_sel_finish's lerp weight"""
    with np.errstate(invalid="ignore"):
        vi = f32(n - 1) * q32_of(q)
        fl = np.floor(vi)
        gamma = f32(vi - fl)
    if n <= 0:
        lo = hi = 0
    elif vi != vi or vi >= f32(n - 1):
        lo = hi = n - 1
    elif vi < 0:
        lo = hi = 0
    else:
        lo = int(fl)
        hi = lo + 1
    return lo, hi, gamma


def lerp32(a, b, t):
    """numpy's _lerp as k_sel_finish computes it: float32, every operation rounded on its own"""
    a, b, t = f32(a), f32(b), f32(t)
    with np.errstate(invalid="ignore", over="ignore"):
        d = f32(b - a)
        return f32(b - f32(d * f32(f32(1) - t))) if t >= f32(0.5) else f32(a + f32(d * t))


Pct = namedtuple("Pct", "thr lo hi a b gamma")
Kth = namedtuple("Kth", "thr rank a")


def percentile_ref(valid, q):
    """np.percentile(valid, q) of float32 values without NaN, by the kernel's own arithmetic.  a, b: the two selected values
    (workspace words SEL_VAL + 2 j, + 1), gamma: word SEL_GAMMA + j"""
    valid = np.asarray(valid, dtype=f32).ravel()
    n = valid.size
    lo, hi, gamma = vindex(n, q)
    if n == 0:
        return Pct(f32(np.nan), lo, hi, f32(np.nan), f32(np.nan), gamma)
    sk = np.sort(key(valid))
    a, b = unkey(sk[lo]), unkey(sk[hi])
    return Pct(lerp32(a, b, gamma), lo, hi, a, b, gamma)


def kth_ref(values, n_valid, k, floor):
    """the OHEM rule of k_sel_finish over ALL values (NaNs sort last): +inf when k > n_valid or k <= 0, else
    max(floor, k-th smallest).  rank, a: the rank looked up (clamped to the array) and the value found there (SEL_VAL)"""
    values = np.asarray(values, dtype=f32).ravel()
    rank = max(min(int(k), values.size) - 1, 0)
    a = unkey(np.sort(sel_key(values))[rank])
    if k > n_valid or k <= 0:
        return Kth(f32(np.inf), rank, a)
    return Kth(a if a > f32(floor) else f32(floor), rank, a)


def slot_ranks(n_valid, n_total, specs):
    """-> ([rank of slot 0 .. 2 nspec - 1], [gamma of each spec])"""
    ranks, gammas = [], []
    for s in specs:
        if s[0] == "pct":
            lo, hi, g = vindex(n_valid, s[1])
        else:
            lo = hi = max(min(int(s[1]), n_total) - 1, 0)
            g = f32(0)
        ranks += [lo, hi]
        gammas.append(g)
    return ranks, gammas


def chain(values, specs, n_valid=None):
    """resolve_chain, level by level (n_valid: workspace word 0, by default the count of non-NaN values).
    -> three dicts, one per level:
      leader     leader of each slot while this level is resolved (level 0: all slots share hist0, owner 0)
      n_leaders  distinct leaders = histogram rows that the pass of this level fills (more than GROUP: a second sweep)
      hist       {leader: histogram of this level's digit over the keys that carry the leader's prefix}
      occupied   {leader: bins of that histogram that are not empty}
      prefix     key bits selected so far, per slot, AFTER this level
      rank       remaining rank inside that prefix, per slot, AFTER this level"""
    values = np.asarray(values, dtype=f32).ravel()
    keys = sel_key(values)
    if n_valid is None:
        n_valid = int((~np.isnan(values)).sum())
    rank, _ = slot_ranks(n_valid, values.size, specs)
    ns = len(rank)
    prefix, leader = [0] * ns, [0] * ns
    levels = []
    for L in range(3):
        sh, nb = SHIFTS[L], NBINS[L]
        hist = {}
        for l in sorted(set(leader)):
            sel = keys if L == 0 else keys[(keys >> u32(SHIFTS[L - 1])) == u32(prefix[l] >> SHIFTS[L - 1])]
            hist[l] = np.bincount(((sel >> u32(sh)) & u32(nb - 1)).astype(np.int64), minlength=nb).astype(u32)
        used = list(leader)
        for s in range(ns):
            h = hist[used[s]].astype(np.int64)
            c = np.cumsum(h)
            d = int(np.searchsorted(c, rank[s], side="right"))
            assert d < nb, "rank outside the array"
            rank[s] -= int(c[d] - h[d])
            prefix[s] |= d << sh
        leader = [next(u for u in range(s + 1) if prefix[u] == prefix[s]) for s in range(ns)]
        levels.append(dict(leader=used, n_leaders=len(hist), hist=hist, occupied={l: int(np.count_nonzero(h)) for l, h in hist.items()},
                           prefix=list(prefix), rank=list(rank)))
    return levels


# ---- spec builders -------------------------------------------------------------------------------------------------------------
def q_between(n, r):
    """a percentile whose float32 virtual index over n values has floor == r and 0 < gamma < 1"""
    assert 0 <= r <= n - 2
    for frac in (0.5, 0.375, 0.625, 0.25, 0.75):
        q = 100.0 * (r + frac) / (n - 1)
        lo, hi, g = vindex(n, q)
        if lo == r and hi == r + 1 and 0 < g < 1:
            return q
    raise AssertionError(("no percentile between ranks", n, r))


def q_exact(n, r):
    """a percentile whose float32 virtual index over n values is exactly r (gamma == 0), 0 <= r <= n - 2"""
    assert 0 <= r <= n - 2
    q0 = f32(100.0 * r / (n - 1))
    cands = [q0]
    up = dn = q0
    for _ in range(64):
        up, dn = np.nextafter(up, f32(np.inf)), np.nextafter(dn, f32(-np.inf))
        cands += [up, dn]
    for q in cands:
        lo, hi, g = vindex(n, float(q))
        if lo == r and hi == r + 1 and g == 0 and f32(n - 1) * q32_of(float(q)) == f32(r):
            return float(q)
    raise AssertionError(("no percentile exactly at rank", n, r))


# ---- families --------------------------------------------------------------------------------------------------------------------
FAMILIES = ("uniform", "low10", "mid11", "octaves", "entropy_like", "constant", "two_values", "runs", "signed_zeros",
            "infinities", "nan_mix")


def family(name, n, seed, **kw):
    """-> float32 array of n values.
    uniform       [0, 1) with one heavy tie value, a few negatives and 10 % 0x7fc00000 (the inputs of test_select_percentiles_bitexact)
    low10         bit patterns 0x3F800000 + k, k < 1024: one 22-bit prefix, the last pass resolves everything
    mid11         bit patterns 0x3F800000 + k, k < 2^21: one 11-bit prefix, spread over pass 1
    octaves       +-m 2^e, e uniform over -149 .. 3 (denormals included), one value in eight negative
    entropy_like  -sum p log p of fp32 softmaxes of 12 randn over 19 classes
    constant      one value (kw value, default float32(ln 19))
    two_values    kw nA copies of kw a, n - nA copies of kw b, shuffled
    runs          kw distinct (default 300) values in tie runs (kw lengths, or random lengths), shuffled; kw nan_frac of 0x7fc00000
    signed_zeros  -0.0, +0.0 and small values of both signs, denormals among them
    infinities    normal values with a few +-inf
    nan_mix       normal values, 10 % NaNs (kw frac) drawn from NAN_PATTERNS: both signs, payloads, signalling"""
    assert name in FAMILIES
    rng = np.random.default_rng([seed, FAMILIES.index(name), n])
    if name == "uniform":
        v = rng.random(n).astype(f32)
        if n > 100:
            v[rng.integers(0, n, n // 7)] = f32(0.25)
            v[: n // 50] *= -1
        if n > 10:
            v[rng.random(n) < 0.1] = np.array([QNAN], u32).view(f32)[0]
    elif name in ("low10", "mid11"):
        v = (u32(0x3F800000) + rng.integers(0, 1024 if name == "low10" else 1 << 21, n).astype(u32)).view(f32)
    elif name == "octaves":
        m = 1.0 + rng.random(n)
        e = rng.integers(-149, 4, n)
        v = np.ldexp(m, e).astype(f32)
        v = np.where(rng.integers(0, 8, n) == 0, -v, v).astype(f32)
        assert (v != 0).all()
    elif name == "entropy_like":
        z = f32(12) * rng.standard_normal((n, 19), dtype=f32)
        z = z - z.max(1, keepdims=True)
        p = np.exp(z)
        p = p / p.sum(1, keepdims=True, dtype=f32)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = -np.where(p > 0, p * np.log(p), f32(0)).sum(1, dtype=f32)
        v = v.astype(f32)
    elif name == "constant":
        v = np.full(n, f32(kw.get("value", np.log(f32(19)))), f32)
    elif name == "two_values":
        nA = kw["nA"]
        v = np.full(n, f32(kw["b"]), f32)
        v[:nA] = f32(kw["a"])
        rng.shuffle(v)
    elif name == "runs":
        if "lengths" in kw:
            lengths = np.asarray(kw["lengths"], np.int64)
            assert lengths.sum() == n
        else:
            lengths = np.bincount(rng.integers(0, min(kw.get("distinct", 300), n), n))
        vals = np.sort(rng.random(lengths.size) * 4).astype(f32)
        assert np.unique(vals).size == vals.size
        v = np.repeat(vals, lengths)
        rng.shuffle(v)
        if kw.get("nan_frac"):
            v[rng.random(n) < kw["nan_frac"]] = np.array([QNAN], u32).view(f32)[0]
    elif name == "signed_zeros":
        pool = np.array([-0.0, 0.0, -0.0, 0.0, 1e-3, -1e-3, 1e-45, -1e-45, 3e-39, -3e-39], f32)
        v = pool[rng.integers(0, pool.size, n)]
    elif name == "infinities":
        v = rng.standard_normal(n, dtype=f32)
        k = max(1, n // 50)
        idx = rng.permutation(n)[: 2 * k]
        v[idx[:k]] = np.inf
        v[idx[k:]] = -np.inf
    else:
        v = rng.standard_normal(n, dtype=f32)
        nan = rng.random(n) < kw.get("frac", 0.1)
        pats = np.array(NAN_PATTERNS, u32)
        pick = pats[rng.integers(0, pats.size, n)]
        where = np.flatnonzero(nan)
        pick[where[: pats.size]] = pats[: where.size][: pats.size]      # every pattern at least once when there is room
        v = np.where(nan, pick, bits(v)).astype(u32).view(f32)
    v = np.ascontiguousarray(v, dtype=f32)
    assert v.shape == (n,)
    return v


# ---- descriptors -------------------------------------------------------------------------------------------------------------------
EDGES = ("split0", "split1", "split2", "run_edge", "in_run")


def _edge_mask(sk, kind):
    """ranks r of the sorted keys at which (r, r + 1) is the named edge:
    split0: different level-0 bins; split1: same 11 bits, different level-1 bins; split2: same 22 bits, different keys;
    run_edge: r the last of a tie run of >= 2 and r + 1 the first of another; in_run: equal keys"""
    a, b = sk[:-1], sk[1:]
    if kind == "split0":
        return (a >> u32(21)) != (b >> u32(21))
    if kind == "split1":
        return ((a >> u32(21)) == (b >> u32(21))) & ((a >> u32(10)) != (b >> u32(10)))
    if kind == "split2":
        return ((a >> u32(10)) == (b >> u32(10))) & (a != b)
    if kind == "in_run":
        return a == b
    m = a != b
    m[1:] &= sk[:-2] == sk[1:-1]
    m[:-1] &= sk[2:] == sk[1:-1]
    m[0] = m[-1] = False
    return m


def edge_rank(valid, kind):
    """the rank nearest to the middle of the sorted valid values at which (r, r + 1) is the named edge"""
    sk = np.sort(key(valid))
    r = np.flatnonzero(_edge_mask(sk, kind))
    assert r.size, ("no such edge in this array", kind)
    return int(r[np.argmin(np.abs(r - sk.size // 2))])


def describe(values, specs):
    """what a (values, specs) pair reaches, as a set of tokens (EXPECT below) plus the figures behind them"""
    values = np.asarray(values, dtype=f32).ravel()
    valid = values[~np.isnan(values)]
    sk = np.sort(key(valid))
    lv = chain(values, specs)
    tok = {"n=%d" % valid.size, "specs=%d" % len(specs)}
    if lv[1]["n_leaders"] > GROUP:
        tok.add("leaders1>4")
    if lv[2]["n_leaders"] > GROUP:
        tok.add("leaders2>4")
    if lv[0]["occupied"][0] == 1:
        tok.add("one_bin0")
        if all(o == 1 for o in lv[1]["occupied"].values()):
            tok.add("one_bin01")
    if {"pct", "kth"} <= {s[0] for s in specs}:
        tok.add("mixed")
    if len({tuple(s) for s in specs}) < len(specs):
        tok.add("duplicates")
    masks = {kind: _edge_mask(sk, kind) for kind in EDGES} if sk.size >= 2 else {}
    for s in specs:
        if s[0] != "pct" or valid.size == 0:
            continue
        lo, hi, g = vindex(valid.size, s[1])
        if s[1] == 0:
            tok.add("q0")
        if s[1] == 100:
            tok.add("q100")
        if hi == lo + 1:
            if g == 0:
                tok.add("gamma0")
            if g == f32(0.5):
                tok.add("gamma_half")
            tok |= {kind for kind, m in masks.items() if m[lo]}
    return tok, dict(n_valid=int(valid.size), n_total=int(values.size), leaders=[l["n_leaders"] for l in lv],
                     occupied=[sorted(l["occupied"].values()) for l in lv])


# ---- the shared cases ----------------------------------------------------------------------------------------------------------------
# specs: literal ("pct", q) / ("kth", k, floor) entries, or entries resolved against the values with the reference arithmetic:
#   ("edge", kind)      -> ("pct", q_between(n_valid, edge_rank(valid, kind)))
#   ("exact", num, den) -> ("pct", q_exact(n_valid, (n_valid - 1) * num // den))
#   ("kth_at", where, floor_rel) -> ("kth", k, floor): k at "one" | "run_edge" (the last member of a tie run) | "n_valid" | "n_valid+1" |
#                          "zero" | "neg" | "above_total"; floor below (-1), equal to (0) or above (+1) the k-th value
Case = namedtuple("Case", "id family n seed kw specs expect")


def P(*qs):
    return tuple(("pct", float(q)) for q in qs)


TODAY = (P(20, 80), P(16.5), P(0, 100, 50, 83.7))


def _today_expect(n, i):
    if n > 7:
        return ()
    e = ("n=%d" % n,)
    if i == 2:
        e += ("q0", "q100") + (("gamma_half",) if n in (2, 4) else ())
    return e


CASES = [Case("uniform-n%d-%d" % (n, i), "uniform", n, n, {}, sp, _today_expect(n, i))
         for n in (1, 2, 3, 4, 5, 7, 1000, 65537) for i, sp in enumerate(TODAY)]
CASES += [
    Case("low10-4", "low10", 70001, 1, {}, P(20, 80, 50, 99.9), ("one_bin01", "specs=4")),
    Case("low10-1", "low10", 4099, 2, {}, P(37.5), ("one_bin01", "specs=1")),
    Case("mid11-2", "mid11", 70001, 1, {}, P(20, 80), ("one_bin0", "specs=2")),
    Case("mid11-4", "mid11", 3001, 2, {}, P(11, 42, 58, 93), ("one_bin0", "leaders2>4", "specs=4")),
    Case("octaves-4", "octaves", 701, 1, {}, P(5, 35, 65, 95), ("leaders1>4", "leaders2>4", "specs=4")),
    Case("octaves-edges", "octaves", 70001, 2, {}, (("edge", "split0"), ("edge", "split1"), ("edge", "split2")),
         ("split0", "split1", "split2", "specs=3")),
    Case("octaves-edges-4", "octaves", 20001, 3, {}, (("edge", "split0"), ("pct", 0.0), ("edge", "split1"), ("pct", 100.0)),
         ("split0", "split1", "q0", "q100", "leaders2>4", "specs=4")),
    Case("octaves-mixed", "octaves", 20001, 4, {}, (("pct", 30.0), ("kth_at", "run_edge", -1), ("pct", 70.0), ("kth_at", "n_valid", 1)),
         ("specs=4",)),
    Case("entropy-3", "entropy_like", 70001, 1, {}, P(20, 80, 50), ("specs=3",)),
    Case("entropy-exact", "entropy_like", 4097, 2, {}, (("exact", 1, 4), ("pct", 50.0), ("exact", 3, 4)), ("gamma0", "specs=3")),
    Case("entropy-half", "entropy_like", 4098, 3, {}, P(50), ("gamma_half", "specs=1")),
    Case("constant-4", "constant", 1000, 1, {}, P(0, 50, 100, 37.5), ("in_run", "q0", "q100", "one_bin01", "specs=4")),
    Case("constant-n5", "constant", 5, 1, {}, P(20, 80), ("n=5", "one_bin01")),
    Case("two-bins", "two_values", 7001, 1, dict(nA=4000, a=0.5, b=0.75), (("edge", "split0"), ("pct", 10.0), ("pct", 90.0)),
         ("split0", "in_run", "run_edge")),
    Case("two-ulp", "two_values", 7001, 2, dict(nA=3000, a=1.0, b=float(np.nextafter(f32(1), f32(2)))),
         (("edge", "split2"), ("pct", 10.0), ("pct", 90.0)), ("split2", "in_run", "run_edge", "one_bin01")),
    Case("runs-edges", "runs", 20000, 1, {}, (("edge", "run_edge"), ("edge", "in_run")), ("run_edge", "in_run", "specs=2")),
    Case("runs-dups", "runs", 20000, 2, {}, P(50, 50, 20, 20), ("duplicates", "specs=4")),
    Case("uniform-dups", "uniform", 1000, 3, {}, P(0, 100, 0, 100), ("duplicates", "q0", "q100", "specs=4")),
    Case("zeros-3", "signed_zeros", 5000, 1, {}, P(50, 20, 80), ("specs=3",)),
    Case("zeros-edge", "signed_zeros", 5000, 2, {}, (("edge", "split0"), ("edge", "in_run")), ("split0", "in_run")),
    Case("inf-4", "infinities", 1000, 1, {}, P(0, 100, 50, 1.5), ("q0", "q100", "specs=4")),
    Case("inf-n7", "infinities", 7, 2, {}, P(50, 99), ("n=7",)),
    Case("nanmix-3", "nan_mix", 70001, 1, {}, P(20, 80, 50), ("specs=3",)),
    Case("nanmix-4", "nan_mix", 1003, 2, {}, (("pct", 0.0), ("pct", 100.0), ("kth_at", "n_valid", -1), ("kth_at", "n_valid+1", -1)),
         ("q0", "q100", "specs=4")),
    Case("nanmix-all", "nan_mix", 100, 3, dict(frac=1.0), (("pct", 50.0), ("kth", 5, 0.5)), ("n=0",)),
]
# layouts: every n % 4, and one full grid-stride trip of the 256 x 256 x 4 launch plus a ragged tail
LAYOUT_CASES = [Case("layout-n%d" % n, "octaves", n, n, {}, P(20, 80, 50), ()) for n in (8192, 8193, 8194, 8195)]
LAYOUT_CASES += [Case("layout-trip", "entropy_like", 262144 + 5, 1, {}, P(20, 80, 50, 99.99), ("specs=4",))]
# the k-th rule: k at 1, at a tie-run boundary, at n_valid, n_valid + 1, 0, -3 and above n_total; floors below, equal, above
KTH_WHERE = ("one", "run_edge", "n_valid", "n_valid+1", "zero", "neg", "above_total")
KTH_CASES = [Case("kth-%s-%s-%+d" % (fam, where, rel), fam, 20000, 5, dict(nan_frac=0.1) if fam == "runs" else {},
                  (("kth_at", where, rel),), ())
             for fam in ("runs", "octaves") for where in KTH_WHERE for rel in (-1, 0, 1)]


def _resolve(values, spec):
    valid = values[~np.isnan(values)]
    nv = valid.size
    if spec[0] == "edge":
        return ("pct", q_between(nv, edge_rank(valid, spec[1])))
    if spec[0] == "exact":
        return ("pct", q_exact(nv, (nv - 1) * spec[1] // spec[2]))
    if spec[0] == "kth_at":
        sk = np.sort(key(valid))
        k = {"one": 1, "n_valid": nv, "n_valid+1": nv + 1, "zero": 0, "neg": -3, "above_total": values.size + 7}.get(spec[1])
        if k is None:
            if spec[1] == "run_edge" and np.unique(sk).size < sk.size:
                k = edge_rank(valid, "run_edge") + 1
            else:      # no tie runs in this family: any interior rank
                k = nv // 3
        at = unkey(sk[max(min(k, nv) - 1, 0)])
        floor = at if spec[2] == 0 else np.nextafter(at, f32(np.inf if spec[2] > 0 else -np.inf))
        return ("kth", int(k), float(floor))
    return tuple(spec)


@functools.lru_cache(maxsize=None)
def _inputs(case_id):
    c = BY_ID[case_id]
    v = family(c.family, c.n, c.seed, **c.kw)
    v.setflags(write=False)
    return v, tuple(_resolve(v, s) for s in c.specs)


BY_ID = {c.id: c for c in CASES + LAYOUT_CASES + KTH_CASES}
assert len(BY_ID) == len(CASES) + len(LAYOUT_CASES) + len(KTH_CASES)


def case_inputs(case):
    """-> (values (read-only, computed once), literal specs) of a shared case"""
    v, specs = _inputs(case.id)
    return v, list(specs)


def expected(values, specs, n_valid=None):
    """-> dict(thr, val, gamma: uint32 words per spec / slot / spec; levels: chain()) of u2pl_select_f32 on a plain array.
    n_valid: workspace word 0 where it is not the count of non-NaN values (the OHEM producer marks ignored pixels with 1.0
    and counts them out: only the k-th rule reads the word then)"""
    values = np.asarray(values, dtype=f32).ravel()
    valid = values[~np.isnan(values)]
    assert n_valid is None or n_valid == valid.size or all(s[0] == "kth" for s in specs)
    nv = valid.size if n_valid is None else n_valid
    thr, val, gam = [], [], []
    for s in specs:
        if s[0] == "pct":
            p = percentile_ref(valid, s[1])
            if valid.size == 0:      # (nothing valid: the slots point at rank 0 of the NaNs, the threshold is the canonical NaN)
                w = bits1(unkey(np.sort(sel_key(values))[0]))
                thr.append(QNAN); val += [w, w]
            else:
                thr.append(bits1(p.thr)); val += [bits1(p.a), bits1(p.b)]
            gam.append(bits1(p.gamma))
        else:
            k = kth_ref(values, nv, s[1], s[2])
            thr.append(bits1(k.thr)); val += [bits1(k.a)] * 2; gam.append(0)
    return dict(thr=np.array(thr, u32), val=np.array(val, u32), gamma=np.array(gam, u32), levels=chain(values, specs, nv))
