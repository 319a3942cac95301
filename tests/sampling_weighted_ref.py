"""The specification of WEIGHTED neighbour sampling (include/gnnagg.h section F, "Weighted sampling") restated in numpy, and the fixture
weights the weighted sampling tests share.  Written from the specification, not from the C++: the key as vectorised integer arithmetic
and one float32 division, the kept set by a full stable sort of a row's (wkey, p) pairs.
"""
import functools

import numpy as np

from sampling_ref import CRAFTED, FANOUTS, NUM_V, crafted_rows, fixture_graph, fmix, key, seed_lists  # noqa: F401

INELIGIBLE = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def log2_table():
    """L[i] = round(2^26 . log2(1 + i/256)), i = 0 ... 256"""
    return np.round(np.log2(1.0 + np.arange(257) / 256.0) * float(1 << 26)).astype(np.int64)


def bit_length(u):
    u = np.asarray(u, np.uint64)
    b = np.zeros(u.shape, np.int64)
    for k in range(32):
        b = np.where(u >> np.uint64(k) != 0, k + 1, b)
    return b


def neg_log2_q26(u):
    """E(u): -log2((u + 1/2) / 2^32) in Q6.26, for uint32 u (int64 arrays)"""
    u = np.asarray(u, np.uint64)
    b = bit_length(u)
    fr = ((np.uint64(2) * u + np.uint64(1)) << (32 - b).astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    i = (fr >> np.uint64(24)).astype(np.int64)
    r = ((fr >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.int64)
    L = log2_table()
    lg = L[i] + (((L[i + 1] - L[i]) * r) >> 16)
    return ((33 - b) << 26) - lg


def eligible(w):
    with np.errstate(invalid="ignore"):
        return np.asarray(w, np.float32) > 0


def wkey_of(u, w):
    """wkey from the uniform key u and the weight w (broadcast): uint32 values in int64 arrays"""
    w = np.asarray(w, np.float32)
    E = neg_log2_q26(u)
    ok = eligible(w)
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        q = E.astype(np.float32) / np.where(ok, w, np.float32(1))        # int64 -> float32 and the division: both round to nearest
    bits = np.ascontiguousarray(q, np.float32).view(np.uint32).astype(np.int64)
    return np.where(ok, bits, INELIGIBLE)


def wkey(seed, p, w):
    return wkey_of(key(seed, p), w)


def kept_positions(ptr, w, r, fanout, seed):
    """the positions p of the kept edges of row r, increasing"""
    p = np.arange(int(ptr[r]), int(ptr[r + 1]), dtype=np.int64)
    p = p[eligible(w[p])]
    if fanout == -1 or p.size <= fanout:
        return p
    assert fanout >= 1
    order = np.argsort(wkey(seed, p, w[p]), kind="stable")     # (p increasing: a stable sort breaks ties by position)
    return np.sort(p[order[:fanout]])


def sample_block(ptr, idx, w, seeds, fanout, seed=0, relabel=True):
    """(blk_ptr, blk_idx, eid, src_nodes or None, num_src): the block of the specification"""
    ptr, idx, w, seeds = np.asarray(ptr), np.asarray(idx), np.asarray(w, np.float32), np.asarray(seeds)
    rows = [kept_positions(ptr, w, int(r), fanout, seed) for r in seeds]
    blk_ptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int32)
    eid = (np.concatenate(rows) if rows else np.zeros(0, np.int64)).astype(np.int32)
    glob = idx[eid].astype(np.int32)
    if not relabel:
        return blk_ptr, glob, eid, None, len(ptr) - 1
    local, src = {}, []
    for i, r in enumerate(seeds):
        src.append(int(r))
        local.setdefault(int(r), i)
    for v in glob:
        if int(v) not in local:
            local[int(v)] = len(src)
            src.append(int(v))
    blk_idx = np.array([local[int(v)] for v in glob], np.int32).reshape(-1)
    return blk_ptr, blk_idx, eid, np.array(src, np.int32), len(src)


# ------------------------------------------------------------------------------------------------ fixture weights
CLASS_DEGREES = [5, 64, 65, 257, 1000, 5000]      # one crafted row per way the device walks a row (and two sizes of the middle one)
VARIANTS = ["mixed", "inf", "zero", "three"]
EXTREME_ROW = 500                                  # (sampling_ref forces a self-loop and a multi-edge there: the row has edges)
EXTREME = [np.float32(1.17549435e-38), np.float32(1e-42), np.float32(3.4028235e38), np.float32(1e-30)]   # FLT_MIN, a denormal, FLT_MAX


def class_rows():
    return [crafted_rows()[CRAFTED.index(d)] for d in CLASS_DEGREES]


@functools.lru_cache(maxsize=None)
def fixture_weights(variant="mixed"):
    """float32 [num_e] for fixture_graph().  Every variant: log-uniform positive weights over about 12 binades, about 30 % zeros, a few
    negative and NaN entries (-0 among them), and EXTREME_ROW cycling through FLT_MIN, a denormal, FLT_MAX and 1e-30.  The crafted rows
    of CLASS_DEGREES are left as drawn ("mixed"), all +Inf ("inf"), all zero ("zero") or zero but for 3 edges ("three")."""
    assert variant in VARIANTS
    ptr, _ = fixture_graph()
    num_e = int(ptr[-1])
    rng = np.random.default_rng(20250311)
    w = np.exp2(rng.uniform(-6.0, 6.0, size=num_e)).astype(np.float32)
    w[rng.random(num_e) < 0.30] = 0.0
    odd = rng.choice(num_e, size=40, replace=False)
    w[odd[:15]] = -w[odd[:15]] - np.float32(0.5)
    w[odd[15:30]] = np.nan
    w[odd[30:]] = -0.0
    b, e = int(ptr[EXTREME_ROW]), int(ptr[EXTREME_ROW + 1])
    assert e - b >= 4
    w[b:e] = np.resize(np.array(EXTREME, np.float32), e - b)
    for r in class_rows():
        b, e = int(ptr[r]), int(ptr[r + 1])
        if variant == "inf":
            w[b:e] = np.inf
        elif variant == "zero":
            w[b:e] = 0.0
        elif variant == "three":
            keep = np.sort(rng.choice(e - b, size=3, replace=False))
            vals = w[b + keep]
            w[b:e] = 0.0
            w[b + keep] = np.where(vals > 0, vals, np.float32(1.0))
    w.setflags(write=False)
    return w
