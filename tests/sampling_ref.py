"""The specification of neighbour sampling (include/gnnagg.h section F) restated in numpy, and the fixture the sampling tests share.
Written from the specification, not from the C++: keys as vectorised uint32 arithmetic, the kept set by a full sort of a row's keys.
"""
import functools

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def fmix(h):
    """murmur3's 32-bit finalizer on uint32 values held in uint64 arrays (every step masked back to 32 bits)"""
    h = np.asarray(h, np.uint64) & M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h = h ^ (h >> np.uint64(16))
    return h


def seed_mix(seed):
    """s of a seed in [0, 2^64) (or an array of them)"""
    seed = np.asarray(seed, dtype=np.uint64)
    lo, hi = seed & M32, seed >> np.uint64(32)
    return fmix(fmix((lo + np.uint64(0x9E3779B9)) & M32) ^ hi)


def key(seed, p):
    """key(seed, p) for an array of positions p (seed and p broadcast)"""
    s = seed_mix(seed)
    return fmix((fmix((np.asarray(p, np.uint64) & M32) ^ s) + s) & M32)


def kept_positions(ptr, r, fanout, seed):
    """the positions p of the kept edges of row r, increasing"""
    p = np.arange(int(ptr[r]), int(ptr[r + 1]), dtype=np.int64)
    if fanout == -1 or p.size <= fanout:
        return p
    assert fanout >= 1
    order = np.argsort(key(seed, p), kind="stable")
    return np.sort(p[order[:fanout]])


def sample_block(ptr, idx, seeds, fanout, seed=0, relabel=True):
    """(blk_ptr, blk_idx, eid, src_nodes or None, num_src): the block of the specification"""
    ptr, idx, seeds = np.asarray(ptr), np.asarray(idx), np.asarray(seeds)
    rows = [kept_positions(ptr, int(r), fanout, seed) for r in seeds]
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


# ------------------------------------------------------------------------------------------------ fixture
CRAFTED = [0, 1, 4, 5, 6, 63, 64, 65, 127, 128, 129, 256, 257, 1000, 5000]
NUM_V = 2000
FANOUTS = [1, 5, 64, 65, 200, -1]


@functools.lru_cache(maxsize=None)
def fixture_graph():
    """(ptr, idx): NUM_V rows; the crafted degrees sit at rows 3, 10, 17, ... (crafted_rows), the rest is random in 0 ... 40; neighbour
    ids random over all rows (multi-edges and self-loops included, some forced)"""
    rng = np.random.default_rng(20240607)
    deg = rng.integers(0, 41, size=NUM_V)
    for k, d in enumerate(CRAFTED):
        deg[3 + 7 * k] = d
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    idx = rng.integers(0, NUM_V, size=int(ptr[-1])).astype(np.int32)
    for r in (3 + 7 * 3, 3 + 7 * 8, 500):          # self-loops and a multi-edge where the row has room
        if deg[r] >= 2:
            idx[ptr[r]] = r
            idx[ptr[r] + 1] = idx[ptr[r + 1] - 1]
    return ptr, idx


def crafted_rows():
    return [3 + 7 * k for k in range(len(CRAFTED))]


@functools.lru_cache(maxsize=None)
def seed_lists():
    """name -> int32 seeds"""
    rng = np.random.default_rng(99)
    lists = {
        "empty": [],
        "one": [crafted_rows()[7]],
        "crafted": crafted_rows(),
        "all_shuffled": list(rng.permutation(NUM_V)),
        "duplicates": [crafted_rows()[9], 5, crafted_rows()[9], 5, 5, crafted_rows()[14], 77, crafted_rows()[14]],
        "mutual": mutual_rows(),
    }
    return {k: np.array(v, np.int32) for k, v in lists.items()}


def mutual_rows():
    """rows whose neighbour lists hold one another (and themselves): found in the fixture, not forced"""
    ptr, idx = fixture_graph()
    hub = crafted_rows()[14]                        # 5000 edges: it reaches most rows
    nb = [int(v) for v in idx[ptr[hub]:ptr[hub + 1]]]
    back = [v for v in dict.fromkeys(nb) if hub in idx[ptr[v]:ptr[v + 1]]]
    return [hub] + back[:6] + [hub]
