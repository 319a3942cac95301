"""The plan-builder census: the size arithmetic of the device plan builder restated in Python, a numpy restatement of the 2-D blocked order,
a graph maker with exact edge counts, and one table of graphs per switch of the builder.

csrc/plan_gpu.hip builds the balanced mode's blocked order (gpu_build_blocked_plan) and the rows mode's chain plan (gpu_build_chain_plan)
from three wave64 primitives of csrc/prims.cuh:
    scan        three kernels over tiles of kTile = kBlock * kItems elements; the tile totals are rescanned kBlock at a time with a carry
    reduce      a grid-stride loop of at most kReduceGrid workgroups of kBlock threads
    sort_pairs  a stable LSD radix sort, kRadixBits per pass; an even pass count leaves the result in the input buffers: one copy back
and csrc/api.hip decides from sizes whether the device builder runs at all.  Every one of these decisions is a switch on a size nobody
chooses on purpose.  The constants below are read out of the sources, the functions restate what the code computes from them, and every
table entry names the side of a switch it CLAIMS to reach: tests/test_plan_census_host.py checks the claims against the arithmetic (and
both sides of every switch against the tables), tests/test_gpu_plan_census.py runs every entry on the device, bit for bit.

The rule: a new primitive or a new guard in the builder gets a row in DESIGN.md "Plan-builder switch points" and an entry here.

Importable without a GPU (numpy and the standard library only)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn_computing_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------ constants from the sources
def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s: expected one match of %r, found %d" % (what, pattern, len(found))
    return found[0]


def read_constants(prims_text=None, plan_text=None, api_text=None):
    """The builder's constants as the sources state them (a source text may be passed in: the host test edits a copy)."""
    prims = prims_text if prims_text is not None else open(os.path.join(CSRC, "prims.cuh")).read()
    plan = plan_text if plan_text is not None else open(os.path.join(CSRC, "plan_gpu.hip")).read()
    api = api_text if api_text is not None else open(os.path.join(CSRC, "api.hip")).read()
    c = {}
    m = _one(r"constexpr int kBlock = (\d+), kItems = (\d+), kTile = kBlock \* kItems;", prims, "prims.cuh tile")
    c["kBlock"], c["kItems"] = int(m[0]), int(m[1])
    c["kTile"] = c["kBlock"] * c["kItems"]
    # k_scan_totals rescans the tile totals one workgroup's worth at a time
    _one(r"for \(int b = 0; b < nt; b \+= kBlock\)", prims, "prims.cuh totals round")
    c["totals_round"] = c["kBlock"]
    m = _one(r"const int passes = bits <= 0 \? 1 : \(bits \+ (\d+)\) / (\d+);", prims, "prims.cuh passes")
    assert int(m[0]) == int(m[1]) - 1
    c["radix_bits"] = int(m[1])
    shifts = set(re.findall(r"dim3\(nt\), dim3\(kBlock\), 0, st, ki, (?:vi, )?n, (\d+) \* p, nt", prims))
    assert shifts == {str(c["radix_bits"])}, "prims.cuh: the passes shift by %s bits" % shifts
    assert re.search(r"\(keys\[i\] >> shift\) & %du\b" % ((1 << c["radix_bits"]) - 1), prims)
    c["reduce_grid"] = int(_one(r"std::min<long>\(\(n \+ kBlock - 1\) / kBlock, (\d+)\)", prims, "prims.cuh reduce grid"))
    guards = re.findall(r"par_num > (\d+)", plan)
    assert len(guards) == 2 and len(set(guards)) == 1, "plan_gpu.hip: one range guard per builder"
    c["range_guard"] = int(guards[0])
    assert int(_one(r"if \(par_num > (\d+)\) return GNNAGG_OK;", api, "api.hip range guard")) == c["range_guard"]
    ids = re.findall(r"\(unsigned\)mx > 0x([0-9a-f]+)u\) return GNNAGG_OK;", api)
    assert len(ids) == 2 and len(set(ids)) == 1, "api.hip: the id guard of the device and of the host span builder"
    c["id_guard"] = int(ids[0], 16)
    mem = re.findall(r"\(size_t\)c->E \* (\d+) > free_b / (\d+)", api)
    assert len(mem) == 2 and mem[0][1] == mem[1][1], "api.hip: one memory guard per builder"
    c["blocked_bytes_per_edge"], c["chain_bytes_per_edge"], c["free_divisor"] = int(mem[0][0]), int(mem[1][0]), int(mem[0][1])
    c["chain_id_bits"] = int(_one(r"if \(mx \+ 1 >= \(1 << (\d+)\)\) \{ \*done = true;", api, "api.hip chain ids"))
    c["kSpanEdges"] = int(_one(r"static constexpr int kSpanEdges = (\d+);", api, "api.hip kSpanEdges"))
    return c


K = read_constants()


# ------------------------------------------------------------------------------------------------------------ the size arithmetic
def tiles(n, k=None):
    k = k or K
    return (n + k["kTile"] - 1) // k["kTile"]


def scan_total_rounds(n, k=None):
    """iterations of k_scan_totals' loop for a scan of n elements: the second one is the first that uses the carry"""
    k = k or K
    return (tiles(n, k) + k["totals_round"] - 1) // k["totals_round"]


def hist_scan_tiles(n, k=None):
    """tiles of the scan over the 2^radix_bits * tiles(n) digit counts of one sort pass"""
    k = k or K
    return tiles((1 << k["radix_bits"]) * tiles(n, k), k)


def sort_passes(bits, k=None):
    k = k or K
    return 1 if bits <= 0 else (bits + k["radix_bits"] - 1) // k["radix_bits"]


def copy_back(passes):
    return passes % 2 == 0


def _bits_ge(n):
    """`int bits = 1; while ((1 << bits) < n) ++bits;`: the smallest b >= 1 with 2^b >= n"""
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def range_bits(P):
    return _bits_ge(P)


def row_bits(V):
    return _bits_ge(V)


def chain_len_bits(E):
    """`int lbits = 1; while ((1L << lbits) <= E && lbits < 32) ++lbits;`: the smallest b >= 1 with 2^b > E"""
    b = 1
    while (1 << b) <= E and b < 32:
        b += 1
    return b


def chain_range_bits(P):
    """the range key of a hub row's group is P itself"""
    return _bits_ge(P + 1)


def clamped_ranges(P, cols):
    return max(1, min(P, cols))


def reduce_sweeps(n, k=None):
    """iterations of k_reduce's grid-stride loop for the threads that do the most"""
    k = k or K
    grid = min((n + k["kBlock"] - 1) // k["kBlock"], k["reduce_grid"])
    return (n + grid * k["kBlock"] - 1) // (grid * k["kBlock"])


def device_built(E, P, max_id, free_bytes, k=None):
    """build_partitioned_gpu's conditions (api.hip): False = the host builder takes the graph"""
    k = k or K
    return (E > 0 and k["blocked_bytes_per_edge"] * E <= free_bytes // k["free_divisor"] and max_id <= k["id_guard"]
            and clamped_ranges(P, max_id + 1) <= k["range_guard"])


def chain_device_built(E, P, max_id, free_bytes, k=None):
    """build_rows_blocked_gpu's conditions for a forced range count P"""
    k = k or K
    return (E > 0 and k["chain_bytes_per_edge"] * E <= free_bytes // k["free_divisor"] and max_id + 1 < (1 << k["chain_id_bits"])
            and 2 <= clamped_ranges(P, max_id + 1) <= k["range_guard"])


# ------------------------------------------------------------------------------------------------------------ the blocked order in numpy
def range_keys(idx, P, cols):
    assert 1 <= P <= cols
    return np.minimum(np.asarray(idx, np.int64) // (cols // P), P - 1)


def blocked_order(ptr, idx, P, cols, ng=0, val=None):
    """The reference's locality schedule (per source range, per row, the sub-row of edges whose id falls in the range, cut every ng
    edges; ng = 0: no cut) without a loop over the ranges: O(E log E) whatever P is.  Every id must lie below cols.
    Returns (ptr_s, idx_s, target, val_s or None) as oracle.locality_schedule does."""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int32)
    E = len(idx)
    assert E == 0 or int(idx.max()) < cols
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    key = range_keys(idx, P, cols)
    order = np.argsort(key, kind="stable")          # CSR order inside a range: row-major, in-row order kept
    ks, rs = key[order], rows[order]
    pos = np.arange(E, dtype=np.int64)
    start = np.ones(E, bool)
    start[1:] = (ks[1:] != ks[:-1]) | (rs[1:] != rs[:-1])
    ss = np.maximum.accumulate(np.where(start, pos, 0)) if E else pos
    gflag = ((pos - ss) % ng == 0) if ng > 0 else start
    ptr_s = np.concatenate([pos[gflag], [E]]).astype(np.int32)
    return ptr_s, idx[order], rs[gflag].astype(np.int32), (None if val is None else np.asarray(val, np.float32)[order])


def subrows(ptr, idx, P, cols):
    """(start, length, row, range) of every (row, range) sub-row, in the blocked order"""
    ps, _, tg, _ = blocked_order(ptr, idx, P, cols, 0)
    key = np.sort(range_keys(idx, P, cols), kind="stable")
    return ps[:-1].astype(np.int64), np.diff(ps).astype(np.int64), tg, key[ps[:-1]]


# ------------------------------------------------------------------------------------------------------------ what the device builder keeps
# The device builders keep only what the segmented-stream kernels read; the host builders keep the permuted ids and the descriptor form
# as well (at least 4 bytes per edge more).  gnnagg_plan_info's plan_bytes therefore tells which builder made a plan, and the exact
# figure checks bookkeeping that no schedule query shows: the span cut, the rows with several groups, the rows without any.
def span_count(ptr_s, span_edges, group_range=None):
    """the greedy cut of both builders: a span takes whole groups until it holds span_edges edges (chain plan: or its range ends)"""
    G, n, g = len(ptr_s) - 1, 0, 0
    while g < G:
        h = max(g + 1, int(np.searchsorted(ptr_s[:G], ptr_s[g] + span_edges, "left")))
        if group_range is not None:
            h = min(h, int(np.searchsorted(group_range, group_range[g], "right")))
        n, g = n + 1, h
    return n


def blocked_plan_bytes(ptr_s, target, V, k=None):
    """device bytes of gpu_build_blocked_plan's arrays: ptr_s, target, eperm, idx_f, span_g, rg_ptr, rg_idx, crows, empty_rows"""
    k = k or K
    G, E = len(target), int(ptr_s[-1])
    groups_of = np.bincount(target, minlength=V)
    n_spans = span_count(np.asarray(ptr_s, np.int64), k["kSpanEdges"])
    return 4 * ((G + 1) + G + 2 * E + (n_spans + 1) + (V + 1) + G + int((groups_of > 1).sum()) + int((groups_of == 0).sum()))


def chain_plan_bytes(ptr, idx, P, cols, hub_edges, k=None):
    """device bytes of gpu_build_chain_plan's arrays before the first run: the groups of the rows that stay, range-major and longest
    first inside a range (stable), their edges twice (eperm, flagged ids), one span list per range, four ints per hub row, one byte
    per row of the hub mask"""
    k = k or K
    V = len(ptr) - 1
    _, length, row, rng_of = subrows(ptr, idx, P, cols)
    hub_rows = np.unique(row[length > hub_edges])
    kept = ~np.isin(row, hub_rows)
    order = np.lexsort((-length[kept], rng_of[kept]))
    nptr = np.concatenate([[0], np.cumsum(length[kept][order])])
    G, NE = int(kept.sum()), int(nptr[-1])
    n_spans = span_count(nptr, k["kSpanEdges"], rng_of[kept][order])
    return 4 * ((G + 1) + G + 2 * NE + (n_spans + 1) + 4 * len(hub_rows)) + V


# ------------------------------------------------------------------------------------------------------------ the graph maker
def plan_graph(V, E, cols, seed, empty=(), live=None, fixed=None, sort_rows=False, dups=False, ids=None, max_at=None):
    """A CSR with exactly E edges over V rows whose largest id is cols - 1 (the library takes its column count from it).
    empty: rows without edges;  live: the only rows that may have edges (default: all but `empty`);  fixed: {row: ids} rows given in
    full (the other live rows share the remaining edges at random);  sort_rows: ids ascending in every row (the chain plan needs it);
    dups: about a quarter of the edges repeat the id before them in their row;  ids: all E ids, in CSR order, given by the caller;
    max_at: the only edge that holds cols - 1 (default: one edge picked at random; sorted rows: the last edge of the last row).
    Returns (ptr int32[V + 1], idx int32[E])."""
    rng = np.random.default_rng(seed)
    fixed = {int(r): np.asarray(a, np.int32) for r, a in (fixed or {}).items()}
    ok = np.ones(V, bool)
    ok[list(empty)] = False
    if live is not None:
        keep = np.zeros(V, bool)
        keep[list(live)] = True
        ok &= keep
    for r in fixed:
        assert ok[r]
        ok[r] = False
    free_rows = np.nonzero(ok)[0]
    rest = E - sum(len(a) for a in fixed.values())
    assert rest >= 0 and (rest == 0 or len(free_rows) > 0)
    deg = np.zeros(V, np.int64)
    if rest:
        deg[free_rows] = rng.multinomial(rest, np.full(len(free_rows), 1.0 / len(free_rows)))
    for r, a in fixed.items():
        deg[r] = len(a)
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    rows = np.repeat(np.arange(V), deg)
    if ids is not None:
        idx = np.asarray(ids, np.int32).copy()
        assert len(idx) == E
    else:
        idx = rng.integers(0, cols - 1 if cols > 1 else 1, E).astype(np.int32)     # cols - 1 itself is placed below
        if dups and E > 1:
            rep = (rng.random(E) < 0.25) & np.concatenate([[False], rows[1:] == rows[:-1]])
            src = np.arange(E)
            src[rep] -= 1
            idx = idx[src]
    for r, a in fixed.items():
        idx[ptr[r]:ptr[r + 1]] = a
    if sort_rows:
        idx = idx[np.lexsort((idx, rows))]
    if ids is None and E > 0 and (max_at is not None or int(idx.max()) != cols - 1):
        if max_at is None:      # an edge of a row that is not given in full; sorted rows: the last edge of such a row
            movable = np.nonzero(~np.isin(rows, list(fixed)))[0]
            if sort_rows:
                movable = movable[np.concatenate([rows[movable][1:] != rows[movable][:-1], [True]])]
            max_at = int(rng.choice(movable))
        idx[max_at] = cols - 1
    assert len(idx) == E and (E == 0 or int(idx.max()) == cols - 1), "the graph does not reach its column count"
    return ptr, idx


def graph_of(entry):
    """(ptr, idx) of a table entry"""
    g = dict(entry.get("graph", {}))
    if callable(g.get("ids")):
        g["ids"] = g["ids"](entry["E"], entry["cols"])
    if callable(g.get("fixed")):
        g["fixed"] = g["fixed"]()
    return plan_graph(entry["V"], entry["E"], entry["cols"], entry.get("seed", 1), **g)


def sparse_live(V, n, seed):
    """n rows of V that may hold edges: both ends and a random spread between them, so every byte of the row id varies"""
    rng = np.random.default_rng(seed)
    return sorted(set([0, V - 1]) | set(int(r) for r in rng.choice(V, min(n, V), replace=False)))


# ------------------------------------------------------------------------------------------------------------ the tables: balanced order
# Every entry: name, V, E, cols (= largest id + 1), P ("partitions"), graph (plan_graph's keywords), claims (the side it is there for,
# checked by tests/test_plan_census_host.py), optionally F (default 64), gat (the entry also runs as an Aggregator_GAT handle, 1 x 64),
# host (the ONE condition of build_partitioned_gpu that the entry fails: the host builder takes it).
def _e(name, V, E, cols, P, claims, graph=None, **kw):
    d = {"name": name, "V": V, "E": E, "cols": cols, "P": P, "claims": claims, "graph": graph or {}}
    d.update(kw)
    return d


# tile edges of the scans and the sort: wavefront, workgroup-round and tile boundaries, one below / on / one above
TILE_EDGES = [
    _e("tile-E%d" % E, 7, E, 50, 2, {"tiles": (E + 4095) // 4096, "ragged_last_tile": E % 4096 != 0}, gat=(E == 4097))
    for E in (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 8193)
]

# k_scan_totals' second round (and the only sizes whose digit-count scan has 16 and 17 tiles)
TOTALS_ROUNDS = [
    _e("totals-256-tiles", 3000, 256 * 4096, 3000, 3, {"tiles": 256, "scan_rounds": 1, "hist_scan_tiles": 16, "ragged_last_tile": False}, F=4),
    _e("totals-257-tiles", 3001, 256 * 4096 + 1, 2999, 3, {"tiles": 257, "scan_rounds": 2, "hist_scan_tiles": 17, "ragged_last_tile": True}, F=4,
       gat=True),
]

# passes of the sort by range, and k_range_keys' clamp (ids at or beyond P * (cols // P) belong to the last range)
_RG = {"dups": True}
RANGE_PASSES = [
    _e("range-P1", 300, 40003, 70001, 1, {"range_passes": 1, "copy_back": False, "clamp": False}, _RG),
    _e("range-P2", 300, 40003, 70001, 2, {"range_passes": 1, "copy_back": False, "clamp": True}, _RG),
    _e("range-P255", 300, 40003, 70001, 255, {"range_passes": 1, "copy_back": False, "clamp": True}, _RG),
    _e("range-P256", 300, 40003, 70001, 256, {"range_passes": 1, "copy_back": False, "clamp": True}, _RG),
    _e("range-P257", 300, 40003, 70001, 257, {"range_passes": 2, "copy_back": True, "clamp": True}, _RG, gat=True),
    _e("range-P1024", 300, 40003, 70001, 1024, {"range_passes": 2, "copy_back": True, "clamp": True}, _RG),
    # width 1: the last range collects every id >= 65534
    _e("range-P65535", 300, 40003, 70001, 65535, {"range_passes": 2, "copy_back": True, "clamp": True, "width": 1, "device": True}, _RG),
    _e("range-P65536-host", 300, 40003, 70001, 65536, {"device": False, "width": 1}, _RG, host="range_guard"),
    _e("range-P-equals-cols", 300, 40003, 1000, 1000, {"range_passes": 2, "copy_back": True, "clamp": False, "width": 1}, _RG),
]

# passes of the sort that lists every row's groups (bits from V): most rows empty at the large V, the last row never
ROW_PASSES = [
    _e("rows-V1", 1, 20000, 500, 4, {"row_passes": 1, "row_copy_back": False}),
    _e("rows-V256", 256, 20000, 500, 4, {"row_passes": 1, "row_copy_back": False}),
    _e("rows-V257", 257, 20000, 500, 4, {"row_passes": 2, "row_copy_back": True, "last_row_live": True}, {"live": sparse_live(257, 200, 3)},
       gat=True),
    _e("rows-V65536", 65536, 20000, 500, 4, {"row_passes": 2, "row_copy_back": True, "last_row_live": True},
       {"live": sparse_live(65536, 300, 4)}),
    _e("rows-V65537", 65537, 20000, 500, 4, {"row_passes": 3, "row_copy_back": False, "last_row_live": True},
       {"live": sparse_live(65537, 300, 5)}),
]

# the max-scan's carry across whole tiles: ONE (row, range) sub-row of 3 * 4096 + 5 edges that starts inside a tile (rows 0..2 put 1500
# edges of range 0 before it), behind a run of empty rows and before short rows
_LONG = 3 * 4096 + 5


def _long_row():
    d = {r: np.random.default_rng(78 + r).integers(0, 999, 1000) for r in range(3)}
    d[13] = np.random.default_rng(77).integers(0, 500, _LONG)
    return d


MAX_SCAN_CARRY = [
    _e("long-subrow", 40, _LONG + 3000 + 2000, 1000, 2, {"longest_subrow": _LONG, "starts_inside_tile": True, "whole_tiles_inside": 2},
       {"empty": range(3, 13), "fixed": _long_row}, gat=True),
]

EMPTY_ROWS = [
    _e("empty-row0", 50, 3000, 200, 3, {"empty": [0]}, {"empty": [0]}),
    _e("empty-rows0-9", 50, 3000, 200, 3, {"empty": list(range(10))}, {"empty": range(10)}, gat=True),
    _e("empty-last-row", 50, 3000, 200, 3, {"empty": [49]}, {"empty": [49]}),
    _e("empty-every-second-row", 50, 3000, 200, 3, {"empty": list(range(0, 50, 2))}, {"empty": range(0, 50, 2)}),
    _e("empty-every-second-row-odd", 51, 3000, 200, 3, {"empty": list(range(1, 51, 2))}, {"empty": range(1, 51, 2)}),
]

# digit patterns of k_sort_scatter at P = 256 (cols 1024: width 4)
DIGIT_PATTERNS = [
    # 64 equal digits in every wavefront: the rank among equal digits runs to 63, one digit takes every element
    _e("digits-one-range", 20, 5000, 1024, 256, {"ranges_per_wave": (1, 1), "ranges_used": 1},
       {"ids": lambda E, cols: cols - 4 + (np.arange(E) * 7) % 4}),
    # 64 consecutive edges hold 64 different ranges: every rank is 0
    _e("digits-cycle", 20, 5000, 1024, 256, {"ranges_per_wave": (64, 64), "ranges_used": 256},
       {"ids": lambda E, cols: (np.arange(E) % 256) * 4 + 3}, gat=True),
    _e("digits-two-alternating", 20, 5000, 1024, 256, {"ranges_per_wave": (2, 2), "ranges_used": 2},
       {"ids": lambda E, cols: np.where(np.arange(E) % 2 == 1, cols - 1, 3)}),
]

# gpu_max_col's reduction: the largest id in ONE place (judged through balanced_partition_columns()); 2048 * 256 + 7 is read in the second
# sweep of the grid-stride loop
REDUCTION = [
    _e("max-at-edge0", 50, 5000, 300, 2, {"max_at": 0, "reduce_sweeps": 1}, {"max_at": 0}),
    _e("max-at-last-edge", 50, 5000, 300, 2, {"max_at": 4999, "reduce_sweeps": 1}, {"max_at": 4999}),
    _e("max-in-second-sweep", 2000, 600001, 3000, 2, {"max_at": 2048 * 256 + 7, "reduce_sweeps": 2}, {"max_at": 2048 * 256 + 7}, F=4, gat=True),
]

BALANCED_GROUPS = {
    "tile_edges": TILE_EDGES, "totals_rounds": TOTALS_ROUNDS, "range_passes": RANGE_PASSES, "row_passes": ROW_PASSES,
    "max_scan_carry": MAX_SCAN_CARRY, "empty_rows": EMPTY_ROWS, "digit_patterns": DIGIT_PATTERNS, "reduction": REDUCTION,
}
BALANCED = [e for g in BALANCED_GROUPS.values() for e in g]

# ------------------------------------------------------------------------------------------------------------ the tables: chain plan
# Rows sorted ascending, "fast_rows" = 0, "partitions" = P >= 2.  hub: the "rows_hub_edges" option (a row with a sub-row of MORE edges
# leaves the chains whole); default: no row is a hub.  claims["ranges"]: what rows_blocked_ranges() answers (0: the row kernels run).
# NOT here: the four-pass length sort.  It needs E >= 2^24; what an even pass count adds (the copy back) is covered by the two-pass cases.
NO_HUBS = 1 << 28


def _c(name, V, E, cols, P, claims, graph=None, hub=NO_HUBS, **kw):
    g = dict(graph or {})
    g.setdefault("sort_rows", True)
    d = _e(name, V, E, cols, P, claims, g, **kw)
    d["hub"] = hub
    return d


def _hub_threshold_rows():
    # range 0 = ids < 100, range 1 = the rest: row 5 has a sub-row of exactly 64 edges (stays), row 9 one of 65 (leaves, whole)
    return {5: np.concatenate([np.arange(64), [150, 160, 170]]), 9: np.concatenate([[3, 4], 100 + np.arange(65)])}


def _all_hub_rows():
    return {r: np.concatenate([np.arange(70) + r, [150 + r]]) for r in range(6)}


def _one_row_stays():
    d = _all_hub_rows()
    d[3] = np.concatenate([np.arange(64), [150]])
    return d


def _empty_ranges_rows():
    # 5 ranges of 20 ids: ordinary rows hold ids of ranges 1 and 3 only; the last range holds only the sub-row of a hub row, whose groups
    # leave the plan (the largest id, which sets the column count, always lies in the last range)
    rng = np.random.default_rng(31)
    d = {r: np.sort(np.concatenate([rng.integers(20, 40, 6), rng.integers(60, 80, 5)])) for r in range(1, 30)}
    d[0] = np.concatenate([np.arange(80, 100), np.repeat(99, 20)])
    return d


def _unsorted_last_edge():
    rng = np.random.default_rng(32)
    d = {r: np.sort(rng.integers(0, 199, 30)) for r in range(20)}
    d[19][-1] = 199
    d[7][-1] = d[7][-2] - 1          # the ONLY descent of the graph: the last edge of row 7
    return d


CHAIN_GROUPS = {
    "length_passes": [
        _c("len-E255", 40, 255, 100, 2, {"len_passes": 1, "len_copy_back": False, "ranges": 2}),
        _c("len-E256", 40, 256, 100, 2, {"len_passes": 2, "len_copy_back": True, "ranges": 2}),
        _c("len-E65535", 40, 65535, 100, 2, {"len_passes": 2, "len_copy_back": True, "ranges": 2}),
        _c("len-E65536", 40, 65536, 100, 2, {"len_passes": 3, "len_copy_back": False, "ranges": 2}),
    ],
    "range_passes": [
        _c("crange-P255", 60, 6000, 512, 255, {"crange_passes": 1, "crange_copy_back": False, "ranges": 255}),
        _c("crange-P256", 60, 6000, 512, 256, {"crange_passes": 2, "crange_copy_back": True, "ranges": 256}),
    ],
    "hub_threshold": [
        _c("hub-64-stays-65-leaves", 30, 67 + 67 + 28 * 12, 200, 2, {"hub_rows": [9], "longest_kept_subrow": 64, "ranges": 2},
           {"fixed": _hub_threshold_rows}, hub=64),
        _c("hub-every-row", 8, 6 * 71, 156, 2, {"hub_rows": [0, 1, 2, 3, 4, 5], "kept_groups": 0, "ranges": 0},
           {"fixed": _all_hub_rows, "empty": [6, 7]}, hub=64),
        _c("hub-all-but-one", 8, 5 * 71 + 65, 156, 2, {"hub_rows": [0, 1, 2, 4, 5], "longest_kept_subrow": 64, "ranges": 2},
           {"fixed": _one_row_stays, "empty": [6, 7]}, hub=64),
    ],
    "empty_ranges": [
        _c("ranges-1-and-3-of-5", 30, 29 * 11 + 40, 100, 5, {"hub_rows": [0], "ranges_with_groups": [1, 3], "ranges": 5},
           {"fixed": _empty_ranges_rows, "sort_rows": False}, hub=32),
    ],
    "unsorted": [
        _c("unsorted-last-edge-of-one-row", 20, 600, 200, 2, {"descents": 1, "ranges": 0}, {"fixed": _unsorted_last_edge, "sort_rows": False}),
    ],
}
CHAIN = [e for g in CHAIN_GROUPS.values() for e in g]
