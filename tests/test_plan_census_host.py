"""CPU half of the plan-builder census (tests/plan_census.py): every table entry sits on the side of the switch it claims, the tables
together reach both sides of every switch of csrc/prims.cuh, csrc/plan_gpu.hip and the guards of csrc/api.hip, and the numpy restatement
of the blocked order is the oracle's and the host builder's, array for array.

The constants come out of the sources: a changed kItems, pass width, grid cap or guard fails these tests until the tables follow."""
import re

import numpy as np
import pytest

import gnn_computing_amd as gnc
from oracle import oracle as orc

import plan_census as pc

HUGE = 1 << 50          # free memory for the guards that are not under test


def evaluate(entry, ptr, idx, k):
    """what the restated arithmetic gives for every key an entry may claim"""
    V, E, P, cols = entry["V"], entry["E"], entry["P"], entry["cols"]
    Pc = pc.clamped_ranges(P, cols)
    width = cols // Pc
    deg = np.diff(ptr)
    key = pc.range_keys(idx, Pc, cols)
    out = {
        "tiles": pc.tiles(E, k), "ragged_last_tile": E % k["kTile"] != 0, "scan_rounds": pc.scan_total_rounds(E, k),
        "hist_scan_tiles": pc.hist_scan_tiles(E, k),
        "range_passes": pc.sort_passes(pc.range_bits(Pc), k), "width": width, "clamp": bool(np.any(idx // width >= Pc)),
        "device": pc.device_built(E, P, cols - 1, HUGE, k),
        "row_passes": pc.sort_passes(pc.row_bits(V), k), "last_row_live": bool(deg[V - 1] > 0),
        "len_passes": pc.sort_passes(pc.chain_len_bits(E), k), "crange_passes": pc.sort_passes(pc.chain_range_bits(Pc), k),
        "ranges_used": len(np.unique(key)),
    }
    out["copy_back"] = pc.copy_back(out["range_passes"])
    out["row_copy_back"] = pc.copy_back(out["row_passes"])
    out["len_copy_back"] = pc.copy_back(out["len_passes"])
    out["crange_copy_back"] = pc.copy_back(out["crange_passes"])
    out["empty"] = [r for r in entry["claims"].get("empty", []) if deg[r] == 0]
    nw = E // 64
    if nw:
        per = [len(np.unique(w)) for w in key[:nw * 64].reshape(nw, 64)]
        out["ranges_per_wave"] = (min(per), max(per))
    at = np.nonzero(idx == cols - 1)[0]
    out["max_at"] = int(at[0]) if len(at) == 1 else [int(a) for a in at[:4]]
    grid = min((E + k["kBlock"] - 1) // k["kBlock"], k["reduce_grid"])
    out["reduce_sweeps"] = 1 + int(at[0]) // (grid * k["kBlock"])            # the sweep that reads the largest id
    start, length, row, rng_of = pc.subrows(ptr, idx, Pc, cols)
    j = int(np.argmax(length))
    out["longest_subrow"] = int(length[j])
    out["starts_inside_tile"] = bool(start[j] % k["kTile"] != 0)
    out["whole_tiles_inside"] = int((start[j] + length[j]) // k["kTile"] - (start[j] + k["kTile"] - 1) // k["kTile"])
    hub = entry.get("hub")
    if hub is not None:
        hub_rows = np.unique(row[length > hub])
        kept = ~np.isin(row, hub_rows)
        rows_of_edges = np.repeat(np.arange(V), deg)
        out["hub_rows"] = [int(r) for r in hub_rows]
        out["kept_groups"] = int(kept.sum())
        out["longest_kept_subrow"] = int(length[kept].max()) if kept.any() else 0
        out["ranges_with_groups"] = [int(p) for p in np.unique(rng_of[kept])]
        out["descents"] = int(np.sum((rows_of_edges[1:] == rows_of_edges[:-1]) & (idx[1:] < idx[:-1])))
        applies = out["descents"] == 0 and out["kept_groups"] > 0 and pc.chain_device_built(E, P, cols - 1, HUGE, k)
        out["ranges"] = Pc if applies else 0
    return out


def mismatches(k):
    bad = []
    for entry in pc.BALANCED + pc.CHAIN:
        ptr, idx = GRAPHS[entry["name"]]
        got = evaluate(entry, ptr, idx, k)
        for key, want in entry["claims"].items():
            if got[key] != want:
                bad.append((entry["name"], key, want, got[key]))
    return bad


class _Graphs(dict):
    """(ptr, idx) of every entry, made on first use (collecting this file makes none)"""
    def __missing__(self, name):
        self[name] = pc.graph_of(ENTRIES[name])
        return self[name]


ENTRIES = {e["name"]: e for e in pc.BALANCED + pc.CHAIN}
GRAPHS = _Graphs()


def test_constants_read_from_the_sources():
    k = pc.K
    assert k["kTile"] == k["kBlock"] * k["kItems"] and k["totals_round"] == k["kBlock"]
    assert k["range_guard"] == 0xffff          # the builder's comment: "keeps the range in 16 bits"
    assert k["id_guard"] == (1 << 30) - 1      # two flag bits above the id
    assert k["free_divisor"] == 2 and k["chain_id_bits"] == 24 and k["kSpanEdges"] > 0
    assert k["chain_bytes_per_edge"] > k["blocked_bytes_per_edge"] > 0


def test_every_graph_is_what_its_entry_says():
    names = [e["name"] for e in pc.BALANCED + pc.CHAIN]
    assert len(set(names)) == len(names)
    for entry in pc.BALANCED + pc.CHAIN:
        ptr, idx = GRAPHS[entry["name"]]
        assert len(ptr) == entry["V"] + 1 and len(idx) == entry["E"] == int(ptr[-1]), entry["name"]
        assert int(idx.min()) >= 0 and int(idx.max()) == entry["cols"] - 1, entry["name"]
        assert np.all(np.diff(ptr) >= 0)
        assert entry["claims"], entry["name"]
    for entry in pc.CHAIN:
        assert entry["P"] >= 2


def test_every_entry_sits_on_the_side_it_claims():
    assert mismatches(pc.K) == []


@pytest.mark.parametrize("name,old,new", [
    ("kItems", "kItems = 16", "kItems = 8"),
    ("kBlock", "kBlock = 256", "kBlock = 128"),
    ("pass width", "(bits + 7) / 8", "(bits + 3) / 4"),
    ("reduce grid", "/ kBlock, 2048)", "/ kBlock, 4096)"),
])
def test_a_changed_constant_in_prims_fails_the_claims(name, old, new):
    """the tables are pinned to the sources: an edited copy of prims.cuh puts entries on the other side of their switch"""
    text = open(pc.CSRC + "/prims.cuh").read()
    assert text.count(old) == 1
    text = text.replace(old, new)
    if name == "pass width":
        text = text.replace("8 * p", "4 * p").replace("& 255u", "& 15u")
    assert mismatches(pc.read_constants(prims_text=text)) != [], name


def test_a_changed_guard_fails_the_claims():
    plan = open(pc.CSRC + "/plan_gpu.hip").read().replace("par_num > 65535", "par_num > 65534")
    api = open(pc.CSRC + "/api.hip").read().replace("par_num > 65535", "par_num > 65534")
    bad = mismatches(pc.read_constants(plan_text=plan, api_text=api))
    assert [b[:2] for b in bad] == [("range-P65535", "device")]
    with pytest.raises(AssertionError):          # the guard of api.hip and the builder's own must stay the same number
        pc.read_constants(plan_text=plan)


def _claimed(key, entries=None):
    return [e["claims"][key] for e in (entries or pc.BALANCED + pc.CHAIN) if key in e["claims"]]


def test_the_tables_reach_both_sides_of_every_switch():
    k = pc.K
    T = k["kTile"]
    bal = {e["name"]: e for e in pc.BALANCED}
    # scans and sort: one partial tile, exact multiples of the tile, one element beyond, the second round of the totals scan
    sizes = sorted(e["E"] for e in pc.TILE_EDGES)
    for n in (1, 63, 64, 65, k["kBlock"] - 1, k["kBlock"], k["kBlock"] + 1, T - 1, T, T + 1, 2 * T, 2 * T + 1):
        assert n in sizes, n
    assert {1, 2, 3} <= set(_claimed("tiles")) and {True, False} == set(_claimed("ragged_last_tile"))
    assert [e["E"] for e in pc.TOTALS_ROUNDS] == [k["totals_round"] * T, k["totals_round"] * T + 1]
    assert set(_claimed("scan_rounds")) == {1, 2}
    assert min(_claimed("hist_scan_tiles")) <= 16 < max(_claimed("hist_scan_tiles"))      # (16: what every other test's graph stays below)
    # the three sorts: every pass count the builder can ask for below E = 2^24, and both parities
    assert set(_claimed("range_passes")) == {1, 2} and set(_claimed("copy_back")) == {True, False}
    assert set(_claimed("row_passes")) == {1, 2, 3} and set(_claimed("row_copy_back")) == {True, False}
    assert set(_claimed("len_passes")) == {1, 2, 3} and set(_claimed("len_copy_back")) == {True, False}
    assert set(_claimed("crange_passes")) == {1, 2} and set(_claimed("crange_copy_back")) == {True, False}
    one = 1 << k["radix_bits"]
    assert {1, 2, one - 1, one, one + 1, 1024, k["range_guard"], k["range_guard"] + 1} <= {e["P"] for e in pc.RANGE_PASSES}
    assert {1, one, one + 1, one * one, one * one + 1} == {e["V"] for e in pc.ROW_PASSES}
    assert {one - 1, one, one * one - 1, one * one} == {e["E"] for e in pc.CHAIN_GROUPS["length_passes"]}
    assert {one - 1, one} == {e["P"] for e in pc.CHAIN_GROUPS["range_passes"]}
    # the guards: the last count the device builder takes and the first it leaves to the host; the clamp on and off; P = cols
    assert set(_claimed("device")) == {True, False} and set(_claimed("clamp")) == {True, False}
    assert any(e["P"] == e["cols"] for e in pc.RANGE_PASSES)
    assert [e["name"] for e in pc.BALANCED if "host" in e] == ["range-P65536-host"]
    # the max-scan carries a sub-row start across at least two whole tiles
    assert max(_claimed("whole_tiles_inside")) >= 2 and all(_claimed("starts_inside_tile"))
    # rows without edges at both ends, runs, alternating on both parities
    empties = _claimed("empty")
    assert any(r == [0] for r in empties) and any(len(r) >= 10 and r[:10] == list(range(10)) for r in empties)
    assert any(r == [e["V"] - 1] for e in pc.EMPTY_ROWS for r in [e["claims"]["empty"]])
    assert any(r[:3] == [0, 2, 4] for r in empties) and any(r[:3] == [1, 3, 5] for r in empties)
    # digit patterns and the reduction's sweeps
    assert {(1, 1), (2, 2), (64, 64)} == set(_claimed("ranges_per_wave"))
    assert set(_claimed("reduce_sweeps")) == {1, 2}
    assert {0, bal["max-at-last-edge"]["E"] - 1, k["reduce_grid"] * k["kBlock"] + 7} == set(_claimed("max_at"))
    # chain plan: hubs on both sides of the threshold, no group left, ranges without a group at both ends and inside, unsorted rows
    assert 64 in _claimed("longest_kept_subrow") and 0 in _claimed("kept_groups")
    assert [1, 3] in _claimed("ranges_with_groups") and 1 in _claimed("descents")
    assert 0 in _claimed("ranges") and max(_claimed("ranges")) >= 256
    # one GAT handle per group of the balanced table
    for name, group in pc.BALANCED_GROUPS.items():
        assert sum(1 for e in group if e.get("gat")) == 1, name
        assert all("host" not in e for e in group if e.get("gat"))


def test_the_guards_restated():
    k = pc.K
    assert pc.device_built(1000, 65535, 70000, 2 * 72 * 1000, k) and not pc.device_built(1000, 65535, 70000, 2 * 72 * 1000 - 2, k)
    assert pc.device_built(1000, 65536, 65534, HUGE, k)            # the clamp to the column count comes first
    assert not pc.device_built(1000, 65536, 65535, HUGE, k)
    assert pc.device_built(10, 2, 0x3fffffff, HUGE, k) and not pc.device_built(10, 2, 0x40000000, HUGE, k)
    assert pc.chain_device_built(10, 2, (1 << 24) - 2, HUGE, k) and not pc.chain_device_built(10, 2, (1 << 24) - 1, HUGE, k)
    assert not pc.chain_device_built(10, 1, 100, HUGE, k) and not pc.chain_device_built(10, 5, 0, HUGE, k)
    assert [pc.range_bits(p) for p in (1, 2, 3, 256, 257, 65535, 65536)] == [1, 1, 2, 8, 9, 16, 16]
    assert [pc.chain_len_bits(e) for e in (1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)] == [1, 8, 9, 16, 17, 24, 25]
    assert [pc.chain_range_bits(p) for p in (2, 255, 256)] == [2, 8, 9]
    assert [pc.sort_passes(b, k) for b in (0, 1, 8, 9, 16, 17, 24, 25, 32)] == [1, 1, 1, 2, 2, 3, 3, 4, 4]


# small graphs for the restatement itself: (V, E, cols, P, ng, plan_graph keywords)
RESTATED = [
    (30, 700, 64, 4, 0, {}),
    (30, 700, 64, 4, 8, {}),
    (30, 700, 67, 5, 3, {}),                                         # cols % P != 0: the last range is wider
    (30, 700, 67, 67, 0, {}),                                        # P = cols
    (30, 700, 67, 67, 2, {"dups": True}),
    (30, 700, 64, 1, 0, {}),                                         # P = 1
    (30, 700, 64, 1, 16, {}),
    (40, 500, 50, 3, 4, {"empty": [0, 1, 2, 17, 18, 39]}),
    (40, 500, 50, 7, 0, {"empty": range(0, 40, 2)}),
    (12, 900, 10, 3, 5, {"dups": True}),                             # unsorted rows, many equal ids: stability shows in val_s
    (12, 900, 10, 10, 0, {"dups": True}),
    (1, 300, 20, 4, 7, {}),
    (25, 600, 90, 6, 128, {"sort_rows": True}),
    (5, 1, 1, 1, 4, {"live": [3]}),
]


@pytest.mark.parametrize("V,E,cols,P,ng,kw", RESTATED)
def test_numpy_restatement_is_the_oracles_and_the_host_builders(V, E, cols, P, ng, kw):
    ptr, idx = pc.plan_graph(V, E, cols, seed=V + E + P + ng, **kw)
    val = np.arange(E, dtype=np.float32) + 0.5           # distinct: an order that is not stable shows
    mine = pc.blocked_order(ptr, idx, P, cols, ng, val)
    for other in (orc.locality_schedule(ptr, idx, P, cols, ng, val), gnc.locality_schedule(ptr, idx, P, cols, ng, val)):
        for a, b in zip(mine, other):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    no_val = pc.blocked_order(ptr, idx, P, cols, ng)
    assert no_val[3] is None and all(np.array_equal(a, b) for a, b in zip(no_val[:3], mine[:3]))


@pytest.mark.parametrize("name", ["tile-E257", "tile-E4097", "empty-rows0-9", "digits-cycle", "digits-two-alternating", "long-subrow",
                                  "range-P257", "range-P-equals-cols", "hub-64-stays-65-leaves", "ranges-1-and-3-of-5"])
def test_numpy_restatement_on_table_entries(name):
    entry = ENTRIES[name]
    ptr, idx = GRAPHS[name]
    val = np.arange(entry["E"], dtype=np.float32)
    P = pc.clamped_ranges(entry["P"], entry["cols"])
    for ng in (0, 128):
        mine = pc.blocked_order(ptr, idx, P, entry["cols"], ng, val)
        for other in (orc.locality_schedule(ptr, idx, P, entry["cols"], ng, val), gnc.locality_schedule(ptr, idx, P, entry["cols"], ng, val)):
            assert all(np.array_equal(a, b) for a, b in zip(mine, other))


def test_span_count_is_the_builders_greedy_walk():
    """plan_census.span_count against a transcription of the loops in gpu_build_blocked_plan / gpu_build_chain_plan"""
    def walk(ps, span, rng=None):
        G, g, n = len(ps) - 1, 0, 0
        while g < G:
            e0, h = ps[g], g + 1
            while h < G and ps[h] - e0 < span and (rng is None or rng[h] == rng[g]):
                h += 1
            n, g = n + 1, h
        return n

    assert pc.span_count(np.array([0, 100, 600, 700, 1300]), 512) == 2
    gen = np.random.default_rng(9)
    for lo, hi in ((1, 3), (1, 200), (300, 900), (1, 2000)):
        lens = gen.integers(lo, hi, 400)
        ps = np.concatenate([[0], np.cumsum(lens)])
        rng = np.sort(gen.integers(0, 7, 400))
        assert pc.span_count(ps, 512) == walk(ps, 512)
        assert pc.span_count(ps, 512, rng) == walk(ps, 512, rng)
    ps, _, tg, _ = pc.blocked_order(*GRAPHS["empty-rows0-9"], 3, 200, 16)
    G, E, V = len(tg), 3000, 50
    assert pc.blocked_plan_bytes(ps, tg, V) == 4 * (3 * G + 2 * E + V + 3 + pc.span_count(ps, pc.K["kSpanEdges"]) + 40 + 10)   # 40 rows with several groups


def test_sources_name_this_census():
    text = open(pc.CSRC + "/plan_gpu.hip").read()
    assert re.search(r"tests/test_gpu_plan_census\.py", text)
