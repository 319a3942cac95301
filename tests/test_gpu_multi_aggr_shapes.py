"""GPU: gnnagg_gcn_run_multi (Aggregator_GCN.run_multi) at the shapes the fixture of tests/test_gpu_multi_aggr.py does not reach:

* many rows: row counts on both sides of the 64 short-row workgroups at which the kernel remaps workgroups onto XCD ranges (xcd_remap),
  with long rows beside them, for every lane-group size;
* degenerate graphs: every row short (no segment, no scratch), every row long, no edge at all, one row of 1100 edges;
* every (aggr_mask, scaler_mask) pair through the C ABI;
* one handle with a history of widths, types, schedules, options, other calls, new edge values and streams against brand-new handles.

The judges are those of tests/test_gpu_multi_aggr.py (check_against_refs): min / max exact, sum / mean bit-equal to the float32
restatement on rows of at most 128 edges, and the BOUNDS of tests/test_multi_aggr_host.py everywhere."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_multi_aggr_host import (AGGRS, BOUNDS, LONG_EDGES, SCALERS, fixture_graph, fixture_val, fixture_x, multi_chain32, multi_layout,
                                  multi_ref, multi_width, scaler64, worst_ratio)
from test_multi_aggr_nonfinite_host import GPB, group_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
CANARY, GUARD = 7.0, 8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def np_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def canary_y(V, W, dtype=torch.float32):
    """(whole buffer, [V, W] view) with GUARD canary elements on either side"""
    buf = torch.full((V * W + 2 * GUARD,), CANARY, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + V * W].view(V, W)


def guards_intact(buf):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all())


def make_graph(deg, n_src, seed):
    deg = np.asarray(deg, np.int64)
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_src, size=int(ptr[-1])).astype(np.int32)
    val = rng.standard_normal(int(ptr[-1])).astype(np.float32)
    return ptr, idx, val


def features(n_src, F, seed, bf16=False):
    x = np.random.default_rng(seed).standard_normal((n_src, F)).astype(np.float32)
    return torch.from_numpy(x).to(BF).float().numpy() if bf16 else x


def run_and_judge(ptr, idx, val, x, xdtype=torch.float32, what=""):
    """all six aggregates x three scalers of one graph into a guarded y, judged by the rules of check_against_refs"""
    V, F = len(ptr) - 1, x.shape[1]
    deg = np.diff(ptr)
    short, has = deg <= LONG_EDGES, deg > 0
    delta = gnc.pna_delta(ptr)
    at = gnc.Aggregator_GCN(dev(ptr), dev(idx), None if val is None else dev(val))
    buf, y = canary_y(V, multi_width(AGGRS, SCALERS, F))
    at.run_multi(dev(x).to(xdtype), y, aggrs=AGGRS, scalers=SCALERS, delta=delta)
    torch.cuda.synchronize()
    assert guards_intact(buf), what + ": a canary word around y was written"
    a = y.cpu().numpy()
    blk = {k: a[:, s] for k, s in multi_layout(AGGRS, SCALERS, F).items()}
    ref, c32 = multi_ref(ptr, idx, val, x), multi_chain32(ptr, idx, val, x)
    assert np.array_equal(blk[("identity", "min")], ref["min"]) and np.array_equal(blk[("identity", "max")], ref["max"]), what + ": min / max"
    for k in ("sum", "mean"):
        assert np.array_equal(np_bits(blk[("identity", k)][short]), np_bits(c32[k][short])), "%s: %s is not the float32 chain on the short rows" % (what, k)
    for k in ("sum", "mean", "var", "std"):
        ratio = worst_ratio(blk[("identity", k)], ref[k], BOUNDS[k](ref))
        print("%s: %s worst |y - ref| / bound = %.4f" % (what, k, ratio))
        assert ratio <= 1.0, (what, k, ratio)
    # the scaler blocks: the identity block times one fp32 scalar per row (1e-6: test_scaler_blocks_are_the_identity_block_times_the_scaler)
    for s in ("amplification", "attenuation"):
        sc = scaler64(s, deg, delta)[:, None]
        for k in AGGRS:
            want = blk[("identity", k)].astype(np.float64) * sc
            assert (np.abs(blk[(s, k)].astype(np.float64) - want) <= 1e-6 * np.abs(want)).all(), (what, s, k)
    for k, b in blk.items():
        assert not np_bits(b[~has]).any(), "%s, %s: a row without edges is not +0" % (what, k)
    assert np.isfinite(a).all()
    return y


# 1 ------------------------------------------------------------------------------------------------ many rows
LONG_ROWS = (129, 600, 1100, 513, 1537)


@functools.lru_cache(maxsize=None)
def many_rows_graph(V):
    """degrees 0 .. 9 drawn per row and five long rows spread through the row range (one, two, three and four segments)"""
    deg = np.random.default_rng(5000 + V).integers(0, 10, size=V)
    for i, d in enumerate(LONG_ROWS):
        deg[1 + i * (V - 3) // (len(LONG_ROWS) - 1)] = d
    return make_graph(deg, V, 6000 + V)


MANY = [(F, torch.float32, V) for F in (5, 13, 128) for V in (504, 512, 513, 575)] + \
       [(F, dt, V) for F, dt in ((602, torch.float32), (512, BF)) for V in (252, 256, 257, 287)]


def test_many_rows_cases_stand_on_both_sides_of_the_remap_threshold():
    seen = {}
    for F, dt, V in MANY:
        g = group_of(F, 2 if dt == BF else 4)
        nb = -(-V // GPB[g])
        seen.setdefault((F, dt), []).append((nb, nb % 8, V % GPB[g]))
        ptr, _, _ = many_rows_graph(V)
        deg = np.diff(ptr)
        assert sorted(deg[deg > LONG_EDGES]) == sorted(LONG_ROWS) and (deg == 0).any() and deg[0] <= 9 and deg[-1] <= 9
    assert {group_of(5), group_of(13), group_of(128), group_of(602), group_of(512, 2)} == {8, 16, 32, 64}
    for key, got in seen.items():
        assert [nb for nb, _, _ in got] == [63, 64, 65, 72], (key, got)            # below, at and above the threshold of 64 workgroups
        assert [r for _, r, _ in got] == [7, 0, 1, 0]                              # ragged XCD ranges beside the segment workgroups
        assert any(rem for _, _, rem in got)                                       # a last workgroup with rows past V


@pytest.mark.parametrize("F,xdtype,V", MANY, ids=["F%d-%s-V%d" % (F, "bf16" if dt == BF else "f32", V) for F, dt, V in MANY])
def test_many_rows_on_both_sides_of_the_xcd_remap(F, xdtype, V):
    ptr, idx, val = many_rows_graph(V)
    x = features(V, F, 7000 + F, bf16=xdtype == BF)
    run_and_judge(ptr, idx, val, x, xdtype, "V = %d, F = %d" % (V, F))


# 2 ------------------------------------------------------------------------------------------------ degenerate graphs
@pytest.mark.parametrize("F", [5, 128])
@pytest.mark.parametrize("shape", ["all short", "all long", "one row of 1100"])
def test_degenerate_graphs(F, shape):
    deg = {"all short": [3, 0, 128, 1, 9, 64, 127, 2, 0, 5, 33], "all long": [129, 1100, 513, 130, 512, 1025, 2048],
           "one row of 1100": [1100]}[shape]
    ptr, idx, val = make_graph(deg, len(deg) + 3, 8000 + len(deg))
    run_and_judge(ptr, idx, val, features(len(deg) + 3, F, 8100 + F), what="%s, F = %d" % (shape, F))


@pytest.mark.parametrize("F", [5, 128])
@pytest.mark.parametrize("ydtype", [torch.float32, BF])
def test_a_graph_without_edges_is_all_plus_zero(F, ydtype):
    V = 11
    at = gnc.Aggregator_GCN(dev(np.zeros(V + 1, np.int32)), dev(np.zeros(0, np.int32)), None)
    x = dev(features(4, F, 1))
    x[1] = float("nan")                                              # never read
    buf, y = canary_y(V, multi_width(AGGRS, SCALERS, F), ydtype)
    at.run_multi(x, y, aggrs=AGGRS, scalers=SCALERS, delta=1.0)
    torch.cuda.synchronize()
    assert not bool(bits(y).any()), "a graph without edges is not all +0"
    assert guards_intact(buf)


# 3 ------------------------------------------------------------------------------------------------ every mask pair
@pytest.mark.parametrize("F", [5, 128])
def test_every_mask_pair_through_the_c_abi(F):
    """all 63 x 7 (aggr_mask, scaler_mask) pairs: y holds popcount x popcount x F columns, every block the bits of its block of the 63 x 7
    call, nothing written around it"""
    L = gnc.lib()
    ptr, idx, n_src = fixture_graph()
    V = len(ptr) - 1
    at = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(fixture_val()))
    x = dev(fixture_x(F))
    delta = gnc.pna_delta(ptr)
    px, f32 = ctypes.c_void_p(x.data_ptr()), _lib.DTYPE_F32
    at._use_current_stream()                                         # the C ABI launches on the handle's stream: the one y is filled on

    def call(amask, smask):
        W = bin(amask).count("1") * bin(smask).count("1") * F
        buf, y = canary_y(V, W)
        assert L.gnnagg_gcn_run_multi(at._h, px, f32, ctypes.c_void_p(y.data_ptr()), f32, F, amask, smask, delta) == _lib.OK, (amask, smask)
        return buf, y

    _, full = call(63, 7)
    lay = multi_layout(AGGRS, SCALERS, F)
    assert bool(torch.isfinite(full).all())
    for amask in range(1, 64):
        for smask in range(1, 8):
            buf, y = call(amask, smask)
            want = torch.cat([full[:, lay[(s, a)]] for j, s in enumerate(SCALERS) if smask >> j & 1 for i, a in enumerate(AGGRS) if amask >> i & 1], 1)
            assert same_bits(y, want.contiguous()), "aggr_mask = %d, scaler_mask = %d: a block is not its block of the full call" % (amask, smask)
            assert guards_intact(buf), "aggr_mask = %d, scaler_mask = %d: a canary word around y was written" % (amask, smask)


# 4 ------------------------------------------------------------------------------------------------ history
@functools.lru_cache(maxsize=None)
def square_fixture():
    """the fixture's rows over its first V sources only: run_bwd writes a [V, F] gradient"""
    ptr, idx, _ = fixture_graph()
    V = len(ptr) - 1
    return ptr, (idx % V).astype(np.int32), V


def test_a_handle_with_a_history_computes_what_a_fresh_one_computes():
    ptr, idx, V = square_fixture()
    dptr, didx = dev(ptr), dev(idx)
    vals = {"v1": dev(fixture_val()), "v2": dev(fixture_val()[::-1].copy())}
    delta = gnc.pna_delta(ptr)
    xs = {(F, dt): dev(fixture_x(F)[:V]).to(dt) for F, dt in ((5, torch.float32), (128, torch.float32), (1024, torch.float32), (1024, BF),
                                                                 (602, torch.float32), (64, torch.float32), (64, BF))}
    w32 = dev(np.random.default_rng(3).standard_normal((64, 32)).astype(np.float32) * np.float32(0.3))
    state = {"val": "v1"}

    def fresh():
        return gnc.Aggregator_GCN(dptr, didx, vals[state["val"]])

    def multi(at, F, dt=torch.float32):
        buf, y = canary_y(V, multi_width(AGGRS, SCALERS, F))
        at.run_multi(xs[(F, dt)], y, aggrs=AGGRS, scalers=SCALERS, delta=delta)
        return buf

    @functools.lru_cache(maxsize=None)
    def fresh_multi(F, val_key):
        return multi(fresh(), F)

    def others(at):
        """run() and run_with_nn_typed in the balanced mode: fp32 and bf16"""
        out = []
        for red in ("sum", "max"):
            buf, y = canary_y(V, 64)
            at.run(xs[(64, torch.float32)], y, 128, "balanced", reduce=red)
            out.append(buf)
        buf, y = canary_y(V, 64, BF)
        at.run(xs[(64, BF)], y, 128, "balanced")
        out.append(buf)
        b1, y = canary_y(V, 64)
        b2, t = canary_y(V, 32)
        at.run_with_nn_typed(xs[(64, torch.float32)], y, w32, t, "balanced")
        return out + [b1, b2]

    old = fresh()
    steps = []

    def check(step):
        steps.append(step)
        for F in (5, 128):
            got = multi(old, F)
            torch.cuda.synchronize()
            assert torch.equal(bits(got), bits(fresh_multi(F, state["val"]))), "after %s: run_multi at F = %d differs from a brand-new handle\n%s" % (
                step, F, "\n".join(steps))

    check("creation")
    for F, dt in ((1024, torch.float32), (5, torch.float32), (1024, BF), (602, torch.float32)):      # scratch grows, is reused, changes geometry
        multi(old, F, dt)
        check("run_multi at F = %d %s" % (F, dt))
    # the reverse direction: the older calls after the run_multi calls
    want = others(fresh())
    got = others(old)
    torch.cuda.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(bits(g), bits(w)), "run / run_with_nn_typed output %d after run_multi differs from a brand-new handle's" % i
    check("run (sum, max, bf16) and run_with_nn_typed, balanced")
    y = torch.empty((V, 64), device=DEV)
    for red in ("sum", "max"):
        old.run(xs[(64, torch.float32)], y, 128, 0, reduce=red)
    check("run, canonical rows")
    old.schedule(gnc.Schedule.neighbor_grouping, [16])
    check("schedule(neighbor_grouping, 16)")
    for red in ("sum", "max"):
        old.run(xs[(64, torch.float32)], y, 128, 1, reduce=red)
    check("run, scheduled")
    old.schedule(gnc.Schedule.locality, [3])
    check("schedule(locality, 3)")
    old.schedule_balanced(4)
    old.run(xs[(64, torch.float32)], y, 128, "balanced")
    check("schedule_balanced(4) and a balanced run")
    old.set_option("rows_blocked", 0)
    old.run(xs[(64, torch.float32)], y, 128, "balanced")
    check("set_option(rows_blocked, 0) and a balanced run")
    t = torch.empty((V, 32), device=DEV)
    old.run_with_nn_typed(xs[(64, torch.float32)], y, w32, t, "balanced", relu=True)
    check("run_with_nn_typed")
    if _lib.has_extras():                                            # (the backward entry points are not part of the shipped library)
        old.run_bwd(xs[(64, torch.float32)], y)
        check("run_bwd")
    state["val"] = "v2"
    old.updateval(vals["v2"])
    check("updateval")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        check("a side stream")
        multi(old, 1024, BF)
        check("run_multi at F = 1024 bf16 on the side stream")
    torch.cuda.current_stream().wait_stream(side)
    check("back on the first stream")
    old.close()
