"""GPU half of the plan-builder census (tests/plan_census.py): the device plan builder (csrc/plan_gpu.hip on csrc/prims.cuh) at every size
where one of its scans, its reduction, one of its sorts or a guard in front of it changes passes or sides.

tests/test_gpu_blocked.py reaches the builder through one graph shape (64 ragged tiles, one-pass range sort, two-pass row sort, three-pass
length sort, a first row with edges).  Here every entry of the census tables runs, and tests/test_plan_census_host.py proves on the CPU
that each sits on the side it claims.

Balanced order: the conditions of build_partitioned_gpu asserted in Python, then the schedule the handle reports against the numpy
restatement (and the oracle's, where its O(P * E) loop is affordable) before and after the first run, and the run itself bit-equal to
the oracle's grouped fold of that schedule -- which is what sees the arrays that never leave the device (the flag bits of the ids, the
row -> groups lists, the edge permutation behind val_s).  Chain plan: the canonical CSR-order chain, bit for bit, with the scratch of the
chained path as the witness that the row kernels did not run instead.

Every comparison of a GCN handle is exact.  The GAT handles (one entry per group) are judged as
test_gpu_blocked.py::test_blocked_gat_and_newval_in_csr_edge_order judges: the schedule exactly, the output inside the 1e-5
condition-aware bound (expf on the device against libm), the weights in CSR edge order."""
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from oracle import oracle as orc
from test_gpu_parity import DEV, assert_within, dev, rand

import plan_census as pc

pytestmark = pytest.mark.gpu

BAL = {e["name"]: e for e in pc.BALANCED}
CHN = {e["name"]: e for e in pc.CHAIN}
ORACLE_LIMIT = 5e8          # P * E up to which the oracle's own scheduler restates the order beside the numpy one


@functools.lru_cache(maxsize=None)
def graph(name):
    return pc.graph_of(BAL.get(name) or CHN[name])      # (shared between the tests of an entry: nothing writes to it)


def x_rows(entry):
    return max(entry["V"], entry["cols"])      # X is gathered by column id, the attention terms by row id too


def restated(entry, ptr, idx, ng, val):
    P = pc.clamped_ranges(entry["P"], entry["cols"])
    mine = pc.blocked_order(ptr, idx, P, entry["cols"], ng, val)
    if P * entry["E"] <= ORACLE_LIMIT:
        theirs = orc.locality_schedule(ptr, idx, P, entry["cols"], ng, val)
        assert all(np.array_equal(a, b) for a, b in zip(mine[:3], theirs[:3]))
        assert val is None or np.array_equal(mine[3], theirs[3])
    return mine


def assert_device_conditions(entry, idx):
    """build_partitioned_gpu's conditions; an entry marked host-side fails exactly the one it names"""
    k, E, P = pc.K, entry["E"], entry["P"]
    free = torch.cuda.mem_get_info()[0]
    conds = {"memory": k["blocked_bytes_per_edge"] * E <= free // k["free_divisor"],
             "range_guard": pc.clamped_ranges(P, int(idx.max()) + 1) <= k["range_guard"],
             "id_guard": int(idx.max()) <= k["id_guard"]}
    assert k["blocked_bytes_per_edge"] == 72 and k["range_guard"] == 65535 and k["id_guard"] == 0x3fffffff
    for what, holds in conds.items():
        assert holds == (what != entry.get("host")), what
    assert pc.device_built(E, P, int(idx.max()), free) == ("host" not in entry)


def balanced_handle(entry, ptr, idx, val, F, **opts):
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    agg.set_option("partitions", entry["P"])
    for name, value in opts.items():      # ("host_plan" goes last: every option that replans returns the handle to the device builder)
        agg.set_option(name, value)
    return agg


def assert_builder(agg, ps, tg, V, device):
    """Which builder made the plan: the device builder keeps exactly the arrays of plan_census.blocked_plan_bytes (a wrong span cut or
    a wrong count of rows with several / without groups changes the figure), the host builder the permuted ids and the descriptors too."""
    kept = agg.plan_info()["plan_bytes"]
    want = pc.blocked_plan_bytes(ps, tg, V)
    assert kept == want if device else kept >= want + 4 * int(ps[-1]), (kept, want)


def run_balanced(entry, agg, ptr, idx, val, x, host_plan=False):
    """every assertion of the balanced order on one handle; returns (schedule, y) for the second tier's comparison"""
    V, cols, F = entry["V"], entry["cols"], x.shape[1]
    assert agg.balanced_partitions() == min(entry["P"], cols)
    assert agg.balanced_partition_columns() == int(idx.max()) + 1 == cols
    ng, seg = agg.balanced_params()
    assert ng >= 1 and seg == 0
    ps, ix, tg, vs = restated(entry, ptr, idx, ng, val)
    before = agg.get_schedule("balanced", with_val=True)
    for a, b in zip(before, (ps, ix, tg, vs)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert_builder(agg, ps, tg, V, device=("host" not in entry and not host_plan))
    y = torch.full((V, F), 7.0, device=DEV)
    agg.run(dev(x), y, 128, "balanced")
    out = y.cpu().numpy()
    assert np.array_equal(out, orc.gcn_grouped(ps, tg, ix, vs, x, V, seg=0))
    assert not np.any(out[np.diff(ptr) == 0].view(np.uint32)), "rows without edges are +0"
    after = agg.get_schedule("balanced", with_val=True)      # (a run that needs descriptors has the host builder make the plan again)
    assert all(np.array_equal(a, b) for a, b in zip(after, before))
    assert agg.balanced_partitions() == min(entry["P"], cols) and agg.balanced_params() == (ng, 0)
    return before, out


@pytest.mark.parametrize("name", list(BAL))
def test_balanced_order(name):
    entry = BAL[name]
    ptr, idx = graph(name)
    F = entry.get("F", 64)
    val, x = rand(entry["E"], 2), rand((x_rows(entry), F), 1)
    assert_device_conditions(entry, idx)
    run_balanced(entry, balanced_handle(entry, ptr, idx, val, F), ptr, idx, val, x)


@pytest.mark.skipif(not _lib.has_extras(), reason="second tier: \"host_plan\" is an option of libgnnagg_extras.so only")
@pytest.mark.parametrize("name", list(BAL))
def test_balanced_order_equals_the_host_builders(name):
    entry = BAL[name]
    ptr, idx = graph(name)
    F = entry.get("F", 64)
    val, x = rand(entry["E"], 2), rand((x_rows(entry), F), 1)
    sched_d, y_d = run_balanced(entry, balanced_handle(entry, ptr, idx, val, F), ptr, idx, val, x)
    sched_h, y_h = run_balanced(entry, balanced_handle(entry, ptr, idx, val, F, host_plan=1), ptr, idx, val, x, host_plan=True)
    assert all(np.array_equal(a, b) for a, b in zip(sched_d, sched_h))
    assert np.array_equal(y_d.view(np.uint32), y_h.view(np.uint32))


def gat_scale_rows(ptr, idx, att, x):
    """test_gpu_parity.gat_scale for one head (sum_e w_e |x_e| with the normalised weights), row block by row block: the census graphs
    reach a million edges"""
    w = orc.gat_att(ptr, idx, att, 1, 0.2)
    V = len(ptr) - 1
    s = np.zeros((V, x.shape[1]))
    for r0 in range(0, V, 256):
        r1 = min(V, r0 + 256)
        e0, e1 = int(ptr[r0]), int(ptr[r1])
        live = np.nonzero(np.diff(ptr[r0:r1 + 1]) > 0)[0]
        if e1 > e0:
            prod = w[e0:e1].astype(np.float64) * np.abs(x[idx[e0:e1]])
            s[r0 + live] = np.add.reduceat(prod, ptr[r0 + live] - e0, axis=0)
    return s.astype(np.float32)


@pytest.mark.parametrize("name", [n for n, e in BAL.items() if e.get("gat")])
def test_balanced_order_gat(name):
    entry = BAL[name]
    ptr, idx = graph(name)
    V, E, cols, F, H = entry["V"], entry["E"], entry["cols"], 64, 1
    x, att = rand((x_rows(entry), F), 1), rand((x_rows(entry), H, 2), 2) * 0.4
    assert_device_conditions(entry, idx)
    gat = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    gat.set_option("partitions", entry["P"])
    assert gat.balanced_partitions() == min(entry["P"], cols) and gat.balanced_partition_columns() == cols
    ng = gat.balanced_params()[0]
    ops, oix, otg, _ = restated(entry, ptr, idx, ng, None)
    for a, b in zip(gat.get_schedule("balanced"), (ops, oix, otg)):
        assert np.array_equal(a, b)
    assert_builder(gat, ops, otg, V, device=True)
    y = torch.full((V, F), 7.0, device=DEV)
    newval = torch.full((E, H), 7.0, device=DEV)
    gat.run(dev(x), dev(att), y, 128, "balanced", heads=H, newval=newval)
    for a, b in zip(gat.get_schedule("balanced"), (ops, oix, otg)):
        assert np.array_equal(a, b)
    ref, _, _ = orc.gat_grouped(ops, otg, oix, att, x, V, H, seg=0)
    assert_within(y.cpu().numpy(), ref, gat_scale_rows(ptr, idx, att, x) + np.abs(ref), "census gat %s" % name)
    assert np.all(y.cpu().numpy()[np.diff(ptr) == 0] == 0)
    _, ref_newval, _ = orc.gat_grouped(*orc.neighbor_grouping(ptr, 1 << 30), idx, att, x, V, H, seg=0)
    np.testing.assert_allclose(newval.cpu().numpy(), ref_newval, rtol=1e-6)
    nv_rows = torch.full((E, H), 7.0, device=DEV)
    gat.run(dev(x), dev(att), y, 128, "rows", heads=H, newval=nv_rows)
    assert torch.equal(newval, nv_rows)


@pytest.mark.parametrize("name", list(CHN))
def test_chain_plan(name):
    entry = CHN[name]
    ptr, idx = graph(name)
    V, E, cols, P, F = entry["V"], entry["E"], entry["cols"], entry["P"], entry.get("F", 64)
    val, x = rand(E, 2), rand((x_rows(entry), F), 1)
    k = pc.K
    free = torch.cuda.mem_get_info()[0]
    assert k["chain_bytes_per_edge"] == 80 and 80 * E <= free // 2
    assert int(idx.max()) + 1 == cols < 2 ** 24 and 2 <= P <= 65535
    assert pc.chain_device_built(E, P, int(idx.max()), free)
    want = entry["claims"]["ranges"]
    assert want in (0, min(P, cols))

    def handle(**opts):
        h = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
        h.set_option("fast_rows", 0)
        h.set_option("partitions", P)
        h.set_option("rows_hub_edges", entry["hub"])
        for o, v in opts.items():
            h.set_option(o, v)
        return h

    a, b = handle(), handle(rows_blocked=0)
    assert a.rows_blocked_ranges() == want and b.rows_blocked_ranges() == 0
    if want:   # the device builder's arrays and nothing else (the host builder keeps the permuted ids of every group as well)
        assert a.plan_info()["plan_bytes"] == pc.chain_plan_bytes(ptr, idx, min(P, cols), cols, entry["hub"])
    empty = np.diff(ptr) == 0
    y, y2 = torch.full((V, F), 7.0, device=DEV), torch.full((V, F), 7.0, device=DEV)
    for kw, ref in (({}, orc.gcn_seq(ptr, idx, val, x)), ({"reduce": "mean"}, orc.gcn_mean(ptr, idx, val, x))):
        y.fill_(7.0)
        y2.fill_(7.0)
        a.run(dev(x), y, 128, 0, **kw)
        b.run(dev(x), y2, 128, 0, **kw)
        out = y.cpu().numpy()
        assert np.array_equal(out, ref), kw
        assert not np.any(out[empty].view(np.uint32)), "rows without edges are +0"
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), kw
        assert a.rows_blocked_ranges() == want
        if want:   # the chained path reserved its image of Y: the row kernels would pass everything above as well
            assert a.plan_info()["scratch_bytes"] >= V * 64 * ((F + 63) // 64) * 4
