"""GPU: weighted neighbour sampling (gnnagg_sampler_set_weights + gnnagg_sampler_sample, csrc/sample.hip) on the fixture of
tests/sampling_ref.py with the weights of tests/sampling_weighted_ref.py -- every output against the numpy restatement bit for bit, in
every row class (8-lane copy, register select, wavefront histograms, the hub row on the workgroup) with +Inf ties, all-zero rows, rows
of 3 eligible edges and weights at the ends of float32; against the host twin; the handle's state across weight vectors; canaries,
capacities, a side stream, the refusals and one forward pass.  The restatement of a (weights, seed list, fanout, seed) is computed once."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

import sampling_ref as sr
import sampling_weighted_ref as wr

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PTR, IDX = sr.fixture_graph()
DEG = np.diff(PTR)
V, E = len(PTR) - 1, len(IDX)
LISTS = sr.seed_lists()
CANARY = -7
PAD = 8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def graph():
    return dev(PTR), dev(IDX)


@functools.lru_cache(maxsize=None)
def weights(variant):
    return dev(wr.fixture_weights(variant).copy())   # (the fixture is read-only; torch wants a writable array)


@functools.lru_cache(maxsize=None)
def veteran():
    """ONE sampler for the whole module, its weights changed from test to test: every test also tests what the calls before it left"""
    return gnc.NeighborSampler(*graph())


def armed(variant):
    s = veteran()
    s.set_prob(None if variant is None else weights(variant))
    return s


@functools.lru_cache(maxsize=None)
def ref(variant, name, fanout, seed, relabel):
    if variant is None:
        return sr.sample_block(PTR, IDX, LISTS[name], fanout, seed, relabel)
    return wr.sample_block(PTR, IDX, wr.fixture_weights(variant), LISTS[name], fanout, seed, relabel)


def room(seeds, fanout):
    """what the wrapper allocates: num_seeds * fanout, or the degree sum"""
    return len(seeds) * fanout if fanout > 0 else int(DEG[np.asarray(seeds, np.int64)].sum()) if len(seeds) else 0


def raw(sampler, seeds, fanout, seed, cap, relabel=True, eid=True, expect=_lib.OK):
    """the C call on canaried buffers: host copies (blk_ptr, blk_idx, eid, src_nodes, counts), each WITH its PAD trailing canaries"""
    n = len(seeds)
    d_seeds = dev(np.asarray(seeds, np.int32)) if n else None
    mk = lambda m: torch.full((m + PAD,), CANARY, dtype=torch.int32, device=DEV)
    bp, bi, be, sn, cn = mk(n + 1), mk(cap), mk(cap), mk(n + cap), mk(2)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = gnc.lib()
    _lib.check(L.gnnagg_sampler_set_stream(sampler._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    rc = L.gnnagg_sampler_sample(sampler._h, p(d_seeds) if n else None, n, fanout, seed, p(bp), p(bi), p(be) if eid else None, cap,
                                 p(sn) if relabel else None, p(cn))
    assert rc == expect, (rc, L.gnnagg_last_error())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (bp, bi, be, sn, cn)]


def judge(outs, want, n, cap, relabel=True, eid=True):
    """against a restatement's block, and the canaries behind every buffer"""
    r_ptr, r_idx, r_eid, r_src, r_nsrc = want
    total = int(r_ptr[-1])
    assert total <= cap
    bp, bi, be, sn, cn = outs
    assert np.array_equal(bp[:n + 1], r_ptr) and (bp[n + 1:] == CANARY).all()
    assert list(cn[:2]) == [total, r_nsrc] and (cn[2:] == CANARY).all()
    assert np.array_equal(bi[:total], r_idx) and (bi[cap:] == CANARY).all()
    if eid:
        assert np.array_equal(be[:total], r_eid) and (be[cap:] == CANARY).all()
    else:
        assert (be == CANARY).all()
    if relabel:
        assert np.array_equal(sn[:r_nsrc], r_src) and (sn[n + cap:] == CANARY).all()
    else:
        assert (sn == CANARY).all()


@pytest.mark.parametrize("fanout", sr.FANOUTS)
@pytest.mark.parametrize("variant", wr.VARIANTS)
def test_block_equals_the_restatement(variant, fanout):
    """every seed list (the crafted rows: every row class; "inf": ties in every class; "zero", "three": rows that keep nothing or 3)"""
    s = armed(variant)
    for name, seeds in LISTS.items():
        if name == "all_shuffled" and variant != "mixed":
            continue
        cap = room(seeds, fanout)
        judge(raw(s, seeds, fanout, 5, cap), ref(variant, name, fanout, 5, True), len(seeds), cap)
        if name in ("crafted", "duplicates"):
            judge(raw(s, seeds, fanout, 5, cap, relabel=False, eid=False), ref(variant, name, fanout, 5, False), len(seeds), cap, False, False)


@pytest.mark.parametrize("fanout", [1100, 2000, 3400, 4999])
@pytest.mark.parametrize("variant", ["mixed", "inf"])
def test_hub_row_at_large_fanouts(variant, fanout):
    """the 5 000-edge row on the workgroup: 3 502 eligible edges in "mixed" (4 999 keeps them all, through the select with k = d+),
    5 000 tied keys in "inf" (the quota of the tie rule summed over sixteen wavefronts and five rounds)"""
    s = armed(variant)
    seeds = LISTS["crafted"]
    cap = room(seeds, fanout)
    want = wr.sample_block(PTR, IDX, wr.fixture_weights(variant), seeds, fanout, 5, True)
    judge(raw(s, seeds, fanout, 5, cap), want, len(seeds), cap)


@pytest.mark.parametrize("variant", ["inf", "zero", "three"])
def test_crafted_rows_by_what_they_must_keep(variant):
    """judged from the weights alone: +Inf rows keep their first `fanout` edges, zero rows nothing, 3-eligible rows those 3"""
    s = armed(variant)
    w = wr.fixture_weights(variant)
    seeds = np.array(wr.class_rows(), np.int32)
    for fanout in (1, 5, 200, -1):
        cap = room(seeds, fanout)
        bp, bi, be, sn, cn = raw(s, seeds, fanout, 12, cap, relabel=False)
        for i, r in enumerate(seeds):
            got = be[bp[i]:bp[i + 1]]
            elig = PTR[r] + np.flatnonzero(wr.eligible(w[PTR[r]:PTR[r + 1]]))
            keep = len(elig) if fanout < 0 else min(len(elig), fanout)
            assert len(got) == keep and set(got.tolist()) <= set(elig.tolist()) and (np.diff(got) > 0).all()
            if variant == "inf" or keep == len(elig):
                assert np.array_equal(got, elig[:keep])
        assert (bi[cap:] == CANARY).all() and (be[cap:] == CANARY).all()


def test_extreme_weights_give_the_restatement_s_keys():
    """FLT_MIN, a denormal, FLT_MAX and 1e-30 in one row: a denormal weight is eligible, the FLT_MAX edges go first, the quotients that
    overflow tie at +Inf and go by position -- all as the restatement has them.  (A denormal QUOTIENT needs E < 4 over a weight near
    FLT_MAX, one key in 2^32: tests/test_sampling_weighted_host.py pins that value on the host.)"""
    s = armed("mixed")
    w = wr.fixture_weights("mixed")
    seeds = np.array([wr.EXTREME_ROW], np.int32)
    differ = 0
    for seed in range(24):
        for fanout in (1, 2, 3):
            want = wr.sample_block(PTR, IDX, w, seeds, fanout, seed, False)
            bp, bi, be, sn, cn = raw(s, seeds, fanout, seed, fanout, relabel=False)
            assert np.array_equal(be[:fanout], want[2]) and cn[0] == fanout, (seed, fanout)
        differ += not np.array_equal(want[2], PTR[wr.EXTREME_ROW] + np.arange(3))
    assert differ       # (the row has more than 3 edges and the weights decide)


@pytest.mark.parametrize("fanout", [5, 200, -1])
def test_device_block_equals_the_host_twin(fanout):
    s = armed("mixed")
    w = wr.fixture_weights("mixed")
    for name in ("crafted", "all_shuffled", "duplicates"):
        blk = s.sample(dev(LISTS[name]), fanout, seed=8, relabel=True, return_eid=True)
        host = gnc.sample_block_host(PTR, IDX, LISTS[name], fanout, seed=8, relabel=True, return_eid=True, prob=w)
        assert (blk.num_dst, blk.num_src, blk.num_edges) == (host.num_dst, host.num_src, host.num_edges)
        for a, b in ((blk.ptr, host.ptr), (blk.idx, host.idx), (blk.eid, host.eid), (blk.src_nodes, host.src_nodes)):
            assert np.array_equal(a.cpu().numpy(), b)


def test_handle_state_across_weight_vectors():
    s = armed("mixed")
    seeds = LISTS["crafted"]
    cap = room(seeds, 5)
    judge(raw(s, seeds, 5, 5, cap), ref("mixed", "crafted", 5, 5, True), len(seeds), cap)
    s.set_prob(None)                                               # uniform again: the unweighted restatement, bit for bit
    assert s.prob is None
    judge(raw(s, seeds, 5, 5, cap), ref(None, "crafted", 5, 5, True), len(seeds), cap)
    for name, fanout in (("all_shuffled", 5), ("crafted", 200), ("duplicates", -1)):
        c = room(LISTS[name], fanout)
        new = gnc.NeighborSampler(*graph())
        a, b = raw(s, LISTS[name], fanout, 9, c), raw(new, LISTS[name], fanout, 9, c)    # the map came back unseen from the weighted calls
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        new.close()
    s.set_prob(weights("three"))                                   # a second weight vector on the same sampler equals a brand-new sampler
    new = gnc.NeighborSampler(*graph(), prob=weights("three"))
    for name, fanout in (("crafted", 5), ("all_shuffled", 2), ("duplicates", -1)):
        c = room(LISTS[name], fanout)
        a, b = raw(s, LISTS[name], fanout, 9, c), raw(new, LISTS[name], fanout, 9, c)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        judge(a, wr.sample_block(PTR, IDX, wr.fixture_weights("three"), LISTS[name], fanout, 9, True), len(LISTS[name]), c)
    new.close()


def test_same_seed_same_bits_and_batch_independence():
    s = armed("mixed")
    seeds = LISTS["crafted"]
    a = raw(s, seeds, 5, 11, 5 * len(seeds))
    b = raw(s, seeds, 5, 11, 5 * len(seeds))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = raw(s, seeds, 5, 12, 5 * len(seeds))
    assert np.array_equal(a[0], c[0]) and not np.array_equal(a[2][:a[4][0]], c[2][:c[4][0]])
    other = LISTS["all_shuffled"]
    o = raw(s, other, 5, 11, 5 * len(other))
    where = {int(r): i for i, r in enumerate(other)}
    for i, r in enumerate(seeds):
        j = where[int(r)]
        assert np.array_equal(a[2][a[0][i]:a[0][i + 1]], o[2][o[0][j]:o[0][j + 1]]), r


@pytest.mark.parametrize("fanout", [5, 200, -1])
def test_exact_capacity_and_too_little_room(fanout):
    s = armed("mixed")
    seeds = LISTS["crafted"]
    n = len(seeds)
    want = ref("mixed", "crafted", fanout, 5, True)
    total = int(want[0][-1])
    assert total < room(seeds, fanout)                             # (the weights keep fewer edges than the unweighted bound)
    judge(raw(s, seeds, fanout, 5, total), want, n, total)         # canaries directly behind the last kept edge
    for cap in (total - 1, total // 2, 0):
        bp, bi, be, sn, cn = raw(s, seeds, fanout, 5, cap)
        assert np.array_equal(bp[:n + 1], want[0]) and (bp[n + 1:] == CANARY).all()
        assert cn[0] == total and (cn[2:] == CANARY).all()
        assert (bi[cap:] == CANARY).all() and (be[cap:] == CANARY).all() and (sn[n + cap:] == CANARY).all()
    judge(raw(s, seeds, fanout, 5, total), want, n, total)         # the map came back unseen from the calls that ran out of room


def test_wrapper_on_a_side_stream_and_layers():
    s = armed(None)
    side = torch.cuda.Stream()
    seeds = dev(LISTS["crafted"])
    w = wr.fixture_weights("mixed")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream != 0
        s.set_prob(weights("mixed"))
        blk = s.sample(seeds, 5, seed=5, relabel=True, return_eid=True)
        blocks = s.sample_layers(seeds, fanouts=(5, 64), seed=5, return_eid=True)
    side.synchronize()
    r_ptr, r_idx, r_eid, r_src, r_nsrc = ref("mixed", "crafted", 5, 5, True)
    assert (blk.num_dst, blk.num_src, blk.num_edges) == (len(LISTS["crafted"]), r_nsrc, int(r_ptr[-1]))
    assert np.array_equal(blk.ptr.cpu().numpy(), r_ptr) and np.array_equal(blk.idx.cpu().numpy(), r_idx)
    assert np.array_equal(blk.eid.cpu().numpy(), r_eid) and np.array_equal(blk.src_nodes.cpu().numpy(), r_src)
    top = wr.sample_block(PTR, IDX, w, LISTS["crafted"], 64, 6, True)
    low = wr.sample_block(PTR, IDX, w, top[3], 5, 5, True)
    assert np.array_equal(blocks[1].idx.cpu().numpy(), top[1]) and np.array_equal(blocks[1].src_nodes.cpu().numpy(), top[3])
    assert np.array_equal(blocks[0].ptr.cpu().numpy(), low[0]) and np.array_equal(blocks[0].idx.cpu().numpy(), low[1])
    assert np.array_equal(blocks[0].eid.cpu().numpy(), low[2]) and np.array_equal(blocks[0].src_nodes.cpu().numpy(), low[3])


def test_every_refusal_leaves_the_sampler_as_it_was():
    s = armed("mixed")
    L = gnc.lib()
    seeds = LISTS["crafted"]
    cap = room(seeds, 5)
    p = ctypes.c_void_p(weights("inf").data_ptr())
    assert L.gnnagg_sampler_set_weights(ctypes.c_int64(0), p) == _lib.ERR_ARG and L.gnnagg_last_error()
    assert L.gnnagg_sampler_set_weights(ctypes.c_int64(12345), p) == _lib.ERR_ARG
    gone = gnc.NeighborSampler(*graph())
    h = ctypes.c_int64(gone._h.value)
    gone.close()
    assert L.gnnagg_sampler_set_weights(h, p) == _lib.ERR_ARG and L.gnnagg_sampler_set_weights(h, None) == _lib.ERR_ARG
    with pytest.raises(TypeError):
        s.set_prob(weights("inf").double())
    with pytest.raises(ValueError):
        s.set_prob(weights("inf")[:-1])
    with pytest.raises(ValueError):
        s.set_prob(torch.from_numpy(wr.fixture_weights("inf").copy()))             # a host tensor
    with pytest.raises(ValueError):
        gnc.NeighborSampler(*graph(), prob=weights("inf")[:5])
    assert s.prob is weights("mixed")
    d_seeds = dev(seeds)
    bad = raw(s, seeds, 0, 5, cap, expect=_lib.ERR_ARG)                           # a refused sample keeps the weights too
    assert all((o == CANARY).all() for o in bad)
    with pytest.raises(ValueError):
        s.sample(d_seeds, 0)
    judge(raw(s, seeds, 5, 5, cap), ref("mixed", "crafted", 5, 5, True), len(seeds), cap)


def test_a_weighted_block_through_the_gcn_aggregation():
    """blk.eid gathers the per-edge values of the full graph; the sum over the block's CSR against the oracle's chain"""
    s = armed("mixed")
    F = 32
    x = np.random.default_rng(5).standard_normal((V, F)).astype(np.float32)
    val = np.random.default_rng(6).standard_normal(E).astype(np.float32)
    seeds = np.concatenate([sr.crafted_rows(), np.random.default_rng(4).choice(V, 200, replace=False)]).astype(np.int32)
    blk = s.sample(dev(seeds), 5, seed=3, relabel=True, return_eid=True)
    want = wr.sample_block(PTR, IDX, wr.fixture_weights("mixed"), seeds, 5, 3, True)
    b_ptr, b_idx, b_eid, b_src = (t.cpu().numpy() for t in (blk.ptr, blk.idx, blk.eid, blk.src_nodes))
    assert np.array_equal(b_ptr, want[0]) and np.array_equal(b_idx, want[1]) and np.array_equal(b_eid, want[2]) and np.array_equal(b_src, want[3])
    assert wr.eligible(wr.fixture_weights("mixed")[b_eid]).all()
    d_val = dev(val)[blk.eid.long()].contiguous()
    agg = blk.gcn(d_val)
    y = torch.full((blk.num_dst, F), 7.0, device=DEV)
    agg.run(dev(x[b_src]), y, 512, 0, reduce="sum")
    torch.cuda.synchronize()
    agg.close()
    y_orc = orc.gcn_seq(b_ptr, b_idx, val[b_eid], x[b_src])
    scale = orc.gcn_abs_scale(b_ptr, b_idx, val[b_eid], x[b_src])
    err = np.abs(y.cpu().numpy().astype(np.float64) - y_orc.astype(np.float64))
    print("worst |y - oracle| / (1e-5 * scale) = %.4f" % float((err / (1e-5 * scale.astype(np.float64) + 1e-30)).max()))
    assert (err <= 1e-5 * scale.astype(np.float64) + 1e-30).all()
