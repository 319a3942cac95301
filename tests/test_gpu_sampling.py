"""GPU: gnnagg_sampler_sample (csrc/sample.hip) on the fixture of tests/sampling_ref.py -- every output against the numpy restatement bit
for bit, the block's properties judged without it, canaries behind every buffer, the sampler's map restored between calls, streams,
unaligned outputs and every refusal.  The restatement of a (seed list, fanout, seed) is computed once and shared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

import sampling_ref as sr

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
def veteran():
    """ONE sampler for the whole module: every test that uses it also tests that the calls before it left the map unseen"""
    return gnc.NeighborSampler(*graph())


@functools.lru_cache(maxsize=None)
def ref(name, fanout, seed, relabel):
    return sr.sample_block(PTR, IDX, LISTS[name], fanout, seed, relabel)


def needed(seeds, fanout):
    d = DEG[np.asarray(seeds, np.int64)] if len(seeds) else np.zeros(0, np.int64)
    return int((d if fanout < 0 else np.minimum(d, fanout)).sum())


def raw(sampler, seeds, fanout, seed, cap, relabel=True, eid=True, shift=0, expect=_lib.OK):
    """the C call on canaried buffers; outputs begin `shift` ints into their allocation (1: 4-byte aligned, no more).  Returns host copies
    (blk_ptr, blk_idx, eid, src_nodes, counts), each WITH its PAD trailing canaries."""
    n = len(seeds)
    d_seeds = dev(np.asarray(seeds, np.int32)) if n else None
    mk = lambda m: torch.full((shift + m + PAD,), CANARY, dtype=torch.int32, device=DEV)
    bp, bi, be, sn, cn = mk(n + 1), mk(cap), mk(cap), mk(n + cap), mk(2)
    p = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * shift)
    L = gnc.lib()
    _lib.check(L.gnnagg_sampler_set_stream(sampler._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    rc = L.gnnagg_sampler_sample(sampler._h, ctypes.c_void_p(d_seeds.data_ptr()) if n else None, n, fanout, seed, p(bp), p(bi),
                                 p(be) if eid else None, cap, p(sn) if relabel else None, p(cn))
    assert rc == expect, (rc, L.gnnagg_last_error())
    torch.cuda.synchronize()
    outs = [t.cpu().numpy() for t in (bp, bi, be, sn, cn)]
    assert all((o[:shift] == CANARY).all() for o in outs)
    return [o[shift:] for o in outs]


def judge(outs, name, fanout, seed, relabel=True, eid=True, cap=None):
    """against the restatement, and the canaries behind every buffer"""
    seeds = LISTS[name]
    n = len(seeds)
    r_ptr, r_idx, r_eid, r_src, r_nsrc = ref(name, fanout, seed, relabel)
    total = int(r_ptr[-1])
    cap = total if cap is None else cap
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


def properties(outs, seeds, fanout):
    """what a block must satisfy, judged from the graph alone (relabelled, with eid)"""
    bp, bi, be, sn, cn = outs
    n = len(seeds)
    assert bp[0] == 0
    cnt = np.diff(bp[:n + 1])
    d = DEG[np.asarray(seeds, np.int64)] if n else np.zeros(0, np.int64)
    assert np.array_equal(cnt, d if fanout < 0 else np.minimum(d, fanout))
    total, nsrc = int(cn[0]), int(cn[1])
    assert total == bp[n] and n <= nsrc <= n + total
    src = sn[:nsrc]
    assert np.array_equal(src[:n], seeds)
    tail = src[n:]
    assert len(set(tail.tolist())) == len(tail) and not set(tail.tolist()) & set(np.asarray(seeds).tolist())   # distinct beyond the seeds
    for i, r in enumerate(seeds):
        e = be[bp[i]:bp[i + 1]]
        assert (np.diff(e) > 0).all() and (len(e) == 0 or (e[0] >= PTR[r] and e[-1] < PTR[r + 1]))
    li = bi[:total]
    assert total == 0 or (li.min() >= 0 and li.max() < nsrc)
    assert np.array_equal(IDX[be[:total]], src[li])
    # an edge to a duplicated seed goes to its first occurrence; every new row is numbered by its first appearance
    first = {}
    for j, v in enumerate(src.tolist()):
        first.setdefault(v, j)
    assert all(first[int(src[j])] == j for j in li.tolist())
    new = li[li >= n]
    assert np.array_equal(new[np.sort(np.unique(new, return_index=True)[1])], np.arange(n, nsrc))


@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("fanout", sr.FANOUTS)
def test_block_equals_the_restatement_and_has_its_properties(fanout, name):
    seeds = LISTS[name]
    cap = len(seeds) * fanout if fanout > 0 else needed(seeds, fanout)
    outs = raw(veteran(), seeds, fanout, 5, cap, shift=1)
    judge(outs, name, fanout, 5, cap=cap)
    properties(outs, seeds, fanout)
    judge(raw(veteran(), seeds, fanout, 5, cap, relabel=False, eid=False), name, fanout, 5, relabel=False, eid=False, cap=cap)


@pytest.mark.parametrize("fanout", [5, 65, -1])
def test_exact_capacity_unaligned_outputs_and_global_ids_with_eid(fanout):
    seeds = LISTS["crafted"]
    cap = needed(seeds, fanout)
    judge(raw(veteran(), seeds, fanout, 5, cap, shift=1), "crafted", fanout, 5, cap=cap)
    judge(raw(veteran(), seeds, fanout, 5, cap, relabel=False, shift=3), "crafted", fanout, 5, relabel=False, cap=cap)
    judge(raw(veteran(), seeds, fanout, 5, cap, eid=False, shift=1), "crafted", fanout, 5, eid=False, cap=cap)


@pytest.mark.parametrize("fanout", [5, 200, -1])
def test_capacity_too_small_says_what_was_needed_and_writes_nothing_past_it(fanout):
    seeds = LISTS["crafted"]
    n, total = len(seeds), needed(seeds, fanout)
    r_ptr = ref("crafted", fanout, 5, True)[0]
    for cap in (total - 1, total // 2, 0):
        bp, bi, be, sn, cn = raw(veteran(), seeds, fanout, 5, cap)
        assert np.array_equal(bp[:n + 1], r_ptr) and (bp[n + 1:] == CANARY).all()
        assert cn[0] == total and (cn[2:] == CANARY).all()
        assert (bi[cap:] == CANARY).all() and (be[cap:] == CANARY).all() and (sn[n + cap:] == CANARY).all()
    # the sampler's map came back unseen from the calls that ran out of room
    judge(raw(veteran(), seeds, fanout, 5, total), "crafted", fanout, 5)


def test_same_seed_same_bits_other_seed_other_sample_and_batch_independence():
    seeds = LISTS["crafted"]
    a = raw(veteran(), seeds, 5, 11, 5 * len(seeds))
    b = raw(veteran(), seeds, 5, 11, 5 * len(seeds))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = raw(veteran(), seeds, 5, 12, 5 * len(seeds))
    assert np.array_equal(a[0], c[0])
    rows_changed = [i for i in range(len(seeds)) if not np.array_equal(a[2][a[0][i]:a[0][i + 1]], c[2][c[0][i]:c[0][i + 1]])]
    assert rows_changed and all(DEG[seeds[i]] > 5 for i in rows_changed)
    hi = raw(veteran(), seeds, 5, (1 << 32) | 11, 5 * len(seeds))                       # the high word of the seed counts
    assert not np.array_equal(a[2][:a[4][0]], hi[2][:hi[4][0]])
    # a row's sample is the same in two different batches
    other = LISTS["all_shuffled"]
    o = raw(veteran(), other, 5, 11, 5 * len(other))
    where = {int(r): i for i, r in enumerate(other)}
    for i, r in enumerate(seeds):
        j = where[int(r)]
        assert np.array_equal(a[2][a[0][i]:a[0][i + 1]], o[2][o[0][j]:o[0][j + 1]]), r


def test_a_sampler_that_served_other_batches_equals_a_brand_new_one():
    old = veteran()
    for name, fanout in (("all_shuffled", -1), ("duplicates", 64), ("mutual", 5)):
        raw(old, LISTS[name], fanout, 3, needed(LISTS[name], fanout))
    for name, fanout in (("all_shuffled", 5), ("crafted", 200), ("duplicates", -1)):
        cap = needed(LISTS[name], fanout)
        new = gnc.NeighborSampler(*graph())
        a, b = raw(old, LISTS[name], fanout, 9, cap), raw(new, LISTS[name], fanout, 9, cap)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        judge(a, name, fanout, 9)
        new.close()
    # and the map itself: unseen everywhere (an edge that found a stale entry would not be a first appearance)
    seeds = np.arange(V, dtype=np.int32)[::-1].copy()
    outs = raw(old, seeds, 1, 9, V)
    properties(outs, seeds, 1)


def test_wrapper_on_a_side_stream_and_layers():
    ptr, idx = graph()
    s = veteran()
    side = torch.cuda.Stream()
    seeds = dev(LISTS["crafted"])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream != 0
        blk = s.sample(seeds, 5, seed=5, relabel=True, return_eid=True)
        glob = s.sample(seeds, 64, seed=5, relabel=False)
        blocks = s.sample_layers(seeds, fanouts=(5, 64), seed=5, return_eid=True)
    side.synchronize()
    r_ptr, r_idx, r_eid, r_src, r_nsrc = ref("crafted", 5, 5, True)
    assert (blk.num_dst, blk.num_src, blk.num_edges) == (len(LISTS["crafted"]), r_nsrc, int(r_ptr[-1]))
    assert np.array_equal(blk.ptr.cpu().numpy(), r_ptr) and np.array_equal(blk.idx.cpu().numpy(), r_idx)
    assert np.array_equal(blk.eid.cpu().numpy(), r_eid) and np.array_equal(blk.src_nodes.cpu().numpy(), r_src)
    g_ptr, g_idx, _, _, g_nsrc = ref("crafted", 64, 5, False)
    assert glob.src_nodes is None and glob.eid is None and glob.num_src == V == g_nsrc
    assert np.array_equal(glob.ptr.cpu().numpy(), g_ptr) and np.array_equal(glob.idx.cpu().numpy(), g_idx)
    # layers: input layer first; layer l uses seed + l and the src_nodes of the block above it as its seeds
    assert len(blocks) == 2 and blocks[1].num_dst == len(LISTS["crafted"]) and blocks[0].num_dst == blocks[1].num_src
    top = sr.sample_block(PTR, IDX, LISTS["crafted"], 64, 6, True)
    assert np.array_equal(blocks[1].idx.cpu().numpy(), top[1]) and np.array_equal(blocks[1].src_nodes.cpu().numpy(), top[3])
    low = sr.sample_block(PTR, IDX, top[3], 5, 5, True)
    assert np.array_equal(blocks[0].ptr.cpu().numpy(), low[0]) and np.array_equal(blocks[0].idx.cpu().numpy(), low[1])
    assert np.array_equal(blocks[0].eid.cpu().numpy(), low[2]) and np.array_equal(blocks[0].src_nodes.cpu().numpy(), low[3])
    empty = s.sample(dev(np.zeros(0, np.int32)), 5)
    assert (empty.num_dst, empty.num_src, empty.num_edges) == (0, 0, 0) and empty.ptr.tolist() == [0]


def test_every_refusal_leaves_the_sampler_as_it_was():
    s = veteran()
    L = gnc.lib()
    seeds = LISTS["crafted"]
    n = len(seeds)
    d_seeds = dev(seeds)
    buf = lambda m: torch.full((m,), CANARY, dtype=torch.int32, device=DEV)
    bp, bi, be, sn, cn = buf(n + 1), buf(5 * n), buf(5 * n), buf(6 * n), buf(2)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(h=s._h, seeds=P(d_seeds), n=n, fanout=5, cap=5 * n, bp=P(bp), bi=P(bi), be=P(be), sn=P(sn), cn=P(cn))
    bad = [dict(fanout=0), dict(fanout=-2), dict(n=-1), dict(cap=-1), dict(cap=(1 << 31) - n), dict(seeds=None), dict(bp=None), dict(bi=None),
           dict(cn=None), dict(h=ctypes.c_int64(0)), dict(h=ctypes.c_int64(12345))]
    for change in bad:
        a = dict(good, **change)
        rc = L.gnnagg_sampler_sample(a["h"], a["seeds"], a["n"], a["fanout"], 5, a["bp"], a["bi"], a["be"], a["cap"], a["sn"], a["cn"])
        assert rc == _lib.ERR_ARG and L.gnnagg_last_error(), change
    torch.cuda.synchronize()
    assert all((t == CANARY).all().item() for t in (bp, bi, be, sn, cn))
    assert L.gnnagg_sampler_set_stream(ctypes.c_int64(0), None) == _lib.ERR_ARG and L.gnnagg_sampler_destroy(ctypes.c_int64(0)) == _lib.ERR_ARG
    out = ctypes.c_int64(7)
    assert L.gnnagg_sampler_create(None, P(bi), V, E, ctypes.byref(out)) == _lib.ERR_ARG and out.value == 0
    assert L.gnnagg_sampler_create(P(bp), P(bi), -1, E, ctypes.byref(out)) == _lib.ERR_ARG
    assert L.gnnagg_sampler_create(P(bp), P(bi), V, E, None) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        s.sample(d_seeds, 0)
    with pytest.raises(TypeError):
        s.sample(d_seeds.long(), 5)
    judge(raw(s, seeds, 5, 5, 5 * n), "crafted", 5, 5, cap=5 * n)
    gone = gnc.NeighborSampler(*graph())
    h = ctypes.c_int64(gone._h.value)
    gone.close()
    assert L.gnnagg_sampler_sample(h, P(d_seeds), n, 5, 5, P(bp), P(bi), P(be), 5 * n, P(sn), P(cn)) == _lib.ERR_ARG


@pytest.mark.parametrize("fanout", [1100, 2000, 4999])
def test_hub_row_with_more_kept_edges_than_its_candidate_buffer_expects(fanout):
    """the 5 000-edge row buffers about 1 250 candidate keys for its select; a fanout above that count takes the walk that buffers nothing"""
    seeds = LISTS["crafted"]
    want = sr.sample_block(PTR, IDX, seeds, fanout, 5, True)
    cap = needed(seeds, fanout)
    bp, bi, be, sn, cn = raw(veteran(), seeds, fanout, 5, cap)
    n, total = len(seeds), int(want[0][-1])
    assert total == cap and np.array_equal(bp[:n + 1], want[0]) and list(cn[:2]) == [total, want[4]]
    assert np.array_equal(bi[:total], want[1]) and np.array_equal(be[:total], want[2]) and np.array_equal(sn[:want[4]], want[3])
    assert (bi[cap:] == CANARY).all() and (be[cap:] == CANARY).all() and (sn[n + cap:] == CANARY).all()
    properties((bp, bi, be, sn, cn), seeds, fanout)
