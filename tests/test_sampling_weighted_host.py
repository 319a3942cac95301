"""CPU: the weighted sampling key and its restatement (tests/sampling_weighted_ref.py), the host sampler
gnnagg_sample_block_host_weighted against the restatement bit for bit, the distribution of the kept subsets against the exact
successive-sampling probabilities, and the surface (header, signatures, exports)."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

import sampling_ref as sr
import sampling_weighted_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn_computing_amd", "csrc")
PTR, IDX = sr.fixture_graph()


def test_known_answers():
    L = wr.log2_table()
    assert (int(L[0]), int(L[1]), int(L[128]), int(L[256])) == (0, 377457, 39256169, 67108864)
    assert [int(e) for e in wr.neg_log2_q26(np.array([0, 0x80000000, 0xFFFFFFFF], np.uint64))] == [2214592512, 67108864, 3]
    p = np.arange(4)
    assert [int(e) for e in wr.neg_log2_q26(sr.key(1, p))] == [152812522, 659169777, 92329303, 34480653]
    assert [int(k) for k in wr.wkey(1, p, np.float32(1.5))] == [0x4cc24fa9, 0x4dd18b60, 0x4c6ace39, 0x4baf60af]
    header = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    for word in ("377457", "39256169", "67108864", "2214592512", "0x4cc24fa9", "0x4dd18b60", "0x4c6ace39", "0x4baf60af", "152812522",
                 "659169777", "92329303", "34480653", "0xFFFFFFFF"):
        assert word in header, word


def test_eligibility_and_the_keys_at_the_ends_of_the_weight_range():
    w = np.array([np.inf, 1.0, 0.0, -0.0, -1.0, np.nan, -np.inf, 1e-45], np.float32)
    assert list(wr.eligible(w)) == [True, True, False, False, False, False, False, True]
    k = wr.wkey_of(np.uint64(0x80000000), w)                       # E = 2^26
    assert int(k[0]) == 0 and int(k[1]) == 0x4c800000 and all(int(x) == wr.INELIGIBLE for x in k[2:7])
    assert int(k[7]) == 0x7f800000                                 # 2^26 / denormal: +Inf, below the ineligible key
    assert int(wr.wkey_of(np.array([0xFFFFFFFF], np.uint64), np.array([3.4028235e38], np.float32))[0]) == 0x600000     # E = 3 over FLT_MAX: a denormal quotient (3 . 2^21 steps of 2^-149), kept, not flushed


def test_the_table_literals_of_sample_key_h_are_the_rounded_logarithms():
    text = open(os.path.join(CSRC, "sample_key.h")).read()
    body = re.search(r"kSampleLog2\[257\] = \{(.*?)\};", text, re.S).group(1)
    lits = [int(x) for x in re.findall(r"(\d+)u,", body)]
    assert len(lits) == 257 and np.array_equal(np.array(lits, np.int64), wr.log2_table())
    exact = np.log2(1.0 + np.arange(257) / 256.0) * float(1 << 26)
    assert np.abs(exact - np.floor(exact) - 0.5).min() > 0.0029    # no literal hangs on the last bits of a libm's log2


def test_neg_log2_is_within_2_to_the_minus_16_of_float64():
    rng = np.random.default_rng(7)
    u = np.concatenate([rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64),
                        np.array([0, 1, 2, 3, 255, 256, 257, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], np.uint64),
                        (np.uint64(1) << np.arange(32, dtype=np.uint64)), (np.uint64(1) << np.arange(1, 33, dtype=np.uint64)) - np.uint64(1)])
    got = wr.neg_log2_q26(u) / float(1 << 26)
    want = 32.0 - np.log2(u.astype(np.float64) + 0.5)
    err = float(np.abs(got - want).max())
    print("max |E / 2^26 - (-log2((u + 1/2) / 2^32))| = %.3g" % err)
    assert err < 2.0 ** -16
    assert (np.diff(wr.neg_log2_q26(np.sort(u))) <= 0).all()        # E decreases in u (weakly: it is quantised)


def check_block(blk, w, seeds, fanout, seed, relabel, eid):
    r_ptr, r_idx, r_eid, r_src, r_nsrc = wr.sample_block(PTR, IDX, w, seeds, fanout, seed, relabel)
    assert blk.num_dst == len(seeds) and blk.num_edges == int(r_ptr[-1]) and blk.num_src == r_nsrc
    assert np.asarray(blk.ptr).dtype == np.int32 and np.array_equal(blk.ptr, r_ptr)
    assert np.array_equal(blk.idx, r_idx)
    if relabel:
        assert np.array_equal(blk.src_nodes, r_src)
    else:
        assert blk.src_nodes is None
    if eid:
        assert np.array_equal(blk.eid, r_eid)
    else:
        assert blk.eid is None


@pytest.mark.parametrize("relabel,eid", [(True, True), (False, False)])
@pytest.mark.parametrize("fanout", sr.FANOUTS)
@pytest.mark.parametrize("variant", wr.VARIANTS)
def test_host_sampler_equals_the_restatement(variant, fanout, relabel, eid):
    w = wr.fixture_weights(variant)
    for name, seeds in sr.seed_lists().items():
        if name == "all_shuffled" and (variant != "mixed" or not relabel):
            continue   # (the largest list once per fanout)
        blk = gnc.sample_block_host(PTR, IDX, seeds, fanout, seed=5, relabel=relabel, return_eid=eid, prob=w)
        check_block(blk, w, seeds, fanout, 5, relabel, eid)


def test_fixture_weights_hold_what_the_tests_lean_on():
    base = wr.fixture_weights("mixed")
    assert base.dtype == np.float32 and base.size == IDX.size
    assert 0.25 < (base == 0).mean() < 0.35 and (base < 0).sum() >= 10 and np.isnan(base).sum() >= 10 and np.signbit(base[base == 0]).any()
    pos = base[(base > 1e-20) & (base < 1e20)]
    assert np.log2(pos.max() / pos.min()) > 11
    x = base[PTR[wr.EXTREME_ROW]:PTR[wr.EXTREME_ROW + 1]]
    assert set(x[:4].tolist()) == {float(v) for v in wr.EXTREME} and (x > 0).all() and x.min() < 1.1754944e-38
    deg = np.diff(PTR)
    assert [int(deg[r]) for r in wr.class_rows()] == wr.CLASS_DEGREES
    for variant, want in (("inf", None), ("zero", 0), ("three", 3)):
        w = wr.fixture_weights(variant)
        for r in wr.class_rows():
            row = w[PTR[r]:PTR[r + 1]]
            assert int(wr.eligible(row).sum()) == (deg[r] if want is None else want)
            assert want is not None or np.isposinf(row).all()
    # every class meets a real select in "mixed": more eligible edges than some fanout, fewer than the degree
    assert all(1 <= int(wr.eligible(base[PTR[r]:PTR[r + 1]]).sum()) < deg[r] for r in wr.class_rows())


@pytest.mark.parametrize("fanout", [1, 5, 64, 200])
def test_crafted_rows_inf_zero_three_and_all_eligible(fanout):
    seeds = np.array(wr.class_rows(), np.int32)
    deg = np.diff(PTR)
    inf = gnc.sample_block_host(PTR, IDX, seeds, fanout, seed=9, relabel=False, return_eid=True, prob=wr.fixture_weights("inf"))
    for i, r in enumerate(seeds):        # all keys tie at 0: the first `fanout` edges in CSR order
        assert np.array_equal(inf.eid[inf.ptr[i]:inf.ptr[i + 1]], PTR[r] + np.arange(min(fanout, deg[r])))
    zero = gnc.sample_block_host(PTR, IDX, seeds, fanout, seed=9, relabel=True, return_eid=True, prob=wr.fixture_weights("zero"))
    assert zero.num_edges == 0 and (zero.ptr == 0).all() and zero.num_src == len(seeds) and np.array_equal(zero.src_nodes, seeds)
    w3 = wr.fixture_weights("three")
    three = gnc.sample_block_host(PTR, IDX, seeds, fanout, seed=9, relabel=False, return_eid=True, prob=w3)
    for i, r in enumerate(seeds):
        elig = PTR[r] + np.flatnonzero(wr.eligible(w3[PTR[r]:PTR[r + 1]]))
        got = three.eid[three.ptr[i]:three.ptr[i + 1]]
        assert len(got) == min(3, fanout) and set(got.tolist()) <= set(elig.tolist())
        assert fanout < 3 or np.array_equal(got, elig)


def test_fanout_minus_one_keeps_exactly_the_eligible_edges():
    w = wr.fixture_weights("mixed")
    seeds = sr.seed_lists()["all_shuffled"]
    blk = gnc.sample_block_host(PTR, IDX, seeds, -1, seed=3, relabel=False, return_eid=True, prob=w)
    want = np.concatenate([PTR[r] + np.flatnonzero(wr.eligible(w[PTR[r]:PTR[r + 1]])) for r in seeds])
    assert np.array_equal(blk.eid, want) and wr.eligible(w[blk.eid]).all()
    x = gnc.sample_block_host(PTR, IDX, [wr.EXTREME_ROW], 2, seed=3, relabel=False, return_eid=True, prob=w)     # FLT_MIN ... FLT_MAX
    check_block(x, w, [wr.EXTREME_ROW], 2, 3, False, True)


def test_null_weights_are_the_unweighted_host_sampler():
    L = gnc.lib()
    seeds = sr.seed_lists()["crafted"]
    n, cap = len(seeds), 5 * len(seeds)

    def call(weighted):
        bp, bi, be, sn, cn = (np.full(m, -7, np.int32) for m in (n + 1, cap, cap, n + cap, 2))
        a = [PTR.ctypes.data, IDX.ctypes.data] + ([None] if weighted else []) + [len(PTR) - 1, seeds.ctypes.data, n, 5, 5, bp.ctypes.data,
                                                                               bi.ctypes.data, be.ctypes.data, cap, sn.ctypes.data, cn.ctypes.data]
        assert (L.gnnagg_sample_block_host_weighted if weighted else L.gnnagg_sample_block_host)(*a) == _lib.OK
        return bp, bi, be, sn, cn

    assert all(np.array_equal(x, y) for x, y in zip(call(True), call(False)))
    a = gnc.sample_block_host(PTR, IDX, seeds, 5, seed=5, return_eid=True, prob=None)
    r = sr.sample_block(PTR, IDX, seeds, 5, 5, True)
    assert np.array_equal(a.ptr, r[0]) and np.array_equal(a.idx, r[1]) and np.array_equal(a.eid, r[2]) and np.array_equal(a.src_nodes, r[3])


def test_host_sampler_refusals_and_capacity():
    L = gnc.lib()
    w = wr.fixture_weights("mixed")
    seeds = sr.seed_lists()["crafted"]
    n = len(seeds)
    want = wr.sample_block(PTR, IDX, w, seeds, 5, 5)[0]

    def call(fanout, cap, s=seeds, ns=None, null=()):
        room = min(max(cap, 0), 1 << 20)
        bp, bi, be = np.full(len(s) + 2, -7, np.int32), np.full(room + 4, -7, np.int32), np.full(room + 4, -7, np.int32)
        sn, cn = np.full(len(s) + room + 4, -7, np.int32), np.full(3, -7, np.int32)
        a = {"ptr": PTR.ctypes.data, "seeds": s.ctypes.data, "bp": bp.ctypes.data, "bi": bi.ctypes.data, "cn": cn.ctypes.data}
        for k in null:
            a[k] = None
        rc = L.gnnagg_sample_block_host_weighted(a["ptr"], IDX.ctypes.data, w.ctypes.data, len(PTR) - 1, a["seeds"], len(s) if ns is None else ns,
                                                 fanout, 5, a["bp"], a["bi"], be.ctypes.data, cap, sn.ctypes.data, a["cn"])
        return rc, bp, bi, be, sn, cn

    for kw in (dict(fanout=0, cap=10), dict(fanout=-2, cap=10), dict(fanout=5, cap=-1), dict(fanout=5, cap=10, ns=-1),
               dict(fanout=5, cap=(1 << 31) - n), dict(fanout=5, cap=80, null=("bp",)), dict(fanout=5, cap=80, null=("cn",)),
               dict(fanout=5, cap=80, null=("seeds",)), dict(fanout=5, cap=80, null=("bi",)), dict(fanout=5, cap=80, null=("ptr",))):
        assert call(**kw)[0] == _lib.ERR_ARG, kw
    assert call(5, 10, s=np.array([0, sr.NUM_V], np.int32))[0] == _lib.ERR_ARG and call(5, 10, s=np.array([-1], np.int32))[0] == _lib.ERR_ARG
    rc, bp, bi, be, sn, cn = call(5, int(want[-1]) - 1)            # too little room: blk_ptr and counts[0] say what was needed
    assert rc == _lib.OK and np.array_equal(bp[:-1], want) and cn[0] == want[-1] and bp[-1] == -7 and cn[2] == -7
    assert (bi == -7).all() and (be == -7).all() and (sn == -7).all()
    rc, bp, bi, be, sn, cn = call(5, int(want[-1]))                # exactly enough: canaries behind every buffer
    assert rc == _lib.OK and cn[0] == want[-1] and (bi[-4:] == -7).all() and (be[-4:] == -7).all() and (sn[-4:] == -7).all() and bp[-1] == -7
    with pytest.raises(ValueError):
        gnc.sample_block_host(PTR, IDX, seeds, 5, prob=w[:-1])


# ------------------------------------------------------------------------------------------------ distribution
def subset_probabilities(w, k):
    """{subset (sorted tuple): probability} of drawing k of the eligible edges one after the other, each in proportion to its weight
    among those left (what Efraimidis-Spirakis keys sample), enumerated over every order"""
    elig = [i for i, x in enumerate(w) if x > 0]
    prob = {}
    for order in itertools.permutations(elig, k):
        p, left = 1.0, float(sum(w[i] for i in elig))
        for i in order:
            p *= w[i] / left
            left -= w[i]
        key = tuple(sorted(order))
        prob[key] = prob.get(key, 0.0) + p
    return prob


def kept_subsets(w, k, seeds, p0):
    """the restatement's kept subset (local indices, sorted) of a row with weights w at positions p0 ..., one draw per seed"""
    w = np.asarray(w, np.float32)
    keys = wr.wkey(np.asarray(seeds, np.uint64)[:, None], p0 + np.arange(len(w))[None, :], w[None, :])
    order = np.argsort(keys, axis=1, kind="stable")[:, :k]
    return np.sort(order, axis=1)


# (weights, fanout, seeds, bins, the 1 - 1e-6 quantile of chi-square with bins - 1 degrees of freedom)
CASES = {
    "six_weights": ([1, 2, 3, 4, 5, 0.5], 2, 6000, 15, 54.6),
    "zeros_between": ([1, 0, 8, 2, 0, 4, 1], 3, 6000, 10, 44.8),
    "one_heavy": ([0.1, 10, 1, 1], 1, 6000, 4, 30.7),
    "eight_equal": ([1] * 8, 3, 5600, 56, 119.9),
}


@pytest.mark.parametrize("p0", [0, 123457])
@pytest.mark.parametrize("case", list(CASES))
def test_kept_subsets_follow_the_successive_sampling_probabilities(case, p0):
    w, k, n, bins, bound = CASES[case]
    prob = subset_probabilities(w, k)
    assert len(prob) == bins and abs(sum(prob.values()) - 1.0) < 1e-12 and min(prob.values()) * n >= 23
    kept = kept_subsets(w, k, np.arange(n), p0)
    counts = dict.fromkeys(prob, 0)
    for row in kept:
        counts[tuple(int(i) for i in row)] += 1                    # (a KeyError: a sample holds an ineligible edge)
    chi2 = sum((counts[s] - n * p) ** 2 / (n * p) for s, p in prob.items())
    print("chi2(%s, p0 = %d) = %.1f (bound %.1f)" % (case, p0, chi2, bound))
    assert chi2 < bound


@pytest.mark.parametrize("case", list(CASES))
def test_chi2_judge_agrees_with_the_host_sampler(case):
    """the counts above are the restatement's; the library draws the same subsets (one row at position 123457, 200 seeds)"""
    w, k, _, _, _ = CASES[case]
    p0, d = 123457, len(w)
    ptr = np.array([0, p0, p0 + d], np.int32)
    idx = np.arange(p0 + d, dtype=np.int32) % 2
    full = np.ones(p0 + d, np.float32)
    full[p0:] = w
    want = kept_subsets(w, k, np.arange(200), p0)
    for seed in range(200):
        blk = gnc.sample_block_host(ptr, idx, [1], k, seed=seed, relabel=False, return_eid=True, prob=full)
        assert np.array_equal(blk.eid, p0 + want[seed]), seed


# ------------------------------------------------------------------------------------------------ surface
DECLS = {
    "gnnagg_sampler_set_weights": (r"int gnnagg_sampler_set_weights\(gnnagg_sampler s, const float \*d_w\);", [ctypes.c_int64, ctypes.c_void_p]),
    "gnnagg_sample_block_host_weighted": (
        r"int gnnagg_sample_block_host_weighted\(const int \*h_ptr, const int \*h_idx, const float \*h_w, int num_v, const int \*h_seeds, "
        r"int num_seeds,\s+int fanout, unsigned long long seed, int \*h_blk_ptr, int \*h_blk_idx, int \*h_blk_eid,\s+long long cap_e, "
        r"int \*h_src_nodes, int \*h_counts\);",
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]),
}


def test_header_signatures_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, (decl, args) in DECLS.items():
        assert re.search(decl, text), name
        assert name in exported
        res, got = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and got == args
        assert getattr(gnc.lib(), name).argtypes == args
    import inspect
    assert "prob" in inspect.signature(gnc.NeighborSampler.__init__).parameters and callable(gnc.NeighborSampler.set_prob)
    assert "prob" in inspect.signature(gnc.sample_block_host).parameters


def test_host_and_device_share_one_weighted_key():
    key = open(os.path.join(CSRC, "sample_key.h")).read()
    assert "sample_wkey" in key and "__fdiv_rn" in key
    for f in ("sample.hip", "host_graph.cpp"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "sample_key.h"' in text and "sample_wkey" in text
        assert not re.search(r"\b(logf?|log2f?|expf?|exp2f?)\s*\(", text)           # no transcendental anywhere near a key


def test_set_weights_refuses_a_handle_that_is_no_sampler():
    L = gnc.lib()
    assert L.gnnagg_sampler_set_weights(0, None) == _lib.ERR_ARG and L.gnnagg_sampler_set_weights(12345, None) == _lib.ERR_ARG
