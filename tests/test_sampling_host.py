"""CPU: the sampling key and its restatement (tests/sampling_ref.py), the host sampler gnnagg_sample_block_host against the restatement,
bit for bit, and the surface (header, signatures, exports, refusals without a GPU)."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

import sampling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn_computing_amd", "csrc")
CHI2_55_Q = 119.9      # the 1 - 1e-6 quantile of chi-square with 55 degrees of freedom


def test_known_answers():
    assert int(sr.seed_mix(0)) == 0xaa3e5b61 and int(sr.seed_mix(1)) == 0x70f6c6d8
    assert [int(k) for k in sr.key(1, np.arange(4))] == [0x34d106be, 0x00486268, 0x62a55a72, 0xb34bc796]
    header = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    for word in ("0xaa3e5b61", "0x70f6c6d8", "0x34d106be", "0x00486268", "0x62a55a72", "0xb34bc796", "0x85EBCA6B", "0xC2B2AE35", "0x9E3779B9"):
        assert word in header, word


@pytest.mark.parametrize("seed", [0, 1, (12345 << 32) | 7])
def test_key_is_injective_on_the_first_2_20_positions(seed):
    k = sr.key(seed, np.arange(1 << 20))
    assert k.max() <= 0xFFFFFFFF and np.unique(k).size == 1 << 20


def _chi2(seeds, p0):
    """chi-square of the 56 subset counts: a row of 8 edges beginning at p0, fanout 3, one draw per seed"""
    keys = sr.key(np.asarray(seeds, np.uint64)[:, None], p0 + np.arange(8)[None, :])
    kept = np.sort(np.argsort(keys, axis=1, kind="stable")[:, :3], axis=1)
    code = kept[:, 0] * 64 + kept[:, 1] * 8 + kept[:, 2]
    subsets = [a * 64 + b * 8 + c for a, b, c in itertools.combinations(range(8), 3)]
    counts = np.array([(code == s).sum() for s in subsets], np.float64)
    assert counts.sum() == len(seeds) and len(subsets) == 56
    e = len(seeds) / 56.0
    return float(((counts - e) ** 2 / e).sum())


@pytest.mark.parametrize("p0,high", [(0, False), (1000, False), (123457, False), (1000, True)])
def test_subsets_of_a_row_are_uniform(p0, high):
    seeds = [(s << 32) | 7 for s in range(5600)] if high else list(range(5600))
    x = _chi2(seeds, p0)
    print("chi2(p0 = %d, high-word seeds %s) = %.1f" % (p0, high, x))
    assert x < CHI2_55_Q


def test_chi2_judge_agrees_with_the_host_sampler():
    """the counts above are the restatement's; the library draws the same subsets (one row, 200 seeds)"""
    ptr = np.array([0, 1000, 1008], np.int32)
    idx = np.arange(1008, dtype=np.int32) % 2
    for seed in range(200):
        blk = gnc.sample_block_host(ptr, idx, [1], 3, seed=seed, relabel=False, return_eid=True)
        want = np.sort(1000 + np.argsort(sr.key(seed, 1000 + np.arange(8)), kind="stable")[:3])
        assert np.array_equal(blk.eid, want), seed


def test_fixture_has_the_crafted_rows_and_the_seed_lists_their_properties():
    ptr, idx = sr.fixture_graph()
    deg = np.diff(ptr)
    assert len(deg) == sr.NUM_V == 2000 and [int(deg[r]) for r in sr.crafted_rows()] == sr.CRAFTED
    assert idx.min() >= 0 and idx.max() < sr.NUM_V
    assert any(r in idx[ptr[r]:ptr[r + 1]] for r in range(sr.NUM_V))                                         # self-loops
    assert any(len(set(idx[ptr[r]:ptr[r + 1]])) < deg[r] for r in range(sr.NUM_V))                           # multi-edges
    lists = sr.seed_lists()
    assert set(lists) == {"empty", "one", "crafted", "all_shuffled", "duplicates", "mutual"}
    assert lists["empty"].size == 0 and lists["one"].size == 1 and sorted(lists["all_shuffled"]) == list(range(sr.NUM_V))
    assert len(set(lists["duplicates"])) < len(lists["duplicates"])
    m = lists["mutual"]
    assert len(set(m)) >= 3
    hub = int(m[0])
    assert all(hub in idx[ptr[v]:ptr[v + 1]] and v in idx[ptr[hub]:ptr[hub + 1]] for v in m[1:-1])


def check_block_against_restatement(blk, ptr, idx, seeds, fanout, seed, relabel, eid):
    """every output of a Block equal to the restatement, bit for bit"""
    r_ptr, r_idx, r_eid, r_src, r_nsrc = sr.sample_block(ptr, idx, seeds, fanout, seed, relabel)
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


@pytest.mark.parametrize("relabel,eid", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("fanout", sr.FANOUTS)
def test_host_sampler_equals_the_restatement(fanout, relabel, eid):
    ptr, idx = sr.fixture_graph()
    for name, seeds in sr.seed_lists().items():
        if name == "all_shuffled" and not (relabel and eid):
            continue   # (the largest list once per fanout)
        blk = gnc.sample_block_host(ptr, idx, seeds, fanout, seed=5, relabel=relabel, return_eid=eid)
        check_block_against_restatement(blk, ptr, idx, seeds, fanout, 5, relabel, eid)


def test_host_sampler_seed_words_and_batch_independence():
    ptr, idx = sr.fixture_graph()
    row = sr.crafted_rows()[9]     # 128 edges
    a = gnc.sample_block_host(ptr, idx, [row], 5, seed=(3 << 32) | 1, relabel=False, return_eid=True)
    b = gnc.sample_block_host(ptr, idx, [7, row, 9], 5, seed=(3 << 32) | 1, relabel=False, return_eid=True)
    c = gnc.sample_block_host(ptr, idx, [row], 5, seed=1, relabel=False, return_eid=True)
    assert np.array_equal(a.eid, b.eid[b.ptr[1]:b.ptr[2]]) and not np.array_equal(a.eid, c.eid)
    check_block_against_restatement(a, ptr, idx, [row], 5, (3 << 32) | 1, False, True)


def _host_call(ptr, idx, seeds, fanout, cap, n=None, null=()):
    L = gnc.lib()
    seeds = np.asarray(seeds, np.int32)
    n = len(seeds) if n is None else n
    room = min(max(cap, 0), 1 << 20)     # (a call with more is one that is refused before it touches anything)
    bp, bi, be = np.full(len(seeds) + 2, -7, np.int32), np.full(room + 4, -7, np.int32), np.full(room + 4, -7, np.int32)
    sn, cn = np.full(len(seeds) + room + 4, -7, np.int32), np.full(3, -7, np.int32)
    a = {"ptr": ptr.ctypes.data, "idx": idx.ctypes.data, "seeds": seeds.ctypes.data, "bp": bp.ctypes.data, "bi": bi.ctypes.data,
         "be": be.ctypes.data, "sn": sn.ctypes.data, "cn": cn.ctypes.data}
    for k in null:
        a[k] = None
    rc = L.gnnagg_sample_block_host(a["ptr"], a["idx"], len(ptr) - 1, a["seeds"], n, fanout, 5, a["bp"], a["bi"], a["be"], cap, a["sn"], a["cn"])
    return rc, bp, bi, be, sn, cn


def test_host_sampler_refusals_and_capacity():
    ptr, idx = sr.fixture_graph()
    seeds = sr.seed_lists()["crafted"]
    for kw in (dict(fanout=0, cap=10), dict(fanout=-2, cap=10), dict(fanout=5, cap=-1), dict(fanout=5, cap=10, n=-1),
               dict(fanout=5, cap=(1 << 31) - len(seeds)), dict(fanout=5, cap=80, null=("bp",)), dict(fanout=5, cap=80, null=("cn",)),
               dict(fanout=5, cap=80, null=("seeds",)), dict(fanout=5, cap=80, null=("bi",)), dict(fanout=5, cap=80, null=("ptr",))):
        rc = _host_call(ptr, idx, seeds, **kw)[0]
        assert rc == _lib.ERR_ARG, kw
    assert _host_call(ptr, idx, [0, sr.NUM_V], 5, 10)[0] == _lib.ERR_ARG and _host_call(ptr, idx, [-1], 5, 10)[0] == _lib.ERR_ARG
    # a capacity that is too small: blk_ptr and counts[0] complete, nothing written past any capacity
    want = sr.sample_block(ptr, idx, seeds, 5, 5)[0]
    rc, bp, bi, be, sn, cn = _host_call(ptr, idx, seeds, 5, int(want[-1]) - 1)
    assert rc == _lib.OK and np.array_equal(bp[:-1], want) and cn[0] == want[-1] and bp[-1] == -7 and cn[2] == -7
    assert (bi[-4:] == -7).all() and (be[-4:] == -7).all() and (sn[-4:] == -7).all()
    # exactly enough: canaries behind every buffer
    rc, bp, bi, be, sn, cn = _host_call(ptr, idx, seeds, 5, int(want[-1]))
    assert rc == _lib.OK and cn[0] == want[-1] and (bi[-4:] == -7).all() and (be[-4:] == -7).all() and (sn[-4:] == -7).all() and bp[-1] == -7
    # no seeds: blk_ptr[0] = 0 and the counts
    rc, bp, bi, be, sn, cn = _host_call(ptr, idx, [], 5, 0)
    assert rc == _lib.OK and bp[0] == 0 and bp[1] == -7 and list(cn) == [0, 0, -7]
    with pytest.raises(ValueError):
        gnc.sample_block_host(ptr, idx, seeds, 0)


DECLS = {
    "gnnagg_sampler_create": (r"int gnnagg_sampler_create\(const int \*d_ptr, const int \*d_idx, int num_v, int num_e, gnnagg_sampler \*out\);",
                              [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    "gnnagg_sampler_destroy": (r"int gnnagg_sampler_destroy\(gnnagg_sampler s\);", [ctypes.c_int64]),
    "gnnagg_sampler_set_stream": (r"int gnnagg_sampler_set_stream\(gnnagg_sampler s, void \*hip_stream\);", [ctypes.c_int64, ctypes.c_void_p]),
    "gnnagg_sampler_sample": (r"int gnnagg_sampler_sample\(gnnagg_sampler s, const int \*d_seeds, int num_seeds, int fanout, unsigned long long seed,\s+"
                              r"int \*d_blk_ptr, int \*d_blk_idx, int \*d_blk_eid, long long cap_e, int \*d_src_nodes, int \*d_counts\);",
                              [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]),
    "gnnagg_sample_block_host": (r"int gnnagg_sample_block_host\(const int \*h_ptr, const int \*h_idx, int num_v, const int \*h_seeds, int num_seeds, "
                                 r"int fanout,\s+unsigned long long seed, int \*h_blk_ptr, int \*h_blk_idx, int \*h_blk_eid, long long cap_e,\s+"
                                 r"int \*h_src_nodes, int \*h_counts\);",
                                 [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]),
}


def test_header_signatures_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"^typedef int64_t gnnagg_sampler;", text, re.M)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, (decl, args) in DECLS.items():
        assert re.search(decl, text), name
        assert name in exported
        res, got = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and got == args
        assert getattr(gnc.lib(), name).argtypes == args
    kfiles = re.search(r"^KFILES := (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "sample" in kfiles and os.path.exists(os.path.join(CSRC, "sample.hip"))
    assert callable(gnc.NeighborSampler) and callable(gnc.sample_block_host) and gnc.Block._fields == (
        "ptr", "idx", "src_nodes", "eid", "num_dst", "num_src", "num_edges")


def test_host_and_device_share_one_key():
    """one text of the key for sample.hip and host_graph.cpp"""
    for f in ("sample.hip", "host_graph.cpp"):
        assert '#include "sample_key.h"' in open(os.path.join(CSRC, f)).read()
    key = open(os.path.join(CSRC, "sample_key.h")).read()
    assert "0x85EBCA6Bu" in key and "0xC2B2AE35u" in key and "0x9E3779B9u" in key


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_device_entry_points_refuse_without_a_gpu():
    L = gnc.lib()
    ptr, idx = sr.fixture_graph()
    h = ctypes.c_int64(0)
    assert L.gnnagg_sampler_create(ptr.ctypes.data, idx.ctypes.data, sr.NUM_V, len(idx), ctypes.byref(h)) == _lib.ERR_HIP and h.value == 0
    assert b"no HIP device" in L.gnnagg_last_error()
    assert L.gnnagg_sampler_sample(0, None, 0, 5, 0, None, None, None, 0, None, None) == _lib.ERR_ARG
    assert L.gnnagg_sampler_set_stream(0, None) == _lib.ERR_ARG and L.gnnagg_sampler_destroy(0) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        gnc.NeighborSampler(torch.from_numpy(ptr), torch.from_numpy(idx))   # host tensors are refused
