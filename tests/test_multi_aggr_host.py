"""CPU: the judges of the multi-aggregation call (gnnagg_gcn_run_multi, csrc/agg_multi.hip) and what tests/test_gpu_multi_aggr.py imports.

* the fixture: one small graph whose row lengths stand on every edge of the walk (batch, window, short / long, one segment / two / three);
* multi_ref: the float64 reference of the six aggregates over the fp32 messages m = val * x[idx], with the terms of the error bounds;
* multi_chain32: the numpy float32 restatement of the kernel's short-row chains (s = s + m in CSR order; mean = s / d);
* multi_layout: the scaler-major block layout of y;
* multi_geometry / multi_case: the lane-geometry picker and the key of the dispatch switch, restated, and CENSUS: one feature width (or
  more) per case label of the switch as csrc/agg_multi.hip spells it.
"""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn_computing_amd", "csrc")

AGGRS = ("sum", "mean", "min", "max", "var", "std")                 # ascending bit order of GNNAGG_AGGR_*
SCALERS = ("identity", "amplification", "attenuation")              # ... and of GNNAGG_SCALER_*
LONG_EDGES, SEG_EDGES, BATCH, MAX_FEAT = 128, 512, 4, 1024          # kGatv2LongEdges, kGatv2SegEdges, kGatv2Batch, kGatv2MaxFeat (csrc/common.h)

# ------------------------------------------------------------------------------------------------ fixture
DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 511, 512, 513, 1100, 0]
SEED = 123


@functools.lru_cache(maxsize=None)
def fixture_graph():
    """(ptr, idx, n_src): rows of DEGREES edges, ids drawn up to n_src - 1 = V + 4 with duplicates"""
    rng = np.random.default_rng(SEED)
    V = len(DEGREES)
    n_src = V + 5
    ptr = np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int32)
    idx = rng.integers(0, n_src, size=int(ptr[-1])).astype(np.int32)
    return ptr, idx, n_src


@functools.lru_cache(maxsize=None)
def fixture_x(F, mean=0.0):
    """standard normal features [n_src, F] (mean 100: the set that exercises the cancellation of the two-moment variance)"""
    _, _, n_src = fixture_graph()
    x = np.random.default_rng(SEED + 1000 + F).standard_normal((n_src, F)).astype(np.float32)
    return (x + np.float32(mean)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture_val():
    ptr, _, _ = fixture_graph()
    return np.random.default_rng(SEED + 1).standard_normal(int(ptr[-1])).astype(np.float32)


# ------------------------------------------------------------------------------------------------ references
def messages32(idx, val, x):
    """the fp32 messages [E, F]: ONE fp32 multiply, or the gathered row itself without val"""
    m = x[idx].astype(np.float32)
    return m if val is None else (val.astype(np.float32)[:, None] * m).astype(np.float32)


def multi_ref(ptr, idx, val, x):
    """float64 reference over the fp32 messages: the six aggregates [V, F] (rows without edges 0), `abs` = sum |m| and `sq` = sum m * m
    (the terms of the bounds), `deg`"""
    V, F = len(ptr) - 1, x.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        m = messages32(idx, val, x)
    m64 = m.astype(np.float64)
    out = {k: np.zeros((V, F)) for k in AGGRS + ("abs", "sq")}
    out["deg"] = np.diff(ptr).astype(np.int64)
    for r in range(V):
        b, e = int(ptr[r]), int(ptr[r + 1])
        if e == b:
            continue
        seg = m64[b:e]
        with np.errstate(invalid="ignore", over="ignore"):
            out["sum"][r] = seg.sum(0)
            out["mean"][r] = out["sum"][r] / (e - b)
            out["min"][r] = m[b:e].min(0)
            out["max"][r] = m[b:e].max(0)
            out["abs"][r] = np.abs(seg).sum(0)
            out["sq"][r] = (seg * seg).sum(0)
            out["var"][r] = np.maximum(out["sq"][r] / (e - b) - out["mean"][r] ** 2, 0.0)
            out["std"][r] = np.sqrt(out["var"][r])
    return out


def multi_chain32(ptr, idx, val, x):
    """numpy float32 restatement: sum = the chain s = s + m_p from +0 in CSR order, mean = s / float32(d), min / max exact, var and std the
    two-moment form in float32 (S2 = the chain s2 + m * m).  Bit-equal to the kernel's sum and mean on rows of at most LONG_EDGES edges."""
    V, F = len(ptr) - 1, x.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        m = messages32(idx, val, x)
    out = {k: np.zeros((V, F), np.float32) for k in AGGRS}
    for r in range(V):
        b, e = int(ptr[r]), int(ptr[r + 1])
        if e == b:
            continue
        s, s2 = np.zeros(F, np.float32), np.zeros(F, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for p in range(b, e):
                s = (s + m[p]).astype(np.float32)
                s2 = (s2 + (m[p] * m[p]).astype(np.float32)).astype(np.float32)
            d = np.float32(e - b)
            out["sum"][r] = s
            out["mean"][r] = (s / d).astype(np.float32)
            out["min"][r] = m[b:e].min(0)
            out["max"][r] = m[b:e].max(0)
            mu = out["mean"][r]
            out["var"][r] = np.maximum(((s2 / d).astype(np.float32) - (mu * mu).astype(np.float32)).astype(np.float32), np.float32(0))
            out["std"][r] = np.sqrt(out["var"][r]).astype(np.float32)
    return out


def sum_bound(ref):
    """the project's 1e-5 bar: |sum - ref| <= 1e-5 * sum |m|"""
    return 1e-5 * ref["abs"]


def mean_bound(ref):
    return sum_bound(ref) / np.maximum(ref["deg"], 1)[:, None]


def var_bound(ref):
    """4e-5 * sum m^2 / d: 1e-5 on S2 / d, 2e-5 on mean^2 (Cauchy-Schwarz: mean^2 <= S2 / d), one rounding of the difference"""
    return 4e-5 * ref["sq"] / np.maximum(ref["deg"], 1)[:, None]


def std_bound(ref):
    """|sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b))"""
    B = var_bound(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(np.sqrt(B), np.where(ref["std"] > 0, B / ref["std"], np.inf))


BOUNDS = {"sum": sum_bound, "mean": mean_bound, "var": var_bound, "std": std_bound}


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 counts as 0, anything / 0 as inf)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max()) if q.size else 0.0


def scaler64(name, deg, delta):
    """the float64 scaler per row [V] (delta as the kernel receives it: one fp32 value); rows without edges 0"""
    d = np.asarray(deg, np.float64)
    delta = float(np.float32(delta))
    with np.errstate(divide="ignore"):
        s = {"identity": np.ones_like(d), "amplification": np.log(d + 1.0) / delta, "attenuation": delta / np.log(d + 1.0)}[name]
    return np.where(d > 0, s, 0.0)


# ------------------------------------------------------------------------------------------------ layout
def multi_layout(aggrs, scalers, F):
    """{(scaler, aggr): slice of y's columns}: blocks in ascending bit order whatever order the names come in, scaler-major"""
    a_sorted = [a for a in AGGRS if a in aggrs]
    s_sorted = [s for s in SCALERS if s in scalers]
    A = len(a_sorted)
    return {(s, a): slice((sp * A + ap) * F, (sp * A + ap + 1) * F) for sp, s in enumerate(s_sorted) for ap, a in enumerate(a_sorted)}


def multi_width(aggrs, scalers, F):
    return len(set(aggrs)) * len(set(scalers)) * F


# ------------------------------------------------------------------------------------------------ geometry
def multi_geometry(F, esize):
    """multi_geometry of csrc/agg_multi.hip: (vec, group, nf) -- 16-byte lanes where F is a multiple of their elements, else scalar lanes"""
    assert 1 <= F <= MAX_FEAT
    vec = 16 // esize
    if F % vec:
        vec = 1
    lanes = F // vec
    group = 8
    while group < 64 and group < lanes:
        group <<= 1
    nf = (lanes + group - 1) // group
    nf = 1 if nf <= 1 else 2 if nf <= 2 else 4 if nf <= 4 else 10 if nf <= 10 else 16
    return vec, group, nf


def multi_case(F, esize):
    """the key multi_launch_typed switches on"""
    vec, group, nf = multi_geometry(F, esize)
    return (10000 if vec > 1 else 0) + group * 100 + nf


# case label -> the fp32 feature widths that reach it (the first of each is what the GPU tests run)
CENSUS = {
    801: [1, 3, 5], 1601: [13], 3201: [30], 6401: [50], 6402: [101], 6404: [250], 6410: [602], 6416: [1001],
    10801: [32], 11601: [64], 13201: [128, 100], 16401: [256], 16402: [512], 16404: [1024],
}
# bf16 widths (16-byte lanes of 8 elements): the same switch, instantiated once more
CENSUS_BF16 = {801: [5], 6402: [100], 10801: [8], 11601: [128], 13201: [256], 16401: [512], 16402: [1024]}
CENSUS_F = [fs[0] for fs in CENSUS.values()]


def switch_labels():
    """the case labels of multi_launch_typed's switch, read from the source"""
    text = open(os.path.join(CSRC, "agg_multi.hip")).read()
    body = text[text.index("static int multi_launch_typed("):]
    body = body[:body.index("\nint launch_multi_aggr(")]
    assert body.count("switch (") == 1
    return sorted(int(n) for n in re.findall(r"\bcase (\d+):", body))


# ------------------------------------------------------------------------------------------------ tests
def tiny_graph():
    ptr = np.array([0, 0, 1, 4, 4, 9], np.int32)
    idx = np.array([2, 0, 0, 3, 6, 1, 1, 5, 2], np.int32)
    rng = np.random.default_rng(7)
    return ptr, idx, rng.standard_normal((7, 3)).astype(np.float32), rng.standard_normal(9).astype(np.float32)


@pytest.mark.parametrize("with_val", [False, True])
def test_references_against_brute_force_loops(with_val):
    ptr, idx, x, val = tiny_graph()
    val = val if with_val else None
    ref, c32 = multi_ref(ptr, idx, val, x), multi_chain32(ptr, idx, val, x)
    for r in range(5):
        for c in range(3):
            ms = [np.float32(x[idx[p], c]) if val is None else np.float32(val[p]) * np.float32(x[idx[p], c]) for p in range(ptr[r], ptr[r + 1])]
            d = len(ms)
            if d == 0:
                assert all(ref[k][r, c] == 0 and c32[k][r, c] == 0 for k in AGGRS)
                continue
            s64 = math.fsum(float(m) for m in ms)
            q64 = math.fsum(float(m) * float(m) for m in ms)
            assert ref["sum"][r, c] == pytest.approx(s64, rel=1e-14, abs=1e-300) and ref["mean"][r, c] == pytest.approx(s64 / d, rel=1e-14)
            assert ref["min"][r, c] == min(ms) and ref["max"][r, c] == max(ms)
            assert ref["var"][r, c] == pytest.approx(max(q64 / d - (s64 / d) ** 2, 0.0), rel=1e-9, abs=1e-15)
            assert ref["std"][r, c] == pytest.approx(math.sqrt(ref["var"][r, c]), rel=1e-14)
            assert ref["abs"][r, c] == pytest.approx(math.fsum(abs(float(m)) for m in ms), rel=1e-14)
            assert ref["sq"][r, c] == pytest.approx(q64, rel=1e-14)
            s = np.float32(0)
            for m in ms:
                s = np.float32(s + m)
            assert c32["sum"][r, c] == s and c32["mean"][r, c] == np.float32(s / np.float32(d))
            assert c32["min"][r, c] == min(ms) and c32["max"][r, c] == max(ms)
    assert list(ref["deg"]) == [0, 1, 3, 0, 5]


def test_fixture_covers_the_edges_of_the_walk():
    ptr, idx, n_src = fixture_graph()
    deg = list(np.diff(ptr))
    assert deg == DEGREES and len(idx) == sum(DEGREES) and n_src == len(DEGREES) + 5 and idx.max() == n_src - 1 > len(DEGREES)
    assert deg[0] == deg[-1] == 0
    assert {BATCH, BATCH + 1} <= set(deg)
    for g in (8, 16, 32, 64):
        assert {g - 1, g, g + 1} <= set(deg)
    assert {LONG_EDGES, LONG_EDGES + 1, SEG_EDGES, SEG_EDGES + 1} <= set(deg) and max(deg) > 2 * SEG_EDGES
    assert len(set(idx[ptr[10]:ptr[11]])) < deg[10] or len(set(idx)) < len(idx)   # duplicates are allowed and present
    text = open(os.path.join(CSRC, "common.h")).read()
    got = re.search(r"kGatv2Batch = (\d+), kGatv2LongEdges = (\d+), kGatv2SegEdges = (\d+), kGatv2MaxFeat = (\d+)", text).groups()
    assert tuple(int(g) for g in got) == (BATCH, LONG_EDGES, SEG_EDGES, MAX_FEAT)


def test_block_layout_is_scaler_major_in_bit_order():
    lay = multi_layout(("std", "mean", "max", "min"), ("attenuation", "identity"), 5)
    assert lay[("identity", "mean")] == slice(0, 5) and lay[("identity", "min")] == slice(5, 10)
    assert lay[("identity", "max")] == slice(10, 15) and lay[("identity", "std")] == slice(15, 20)
    assert lay[("attenuation", "mean")] == slice(20, 25) and lay[("attenuation", "std")] == slice(35, 40)
    assert multi_width(("std", "mean", "max", "min"), ("attenuation", "identity"), 5) == 40
    full = multi_layout(AGGRS, SCALERS, 3)
    assert sorted(s.start for s in full.values()) == list(range(0, 54, 3))
    assert full[("amplification", "sum")].start == 18 and full[("attenuation", "std")].stop == 54
    # the bit values of the names are those of the header and of the wrapper's tables
    header = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    for i, a in enumerate(AGGRS):
        assert re.search(r"#define GNNAGG_AGGR_%s %d\b" % (a.upper(), 1 << i), header) and gnc.aggregator.AGGRS[a] == 1 << i
    for i, s in enumerate(SCALERS):
        assert re.search(r"#define GNNAGG_SCALER_%s %d\b" % (s.upper(), 1 << i), header) and gnc.aggregator.SCALERS[s] == 1 << i


@pytest.mark.parametrize("mean", [0.0, 100.0])
@pytest.mark.parametrize("with_val", [False, True])
def test_restatement_stays_inside_the_bounds_on_the_fixture(mean, with_val):
    ptr, idx, _ = fixture_graph()
    x, val = fixture_x(5, mean), (fixture_val() if with_val else None)
    ref, c32 = multi_ref(ptr, idx, val, x), multi_chain32(ptr, idx, val, x)
    assert np.array_equal(c32["min"], ref["min"]) and np.array_equal(c32["max"], ref["max"])
    for k in ("sum", "mean", "var", "std"):
        ratio = worst_ratio(c32[k], ref[k], BOUNDS[k](ref))
        print("%s (mean %g, val %s): worst |restatement - ref| / bound = %.4f" % (k, mean, with_val, ratio))
        assert ratio <= 1.0, (k, ratio)
    assert (c32["var"] >= 0).all() and np.isfinite(c32["std"]).all()


def test_geometry_picker_covers_every_width():
    for esize in (4, 2):
        for F in range(1, MAX_FEAT + 1):
            vec, group, nf = multi_geometry(F, esize)
            assert vec in (1, 16 // esize) and F % vec == 0 and group in (8, 16, 32, 64) and nf in (1, 2, 4, 10, 16)
            assert group * nf * vec >= F and (vec > 1) == (F % (16 // esize) == 0)
            assert group == 8 or (group // 2) * vec < F       # the narrowest group that has a lane per element pack
            assert nf == 1 or group == 64
    assert multi_geometry(128, 4) == (4, 32, 1) and multi_geometry(128, 2) == (8, 16, 1) and multi_geometry(64, 4) == (4, 16, 1)
    assert multi_geometry(100, 4) == (4, 32, 1) and multi_geometry(100, 2) == (1, 64, 2) and multi_geometry(602, 4) == (1, 64, 10)
    assert multi_geometry(1024, 4) == (4, 64, 4) and multi_geometry(1024, 2) == (8, 64, 2) and multi_geometry(3, 4) == (1, 8, 1)
    # the picker in the source is this one: its constants, spelled there
    text = open(os.path.join(CSRC, "agg_multi.hip")).read()
    pick = text[text.index("static bool multi_geometry("):text.index("size_t multi_aggr_slot_floats(")]
    for piece in ("int vec = 16 / esize;", "if (F % vec != 0) vec = 1;", "while (group < 64 && group < lanes) group <<= 1;",
                  "nf <= 1 ? 1 : nf <= 2 ? 2 : nf <= 4 ? 4 : nf <= 10 ? 10 : 16", "F > kGatv2MaxFeat"):
        assert piece in pick, piece


def test_census_reaches_every_case_of_the_dispatch_switch_and_nothing_else():
    labels = switch_labels()
    assert labels == sorted(CENSUS), "a case of multi_launch_typed without a census entry (or the reverse): %s vs %s" % (labels, sorted(CENSUS))
    for case, widths in CENSUS.items():
        for F in widths:
            assert multi_case(F, 4) == case, (F, case, multi_case(F, 4))
    for case, widths in CENSUS_BF16.items():
        assert case in labels
        for F in widths:
            assert multi_case(F, 2) == case, (F, case, multi_case(F, 2))
    # every width the picker can see lands on a label (fp32), and on a label other than the fp32-only one (bf16)
    assert {multi_case(F, 4) for F in range(1, MAX_FEAT + 1)} == set(labels)
    assert {multi_case(F, 2) for F in range(1, MAX_FEAT + 1)} == set(labels) - {16404}
    assert {1, 3, 5, 100, 128, 602, 1024} <= {F for fs in CENSUS.values() for F in fs}


def test_a_case_without_a_census_entry_is_noticed(monkeypatch):
    monkeypatch.delitem(CENSUS, 6410)
    with pytest.raises(AssertionError):
        test_census_reaches_every_case_of_the_dispatch_switch_and_nothing_else()


def test_the_call_exists_at_every_layer():
    assert callable(getattr(gnc.Aggregator_GCN, "run_multi", None)) and callable(getattr(gnc, "gcn_run_multi", None))
    assert callable(getattr(gnc, "pna_delta", None))
    assert "gnnagg_gcn_run_multi" in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert any(l.split()[-1] == "gnnagg_gcn_run_multi" and " T " in l for l in out.splitlines())
    kfiles = re.search(r"^KFILES := (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "agg_multi" in kfiles and os.path.exists(os.path.join(CSRC, "agg_multi.hip"))
    # without a handle the call refuses like its neighbours
    assert gnc.lib().gnnagg_gcn_run_multi(0, None, 0, None, 0, 4, 1, 1, 1.0) in (_lib.ERR_ARG, _lib.ERR_HIP)


def test_pna_delta_against_numpy():
    import torch
    ptr, _, _ = fixture_graph()
    want = float(np.mean(np.log(np.diff(ptr).astype(np.float64) + 1.0)))
    assert gnc.pna_delta(ptr) == pytest.approx(want, rel=1e-15) and gnc.pna_delta(torch.from_numpy(ptr)) == pytest.approx(want, rel=1e-15)
    assert gnc.pna_delta([0, 1, 3]) == pytest.approx((math.log(2.0) + math.log(3.0)) / 2)
    assert gnc.pna_delta([0]) == 1.0
    with pytest.raises(ValueError):
        gnc.pna_delta(np.zeros((2, 2), np.int32))
