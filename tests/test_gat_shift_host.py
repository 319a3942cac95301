"""Host: the judges and generators of tests/test_gpu_gat_shift.py (the max-shifted edge softmax, gnnagg_gat_row_shift /
gnnagg_gat_run_shifted), pinned without a GPU.

  row_shift_ref      the per-edge fp32 leaky logits max(s, s * slope), s = att[dst, h, 0] + att[src, h, 1], and their per-row maximum
                     (+0 for a row without edges): what the shift IS.
  row_shift_formula  leaky(fl32(att[r, h, 0] + max_s att[s, h, 1])): how the kernel forms it.  For slope > 0 the fp32 addition, the fp32
                     multiplication by the slope and the select are non-decreasing, so the two are bit-equal (test (a)).
  gat_ref_shifted    d = fl32(leaky - shift[row]) and w = exp(d) in fp32 numpy, in that order; numerator and denominator in float64.
  gat_scale_shifted  sum w |x| / sum w with the same weights: the error scale of the suite's bound |y - ref| <= 1e-5 (scale + |ref|).

The "huge" regime -- a_dst ~ U[-30, 30], a_src ~ U[-320, 400] -- has leaky logits up to 430: the unshifted fp32 weights overflow in nearly
every row (test (d)), the shifted ones are <= 1 with the row's maximal edge at exactly 1."""
import os
import re

import numpy as np
import pytest

import gnn_computing_amd as gnc
from oracle import oracle as orc
from test_gat_logits_host import RTOL, SLOPES, edge_weights32, gat_scale, logit_graph, worst_ratio
from test_nonfinite_host import _per_row, powerlaw, rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference
def leaky_logits32(ptr, idx, att, heads=1, slope=0.2):
    """[E, H] float32: max(s, s * slope) formed in fp32 like edge_weight() of kernel_util.cuh, before the exp"""
    V = len(ptr) - 1
    rows = np.repeat(np.arange(V), np.diff(ptr))
    a = np.ascontiguousarray(att, dtype=np.float32).reshape(-1, heads, 2)
    with np.errstate(all="ignore"):
        s = a[rows, :, 0] + a[idx, :, 1]
        l = s * np.float32(slope)
        m = np.where(s > l, s, l)
    assert m.dtype == np.float32
    return m


def row_shift_ref(ptr, idx, att, heads=1, slope=0.2):
    """[V, H] float32: the per-row maximum of the per-edge fp32 leaky logits, +0 for rows without edges"""
    V = len(ptr) - 1
    m = leaky_logits32(ptr, idx, att, heads, slope)
    out = _per_row(np.maximum, ptr, np.ascontiguousarray(m.T, dtype=np.float64), -np.inf).T     # (fp32 values are exact in float64)
    out[np.diff(ptr) == 0] = 0.0
    return np.ascontiguousarray(out).astype(np.float32)


def row_shift_formula(ptr, idx, att, heads=1, slope=0.2):
    """[V, H] float32: leaky(fl32(att[r, h, 0] + max over the row's sources of att[s, h, 1])), +0 for rows without edges"""
    V = len(ptr) - 1
    a = np.ascontiguousarray(att, dtype=np.float32).reshape(-1, heads, 2)
    smax = _per_row(np.maximum, ptr, np.ascontiguousarray(a[idx, :, 1].T, dtype=np.float64), -np.inf).T.astype(np.float32)
    with np.errstate(all="ignore"):
        s = a[:V, :, 0] + smax
        l = s * np.float32(slope)
        out = np.where(s > l, s, l)
    assert out.dtype == np.float32
    out[np.diff(ptr) == 0] = 0.0
    return out


def shifted_weights32(ptr, idx, att, shift, heads=1, slope=0.2):
    """[E, H] float32: exp(fl32(leaky - shift[row])), the subtraction and the exp in fp32, in that order"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    with np.errstate(all="ignore"):
        d = leaky_logits32(ptr, idx, att, heads, slope) - np.asarray(shift, np.float32).reshape(-1, heads)[rows]
        w = np.exp(d)
    assert d.dtype == np.float32 and w.dtype == np.float32
    return w


def _weighted(ptr, idx, w, x, heads, absolute, block=16):
    """float64 [V, F]: sum_e w_e x_e / sum_e w_e per head (|x_e| when `absolute`), rows without edges 0, a zero denominator divided like
    any other (NaN)"""
    V, F = len(ptr) - 1, x.shape[1]
    D = F // heads
    wt = np.ascontiguousarray(w.T, dtype=np.float64)
    xt = np.ascontiguousarray(x.T, dtype=np.float64)
    if absolute:
        xt = np.abs(xt)
    out = np.zeros((F, V))
    nz = np.diff(ptr) > 0
    with np.errstate(all="ignore"):
        den = _per_row(np.add, ptr, wt, 0.0)
        for c0 in range(0, F, block):
            heads_of = np.arange(c0, min(c0 + block, F)) // D
            num = _per_row(np.add, ptr, np.take(xt[c0:c0 + block], idx, axis=1) * wt[heads_of], 0.0)
            out[c0:c0 + block][:, nz] = num[:, nz] / den[heads_of][:, nz]
    return np.ascontiguousarray(out.T)


def gat_ref_shifted(ptr, idx, att, x, shift, heads=1, slope=0.2):
    return _weighted(ptr, idx, shifted_weights32(ptr, idx, att, shift, heads, slope), x, heads, False)


def gat_scale_shifted(ptr, idx, att, x, shift, heads=1, slope=0.2):
    return _weighted(ptr, idx, shifted_weights32(ptr, idx, att, shift, heads, slope), x, heads, True)


def denominators_shifted(ptr, idx, att, shift, heads=1, slope=0.2):
    """float64 [V, H]: sum_e w_e of the shifted weights"""
    w = shifted_weights32(ptr, idx, att, shift, heads, slope)
    return _per_row(np.add, ptr, np.ascontiguousarray(w.T, dtype=np.float64), 0.0).T


# ------------------------------------------------------------------------------------------------ the generators
def huge_att(n, H, seed):
    """the huge regime: a_dst ~ U[-30, 30], a_src ~ U[-320, 400] -- leaky logits up to 430, far above expf's overflow threshold 88.7"""
    rng = np.random.default_rng(seed)
    att = np.empty((n, H, 2), np.float32)
    att[:, :, 0] = rng.uniform(-30.0, 30.0, (n, H))
    att[:, :, 1] = rng.uniform(-320.0, 400.0, (n, H))
    return att


def mild_att(n, H, seed):
    return rand((n, H, 2), seed) * np.float32(0.5)


def rows_with_a_nonfinite_weight(ptr, idx, att, heads, slope=0.2):
    """bool [V]: rows where the UNSHIFTED fp32 weights of some head hold an Inf or NaN"""
    w = edge_weights32(ptr, idx, att, heads, slope)
    bad = (~np.isfinite(w)).any(axis=1).astype(np.float64)[None, :]
    return _per_row(np.maximum, ptr, bad, 0.0)[0] > 0


def chain_emulation32(ptr, idx, w, x, heads):
    """fp32 [V, F]: numerator and denominator accumulated edge by edge in CSR order in fp32 (cumsum is sequential), one fp32 division:
    the arithmetic of a canonical chain, with a rounded product where the kernels use fma"""
    V, F = len(ptr) - 1, x.shape[1]
    D = F // heads
    y = np.zeros((V, F), np.float32)
    for r in np.flatnonzero(np.diff(ptr) > 0):
        b, e = ptr[r], ptr[r + 1]
        wr = w[b:e]
        num = np.cumsum(x[idx[b:e]] * np.repeat(wr, D, axis=1), axis=0, dtype=np.float32)[-1]
        den = np.cumsum(wr, axis=0, dtype=np.float32)[-1]
        y[r] = num / np.repeat(den, D)
    return y


_big = {}


def big_graph():
    """the 4000 x 100 000 power-law graph of tests/test_gpu_bf16_gat.py"""
    if "g" not in _big:
        _big["g"] = powerlaw(4000, 100000, 9, 1.1)
    return _big["g"]


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", [1, 8])
def test_a_the_shift_formula_is_the_per_edge_maximum_bit_for_bit(slope, H):
    ptr, idx = big_graph()
    V = len(ptr) - 1
    for name, att in (("huge", huge_att(V, H, 3)), ("mild", mild_att(V, H, 4))):
        ref, got = row_shift_ref(ptr, idx, att, H, slope), row_shift_formula(ptr, idx, att, H, slope)
        assert ref.dtype == np.float32 and ref.shape == (V, H)
        assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)), (name, slope, H)
    empty = np.diff(ptr) == 0
    small = gnc.graph.uniform_random_csr(500, 9000, seed=5)
    assert (np.diff(small[0]) == 0).any()
    r = row_shift_ref(*small, huge_att(500, H, 5), H, slope)
    assert np.all(r[np.diff(small[0]) == 0] == 0) and not np.signbit(r[np.diff(small[0]) == 0]).any()
    assert np.array_equal(r, row_shift_formula(*small, huge_att(500, H, 5), H, slope))
    assert not np.signbit(ref[empty]).any()


@pytest.mark.parametrize("F,H", [(30, 3), (64, 1), (32, 8)])
def test_b_on_mild_attention_the_shifted_reference_is_the_oracles_softmax(F, H):
    for ptr, idx in (logit_graph("host")[:2], gnc.graph.uniform_random_csr(500, 9000, seed=5)):
        V = len(ptr) - 1
        x, att = rand((V, F), 1), mild_att(V, H, 2)
        shift = row_shift_ref(ptr, idx, att, H)
        ref = gat_ref_shifted(ptr, idx, att, x, shift, H)
        fused = orc.gat_fused(ptr, idx, att, x, H)
        ratio = worst_ratio(fused, ref, gat_scale(ptr, idx, att, x, H) + np.abs(ref))
        print("F=%d H=%d: gat_fused against gat_ref_shifted, worst ratio %.3g of the bound" % (F, H, ratio))
        assert ratio < 1
        # ... and the two scales agree
        np.testing.assert_allclose(gat_scale_shifted(ptr, idx, att, x, shift, H), gat_scale(ptr, idx, att, x, H), rtol=1e-5, atol=1e-12)
        out = ref[np.diff(ptr) == 0]
        assert np.all(out == 0)


@pytest.mark.parametrize("F,H", [(4, 1), (16, 8)])
def test_c_huge_regime_a_fp32_chain_is_within_the_bound(F, H):
    ptr, idx = big_graph()
    V = len(ptr) - 1
    x, att = rand((V, F), 6), huge_att(V, H, 7)
    shift = row_shift_ref(ptr, idx, att, H)
    w = shifted_weights32(ptr, idx, att, shift, H)
    assert np.isfinite(w).all() and w.max() == 1.0 and w.min() >= 0.0
    den = denominators_shifted(ptr, idx, att, shift, H)
    has = np.diff(ptr) > 0
    assert (den[has] >= 1.0).all() and (den[has] <= np.diff(ptr)[has][:, None]).all()
    ref = gat_ref_shifted(ptr, idx, att, x, shift, H)
    assert np.isfinite(ref).all()
    scale = gat_scale_shifted(ptr, idx, att, x, shift, H)
    ratio = worst_ratio(chain_emulation32(ptr, idx, w, x, H), ref, scale + np.abs(ref))
    print("F=%d H=%d: fp32 CSR-order chain against gat_ref_shifted, worst ratio %.3g of the bound" % (F, H, ratio))
    assert ratio < 1


@pytest.mark.parametrize("H", [1, 8])
def test_d_huge_regime_overflows_the_unshifted_weights_in_most_rows(H):
    ptr, idx = big_graph()
    V = len(ptr) - 1
    bad = rows_with_a_nonfinite_weight(ptr, idx, huge_att(V, H, 7), H)
    has = np.diff(ptr) > 0
    print("H=%d: %d of %d rows with edges hold a non-finite unshifted weight" % (H, int(bad.sum()), int(has.sum())))
    assert not bad[~has].any() and 2 * bad.sum() >= has.sum()


def test_python_mirror_of_the_kernel_thresholds():
    """tests/test_gpu_gat_shift.py builds rows at the kernel's length thresholds from these"""
    text = open(os.path.join(ROOT, "gnn_computing_amd", "csrc", "common.h")).read()
    m = re.search(r"kShiftGroup = (\d+), kShiftHeads = (\d+), kShiftHubEdges = (\d+);", text)
    assert m and tuple(int(v) for v in m.groups()) == gnc.Aggregator_GAT.ROW_SHIFT_THRESHOLDS
