"""GPU: the edges of the fp32 dense combine (gnnagg_matmul_nn, csrc/dense_f32.hip) -- what tests/test_gpu_bf16_gemm.py checks for the bf16
GEMM.  launch_dense_nn picks its kernel from the shape AND from the alignment of A and B, so operands are carved out of larger buffers at
float offsets; the buffers around A and B hold NaN (a k, row or column tail that reads on meets one), C lies between sentinels and is
itself NaN before the call (every element has to be written, none outside).  Inf and NaN in A stay in their rows: the judge there is the
class map of the float64 product (tests/test_nonfinite_host.py).  Every fp32 kernel keeps the ascending-k chain, so every finite
expectation is bit-equal to the oracle's orc.matmul_nn."""
import ctypes

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from oracle import oracle as orc
from test_gpu_parity import DEV, rand
from test_nonfinite_host import FINITE, assert_same_classes, classes, gemm_poison_inf, gemm_ref64, weights

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -77.0

# (M, N, K, float offset of A, float offset of B)                                      the route launch_dense_nn takes, first match
ROUTES = [
    (129, 33, 7, 0, 0),          # k_dense_nn            M < 1024, K % 32 != 0
    (300, 32, 100, 0, 0),        # k_dense_nn            K % 32 != 0
    (300, 32, 128, 1, 0),        # k_dense_nn            K = 128 but A is 4-byte aligned: not k_dense_nn_up; the scalar branch of the A loads
    (300, 32, 32, 0, 0),         # k_dense_nn_up<1, 1>
    (257, 64, 64, 0, 0),         # k_dense_nn_up<2, 2>   33 .. 64 columns: both column blocks in one workgroup
    (200, 33, 96, 0, 0),         # k_dense_nn_up<3, 2>   ragged second column block
    (127, 64, 128, 0, 0),        # k_dense_nn_up<4, 2>   one ragged row tile
    (1100, 100, 72, 0, 0),       # k_dense_nn_strip<4>   N > 64, M >= 1024; N % 128 != 0, K % 4 == 0
    (1100, 100, 70, 0, 0),       # k_dense_nn_strip<2>   K even
    (1100, 129, 33, 0, 0),       # k_dense_nn_strip<1>   N % 4 != 0: scalar loads of A and B
    (1100, 128, 64, 0, 1),       # k_dense_nn_strip<1>   B not 16-byte aligned, whatever N is
    (1100, 128, 64, 1, 0),       # k_dense_nn_strip<1>   A 4-byte aligned
    (1100, 128, 36, 0, 0),       # k_dense_nn_lean<4>    N % 128 == 0, 16-byte rows, K % 32 != 0: a masked ragged last chunk
    (1100, 256, 100, 0, 0),      # k_dense_nn_lean<4>    two column tiles
    (1100, 128, 64, 0, 0),       # k_dense_nn_ahead<4>   N % 128 == 0, 16-byte rows, K % 32 == 0
    (1300, 256, 96, 0, 0),       # k_dense_nn_ahead<4>   two column tiles, three chunks
    (1100, 128, 34, 0, 0),       # k_dense_nn_ahead<2>   K even, K % 4 != 0
    (1100, 128, 64, 2, 0),       # k_dense_nn_ahead<2>   A 8-byte aligned
    (1100, 128, 602, 2, 0),      # k_dense_nn_ahead<2>   A 8-byte aligned, ragged last chunk
]
# the only large cases: k_dense_nn_tall (64 < K <= 128, K % 4 == 0, M >= 500 000, 16-byte A), and its refusal of an 8-byte aligned A: the
# call falls through to k_dense_nn (N <= 64, K % 32 != 0)
TALL = [(500001, 7, 68, 0, 0), (500001, 7, 68, 2, 0)]

GUARD = 512   # floats around A and B (a multiple of 64: an operand at offset 0 keeps the allocation's 256-byte alignment)


def carve(values, offset, fill, guard=GUARD):
    """`values` as a contiguous fp32 device tensor `guard + offset` floats into a flat buffer filled with `fill`, `guard` floats and more behind it"""
    n = values.numel()
    buf = torch.full((guard + offset + n + guard + 8,), fill, dtype=torch.float32, device=DEV)
    view = buf[guard + offset:guard + offset + n].view(values.shape)
    view.copy_(values)
    return buf, view


def c_guard(N):
    return -(-2 * N // 64) * 64   # at least 2 N sentinels on each side, a multiple of 64 floats


def guarded_c(M, N, offset):
    """(buffer of sentinels, C inside it `offset` floats past a 256-byte boundary and NaN-filled)"""
    buf, C = carve(torch.full((M, N), NAN), offset, SENTINEL, guard=c_guard(N))
    return buf, C


def sentinels_intact(buf, C, offset):
    g, n = c_guard(C.shape[1]) + offset, C.numel()
    return bool((buf[:g] == SENTINEL).all()) and bool((buf[g + n:] == SENTINEL).all())


def operands(M, N, K, offA, offB, a, b):
    _, A = carve(torch.tensor(a), offA, NAN)
    _, B = carve(torch.tensor(b), offB, NAN)
    assert A.data_ptr() % 256 == 4 * offA and B.data_ptr() % 256 == 4 * offB and A.is_contiguous() and B.is_contiguous()
    return A, B


_cases = {}


def case(M, N, K):
    """(A, B, the oracle's product, the float64 product) of a shape, computed once and left unchanged"""
    if (M, N, K) not in _cases:
        a, b = rand((M, K), 1000 * M + K), weights((K, N), 77 * K + N)
        for arr in (a, b):
            arr.setflags(write=False)
        _cases[(M, N, K)] = (a, b, orc.matmul_nn(a, b), gemm_ref64(a, b))
    return _cases[(M, N, K)]


def check_tails_and_guards(M, N, K, offA, offB):
    a, b, want, ref64 = case(M, N, K)
    A, B = operands(M, N, K, offA, offB, a, b)
    for offC in (0, 1):
        cbuf, C = guarded_c(M, N, offC)
        assert gnc.matmul_NN(A, B, C) is C
        got = C.cpu().numpy()
        assert not np.isnan(got).any(), "an element of C was not written, or a tail read past its operand (C at float offset %d)" % offC
        assert np.array_equal(got, want), "C at float offset %d" % offC
        assert sentinels_intact(cbuf, C, offC), "a store outside C (C at float offset %d)" % offC
        # asymmetric operands against the float64 product: a transposed or shifted tile cannot pass through an oracle quirk
        np.testing.assert_allclose(got, ref64, rtol=1e-4, atol=2e-4)


def check_inf_stays_in_its_row(M, N, K, offA, offB):
    a, b, want, _ = case(M, N, K)
    ai = gemm_poison_inf(a)
    A, B = operands(M, N, K, offA, offB, ai, b)
    cbuf, C = guarded_c(M, N, 0)
    gnc.matmul_NN(A, B, C)
    got = C.cpu().numpy()
    ref64 = gemm_ref64(ai, b)
    assert_same_classes(got, ref64, "Inf in A")
    rows = np.arange(M)
    clean = (rows % 2 == 0) & (rows % 5 != 0) & (rows != M - 1)
    assert (classes(ref64)[clean] == FINITE).all() and (classes(ref64)[~clean] != FINITE).all()
    assert np.array_equal(got[clean], want[clean]), "a row without an Inf differs from the run on the clean A"
    assert np.array_equal(got, orc.matmul_nn(ai, b), equal_nan=True)
    assert sentinels_intact(cbuf, C, 0)


@pytest.mark.parametrize("M,N,K,offA,offB", ROUTES + TALL)
def test_tails_do_not_leak_and_no_store_leaves_c(M, N, K, offA, offB):
    check_tails_and_guards(M, N, K, offA, offB)


@pytest.mark.parametrize("M,N,K,offA,offB", ROUTES + TALL)
def test_inf_stays_in_its_row(M, N, K, offA, offB):
    check_inf_stays_in_its_row(M, N, K, offA, offB)


@pytest.mark.parametrize("M,N,K,offA,offB", [(300, 32, 100, 0, 0), (127, 64, 128, 0, 0), (1100, 100, 70, 0, 0), (1100, 128, 36, 0, 0),
                                             (1100, 128, 64, 0, 0), (1100, 128, 602, 2, 0)])
def test_a_nan_row_stays_in_its_row(M, N, K, offA, offB):
    """A[r, :] = NaN for one r in the middle of a 32-row block: row r of C is NaN, every other row is the clean run's"""
    a, b, want, _ = case(M, N, K)
    r = M // 2 + 5
    an = a.copy()
    an[r, :] = np.nan
    A, B = operands(M, N, K, offA, offB, an, b)
    _, C = guarded_c(M, N, 0)
    gnc.matmul_NN(A, B, C)
    got = C.cpu().numpy()
    assert_same_classes(got, gemm_ref64(an, b), "a NaN row of A")
    assert np.isnan(got[r]).all()
    keep = np.arange(M) != r
    assert np.array_equal(got[keep], want[keep])


def typed_f32(A, B, C, M, N, K):
    f32 = _lib.DTYPE_F32
    _lib.check(gnc.lib().gnnagg_matmul_nn_typed(ctypes.c_void_p(A.data_ptr()), f32, ctypes.c_void_p(B.data_ptr()), f32, ctypes.c_void_p(C.data_ptr()),
                                               f32, M, N, K, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("entry", ["matmul_nn", "matmul_nn_typed"])
def test_empty_sums_and_empty_outputs(entry):
    """K = 0: C = +0 everywhere (no sign bit), nothing outside it; M = 0 or N = 0: the call returns without touching anything"""
    def call(A, B, C, M, N, K):
        if entry == "matmul_nn":
            gnc.matmul_NN(A, B, C)
        else:
            typed_f32(A, B, C, M, N, K)
    for M, N in ((5, 7), (1100, 128), (300, 32)):
        for offC in (0, 1):
            cbuf, C = guarded_c(M, N, offC)
            call(torch.empty((M, 0), device=DEV), torch.empty((0, N), device=DEV), C, M, N, 0)
            assert bool((C == 0).all()) and not bool(torch.signbit(C).any()), (M, N, offC)
            assert sentinels_intact(cbuf, C, offC), "a store outside C"
    for M, N, K in ((0, 8, 4), (4, 0, 8), (0, 128, 64), (1100, 0, 64)):
        A, B = torch.ones((M, K), device=DEV), torch.ones((K, N), device=DEV)
        cbuf = torch.full((4096,), SENTINEL, device=DEV)
        call(A, B, cbuf[1024:1024 + M * N].view(M, N), M, N, K)
        assert bool((cbuf == SENTINEL).all())
    torch.cuda.synchronize()
