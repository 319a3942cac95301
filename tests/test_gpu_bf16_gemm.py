"""GPU: the bf16 dense combine (gnnagg_matmul_nn_typed, gnc.matmul_NN on bfloat16 operands; csrc/dense_bf16.hip).

The order of the additions inside a bf16 MFMA is not documented, so nothing here compares bits with the fp32 GEMM's ascending-k chain.
The contract (include/gnnagg.h): (a) where every partial sum is an integer below 2^24 the result is exact; (b) otherwise
|C - C64| <= 1e-5 . sum_k |a_k b_k| against the float64 product of the same bf16 operands; (c) tails contribute exact zeros, a bf16 C is
one rounding of the fp32 C, and the same call gives the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
RTOL = 1e-5   # the project's bound (tests/test_gpu_parity.py)

MS = [1, 31, 33, 127, 129, 1000]
# every K in {1, 7, 8, 9, 15, 16, 17, 100, 602} and N in {1, 2, 31, 32, 33, 64, 100, 128, 129} once: octet / alignment-class tails, the
# three column-block widths, a second column block (129), the widest K that fits the LDS image of a 128-column block (602)
KNS = [(1, 1), (7, 2), (8, 31), (9, 32), (15, 33), (16, 64), (17, 100), (100, 128), (602, 129)]
BOUND_SHAPES = [(129, 602, 33), (1000, 512, 128), (257, 100, 2), (64, 1024, 128)]


def ints(shape, seed):
    """integers in [-8, 8] (asymmetric random data: a swapped row / column or a wrong k map cannot pass), CPU int64"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g)


def carve(values, dtype, offset, fill, guard=0):
    """`values` as a contiguous device tensor `offset` (+ guard) elements into a flat buffer filled with `fill`, `guard` more behind it"""
    n = values.numel()
    buf = torch.full((guard + offset + n + guard + 8,), fill, dtype=dtype, device=DEV)
    view = buf[guard + offset:guard + offset + n].view(values.shape)
    view.copy_(values.to(dtype))
    return buf, view


def run(A, B, out_dtype, C=None):
    M, N = A.shape[0], B.shape[1]
    if C is None:
        C = torch.full((M, N), float("nan"), dtype=out_dtype, device=DEV)   # poisoned: every element has to be written
    out = gnc.matmul_NN(A, B, C)
    assert out is C
    return C


@pytest.mark.parametrize("K,N", KNS)
@pytest.mark.parametrize("M", MS)
def test_exact_on_integers(M, K, N):
    a, b = ints((M, K), 1000 * M + K), ints((K, N), 77 * K + N)
    ref = a @ b
    C = run(a.to(BF).to(DEV), b.to(BF).to(DEV), torch.float32)
    assert torch.equal(C.cpu(), ref.float())
    Cb = run(a.to(BF).to(DEV), b.to(BF).to(DEV), BF)
    assert torch.equal(Cb.cpu(), ref.float().to(BF))


@pytest.mark.parametrize("M,K,N", [(70, 632, 128), (70, 1500, 100), (70, 2600, 33), (40, 5000, 129)])
def test_k_beyond_one_lds_image(M, K, N):
    """K too wide for the LDS image of a 128-column block: 64-column blocks (632), 32-column blocks (1500), and beyond those the image
    restaged per chunk of K (2600: two chunks; 5000: three, and five column blocks).  |sums| <= 64 K < 2^24: exact."""
    a, b = ints((M, K), 7 * M + K), ints((K, N), 9 * K + N)
    C = run(a.to(BF).to(DEV), b.to(BF).to(DEV), torch.float32)
    assert torch.equal(C.cpu(), (a @ b).float())


@pytest.mark.parametrize("cdt", [torch.float32, BF])
@pytest.mark.parametrize("M,K,N", [(33, 9, 33), (129, 16, 64), (127, 100, 128), (31, 602, 129), (1000, 17, 2)])
def test_unaligned_operands_and_guarded_output(M, K, N, cdt):
    """A, B, C one element into their buffers (2-byte aligned bf16, 4-byte aligned fp32 C); 64 sentinel elements on each side of C"""
    a, b = ints((M, K), 5 * M + K), ints((K, N), 3 * K + N)
    _, A = carve(a, BF, 1, 0.0)
    _, B = carve(b, BF, 1, 0.0)
    cbuf, C = carve(torch.zeros((M, N)), cdt, 1, -77.0, guard=64)
    assert A.data_ptr() % 4 == 2 and B.data_ptr() % 4 == 2 and C.data_ptr() % 16 != 0
    C.fill_(float("nan"))
    run(A, B, cdt, C)
    assert torch.equal(C.cpu().float(), (a @ b).float().to(cdt).float())
    lo, hi = cbuf[:65], cbuf[65 + M * N:]
    assert bool((lo == -77.0).all()) and bool((hi == -77.0).all()), "a store outside C"


@pytest.mark.parametrize("offset", [1, 2, 4, 8])     # 2-, 4-, 8- and 16-byte aligned operands: every load width
@pytest.mark.parametrize("M,K,N", [(33, 9, 33), (33, 16, 33), (5, 100, 33), (70, 72, 8)])
def test_tails_do_not_leak(M, K, N, offset):
    """the elements around A and B are NaN: k, row and column tails are zeros built in registers, not whatever lies behind the operand"""
    a, b = ints((M, K), 11 * M + K + offset), ints((K, N), 13 * K + N + offset)
    _, A = carve(a, BF, offset, float("nan"))
    _, B = carve(b, BF, offset, float("nan"))
    C = run(A, B, torch.float32)
    assert torch.equal(C.cpu(), (a @ b).float())


def test_nan_and_inf_stay_in_their_row():
    M, K, N, r = 70, 100, 33, 37
    a, b = ints((M, K), 21).float(), ints((K, N), 22).float()
    b[b == 0] = 1.0                      # (inf * 0 would be a NaN of the product's own making; either way it is row r's)
    a[r, 3], a[r, 77] = float("nan"), float("inf")
    C = run(a.to(BF).to(DEV), b.to(BF).to(DEV), torch.float32).cpu()
    finite = torch.isfinite(C)
    assert not finite[r].any() and finite[:r].all() and finite[r + 1:].all()
    keep = torch.arange(M) != r
    assert torch.equal(C[keep], (a[keep].double() @ b.double()).float())


_bound_cache = {}


def bound_case(M, K, N):
    """(A, B on the device in bf16, float64 product of those bf16 operands, sum_k |a_k b_k|), computed once per shape"""
    if (M, K, N) not in _bound_cache:
        g = torch.Generator().manual_seed(M + K + N)
        A = torch.randn((M, K), generator=g).to(BF)
        B = (torch.randn((K, N), generator=g) * K ** -0.5).to(BF)
        a64, b64 = A.double().numpy(), B.double().numpy()
        _bound_cache[(M, K, N)] = (A.to(DEV), B.to(DEV), a64 @ b64, np.abs(a64) @ np.abs(b64))
    return _bound_cache[(M, K, N)]


@pytest.mark.parametrize("M,K,N", BOUND_SHAPES)
def test_bound_one_rounding_and_determinism(M, K, N):
    A, B, ref, scale = bound_case(M, K, N)
    C32 = run(A, B, torch.float32)
    err = np.abs(C32.cpu().numpy().astype(np.float64) - ref)
    ratio = float((err / (scale + 1e-300)).max())
    print("bf16 GEMM M=%d K=%d N=%d: max |C - C64| / sum|a b| = %.3e (bar %.0e)" % (M, K, N, ratio, RTOL))
    assert (err <= RTOL * scale + 1e-30).all(), "outside 1e-5 * sum|a b|: worst ratio %.3g" % ratio
    # a bf16 C is exactly one round-to-nearest-even of what the fp32-out call stores
    Cb = run(A, B, BF)
    assert torch.equal(Cb, C32.to(BF))
    # same inputs, same bits
    assert torch.equal(run(A, B, torch.float32), C32) and torch.equal(run(A, B, BF), Cb)
    # out_dtype picks C's type; the default follows A
    assert gnc.matmul_NN(A, B).dtype == BF and torch.equal(gnc.matmul_NN(A, B, out_dtype=torch.float32), C32)


def test_bf16_c_overflows_to_inf_where_the_rounding_does():
    """a sum above bf16's largest finite value, finite in fp32 in whatever order it is added: 2^127 (2 - 2^-9) lies above the midpoint
    between bf16's largest finite value and 2^128, so the one rounding gives inf, as torch's own conversion does"""
    a = torch.zeros((2, 10))
    a[0] = torch.tensor([2.0 ** (127 - j) for j in range(10)])
    a[1] = 1.5
    b = torch.ones((10, 3))
    A, B = a.to(BF).to(DEV), b.to(BF).to(DEV)
    C32, Cb = run(A, B, torch.float32), run(A, B, BF)
    assert torch.isfinite(C32).all() and torch.isinf(Cb[0]).all() and bool((Cb[0] > 0).all()) and torch.isfinite(Cb[1]).all()
    assert torch.equal(Cb, C32.to(BF)) and torch.equal(C32[1].cpu(), torch.full((3,), 15.0))


def test_fp32_through_the_typed_entry_is_the_fp32_gemm():
    g = torch.Generator().manual_seed(5)
    A, B = torch.randn((257, 100), generator=g).to(DEV), torch.randn((100, 33), generator=g).to(DEV)
    want = gnc.matmul_NN(A, B)
    C = torch.full((257, 33), float("nan"), device=DEV)
    f32 = _lib.DTYPE_F32
    _lib.check(gnc.lib().gnnagg_matmul_nn_typed(ctypes.c_void_p(A.data_ptr()), f32, ctypes.c_void_p(B.data_ptr()), f32, ctypes.c_void_p(C.data_ptr()),
                                               f32, 257, 33, 100, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(C, want)


@pytest.mark.parametrize("cdt", [torch.float32, BF])
def test_empty_sums_and_empty_outputs(cdt):
    for M, N in ((5, 7), (64, 8), (3, 1)):   # (an odd count of bf16 elements at an odd offset too)
        _, C = carve(torch.full((M, N), 3.0), cdt, 1, 3.0)
        gnc.matmul_NN(torch.empty((M, 0), dtype=BF, device=DEV), torch.empty((0, N), dtype=BF, device=DEV), C)
        assert bool((C == 0).all()) and not bool(torch.signbit(C).any())
    for M, K, N in ((0, 8, 4), (4, 8, 0)):
        C = gnc.matmul_NN(torch.ones((M, K), dtype=BF, device=DEV), torch.ones((K, N), dtype=BF, device=DEV), out_dtype=cdt)
        assert C.shape == (M, N) and C.dtype == cdt
    torch.cuda.synchronize()


def test_many_row_groups_per_workgroup():
    """M = 300 000 rows on at most 256 persistent workgroups of 8 wavefronts: every wavefront walks a range of 147 rows, five tiles, the
    last one partial, and the ring of requests runs across the tile boundaries.  (A launch recipe with more wavefronts needs a larger M
    here: M > 32 x wavefronts.)  Integer data: exact in any order, compared on the device."""
    M, K, N = 300000, 16, 8
    g = torch.Generator(device=DEV).manual_seed(9)
    A = torch.randint(-8, 9, (M, K), device=DEV, generator=g).to(BF)
    B = torch.randint(-8, 9, (K, N), device=DEV, generator=g).to(BF)
    want = A.float() @ B.float()
    assert torch.equal(run(A, B, torch.float32), want)
    assert torch.equal(run(A, B, BF), want.to(BF))


def test_past_2_to_31_elements():
    """M K = (2^22 + 33) 512 > 2^31 elements of A: row offsets need 64 bits"""
    M, K, N = 2 ** 22 + 33, 512, 8
    g = torch.Generator(device=DEV).manual_seed(10)
    A8 = torch.randint(-8, 9, (M, K), device=DEV, generator=g, dtype=torch.int8)
    A = A8.to(BF)
    del A8
    B = torch.randint(-8, 9, (K, N), device=DEV, generator=g).to(BF)
    C = torch.full((M, N), float("nan"), device=DEV)
    gnc.matmul_NN(A, B, C)
    assert not bool(torch.isnan(C).any())
    for lo, hi in ((0, 64), (M - 64, M), (2 ** 22 - 32, 2 ** 22 + 32)):
        assert torch.equal(C[lo:hi], A[lo:hi].float() @ B.float()), "rows %d .. %d" % (lo, hi)
    del A, B, C
    torch.cuda.empty_cache()


@pytest.mark.parametrize("cdt", [torch.float32, BF])
def test_graph_capture(cdt):
    A, B, _, _ = bound_case(1000, 512, 128)
    eager = run(A, B, cdt)
    C = torch.empty((1000, 128), dtype=cdt, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gnc.matmul_NN(A, B, C)          # warm-up: the function attribute is set outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            gnc.matmul_NN(A, B, C)
        for _ in range(2):
            C.fill_(float("nan"))
            graph.replay()
            side.synchronize()
            assert torch.equal(C, eager)
    torch.cuda.current_stream().wait_stream(side)
