"""Host: the judges of tests/test_gpu_nonfinite.py and tests/test_gpu_gemm_f32_edges.py, pinned without a GPU.

Every output element of an aggregation or a GEMM is finite, +Inf, -Inf or NaN, and which of the four does not depend on the order of the
additions as long as every weight is finite and non-zero and the finite magnitudes stay far from overflow: an Inf operand times a non-zero
weight is an Inf of the product's sign, Infs of one sign add up to that Inf, Infs of both signs or any NaN give NaN, everything else stays
finite.  So the judge of a non-finite result is its CLASS MAP against a plain float64 numpy reference written here (gcn_ref64, gat_ref64,
gemm_ref64), and the generators (weights, nonzero) never emit the one thing that would make the class depend on the kernel: an exact zero
weight, whose product with an Inf is a NaN of the reference's own making.  The GPU files import the generators and references from here;
this file checks them against the C oracle (same classes element for element) and checks the choice of the NaN sources."""
import numpy as np
import pytest

import gnn_computing_amd as gnc
from oracle import oracle as orc

FINITE, PINF, NINF, NAN = 0, 1, 2, 3
INF = float("inf")


def rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def classes(a):
    """int8 map: 0 finite, 1 +Inf, 2 -Inf, 3 NaN"""
    a = np.asarray(a)
    c = np.zeros(a.shape, np.int8)
    c[a == np.inf] = PINF
    c[a == -np.inf] = NINF
    c[np.isnan(a)] = NAN
    return c


def assert_same_classes(got, ref, what):
    cg, cr = classes(got), classes(ref)
    bad = cg != cr
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        names = ("finite", "+Inf", "-Inf", "NaN")
        raise AssertionError("%s: %d elements of another class than the float64 reference; first at %s: %s, reference %s"
                             % (what, int(bad.sum()), at, names[cg[at]], names[cr[at]]))


def nonzero(a, seed=12345):
    """`a` (float32) with its exact zeros redrawn: 0 * Inf would be a NaN of the reference's own making"""
    a = np.array(a, dtype=np.float32, copy=True)
    rng = np.random.default_rng(seed)
    while True:
        z = a == 0
        if not z.any():
            return a
        a[z] = rng.standard_normal(int(z.sum()), dtype=np.float32)


def weights(n, seed, positive=False):
    """edge values / GEMM operands without an exact zero; positive: |randn| + 0.1"""
    v = rand(n, seed)
    return (np.abs(v) + np.float32(0.1)).astype(np.float32) if positive else nonzero(v, seed + 1)


def signed_weights(ptr, seed):
    """edge values of both signs, all negative in the rows r % 7 == 3 and all positive in the rows r % 7 == 5: with +Inf in every source
    such rows sum to -Inf / +Inf whatever their degree, the mixed rows (nearly all of the others) to NaN"""
    v = weights(int(ptr[-1]), seed)
    r = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)) % 7
    v[r == 3] = -np.abs(v[r == 3])
    v[r == 5] = np.abs(v[r == 5])
    return v


def inf_columns(F, H=1):
    """column 0, column F - 1 and one column inside every head (h D + h % D)"""
    D = F // H
    return sorted({0, F - 1} | {h * D + h % D for h in range(H)})


def poison_inf(x, cols):
    x = x.copy()
    x[:, cols] = INF
    return x


def poison_nan(x, sources):
    x = x.copy()
    x[np.atleast_1d(sources), :] = np.nan
    return x


def reached(ptr, idx, sources):
    """bool [V]: rows that have one of `sources` as a neighbor"""
    V = len(ptr) - 1
    rows = np.repeat(np.arange(V), np.diff(ptr))
    hit = np.zeros(V, bool)
    hit[rows[np.isin(idx, np.atleast_1d(sources))]] = True
    return hit


def nan_sources(ptr, idx, most=5):
    """One source (up to `most` on a sparse graph) whose rows number at least 8 and at most half of all rows: the most widely
    referenced sources that still leave half of the rows clean, added until 8 rows are reached."""
    V = len(ptr) - 1
    rows = np.repeat(np.arange(V), np.diff(ptr))
    pairs = np.unique(np.stack([rows, idx.astype(np.int64)], axis=1), axis=0)
    reach = np.bincount(pairs[:, 1], minlength=V)
    picked, hit = [], np.zeros(V, bool)
    for s in np.argsort(-reach, kind="stable"):
        if len(picked) == most or hit.sum() >= 8:
            break
        trial = hit | reached(ptr, idx, [s])
        if reach[s] > 0 and trial.sum() <= V // 2:
            picked.append(int(s))
            hit = trial
    return picked


def hub_last_source(ptr, idx):
    """the source of the last edge of the longest row: where the clamps of a ragged last round / window point"""
    r = int(np.argmax(np.diff(ptr)))
    return int(idx[ptr[r + 1] - 1])


def _per_row_at(ufunc, ptr, prod_t, init):
    """np.add.at / np.maximum.at of the per-edge products `prod_t` [columns, E] onto their target rows: [columns, V]"""
    V = len(ptr) - 1
    out = np.full((V, prod_t.shape[0]), init, np.float64)
    ufunc.at(out, np.repeat(np.arange(V), np.diff(ptr)), prod_t.T)
    return np.ascontiguousarray(out.T)


def _per_row(ufunc, ptr, prod_t, init):
    """The same reduction as _per_row_at, through ufunc.reduceat over the contiguous edge range of every row that has edges (a CSR lists a
    row's edges together; ufunc.at takes seconds on the dense test graphs).  test_reduceat_is_the_per_row_ufunc_at pins the equivalence."""
    V = len(ptr) - 1
    out = np.full((prod_t.shape[0], V), init, np.float64)
    nz = np.flatnonzero(np.diff(ptr) > 0)
    if len(nz):
        out[:, nz] = ufunc.reduceat(prod_t, np.asarray(ptr)[nz].astype(np.intp), axis=1)
    return out


def gcn_ref64(ptr, idx, val, x, reduce="sum", block=16):
    """float64: per row the sum / mean / max over its edges of val[e] . x[idx[e]] (val None: 1); rows without edges are 0"""
    V, F = len(ptr) - 1, x.shape[1]
    deg = np.diff(ptr)
    xt = np.ascontiguousarray(x.T, dtype=np.float64)      # columns as rows: a column's per-edge products are contiguous
    v = None if val is None else val.astype(np.float64)
    out = np.zeros((F, V))
    with np.errstate(invalid="ignore"):
        for c0 in range(0, F, block):                     # (column blocks: the per-edge products of a dense graph do not fit at once)
            prod = np.take(xt[c0:c0 + block], idx, axis=1)
            if v is not None:
                prod *= v
            if reduce == "max":
                m = _per_row(np.maximum, ptr, prod, -np.inf)
                m[:, deg == 0] = 0.0
                out[c0:c0 + block] = m
            else:
                out[c0:c0 + block] = _per_row(np.add, ptr, prod, 0.0)
        if reduce == "mean":
            out /= np.maximum(deg, 1)
    return np.ascontiguousarray(out.T)


def gat_ref64(ptr, idx, att, x, heads=1, slope=0.2, block=16):
    """float64: w_e = exp(leaky_relu(att[dst, h, 0] + att[src, h, 1])), y = sum_e w_e x_e / sum_e w_e per head; empty rows are 0"""
    V, F = len(ptr) - 1, x.shape[1]
    D = F // heads
    rows = np.repeat(np.arange(V), np.diff(ptr))
    att = att.reshape(V, heads, 2).astype(np.float64)
    z = att[rows, :, 0] + att[idx, :, 1]
    wt = np.ascontiguousarray(np.exp(np.where(z > 0, z, slope * z)).T)     # [H, E], positive and finite
    den = _per_row(np.add, ptr, wt, 0.0)                                    # [H, V]
    xt = np.ascontiguousarray(x.T, dtype=np.float64)
    out = np.zeros((F, V))
    nz = np.diff(ptr) > 0
    with np.errstate(invalid="ignore"):
        for c0 in range(0, F, block):
            heads_of = np.arange(c0, min(c0 + block, F)) // D
            num = _per_row(np.add, ptr, np.take(xt[c0:c0 + block], idx, axis=1) * wt[heads_of], 0.0)
            out[c0:c0 + block][:, nz] = num[:, nz] / den[heads_of][:, nz]
    return np.ascontiguousarray(out.T)


def gemm_ref64(A, B):
    with np.errstate(invalid="ignore", over="ignore"):
        return A.astype(np.float64) @ B.astype(np.float64)


def gemm_poison_inf(A):
    """A[r, 0] = +Inf for every odd r and r = M - 1 (a k tail that reads on into the next row meets an Inf), A[r, K - 1] = -Inf for r % 5 == 0"""
    A = A.copy()
    M, K = A.shape
    A[1::2, 0] = INF
    A[M - 1, 0] = INF
    A[0::5, K - 1] = -INF
    return A


# ------------------------------------------------------------------------------------------------ the graphs of the GPU files
def powerlaw(V, E, seed, alpha):
    p, i = gnc.graph.powerlaw_csr(V, E, seed=seed, alpha=alpha)
    return p.numpy(), i.numpy()


def gat_hub_graph():
    """the graph of test_gpu_parity.py::test_gat_balanced_plan_with_hubs"""
    V = 350
    rng = np.random.default_rng(13)
    deg = rng.integers(0, 7, V)
    deg[11], deg[180], deg[349] = 4000, 900, 70
    ptr = np.zeros(V + 1, np.int32)
    ptr[1:] = np.cumsum(deg)
    return ptr, rng.integers(0, V, int(ptr[-1])).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the tests
def test_generators_never_emit_a_zero_weight():
    for seed in range(20):
        for positive in (False, True):
            v = weights(5000, seed, positive)
            assert v.dtype == np.float32 and np.isfinite(v).all() and not (v == 0).any()
            assert not positive or (v >= 0.1).all()
    a = np.zeros((7, 9), np.float32)
    a[3, 4] = 2.0
    b = nonzero(a)
    assert not (b == 0).any() and b[3, 4] == 2.0 and (a == 0).sum() == 62    # (a copy: the argument is left alone)


def test_class_map_and_poison_patterns():
    a = np.array([[0.0, -0.0, 1e38, -1e-45], [INF, -INF, np.nan, -np.nan]], np.float32)
    assert classes(a).tolist() == [[0, 0, 0, 0], [1, 2, 3, 3]]
    with pytest.raises(AssertionError, match=r"first at \(0, 1\): NaN, reference \+Inf"):
        assert_same_classes(np.array([[1.0, np.nan]]), np.array([[2.0, INF]]), "x")
    assert inf_columns(128) == [0, 127] and inf_columns(33) == [0, 32] and inf_columns(1) == [0]
    assert inf_columns(256, 8) == [0, 33, 66, 99, 132, 165, 198, 231, 255] and inf_columns(30, 3) == [0, 11, 22, 29]
    assert inf_columns(96, 3) == [0, 33, 66, 95]
    x = rand((6, 5), 1)
    xi, xn = poison_inf(x, [0, 4]), poison_nan(x, [2])
    assert np.isposinf(xi[:, [0, 4]]).all() and np.array_equal(xi[:, 1:4], x[:, 1:4]) and np.isfinite(x).all()
    assert np.isnan(xn[2]).all() and np.array_equal(np.delete(xn, 2, 0), np.delete(x, 2, 0))
    A = gemm_poison_inf(rand((11, 7), 2))
    assert np.isposinf(A[[1, 3, 5, 7, 9, 10], 0]).all() and np.isneginf(A[[0, 5, 10], 6]).all() and np.isfinite(A[[2, 4, 6, 8]]).all()


def test_reduceat_is_the_per_row_ufunc_at():
    ptr, idx = gnc.graph.uniform_random_csr(500, 9000, seed=5)
    x = rand((500, 9), 1)
    for xp in (x, poison_inf(x, [0, 8]), poison_nan(x, nan_sources(ptr, idx))):
        prod = np.ascontiguousarray((xp[idx].astype(np.float64) * weights(len(idx), 2).astype(np.float64)[:, None]).T)
        with np.errstate(invalid="ignore"):
            for ufunc, init in ((np.add, 0.0), (np.maximum, -np.inf)):
                a, b = _per_row(ufunc, ptr, prod, init), _per_row_at(ufunc, ptr, prod, init)
                assert np.array_equal(classes(a), classes(b))
                fin = classes(a) == FINITE
                np.testing.assert_allclose(a[fin], b[fin], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("graph,n_sources", [(("powerlaw", 900, 260000, 5, 0.9), 1), (("powerlaw", 4000, 100000, 9, 1.1), 5),
                                             (("uniform", 500, 9000, 5), 5), (("powerlaw", 3000, 120000, 5, 1.1), 5),
                                             (("powerlaw", 3000, 60000, 5, 1.0), 5), (("gat_hubs",), 5),
                                             (("uniform", 600, 72000, 13), 1), (("uniform", 120, 4000, 81), 5)])
def test_nan_sources_reach_at_least_8_rows_and_at_most_half(graph, n_sources):
    if graph[0] == "powerlaw":
        ptr, idx = powerlaw(*graph[1:])
    elif graph[0] == "uniform":
        ptr, idx = gnc.graph.uniform_random_csr(*graph[1:])
    else:
        ptr, idx = gat_hub_graph()
    V = len(ptr) - 1
    s = nan_sources(ptr, idx, n_sources)
    hit = reached(ptr, idx, s)
    assert 1 <= len(s) <= n_sources and 8 <= hit.sum() <= V // 2, (s, int(hit.sum()), V)
    # by the float64 reference itself, on one column
    ref = gcn_ref64(ptr, idx, None, poison_nan(rand((V, 1), 1), s))
    assert np.array_equal(np.isnan(ref[:, 0]), hit)
    # the hub row's last source reaches the hub row
    hs = hub_last_source(ptr, idx)
    assert reached(ptr, idx, [hs])[int(np.argmax(np.diff(ptr)))]


@pytest.mark.parametrize("F", [33, 8])
@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("with_val", [True, False])
def test_gcn_reference_and_oracle_agree_on_every_class(F, positive, with_val):
    ptr, idx = gnc.graph.uniform_random_csr(500, 9000, seed=5)
    V, E = len(ptr) - 1, len(idx)
    assert (np.diff(ptr) == 0).any()
    x = rand((V, F), 1)
    val = (weights(E, 2, True) if positive else signed_weights(ptr, 2)) if with_val else None
    assert val is None or not (val == 0).any()
    ps, tg = orc.neighbor_grouping(ptr, 16)
    seen = set()
    for xp in (poison_inf(x, inf_columns(F)), poison_nan(x, nan_sources(ptr, idx)), poison_nan(x, hub_last_source(ptr, idx)), x):
        ref = gcn_ref64(ptr, idx, val, xp)
        seen |= set(np.unique(classes(ref)).tolist())
        assert_same_classes(orc.gcn_seq(ptr, idx, val, xp), ref, "gcn_seq")
        assert_same_classes(orc.gcn_grouped(ps, tg, idx, val, xp, V, seg=16), ref, "gcn_grouped")
        assert_same_classes(orc.gcn_mean(ptr, idx, val, xp), gcn_ref64(ptr, idx, val, xp, "mean"), "gcn_mean")
        assert np.all(ref[np.diff(ptr) == 0] == 0)
        fin = classes(ref) == FINITE
        np.testing.assert_allclose(orc.gcn_seq(ptr, idx, val, xp)[fin], ref[fin], rtol=1e-4, atol=1e-4)
    xi = poison_inf(x, inf_columns(F))
    assert_same_classes(orc.gcn_max(ptr, idx, val, xi), gcn_ref64(ptr, idx, val, xi, "max"), "gcn_max")
    np.testing.assert_array_equal(orc.gcn_max(ptr, idx, val, x), gcn_ref64(ptr, idx, val, x, "max").astype(np.float32))
    # signed weights mix the signs (NaN and both Infs occur); positive or implicit weights give +Inf only
    assert seen == ({FINITE, PINF, NAN} if (positive or not with_val) else {FINITE, PINF, NINF, NAN})
    if positive or not with_val:
        got = gcn_ref64(ptr, idx, val, xi)[np.diff(ptr) > 0][:, inf_columns(F)]
        assert np.isposinf(got).all()


@pytest.mark.parametrize("F,H", [(30, 3), (64, 1), (32, 8)])
def test_gat_reference_and_oracle_agree_on_every_class(F, H):
    ptr, idx = gnc.graph.uniform_random_csr(500, 9000, seed=5)
    V = len(ptr) - 1
    x, att = rand((V, F), 1), rand((V, H, 2), 2) * np.float32(0.4)
    nz = np.diff(ptr) > 0
    for xp in (poison_inf(x, inf_columns(F, H)), poison_nan(x, nan_sources(ptr, idx)), x):
        ref = gat_ref64(ptr, idx, att, xp, H)
        got = orc.gat_fused(ptr, idx, att, xp, H)
        assert_same_classes(got, ref, "gat_fused")
        fin = classes(ref) == FINITE
        np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-4, atol=1e-5)
        assert np.all(ref[~nz] == 0) and not np.signbit(ref[~nz]).any()
    ref = gat_ref64(ptr, idx, att, poison_inf(x, inf_columns(F, H)), H)
    assert np.isposinf(ref[nz][:, inf_columns(F, H)]).all() and not np.isnan(ref).any()   # positive weights: +Inf, never NaN


GEMM_SMALLEST = [(129, 33, 7), (300, 32, 32), (127, 64, 128), (200, 33, 96)]


@pytest.mark.parametrize("M,N,K", GEMM_SMALLEST)
def test_gemm_reference_and_oracle_agree_on_every_class(M, N, K):
    A, B = rand((M, K), 1), weights((K, N), 2)
    Ai = gemm_poison_inf(A)
    ref = gemm_ref64(Ai, B)
    assert_same_classes(orc.matmul_nn(Ai, B), ref, "matmul_nn")
    cl = classes(ref)
    rows = np.arange(M)
    clean = (rows % 2 == 0) & (rows % 5 != 0) & (rows != M - 1)
    assert (cl[clean] == FINITE).all() and (cl[~clean] != FINITE).all()     # a non-zero B: every element of a poisoned row
    assert np.array_equal(orc.matmul_nn(Ai, B)[clean], orc.matmul_nn(A, B)[clean])
    An = A.copy()
    An[M // 2, :] = np.nan
    ref = gemm_ref64(An, B)
    assert_same_classes(orc.matmul_nn(An, B), ref, "matmul_nn, a NaN row")
    assert np.isnan(ref[M // 2]).all() and np.isfinite(np.delete(ref, M // 2, 0)).all()
