"""GPU: every kernel at the sizes where its addressing switches ("size switch points").

The library picks another instruction, kernel instantiation or launch recipe when a byte count crosses 2^31 - 1 or 2^32 - 1 or an id
count crosses 2^24.  Each test here restates, in Python, the arithmetic that puts it on the far side of one of those switches, runs
the call on a NaN-poisoned output and compares the COMPLETE output with a plain float64 gather-and-reduce of the same operation.

Data that makes the answer order-independent: features and GEMM operands are integers in [-8, 8], edge values integers in [1, 3], and
degree x 24 < 2^24, so every partial sum in any order is an integer below 2^24: sum / max / ReLU are exact in every association, the
mean is that exact sum cast to fp32 and divided once by the degree, and a wrong address shows as a wrong integer -- no tolerance.
GAT weights are expf, so GAT is compared with a float64 evaluation of the same softmax aggregation under the bound of
tests/test_gpu_fullsize.py: |got - ref| <= 1e-5 (sum_e w_e |x_e| + |ref|) + 1e-30 (w_e the normalised weights)."""
import ctypes

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
GB = 1 << 30
SLOPE = float(np.float32(0.2))   # the slope the kernels hold


# ------------------------------------------------------------------------------------------------------------------ helpers
def need_gb(gb):
    """the guard of tests/test_gpu_fullsize.py: what the test allocates at its peak (an MI355X has 288 GB: never skips there)"""
    free, _ = torch.cuda.mem_get_info()
    if free < gb * GB:
        pytest.skip("needs ~%d GB of free device memory" % gb)


def release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def ints(shape, g, lo=-8, hi=8, dtype=torch.float32):
    """integers in [lo, hi] drawn on the device as int8 and converted: milliseconds for gigabytes"""
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=g, dtype=torch.int8).to(dtype)


def stream():
    """torch's current stream, for the entry points that take one"""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def poisoned(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


class Graph:
    """a CSR on the host (numpy) and on the device, with the row blocks the references walk"""

    def __init__(self, ptr, idx, cols):
        self.ptr_h = np.asarray(ptr, np.int64)
        self.V, self.E, self.cols = len(ptr) - 1, len(idx), int(cols)
        self.deg_h = np.diff(self.ptr_h)
        assert self.ptr_h[-1] == self.E < 2 ** 31 and int(self.deg_h.max()) * 24 < 2 ** 24, "sums stay integers below 2^24"
        self.ptr = torch.from_numpy(self.ptr_h.astype(np.int32)).to(DEV)
        self.idx = idx.to(DEV) if isinstance(idx, torch.Tensor) else torch.from_numpy(np.asarray(idx, np.int32)).to(DEV)
        self.deg = torch.from_numpy(self.deg_h).to(DEV)

    def blocks(self, max_edges=1 << 20, heavy=1 << 14):
        """row ranges [r0, r1) of at most max_edges edges; a row of more than `heavy` edges is a block of its own"""
        cut = {0, self.V}
        for r in np.nonzero(self.deg_h > heavy)[0]:
            cut.update((int(r), int(r) + 1))
        cut = sorted(cut)
        for a, b in zip(cut[:-1], cut[1:]):
            r0 = a
            while r0 < b:
                r1 = int(np.searchsorted(self.ptr_h, self.ptr_h[r0] + max_edges, side="right")) - 1
                r1 = min(b, max(r1, r0 + 1))
                yield r0, r1
                r0 = r1

    def edges(self, r0, r1):
        """(first edge, last edge + 1, source ids as int64, local row of every edge) of rows [r0, r1)"""
        e0, e1 = int(self.ptr_h[r0]), int(self.ptr_h[r1])
        seg = torch.repeat_interleave(torch.arange(r1 - r0, device=DEV), self.deg[r0:r1], output_size=e1 - e0)
        return e0, e1, self.idx[e0:e1].long(), seg


def seg_sum(g, seg, n):
    """per-row sums of the edge rows g (float64): rows of one block"""
    if n == 1:
        return g.sum(0, keepdim=True)
    return torch.zeros((n,) + tuple(g.shape[1:]), dtype=g.dtype, device=DEV).index_add_(0, seg, g)


def gcn_block(G, x, val, r0, r1, op):
    """float64 sum (or max) of val_e x[idx_e] over the edges of every row in [r0, r1): plain indexing arithmetic"""
    e0, e1, ids, seg = G.edges(r0, r1)
    g = x[ids].double()
    if val is not None:
        g.mul_(val[e0:e1].double()[:, None])
    if op != "max":
        return seg_sum(g, seg, r1 - r0)
    if r1 - r0 == 1:
        return g.amax(0, keepdim=True) if e1 > e0 else torch.zeros((1, x.shape[1]), dtype=torch.float64, device=DEV)
    out = torch.full((r1 - r0, x.shape[1]), -float("inf"), dtype=torch.float64, device=DEV)
    out.scatter_reduce_(0, seg[:, None].expand(-1, x.shape[1]), g, "amax", include_self=True)
    out[G.deg[r0:r1] == 0] = 0.0    # rows without edges: 0 (aggr_gcn's initial value is never stored)
    return out


def gcn_expect(G, x, val, r0, r1, reduce="sum", relu=False, base=None, dtype=torch.float32):
    """what rows [r0, r1) of Y must hold, bit for bit"""
    want = gcn_block(G, x, val, r0, r1, "max" if reduce == "max" else "sum")
    assert float(want.abs().max()) < 2 ** 24
    want = want.float()
    if reduce == "mean":
        want = want / G.deg[r0:r1].clamp(min=1).float()[:, None]    # one fp32 division of the exact sum
    if relu:
        want = want.clamp_min(0.0)
    if base is not None:
        want = base[r0:r1] + want       # accumulate: integers again
    return want.to(dtype)               # a bf16 Y is one rounding of the fp32 result


def check_gcn(y, G, x, val, what, **kw):
    for r0, r1 in G.blocks():
        want = gcn_expect(G, x, val, r0, r1, dtype=y.dtype, **kw)
        if not torch.equal(y[r0:r1], want):
            bad = torch.nonzero((y[r0:r1] != want) | torch.isnan(y[r0:r1]))[0]
            raise AssertionError("%s: first wrong element at row %d (degree %d), column %d: got %r, want %r" % (
                what, r0 + int(bad[0]), int(G.deg_h[r0 + int(bad[0])]), int(bad[1]), float(y[r0 + int(bad[0]), int(bad[1])]),
                float(want[int(bad[0]), int(bad[1])])))


def gat_block(G, x, att, H, r0, r1):
    """float64 softmax aggregation of rows [r0, r1): (result, sum_e w_e |x_e| with the normalised weights, un-normalised weights [e, H]).
    att [., H, 2]: [row, h, 0] the centre term, [id, h, 1] the source term; s = centre + source, w = exp(max(s, slope s))"""
    e0, e1, ids, seg = G.edges(r0, r1)
    n, F = r1 - r0, x.shape[1]
    s = att[r0:r1, :, 0].double()[seg] + att[:, :, 1][ids].double()
    w = torch.exp(torch.maximum(s, s * SLOPE))
    g = x[ids].double().view(-1, H, F // H)
    den = seg_sum(w, seg, n)
    den = torch.where(den > 0, den, torch.ones_like(den))[:, :, None]
    num = seg_sum(g * w[:, :, None], seg, n) / den
    scale = seg_sum(g.abs_() * w[:, :, None], seg, n) / den
    return num.view(n, F), scale.view(n, F), w


def check_gat(y, G, x, att, H, what, newval=None, extra_rel=0.0):
    """the condition-aware bound of tests/test_gpu_fullsize.py on every element (NaN fails it); extra_rel: the one rounding of a 16-bit Y"""
    for r0, r1 in G.blocks(max_edges=1 << 19):
        ref, scale, w = gat_block(G, x, att, H, r0, r1)
        bound = 1e-5 * (scale + ref.abs()) + 1e-30
        bound = bound + extra_rel * (ref.abs() + bound)
        err = (y[r0:r1].double() - ref).abs()
        ok = err <= bound
        if not bool(ok.all()):
            bad = torch.nonzero(~ok)[0]
            raise AssertionError("%s: row %d (degree %d), column %d: got %r, want %r, bound %.3g" % (
                what, r0 + int(bad[0]), int(G.deg_h[r0 + int(bad[0])]), int(bad[1]), float(y[r0 + int(bad[0]), int(bad[1])]),
                float(ref[int(bad[0]), int(bad[1])]), float(bound[int(bad[0]), int(bad[1])])))
        if newval is not None:   # un-normalised weights in CSR edge order: the same 1e-5, relative to the weight itself
            e0, e1 = int(G.ptr_h[r0]), int(G.ptr_h[r1])
            assert bool(((newval[e0:e1].double() - w).abs() <= 1e-5 * w + 1e-30).all()), "%s: newval of rows %d .. %d" % (what, r0, r1)


def num_groups(agg, mode="balanced"):
    n = ctypes.c_int(0)
    _lib.check(gnc.lib().gnnagg_num_target(agg._h, {"balanced": _lib.MODE_BALANCED, "scheduled": _lib.MODE_SCHEDULED}[mode], ctypes.byref(n)))
    return n.value


# ------------------------------------------------------------------------------- A. the 2-D blocked order beyond its fast addresses
def rect_graph(V, total_cols, mark, seed, hub_deg=5000):
    """V rows whose sorted neighbor ids reach into total_cols source rows: degrees 100 .. 300, three long rows (first, middle, last),
    medium rows of 900, rows without edges next to them.  Every row takes half of its ids below `mark` and half at or above it, from two
    pools of about equal size (there are only total_cols - mark ids above), so half of the references AND half of the distinct source
    rows lie beyond the mark; the pools hold the ids on either side of it and both ends of the range."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(100, 301, V)
    deg[[0, V // 2, V - 1]] = hub_deg
    deg[[7, V // 3, V - 9]] = 900
    deg[[1, V // 2 + 1, V - 2]] = 0
    ptr = np.zeros(V + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    E = int(ptr[-1])
    n_hi = total_cols - mark
    hi_pool = np.arange(mark, total_cols)
    lo_pool = np.unique(np.concatenate([[0, 1, mark - 1], rng.integers(0, mark, n_hi - 100)]))
    row = np.repeat(np.arange(V), deg)
    pos = np.arange(E) - ptr[row]
    ids = np.where(pos >= deg[row] // 2, hi_pool[rng.integers(0, n_hi, E)], lo_pool[rng.integers(0, len(lo_pool), E)])
    ids = np.sort(row * (1 << 32) + ids) & 0xffffffff     # ascending inside every row: the rows mode qualifies for its chains
    ids[-1] = total_cols - 1
    assert (ids >= mark).mean() >= 0.5, "half of the references lie beyond the mark"
    used = np.unique(ids)
    assert (used >= mark).mean() >= 0.5, "half of the distinct source rows lie beyond the mark"
    G = Graph(ptr, ids.astype(np.int32), total_cols)
    G.val = ints((E,), gen(seed + 1), 1, 3)
    return G


def compacted(G, x, att=None, H=1):
    """the same rows on the source rows they reference only: ids remapped, order inside every row unchanged"""
    used = torch.unique(G.idx.long())
    C = Graph(G.ptr_h, torch.searchsorted(used, G.idx.long()).int(), used.numel())
    C.val = G.val
    if att is None:
        return C, x[used], None
    att_c = torch.zeros((max(G.V, used.numel()), H, 2), device=DEV)
    att_c[:G.V, :, 0] = att[:G.V, :, 0]
    att_c[:used.numel(), :, 1] = att[used, :, 1]
    return C, x[used], att_c


# (name, total_cols, first id whose byte offset in a tile image lies beyond the mark, F, tile_width)
# ids24: ids of 2^24 and more (x_rows fails the test whatever the pitch).  off32: ids below 2^24 and a tile image of 4 GiB.  The library
# always gathers from its column-tiled image of X (plan_tiles, api.hip: "retile" is a constant 1 in the shipped build), so the pitch is
# the tile width, never F: with ids below 2^24 an image reaches 4 GiB only at tiles of 128 floats (2^23 rows) or 256 (2^22 rows); a
# tile of 64 cannot.  One case per lane-group width of k_gcn_span (tile / 4 = 8, 16, 32, 64), a ragged last tile, two tiles.
BLOCKED = [("ids24-group8", 2 ** 24 + 1000, 2 ** 24, 32, 32), ("ids24-group16", 2 ** 24 + 1000, 2 ** 24, 64, 64),
           ("ids24-group16-ragged", 2 ** 24 + 1000, 2 ** 24, 100, 64), ("off32-group32", 2 ** 23 + 1000, 2 ** 23, 128, 128),
           ("off32-group64", 2 ** 22 + 1000, 2 ** 22, 256, 256), ("off32-group64-2tiles", 2 ** 22 + 1000, 2 ** 22, 512, 256)]


def assert_beyond_fast_addresses(name, total_cols, mark, F, tile_w, agg):
    """launch_gcn_span (agg_span.hip): fast = x_rows < 2^24 && xpitch < 2^24 && x_rows * xpitch * 4 < 0xffffffff, and fill_span_args'
    xshift_bytes under the same two marks, with xpitch = the tile width (the retiled image; `agg` has run: its scratch holds that image)"""
    xpitch = tile_w
    fast = total_cols < 2 ** 24 and xpitch < 2 ** 24 and total_cols * xpitch * 4 < 0xffffffff
    assert not fast
    if name.startswith("ids24"):
        assert total_cols >= 2 ** 24 == mark, "ids beyond 24 bits"
    else:
        assert total_cols < 2 ** 24 and total_cols * xpitch * 4 >= 0xffffffff and mark * xpitch * 4 == 2 ** 32, "the image size alone"
    ntiles = -(-F // tile_w)
    # (scratch_bytes sums every scratch buffer, api.hip gnnagg_plan_info; the partial rows here are a few MB: the bulk is the image)
    assert agg.plan_info()["scratch_bytes"] >= total_cols * tile_w * ntiles * 4, "the library gathers from its tiled image: pitch = tile width"


@pytest.mark.parametrize("with_val", [False, True], ids=["unit", "val"])
@pytest.mark.parametrize("name,total_cols,mark,F,tile_w", BLOCKED, ids=[b[0] for b in BLOCKED])
def test_blocked_gcn_beyond_fast_addresses(name, total_cols, mark, F, tile_w, with_val):
    """k_gcn_span<..., FAST_ADDR = false> (64-bit gather addresses) for every lane-group width, with and without val: sum / mean / max /
    ReLU on 8 forced source ranges.  Then the rows mode on the same input, which runs on the row kernels here -- ids24: the chain plan is
    never built (24-bit ids, build_rows_blocked, api.hip); off32: it is built, and run_rows_blocked leaves it because its chains exist
    for tiles of 64 floats only -- : the exact result, and the bits of the same call on the compacted problem.
    (The issue's shape for the 4 GiB image, 2^21 + 1000 rows of 512 floats gathered in place, does not exist in the shipped library: it
    always retiles.  The route is kept and the shape changed.)"""
    need_gb(40)
    V = 4000
    G = rect_graph(V, total_cols, mark, seed=len(name))
    x = ints((total_cols, F), gen(3))
    val = G.val if with_val else None
    agg = gnc.Aggregator_GCN(G.ptr, G.idx, val, F, F)
    agg.set_option("partitions", 8)
    agg.set_option("fast_rows", 0)
    agg.set_option("tile_width", tile_w)
    y = poisoned((V, F))
    for reduce, relu in (("sum", False), ("mean", False), ("max", False), ("sum", True)):
        y.fill_(NAN)
        agg.run(x, y, 128, "balanced", reduce=reduce, relu=relu)
        assert agg.balanced_partitions() == 8 and agg.balanced_partition_columns() == total_cols, "still on the 2-D blocked order"
        check_gcn(y, G, x, val, "%s balanced %s relu=%d" % (name, reduce, relu), reduce=reduce, relu=relu)
    assert_beyond_fast_addresses(name, total_cols, mark, F, tile_w, agg)
    C, xc, _ = compacted(G, x)
    small = gnc.Aggregator_GCN(C.ptr, C.idx, val, F, F)
    small.set_option("fast_rows", 0)
    small.set_option("rows_blocked", 0)
    ys = poisoned((V, F))
    for reduce in ("sum", "mean"):
        y.fill_(NAN)
        ys.fill_(NAN)
        agg.run(x, y, 128, 0, reduce=reduce)
        small.run(xc, ys, 128, 0, reduce=reduce)
        check_gcn(y, G, x, val, "%s rows %s" % (name, reduce), reduce=reduce)
        assert torch.equal(y, ys), "the canonical chains do not depend on where the source rows lie"
    assert (agg.rows_blocked_ranges() >= 2) == name.startswith("off32")
    del x, y, ys, xc, agg, small
    release()


# (name, total_cols, mark id, F, heads, tile_width): heads per tile 1, 4 (ids24, tiles of 64), 2, 1 and 4 (off32)
BLOCKED_GAT = [("ids24-1x64", 2 ** 24 + 1000, 2 ** 24, 64, 1, 64), ("ids24-4x16", 2 ** 24 + 1000, 2 ** 24, 64, 4, 64),
               ("off32-2x64-tile128", 2 ** 23 + 1000, 2 ** 23, 128, 2, 128), ("off32-1x256-tile256", 2 ** 22 + 1000, 2 ** 22, 256, 1, 256),
               ("off32-8x64-tile256", 2 ** 22 + 1000, 2 ** 22, 512, 8, 256)]


@pytest.mark.parametrize("name,total_cols,mark,F,H,tile_w", BLOCKED_GAT, ids=[b[0] for b in BLOCKED_GAT])
def test_blocked_gat_beyond_fast_addresses(name, total_cols, mark, F, H, tile_w):
    """k_gat_span's slow address form through SIZE (xshift_bytes = -1 although the pitch is a power of two), balanced mode on 8 forced
    ranges, and the rows mode (on the row kernels, as in the GCN test); the float64 reference runs on the compacted problem, and the
    rows mode gives the bits of the compacted call.  (8 x 64 at a tile of 64 cannot reach a 4 GiB image with ids below 2^24: see BLOCKED.)"""
    need_gb(40)
    V = 4000
    G = rect_graph(V, total_cols, mark, seed=10 + len(name))
    g = gen(4)
    x = ints((total_cols, F), g)
    att = torch.randn((total_cols, H, 2), device=DEV, generator=g) * 0.5
    C, xc, att_c = compacted(G, x, att, H)
    gat = gnc.Aggregator_GAT(G.ptr, G.idx, F, F)
    gat.set_option("partitions", 8)
    gat.set_option("fast_rows", 0)
    gat.set_option("tile_width", tile_w)
    y = poisoned((V, F))
    gat.run(x, att, y, 128, "balanced", heads=H)
    assert gat.balanced_partitions() == 8 and gat.balanced_partition_columns() == total_cols
    assert_beyond_fast_addresses(name, total_cols, mark, F, tile_w, gat)
    check_gat(y, C, xc, att_c, H, name + " balanced")
    y.fill_(NAN)
    gat.run(x, att, y, 128, 0, heads=H)
    check_gat(y, C, xc, att_c, H, name + " rows")
    assert (gat.rows_blocked_ranges() >= 2) == name.startswith("off32")
    small = gnc.Aggregator_GAT(C.ptr, C.idx, F, F)
    small.set_option("fast_rows", 0)
    small.set_option("rows_blocked", 0)
    ys = poisoned((V, F))
    small.run(xc, att_c, ys, 128, 0, heads=H)
    assert torch.equal(y, ys), "the canonical chains do not depend on where the source rows lie"
    del x, att, y, ys, xc, att_c, gat, small
    release()


@pytest.fixture(scope="module")
def tall_graph():
    """2^23 + 1000 rows of two sorted neighbors among 65 536 source rows; long rows (5000 edges) first, in the middle and last, medium
    rows (900) and rows without edges next to them.  Built on the device."""
    V, cols = 2 ** 23 + 1000, 1 << 16
    deg = np.full(V, 2, np.int64)
    deg[[0, V // 2, V - 1]] = 5000
    deg[[7, V // 3, V - 9]] = 900
    deg[[1, V // 2 + 1, V - 2]] = 0
    ptr = np.zeros(V + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    E = int(ptr[-1])
    row = torch.repeat_interleave(torch.arange(V, device=DEV), torch.from_numpy(deg).to(DEV), output_size=E)
    ids = torch.randint(0, cols, (E,), device=DEV, generator=gen(81))
    ids = torch.sort(row * (1 << 32) + ids).values & 0xffffffff     # ascending inside every row: the rows mode qualifies for its chains
    ids[-1] = cols - 1
    G = Graph(ptr, ids.int(), cols)
    G.val = ints((E,), gen(82), 1, 3)
    return G


@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_rows_mode_leaves_its_chains_at_a_yt_tile_of_2_gib(tall_graph, kind):
    """run_rows_blocked / run_rows_blocked_gat (api.hip): V * 64 * 4 >= 0x7fffffff -- a tile of the Yt image the chains pass through
    would reach 2 GiB -- sends a handle whose chain plan exists (sorted rows, 8 forced ranges, tiles of 64, a small image of X) back
    to the row kernels.  (The other clause of that line, an image of X of 4 GiB at tiles of 64, needs ids of 2^24 and more, and for
    those the plan is never built: it cannot be reached in the shipped library.)  Whole Y against the reference, and the bits of a
    handle with "rows_blocked" = 0."""
    need_gb(16)
    G, F = tall_graph, 64
    assert G.V * 64 * 4 >= 0x7fffffff and G.cols * 64 * 4 < 0xffffffff and G.cols < 2 ** 24
    g = gen(83)
    x = ints((G.cols, F), g)
    y, y2 = poisoned((G.V, F)), poisoned((G.V, F))
    if kind == "gcn":
        a, b = gnc.Aggregator_GCN(G.ptr, G.idx, G.val, F, F), gnc.Aggregator_GCN(G.ptr, G.idx, G.val, F, F)
    else:
        att = torch.randn((G.V, 1, 2), device=DEV, generator=g) * 0.5
        a, b = gnc.Aggregator_GAT(G.ptr, G.idx, F, F), gnc.Aggregator_GAT(G.ptr, G.idx, F, F)
    for h in (a, b):
        h.set_option("partitions", 8)
        h.set_option("fast_rows", 0)
    b.set_option("rows_blocked", 0)
    if kind == "gcn":
        for reduce in ("sum", "mean"):
            y.fill_(NAN)
            y2.fill_(NAN)
            a.run(x, y, 128, 0, reduce=reduce)
            b.run(x, y2, 128, 0, reduce=reduce)
            check_gcn(y, G, x, G.val, "tall rows " + reduce, reduce=reduce)
            assert torch.equal(y, y2)
    else:
        a.run(x, att, y, 128, 0)
        b.run(x, att, y2, 128, 0)
        check_gat(y, G, x, att, 1, "tall gat rows")
        assert torch.equal(y, y2)
    assert a.rows_blocked_ranges() == 8, "the chain plan exists: below the mark this handle runs its chains"
    del x, y, y2, a, b
    release()


@pytest.fixture(scope="module")
def many_groups():
    """34 000 rows x 64 source ranges of 512 columns, one or two neighbors in every range: one group per (row, range)"""
    V, P, W = 34000, 64, 512
    rng = np.random.default_rng(41)
    a = rng.integers(0, W, (V, P, 2))
    a.sort(axis=2)
    ids = a + (np.arange(P) * W)[None, :, None]
    keep = np.ones((V, P, 2), bool)
    keep[:, :, 0] = rng.random((V, P)) < 0.5
    deg = keep.sum(axis=(1, 2))
    ptr = np.zeros(V + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    flat = ids[keep]
    flat[-1] = P * W - 1     # the largest id: the library cuts its ranges from it
    G = Graph(ptr, flat.astype(np.int32), P * W)
    G.val = ints((G.E,), gen(42), 1, 3)
    return G


@pytest.mark.parametrize("kind", ["gcn-sum-val", "gcn-max", "gat-4x64", "gat-32x8-descriptors"])
def test_partial_tile_of_2_gib(many_groups, kind):
    """ptile_bytes = 0: a tile of partial rows reaches 2 GiB and the streaming buffer stores through its descriptor give way to plain
    stores; every row has 64 groups and meets in the ordered combine.  The span kernels (fill_span_args, agg_span.hip) for GCN and for GAT
    heads that tile; 32 heads of 8 columns do not tile 256-float tiles (gat_span_tiles, common.h: 32 heads per tile), so that case runs
    the tiled plan kernel on the descriptor form of the order (plan_grid, kernel_util.cuh)."""
    need_gb(12)
    G, F, TW = many_groups, 256, 256
    g = gen(43)
    x = ints((G.cols, F), g)
    y = poisoned((G.V, F))
    H = {"gat-4x64": 4, "gat-32x8-descriptors": 32}.get(kind, 0)
    if H:
        assert (TW // (F // H) in (1, 2, 4, 8)) == (kind == "gat-4x64"), "heads per tile the span kernel has an instantiation for"
        att = torch.randn((max(G.V, G.cols), H, 2), device=DEV, generator=g) * 0.5   # centre terms by row, source terms by id
        agg = gnc.Aggregator_GAT(G.ptr, G.idx, F, F)
    else:
        val = G.val if kind == "gcn-sum-val" else None
        agg = gnc.Aggregator_GCN(G.ptr, G.idx, val, F, F)
    agg.set_option("partitions", 64)
    agg.set_option("tile_width", TW)
    if H:
        agg.run(x, att, y, 128, "balanced", heads=H)
        check_gat(y, G, x, att, H, kind)
    else:
        reduce = "max" if kind == "gcn-max" else "sum"
        agg.run(x, y, 128, "balanced", reduce=reduce)
        check_gcn(y, G, x, val, kind, reduce=reduce)
    assert agg.balanced_partitions() == 64
    n_groups = num_groups(agg)     # one partial row per group (span form) or per group of a row with several (descriptor form): every row has 64
    assert n_groups >= 64 * G.V and n_groups * TW * 4 >= 2 ** 31 - 1, "tb = n_groups * ppitch * 4 >= 0x7fffffff: ptile_bytes = 0"
    # (scratch_bytes sums every scratch buffer, api.hip gnnagg_plan_info: a weaker statement than the product above, which is the
    # switch's own arithmetic; it shows that the handle was not demoted to an order without these partial rows)
    assert agg.plan_info()["scratch_bytes"] >= 2 ** 31 - 1
    del x, y, agg
    release()


# ------------------------------------------------------------------------------- B. chunked plan, partial scratch of 2 GiB and more
B_F = 256   # pick_geometry (kernel_util.cuh): 16-byte lanes in groups of at most 64 -- 256 floats is the widest row of ONE column tile


@pytest.fixture(scope="module")
def hub_scratch_graph():
    """52 rows of 660 000 edges (first and last row among them) between rows of 0 .. 16 edges: with schedule_balanced(1) a row of more
    than 16 edges is cut into segments of 16, each with a partial row in scratch"""
    V, cols, hubs, hub_deg = 2000, 1 << 20, 52, 660000
    rng = np.random.default_rng(51)
    deg = rng.integers(0, 17, V)
    hub_rows = np.unique(np.concatenate([[0, V - 1], rng.choice(np.arange(1, V - 1), hubs - 2, replace=False)]))
    deg[hub_rows] = hub_deg
    ptr = np.zeros(V + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    G = Graph(ptr, torch.randint(0, cols, (int(ptr[-1]),), device=DEV, generator=gen(52), dtype=torch.int32), cols)
    G.val = ints((G.E,), gen(53), 1, 3)
    G.n_slots = int(sum(-(-d // 16) for d in deg if d > 16))
    # launch_gcn_plan (agg_gcn.hip) / launch_gat_plan (agg_gat.hip): pbytes = n_slots * F * 4 >= 0x7fffffff takes the hubs out of the in-kernel fold
    assert G.n_slots * B_F * 4 >= 0x7fffffff
    return G


def test_chunked_plan_gcn_partial_scratch_of_2_gib(hub_scratch_graph):
    """hub rows leave the in-kernel fold for the ordered combine BECAUSE OF SIZE, with partial-row offsets beyond 2^31 bytes (the last
    row is a hub: its partial rows are the last ones).  Below the mark this configuration (one column tile) folds in the kernel."""
    need_gb(16)
    G, F = hub_scratch_graph, B_F
    x = ints((G.cols, F), gen(54))
    agg = gnc.Aggregator_GCN(G.ptr, G.idx, G.val, F, F)
    agg.schedule_balanced(1)
    y = poisoned((G.V, F))
    for reduce, relu in (("sum", False), ("mean", False), ("max", False), ("sum", True)):
        y.fill_(NAN)
        agg.run(x, y, 128, "balanced", reduce=reduce, relu=relu)
        check_gcn(y, G, x, G.val, "chunked plan %s relu=%d" % (reduce, relu), reduce=reduce, relu=relu)
    assert agg.balanced_partitions() == 0 and agg.balanced_params() == (1, 16)
    # (the sum of every scratch buffer: weaker than the fixture's assertion on n_slots * F * 4, the switch's own arithmetic)
    assert agg.plan_info()["scratch_bytes"] >= 2 ** 31 - 1
    # typed: bf16 X (exact: the same integers), fp32 and bf16 Y; the bf16 Y is one rounding of the fp32 Y
    xb = x.to(BF)
    y32, yb = poisoned((G.V, F)), poisoned((G.V, F), BF)
    agg.run(xb, y32, 128, "balanced")
    check_gcn(y32, G, x, G.val, "chunked plan bf16 -> fp32")
    agg.run(xb, yb, 128, "balanced")
    check_gcn(yb, G, x, G.val, "chunked plan bf16 -> bf16")
    assert torch.equal(yb, y32.to(BF))
    del x, xb, y, y32, yb, agg
    release()


@pytest.mark.parametrize("H", [1, 8])
def test_chunked_plan_gat_partial_scratch_of_2_gib(hub_scratch_graph, H):
    need_gb(16)
    G, F = hub_scratch_graph, B_F
    g = gen(55)
    x = ints((G.cols, F), g)
    att = torch.randn((G.cols, H, 2), device=DEV, generator=g) * 0.5
    gat = gnc.Aggregator_GAT(G.ptr, G.idx, F, F)
    gat.schedule_balanced(1)
    y = poisoned((G.V, F))
    newval = poisoned((G.E, H)) if H == 8 else None
    gat.run(x, att, y, 128, "balanced", heads=H, newval=newval)
    assert gat.balanced_partitions() == 0 and gat.plan_info()["scratch_bytes"] >= 2 ** 31 - 1
    check_gat(y, G, x, att, H, "chunked plan gat %d heads" % H, newval=newval)
    del x, att, y, newval, gat
    release()


# ------------------------------------------------------------------------ C. outputs and destinations beyond 2^31 elements
C_V, C_F = 4_300_000, 512
C_MARK = 2 ** 31 // C_F     # the first row whose elements lie beyond 2^31


@pytest.fixture(scope="module")
def big_graph():
    """4.3 M rows of two neighbors (tests/test_gpu_fullsize.py), 20 hub rows (20 000 .. 60 000 edges), 200 medium rows (200 .. 900) and
    200 rows without edges; 12 / 120 / 120 of them above row 2^31 / F, the first row a hub, the last a hub, rows without edges next to
    them.  Every row takes half of its ids below that row and half at or above it.  (The two-neighbor rows fill the whole range: 105 696 of
    them lie above the mark.)"""
    V, M = C_V, C_MARK
    assert V * C_F > 2 ** 31
    rng = np.random.default_rng(61)
    deg = np.full(V, 2, np.int64)
    lo = rng.choice(np.arange(2, M), 8 + 80 + 80, replace=False)
    hi = rng.choice(np.arange(M, V - 2), 11 + 120 + 120, replace=False)
    hubs = np.concatenate([[0], lo[:7], [V - 1], hi[:11]])
    med = np.concatenate([lo[8:88], hi[11:131]])
    empty = np.concatenate([[1], lo[89:168], [V - 2], hi[132:251]])
    deg[hubs] = rng.integers(20000, 60001, len(hubs))
    deg[med] = rng.integers(200, 901, len(med))
    deg[empty] = 0
    for rows in (hubs, med, empty):
        assert (rows >= M).mean() >= 0.5, "at least half of each row class writes beyond the mark"
    ptr = np.zeros(V + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    E = int(ptr[-1])
    row = np.repeat(np.arange(V), deg)
    pos = np.arange(E) - ptr[row]
    ids = np.where(pos >= deg[row] // 2, rng.integers(M, V, E), rng.integers(0, M, E))
    ids = np.sort(row * (1 << 32) + ids) & 0xffffffff
    assert (ids >= M).mean() >= 0.5, "half of all neighbor ids read beyond the mark"
    G = Graph(ptr, ids.astype(np.int32), V)
    G.val = ints((E,), gen(62), 1, 3)
    return G


@pytest.mark.parametrize("mode", ["balanced", "rows"])
def test_big_gcn_fp32(big_graph, mode):
    """Y of 8.8 GB (plain stores instead of the write-through buffer stores, agg_gcn.hip `a.wt`), hub / medium / empty rows on both sides
    of the mark: max, ReLU, mean, val present; accumulate onto a non-zero Y (balanced mode only)"""
    need_gb(45)
    G = big_graph
    assert G.V * C_F * 4 >= 0x7fffffff
    x = ints((G.V, C_F), gen(63))
    agg = gnc.Aggregator_GCN(G.ptr, G.idx, G.val, C_F, C_F)
    agg.set_option("fast_rows", 0)
    y = poisoned((G.V, C_F))
    m = 0 if mode == "rows" else mode
    for reduce, relu in (("max", False), ("sum", True), ("mean", False)):
        y.fill_(NAN)
        agg.run(x, y, 128, m, reduce=reduce, relu=relu)
        check_gcn(y, G, x, G.val, "%s %s relu=%d" % (mode, reduce, relu), reduce=reduce, relu=relu)
    if mode == "balanced":
        base = ints((G.V, C_F), gen(64))
        y.copy_(base)
        agg.run(x, y, 128, m, accumulate=True)
        check_gcn(y, G, x, G.val, "balanced accumulate", base=base)
        del base
    del x, y, agg
    release()


@pytest.mark.parametrize("xdt,ydt", [(BF, BF), (BF, torch.float32), (torch.float32, BF)], ids=["bf16-bf16", "bf16-fp32", "fp32-bf16"])
def test_big_gcn_typed(big_graph, xdt, ydt):
    """typed launches past 2^31 elements; a bf16 Y of 4.4 GB lies beyond the write-through limit too"""
    need_gb(30)
    G = big_graph
    assert G.V * C_F * 2 >= 0x7fffffff
    x = ints((G.V, C_F), gen(65), dtype=xdt)
    agg = gnc.Aggregator_GCN(G.ptr, G.idx, None, C_F, C_F)
    y = poisoned((G.V, C_F), ydt)
    agg.run(x, y, 128, "balanced")
    check_gcn(y, G, x, None, "typed balanced")     # (bf16: one rounding of the exact fp32 sum)
    del x, y, agg
    release()


@pytest.mark.parametrize("fast_scheduled", [1, 0])
def test_big_gcn_scheduled_neighbor_grouping(big_graph, fast_scheduled):
    """scheduled mode with groups of 32 neighbors: the balanced order in its place (default) and the user's groups"""
    need_gb(45)
    G = big_graph
    x = ints((G.V, C_F), gen(66))
    agg = gnc.Aggregator_GCN(G.ptr, G.idx, G.val, C_F, C_F)
    agg.set_option("fast_scheduled", fast_scheduled)
    agg.schedule(gnc.Schedule.neighbor_grouping, [32])
    y = poisoned((G.V, C_F))
    agg.run(x, y, 128, 1)
    check_gcn(y, G, x, G.val, "scheduled, fast_scheduled=%d" % fast_scheduled)
    del x, y, agg
    release()


@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("mode", ["balanced", "rows"])
def test_big_gat(big_graph, mode, H):
    """1 x 512 and 8 x 64 on the big graph, the whole Y under the bound; balanced mode also bf16 -> fp32 and bf16 -> bf16 (the typed entry
    refuses the canonical rows mode: include/gnnagg.h)"""
    need_gb(40)
    G = big_graph
    g = gen(67)
    x = ints((G.V, C_F), g)
    att = torch.randn((G.V, H, 2), device=DEV, generator=g) * 0.5
    gat = gnc.Aggregator_GAT(G.ptr, G.idx, C_F, C_F)
    gat.set_option("fast_rows", 0)
    y = poisoned((G.V, C_F))
    gat.run(x, att, y, 128, 0 if mode == "rows" else mode, heads=H)
    check_gat(y, G, x, att, H, "gat %s %d heads" % (mode, H))
    if mode == "balanced":   # bf16 -> bf16: the fp32 result of the same integers, rounded once
        xb = x.to(BF)
        del x
        y32 = y
        y32.fill_(NAN)
        gat.run(xb, att, y32, 128, mode, heads=H)
        check_gat(y32, G, xb, att, H, "gat bf16 -> fp32 %d heads" % H)
        yb = poisoned((G.V, C_F), BF)
        gat.run(xb, att, yb, 128, mode, heads=H)
        check_gat(yb, G, xb, att, H, "gat bf16 -> bf16 %d heads" % H, extra_rel=2.0 ** -8)   # the unit roundoff of bf16 (8 significand bits)
        assert torch.equal(yb, y32.to(BF))
        del xb, yb, y32
    else:
        del x
    del att, y, gat
    release()


@pytest.mark.parametrize("mode", ["balanced", "rows"])
def test_big_run_with_nn(big_graph, mode):
    """both outputs of run_with_nn: vout = A x, transformed = vout @ weight (OUT = 32, weights in [-1, 1])"""
    need_gb(45)
    G, OUT = big_graph, 32
    g = gen(68)
    x = ints((G.V, C_F), g)
    w = ints((C_F, OUT), g, -1, 1)
    agg = gnc.Aggregator_GCN(G.ptr, G.idx, None, C_F, C_F)
    agg.set_option("fast_rows", 0)
    y, t = poisoned((G.V, C_F)), poisoned((G.V, OUT))
    agg.run_with_nn(x, y, w, t, 128, 0 if mode == "rows" else mode)
    check_gcn(y, G, x, None, "run_with_nn vout, " + mode)
    for r0, r1 in G.blocks():
        want = gcn_block(G, x, None, r0, r1, "sum")
        assert float((want.abs() @ w.abs().double()).max()) < 2 ** 24, "every partial sum of the product is an integer below 2^24"
        assert torch.equal(t[r0:r1], (want @ w.double()).float()), "transformed, rows %d .. %d" % (r0, r1)
    del x, y, t, agg
    release()


def test_big_edgewise_and_spmm_naive(big_graph):
    """(the seconds this takes are gnnagg_spmm_naive itself: the reference's thread-per-row baseline walks a hub row of 60 000 edges x 512
    columns in one thread)"""
    need_gb(45)
    G = big_graph
    x = ints((G.V, C_F), gen(69))
    agg = gnc.Aggregator_GCN(G.ptr, G.idx, G.val, C_F, C_F)
    y = poisoned((G.V, C_F))
    agg.runEdgeWise(x, y)
    check_gcn(y, G, x, G.val, "runEdgeWise")
    y.fill_(NAN)
    _lib.check(gnc.lib().gnnagg_spmm_naive(G.ptr.data_ptr(), G.idx.data_ptr(), G.val.data_ptr(), x.data_ptr(), y.data_ptr(), G.V, C_F, stream()))
    empty = G.deg == 0
    assert bool(torch.isnan(y[empty]).all()), "rows without edges stay untouched (spmm.h:236-237)"
    y[empty] = 0.0
    check_gcn(y, G, x, G.val, "spmm_naive")
    del x, y, agg
    release()


def test_big_pack_rows_and_validate_reordered():
    """gnnagg_pack_rows with ids that permute all rows (8.8 GB out), then gnnagg_validate_reordered of the packed rows against the
    source through the same map: 0 mismatches, and exactly the k planted beyond element 2^31"""
    need_gb(30)
    V, F = C_V, C_F
    g = gen(70)
    x = ints((V, F), g)
    perm = torch.randperm(V, device=DEV, generator=g).int()
    out = poisoned((V, F))
    _lib.check(gnc.lib().gnnagg_pack_rows(x.data_ptr(), perm.data_ptr(), V, F, out.data_ptr(), stream()))
    step = 1 << 20
    for r0 in range(0, V, step):
        assert torch.equal(out[r0:r0 + step], x[perm[r0:r0 + step].long()]), "rows %d .." % r0
    n = ctypes.c_int(-1)
    _lib.check(gnc.lib().gnnagg_validate_reordered(out.data_ptr(), x.data_ptr(), perm.data_ptr(), V, F, ctypes.byref(n), stream()))
    assert n.value == 0
    flat = out.view(-1)
    spots = torch.tensor([2 ** 31, 2 ** 31 + 1, 2 ** 31 + 12345, V * F - 1, V * F - F, (C_MARK + 1000) * F + 7, 2 ** 31 + 2 ** 20], device=DEV)
    assert int(spots.min()) >= 2 ** 31
    flat[spots] += 100.0
    _lib.check(gnc.lib().gnnagg_validate_reordered(out.data_ptr(), x.data_ptr(), perm.data_ptr(), V, F, ctypes.byref(n), stream()))
    assert n.value == spots.numel()
    del x, out, flat, perm
    release()


def test_big_pack_rows2_and_unpack_rows2():
    """the GAT halo pack: [x row | 2 x 8 attention terms] per id, more than 2^31 elements in and out, and its inverse"""
    need_gb(45)
    V, F, A = C_V, C_F, 16
    g = gen(71)
    x = ints((V, F), g)
    att = ints((V, A), g)
    perm = torch.randperm(V, device=DEV, generator=g).int()
    out = poisoned((V, F + A))
    _lib.check(gnc.lib().gnnagg_pack_rows2(x.data_ptr(), att.data_ptr(), perm.data_ptr(), V, F, A, out.data_ptr(), stream()))
    step = 1 << 20
    for r0 in range(0, V, step):
        ids = perm[r0:r0 + step].long()
        assert torch.equal(out[r0:r0 + step, :F], x[ids]) and torch.equal(out[r0:r0 + step, F:], att[ids]), "rows %d .." % r0
    x.fill_(NAN)
    att.fill_(NAN)
    _lib.check(gnc.lib().gnnagg_unpack_rows2(out.data_ptr(), V, F, A, x.data_ptr(), att.data_ptr(), stream()))
    for r0 in range(0, V, step):
        assert torch.equal(x[r0:r0 + step], out[r0:r0 + step, :F]) and torch.equal(att[r0:r0 + step], out[r0:r0 + step, F:]), "rows %d .." % r0
    del x, att, out, perm
    release()


# ------------------------------------------------------------------------------------ D. fp32 dense GEMM beyond 4 GiB, every route
def gemm_route(M, K, N, a_ptr, b_ptr):
    """launch_dense_nn's route table (dense_f32.hip) restated: the kernel a shape lands on"""
    if 64 < K <= 128 and K % 4 == 0 and M >= 500000 and a_ptr % 16 == 0:
        return "tall"
    if N > 64 and M >= 1024:
        bvec = N % 4 == 0 and b_ptr % 16 == 0
        av = 1 if not bvec else 4 if (K % 4 == 0 and a_ptr % 16 == 0) else 2 if (K % 2 == 0 and a_ptr % 8 == 0) else 1
        lean = N % 128 == 0 and bvec and av >= 2
        if lean and av == 4 and K % 32 == 0:
            return "ahead<4>"
        if lean:
            return "ahead<2>" if av == 2 else "lean<4>"
        return "strip<%d>" % av
    if K % 32 == 0 and K <= 128 and a_ptr % 16 == 0:
        return "up<%d>" % (2 if 32 < N <= 64 else 1)
    return "plain"


GEMMS = [("tall", 2 ** 24 + 33, 128, 8, 0), ("tall", 2 ** 24 + 33, 128, 33, 0),
         ("ahead<4>", 2 ** 22 + 33, 512, 128, 0), ("ahead<4>", 2 ** 22 + 33, 512, 256, 0),
         ("ahead<2>", 2 ** 22 + 33, 512, 128, 2), ("ahead<2>", 2 ** 22 + 33, 512, 256, 2),
         ("lean<4>", 2 ** 22 + 33, 516, 128, 0), ("strip<1>", 2 ** 22 + 33, 512, 129, 0),
         ("up<1>", 2 ** 25 + 33, 64, 32, 0), ("up<2>", 2 ** 25 + 33, 64, 64, 0),
         ("plain", 2 ** 22 + 33, 513, 33, 0), ("ahead<4>-typed-entry", 2 ** 22 + 33, 512, 128, 0)]


@pytest.mark.parametrize("route,M,K,N,a_off", GEMMS, ids=["%s-%dx%dx%d-off%d" % (g[0], g[1], g[2], g[3], g[4]) for g in GEMMS])
def test_fp32_gemm_operands_beyond_4_gib(route, M, K, N, a_off):
    """A of more than 4 GiB on every route of launch_dense_nn: the buffer descriptors rebased per workgroup saturate at 0xfffffffc bytes
    left (C's too at N = 256).  a_off = 2: A carved two floats into its buffer (8-byte, not 16-byte aligned rows).  The whole C against
    the float64 product, row block by row block; integer operands, |sums| <= 64 K < 2^24: exact."""
    need_gb(30)
    assert M * K * 4 > 0xfffffffc, "A beyond the descriptor clamp"
    if N == 256:
        assert M * N * 4 > 0xfffffffc, "C beyond the descriptor clamp"
    assert 64 * K < 2 ** 24
    g = gen(M % 1000 + K + N)
    buf = ints((M * K + 8,), g)
    A = buf[a_off:a_off + M * K].view(M, K)
    B = ints((K, N), g)
    assert A.data_ptr() % 16 == 4 * a_off and B.data_ptr() % 16 == 0
    assert gemm_route(M, K, N, A.data_ptr(), B.data_ptr()) == route.split("-")[0]
    C = poisoned((M, N))
    if route.endswith("typed-entry"):
        f32 = _lib.DTYPE_F32
        _lib.check(gnc.lib().gnnagg_matmul_nn_typed(ctypes.c_void_p(A.data_ptr()), f32, ctypes.c_void_p(B.data_ptr()), f32, ctypes.c_void_p(C.data_ptr()),
                                                    f32, M, N, K, stream()))
    else:
        assert gnc.matmul_NN(A, B, C) is C
    B64 = B.double()
    for r0 in range(0, M, 1 << 20):
        want = (A[r0:r0 + (1 << 20)].double() @ B64).float()
        if not torch.equal(C[r0:r0 + (1 << 20)], want):
            bad = torch.nonzero((C[r0:r0 + (1 << 20)] != want) | torch.isnan(C[r0:r0 + (1 << 20)]))[0]
            raise AssertionError("%s: first wrong element at row %d, column %d: got %r, want %r" % (
                route, r0 + int(bad[0]), int(bad[1]), float(C[r0 + int(bad[0]), int(bad[1])]), float(want[int(bad[0]), int(bad[1])])))
    del buf, A, B, B64, C, want
    release()
