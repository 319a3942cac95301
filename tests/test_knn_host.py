"""CPU: the kNN graph (include/gnnagg.h section I) without a device -- the surface at every layer, every refusal of gnnagg_knn_run decided
before any device work, gnnagg_knn_supported at the edges of its range, the closed form of ptr, and knn_graph(fused=False) on CPU tensors
against the reference of this file: float64 distances by the same formula and a stable sort (the order of np.lexsort((j, d)))."""
import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_knn_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(x=0x1000, y=0x2000, x_dtype=F32, x_pitch=16, y_pitch=16, n=100, m=80, feat=16, k=20, x_ptr=0x3000, y_ptr=0x4000, num_seg=2, loop=0,
            out_ptr=0x5000, idx=0x6000, dist=0x7000, work=0x8000, work_bytes=1 << 30, splits=3, stream=None)
REFUSALS = [
    ("k 0", dict(k=0), "k ="), ("k 65", dict(k=65), "k ="), ("feat 0", dict(feat=0), "feat"), ("feat 257", dict(feat=257, x_pitch=300, y_pitch=300), "feat"),
    ("negative n", dict(n=-1), "n ="), ("negative m", dict(m=-1), "m ="), ("unknown dtype", dict(x_dtype=2), "x_dtype"),
    ("x pitch below feat", dict(x_pitch=15), "x_pitch"), ("y pitch below feat", dict(y_pitch=15), "y_pitch"),
    ("y null, m != n", dict(y=None), "d_y"), ("one pointer array", dict(y_ptr=None), "d_y_ptr"), ("num_seg 0", dict(num_seg=0), "num_seg"),
    ("splits 17", dict(splits=17), "splits"), ("null x", dict(x=None), "d_x"), ("null out_ptr", dict(out_ptr=None), "d_out_ptr"),
    ("null idx", dict(idx=None), "d_idx"), ("null work", dict(work=None), "d_work"),
    ("work too small", dict(work_bytes=100 * 3 * 20 * 8 + 100 * 4 - 1), "work_bytes"),
]

# the segment layouts of the exact tests: (query segment sizes, candidate segment sizes or None: the candidates are the queries)
LAYOUTS = {"one": ([1], None), "short": ([5], None), "straddle": ([63, 65, 1, 130], None), "cloud": ([300], None),
           "bipartite": ([40, 0, 70, 3], [100, 7, 0, 65])}


def int_points(rows, F, seed):
    """integers in [-4, 4]: exact in bf16 and in every fp32 product and sum up to F = 256, so fp32 is float64 and ties are everywhere"""
    return np.random.default_rng(seed).integers(-4, 5, (rows, F)).astype(np.float32)


def knn_ref(x, y, k, xp, yp, excl):
    """(ptr, idx, dist) in float64: per query the candidates of its segment by (d, j) ascending, the first k"""
    x, y = x.astype(np.float64), y.astype(np.float64)
    ptr, idx, dist = [0], [], []
    for a, b, c, d in zip(xp, xp[1:], yp, yp[1:]):
        dm = np.maximum((x[a:b] ** 2).sum(1)[:, None] + (y[c:d] ** 2).sum(1)[None, :] - 2.0 * x[a:b] @ y[c:d].T, 0.0)
        for i in range(a, b):
            j = np.array([j for j in range(c, d) if not (excl and j == i)], np.int64)
            o = np.lexsort((j, dm[i - a, j - c]))[:k]
            idx.append(j[o])
            dist.append(dm[i - a, j[o] - c])
            ptr.append(ptr[-1] + len(o))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.array(ptr, np.int32), cat(idx, np.int32), cat(dist, np.float64)


def layout_case(name, F, seed=0):
    """(x, y or None, x pointers, y pointers) of a layout as numpy"""
    xs, ys = LAYOUTS[name]
    xp = np.concatenate([[0], np.cumsum(xs)]).astype(np.int32)
    yp = xp if ys is None else np.concatenate([[0], np.cumsum(ys)]).astype(np.int32)
    return int_points(xp[-1], F, seed), (None if ys is None else int_points(yp[-1], F, seed + 1)), xp, yp


def call(**over):
    return gnc.lib().gnnagg_knn_run(*dict(GOOD, **over).values())


def test_the_surface_exists_at_every_layer():
    assert len(_lib.SIGNATURES[NAME][1]) == len(GOOD)
    assert all(n in _lib.SIGNATURES for n in ("gnnagg_knn_supported", "gnnagg_knn_work_bytes"))
    assert all(callable(getattr(gnc, n)) for n in ("knn_graph", "knn_run", "knn_out_ptr", "knn_supported", "knn_prefers_fused", "knn_work_bytes"))
    assert gnc.Block._fields == ("ptr", "idx", "src_nodes", "eid", "num_dst", "num_src", "num_edges")


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_n_0_launches_nothing_and_still_refuses_what_is_wrong():
    none = dict(n=0, x=None, out_ptr=None, idx=None, dist=None, work=None, work_bytes=0)
    assert call(**none) == _lib.OK and call(k=65, **none) == _lib.ERR_ARG


def test_supported_and_work_bytes_at_the_edges_of_the_range():
    # the LDS formula: a query tile of 32 rows, one candidate tile and 32 x (64 + 128) keys fit at feat = 256 for both types
    for dt in (torch.float32, torch.bfloat16):
        assert gnc.knn_supported(256, 64, dt) and gnc.knn_supported(1, 1, dt)
        assert not gnc.knn_supported(257, 64, dt) and not gnc.knn_supported(256, 65, dt) and not gnc.knn_supported(0, 1, dt)
    assert not gnc.knn_supported(64, 20, torch.float16)
    assert gnc.knn_work_bytes(100, 80, 16, 20, torch.float32, 2, splits=3) == 100 * 3 * 20 * 8 + 100 * 4
    assert gnc.knn_work_bytes(100, 80, 16, 20, torch.float32, 2, splits=1) == 0
    with pytest.raises(ValueError, match="k ="):
        gnc.knn_work_bytes(100, 80, 16, 65, torch.float32)


def test_the_wrapper_refuses_before_device_work():
    x = torch.zeros(6, 4)
    with pytest.raises(ValueError, match="fused=True"):
        gnc.knn_graph(x, 2, fused=True)   # CPU tensors have no kernel
    with pytest.raises(ValueError, match="ascend"):
        gnc.knn_graph(x, 2, ptr=torch.tensor([0, 4, 2, 6], dtype=torch.int32), fused=False)
    with pytest.raises(ValueError, match="from 0 to 6"):
        gnc.knn_graph(x, 2, ptr=torch.tensor([0, 4], dtype=torch.int32), fused=False)
    with pytest.raises(ValueError, match="k ="):
        gnc.knn_graph(x, 0, fused=False)
    with pytest.raises(TypeError):
        gnc.knn_graph(x.double(), 2, fused=False)


def test_ptr_is_the_closed_form_of_the_segment_sizes():
    t = lambda a: torch.tensor(a, dtype=torch.int32)
    assert gnc.knn_out_ptr(3, 3, 5, exclude_self=True).tolist() == [0, 2, 4, 6]
    assert gnc.knn_out_ptr(3, 3, 2).tolist() == [0, 2, 4, 6]
    # segments of 2, 0 and 3 queries over 4, 9 and 1 candidates, k = 3: counts 3 3 | | 1 1 1; the row itself excluded: 3 3 | | 0 0 0
    assert gnc.knn_out_ptr(5, 14, 3, t([0, 2, 2, 5]), t([0, 4, 13, 14])).tolist() == [0, 3, 6, 7, 8, 9]
    assert gnc.knn_out_ptr(5, 14, 3, t([0, 2, 2, 5]), t([0, 4, 13, 14]), exclude_self=True).tolist() == [0, 3, 6, 6, 6, 6]


@pytest.mark.parametrize("name,k,loop,dt", [("one", 1, False, torch.float32), ("short", 20, False, torch.bfloat16), ("straddle", 20, True, torch.float32),
                                            ("cloud", 64, False, torch.bfloat16), ("bipartite", 20, False, torch.float32)])
def test_the_composition_on_cpu_tensors_is_the_reference(name, k, loop, dt):
    x, y, xp, yp = layout_case(name, 5)
    rp, ri, rd = knn_ref(x, x if y is None else y, k, xp, yp, y is None and not loop)
    blk, dist = gnc.knn_graph(torch.from_numpy(x).to(dt), k, ptr=torch.from_numpy(xp), y=None if y is None else torch.from_numpy(y).to(dt),
                              y_ptr=None if y is None else torch.from_numpy(yp), loop=loop, return_dist=True, fused=False)
    assert blk.ptr.dtype == blk.idx.dtype == torch.int32 and (blk.num_dst, blk.num_src, blk.num_edges) == (len(x), yp[-1], len(ri))
    assert np.array_equal(blk.ptr.numpy(), rp) and np.array_equal(blk.idx.numpy(), ri) and np.array_equal(dist.numpy().astype(np.float64), rd)
