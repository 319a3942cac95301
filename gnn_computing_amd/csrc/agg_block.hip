// agg_block.hip -- the GCN / SAGE aggregation of ONE sampled block in one launch: gnnagg_block_gcn_run (include/gnnagg.h section F).
//
// A handle's plan is amortised over thousands of runs on a fixed graph; a block is used once, and after sampling its rows hold at most
// `fanout` edges -- there is nothing to balance.  k_block_gcn walks the block's own CSR: one lane group per (destination row, column
// tile), the chain of chain_edges (kernel_util.cuh) in CSR order, so the bits are those of a handle's rows mode.  While a lane loads
// an edge's id it can translate it through src_nodes (and fetch val through eid): the input layer then reads the full feature matrix
// in place and the [num_src, F] gathered copy of it is never made.
//
// A row of any length is walked by its one lane group (the chain cannot be split without changing its bits).  For blocks taken with
// fanout = -1 that hold hub rows, a handle's rows mode (k_gcn_rows_long) remains the fast path.
//
// No atomics, no LDS, no scratch: the result is a function of the arguments.
#include "kernel_util.cuh"

namespace gnnagg {
namespace {

struct BlockArgs {
    const int *ptr, *idx, *src, *eid;
    const float *val;
    const void *x;
    void *y, *xdst;
    long long xpitch;   // elements between rows of x
    int num_dst, feat, ntiles, mean, relu, y_bf16, yvec;
};

// chain_edges with the two maps of a block: the row of x of edge p is src[idx[p]] (src given) and its weight val[eid[p]] (eid
// given).  Lane j of the group loads idx[p] of its edge of the window and then does the dependent loads; the next window's
// metadata -- maps applied -- is prefetched while this window's gathers and FMAs run.  Ids and weights are broadcast inside the
// group, UNROLL row gathers are issued before the first FMA, lanes with col_ok == false still carry metadata, and no padding
// lane ever multiplies a real source row by zero.  MAPPED = false: neither map, and no test for one.
template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, int UNROLL, typename TX>
__device__ __forceinline__ void chain_block_edges(float (&acc)[VEC], int beg, int end, int lane, bool col_ok,
                                                  const int *__restrict__ idx, const int *__restrict__ src,
                                                  const float *__restrict__ val, const int *__restrict__ eid,
                                                  const TX *__restrict__ xcol, long long pitch)
{
    auto edge_meta = [&](int p, int &s, float &w) {
        s = idx[p];
        if constexpr (MAPPED) {
            if (src) s = src[s];
            if (val) w = val[eid ? eid[p] : p];
        } else {
            if (val) w = val[p];
        }
    };
    int my_s = 0;
    float my_w = 1.0f;
    if (beg + lane < end) edge_meta(beg + lane, my_s, my_w);
    for (int cb = beg; cb < end; cb += GROUP) {
        int nx_s = 0;
        float nx_w = 1.0f;
        if (cb + GROUP + lane < end) edge_meta(cb + GROUP + lane, nx_s, nx_w);
        const int n = end - cb < GROUP ? end - cb : GROUP;
        for (int j = 0; j < n; j += UNROLL) {
            int s[UNROLL];
            float w[UNROLL];
            Pack<VEC, TX> xv[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                s[u] = __shfl(my_s, j + u, GROUP);
                w[u] = __shfl(my_w, j + u, GROUP);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if (j + u < n && col_ok) xv[u] = load_pack<VEC>(xcol + (size_t)s[u] * (size_t)pitch);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if (j + u < n && col_ok) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        if (IS_MAX) {
                            const float p = xv[u].at(k) * w[u];
                            acc[k] = p > acc[k] ? p : acc[k];
                        } else {
                            acc[k] = __builtin_fmaf(xv[u].at(k), w[u], acc[k]);
                        }
                    }
                }
        }
        my_s = nx_s;
        my_w = nx_w;
    }
}

// a lane's loaded elements back to memory as they are (x_dst; the launch picks lanes no wider than x_dst's alignment)
template <int VEC, typename TX>
__device__ __forceinline__ void store_raw_pack(TX *p, const Pack<VEC, TX> &v)
{
    if constexpr (std::is_same<TX, __bf16>::value) {
        if constexpr (VEC == 8) *reinterpret_cast<uint4 *>(p) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
        else if constexpr (VEC == 4) *reinterpret_cast<uint2 *>(p) = make_uint2(v.w[0], v.w[1]);
        else if constexpr (VEC == 2) *reinterpret_cast<unsigned *>(p) = v.w[0];
        else *reinterpret_cast<unsigned short *>(p) = (unsigned short)v.w[0];
    } else {
        store_pack<VEC>(p, v.v);
    }
}

// 8 lane groups per workgroup (block_of), one (row, column tile) each; the tiles of a row block are adjacent in the grid
template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, int UNROLL, typename TX>
__global__ __launch_bounds__(block_of<GROUP>()) void k_block_gcn(const BlockArgs a)
{
    constexpr int GPB = block_of<GROUP>() / GROUP;
    const int lane = threadIdx.x % GROUP, grp = threadIdx.x / GROUP;
    const int tile = (int)blockIdx.x % a.ntiles;
    const int row = ((int)blockIdx.x / a.ntiles) * GPB + grp;
    if (row >= a.num_dst) return;
    const int F = a.feat;
    const int col = (tile * GROUP + lane) * VEC;
    const bool col_ok = col < F;
    const TX *__restrict__ xcol = static_cast<const TX *>(a.x) + col;
    const int beg = a.ptr[row], end = a.ptr[row + 1];
    Pack<VEC, TX> self;
    if constexpr (MAPPED) {
        if (a.xdst && col_ok) self = load_pack<VEC>(xcol + (size_t)a.src[row] * (size_t)a.xpitch);
    }
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = IS_MAX ? -INFINITY : 0.0f;
    chain_block_edges<VEC, GROUP, IS_MAX, MAPPED, UNROLL, TX>(acc, beg, end, lane, col_ok, a.idx, a.src, a.val, a.eid, xcol, a.xpitch);
    if (!col_ok) return;
    if constexpr (MAPPED) {
        if (a.xdst) store_raw_pack<VEC, TX>(static_cast<TX *>(a.xdst) + (size_t)row * F + col, self);
    }
    if (beg == end) {  // no edges: 0, whatever the reduce
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
    } else {
        finish_gcn_row<VEC, IS_MAX>(acc, end - beg, row, nullptr, a.mean, 0, a.relu, nullptr);
    }
    store_y_typed<VEC>(a.y, a.y_bf16, a.yvec, 0, 0u, (size_t)row * F + col, acc);
}

// Gathers in flight per lane group: 8 (kUnroll) everywhere.  A block's rows are short and few, the launch rarely fills the device, and
// what limits it is the latency of the id -> (src_nodes) -> row chain, not the waves per SIMD the registers leave (DESIGN.md "Block
// aggregation" has every instantiation's registers).
template <int VEC, int GROUP, typename TX>
static void launch_block(const BlockArgs &a, int is_max, int mapped, hipStream_t st)
{
    constexpr int B = block_of<GROUP>();
    const dim3 grid((unsigned)(ceil_div(a.num_dst, B / GROUP) * a.ntiles)), block(B);
    if (is_max) {
        if (mapped) hipLaunchKernelGGL((k_block_gcn<VEC, GROUP, true, true, kUnroll, TX>), grid, block, 0, st, a);
        else        hipLaunchKernelGGL((k_block_gcn<VEC, GROUP, true, false, kUnroll, TX>), grid, block, 0, st, a);
    } else {
        if (mapped) hipLaunchKernelGGL((k_block_gcn<VEC, GROUP, false, true, kUnroll, TX>), grid, block, 0, st, a);
        else        hipLaunchKernelGGL((k_block_gcn<VEC, GROUP, false, false, kUnroll, TX>), grid, block, 0, st, a);
    }
}

static long long gcd_ll(long long a, long long b)
{
    while (b) { const long long t = a % b; a = b; b = t; }
    return a;
}

static int block_gcn_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const float *val, const int *eid, const void *x,
                         int x_dtype, long long x_pitch, void *y, int y_dtype, void *x_dst, int feat, int reduce, int flags, void *stream)
{
    static const char *who = "gnnagg_block_gcn_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    if (num_dst < 0) return bad("num_dst = " + std::to_string(num_dst) + " is negative");
    if (feat < 1) return bad("feat = " + std::to_string(feat) + " must be >= 1");
    if (x_pitch < feat) return bad("x_pitch = " + std::to_string(x_pitch) + " is below feat = " + std::to_string(feat));
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (y_dtype != GNNAGG_DTYPE_F32 && y_dtype != GNNAGG_DTYPE_BF16) return bad("unknown y_dtype " + std::to_string(y_dtype));
    if (reduce != GNNAGG_REDUCE_SUM && reduce != GNNAGG_REDUCE_MEAN && reduce != GNNAGG_REDUCE_MAX)
        return bad("unknown reduce " + std::to_string(reduce));
    if (flags & ~GNNAGG_FLAG_RELU) return bad("flags = " + std::to_string(flags) + ": GNNAGG_FLAG_RELU is the only flag");
    if (eid && !val) return bad("d_eid needs d_val (d_eid indexes it)");
    if (x_dst && !src) return bad("d_x_dst needs d_src_nodes (x_dst[i] = x[d_src_nodes[i]])");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!x) return bad("d_x is null");
        if (!y) return bad("d_y is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16, y16 = y_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: a divisor of feat AND of the pitch (every row of x then has the alignment of the first), no wider than the
    // alignment of x and of x_dst (same element type; their addresses OR-ed have the alignment of the worse one).  y has its own class.
    const int fp = (int)gcd_ll(feat, x_pitch);
    const void *xa = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_dst));
    const Geometry g = x16 ? typed_geometry(feat, xa, 2, fp) : pick_geometry(feat, xa, y16 ? nullptr : y, nullptr, fp);
    BlockArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.eid = eid; a.val = val;
    a.x = x; a.y = y; a.xdst = x_dst; a.xpitch = x_pitch;
    a.num_dst = num_dst; a.feat = feat; a.ntiles = g.ntiles;
    a.mean = reduce == GNNAGG_REDUCE_MEAN; a.relu = (flags & GNNAGG_FLAG_RELU) != 0;
    a.y_bf16 = y16; a.yvec = align_class(feat, y, y16 ? 2 : 4, g.vec);
    const int is_max = reduce == GNNAGG_REDUCE_MAX, mapped = src != nullptr || eid != nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (x16) {
        DISPATCH_GEOM_16BIT(g, (launch_block<VEC, GROUP, __bf16>(a, is_max, mapped, st)))
    } else {
        DISPATCH_GEOM(g, (launch_block<VEC, GROUP, float>(a, is_max, mapped, st)))
    }
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_gcn_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const float *d_val,
                         const int *d_eid, const void *d_x, int x_dtype, long long x_pitch, void *d_y, int y_dtype, void *d_x_dst,
                         int feat, int reduce, int flags, void *hip_stream)
{
    return block_gcn_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_val, d_eid, d_x, x_dtype, x_pitch, d_y, y_dtype, d_x_dst, feat, reduce,
                         flags, hip_stream);
}

}  // extern "C"
#pragma GCC visibility pop
