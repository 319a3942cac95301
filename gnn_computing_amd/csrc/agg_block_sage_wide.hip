// agg_block_sage_wide.hip -- the SAGE layer of agg_block_sage.hip for rows of ANY width up to 4096 features: gnnagg_block_sage_wide_run
// (include/gnnagg.h section F, "Block SAGE layer, wide rows").
//
//   out[i] = act( x_dst[i] . W_self + aggr_{p in row i}(x_src) . W_neigh + bias )
//
// k_block_sage holds a tile row of 2 feat columns (and, bf16, the image of both weights) in LDS, so its LDS grows with feat.  Here the k
// dimension of [W_self; W_neigh] runs in CHUNKS of KC columns through a tile of ROWS x KC: the LDS of a workgroup depends on KC and n_out,
// never on feat.  A workgroup of 256 threads owns tiles of ROWS = 16 R destination rows (R MFMA row blocks) and walks the tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...  Per tile the chunks run: all chunks of the self half, then all chunks of the neighbour half,
// each ascending -- the k order of matmul_NN(cat([x_dst, y]), cat([W_self, W_neigh])).
//   fill     one lane group per row (ROWS / (256 / GROUP) passes).  A self chunk is a plain copy of KC columns of x_dst; a neighbour chunk
//            walks the row's edges with chain_block_edges on the chunk's columns (idx / src / val are read again per chunk: 4 - 12 bytes
//            from L1 / L2 beside KC x esize of gather).  The ragged last chunk of a half is zero-padded to the MFMA's k block in LDS.
//            bf16: the chunk [roundup16(n_out)][KC] of the weight image, k contiguous, is staged by stage_weight_half on the k window.
//   product  wavefront w owns the column blocks w, w + 4, w + 8, w + 12 of all R row blocks; their f32x4 accumulators stay in registers
//            across all chunks of the tile.  fp32: half_times_weight on the chunk (W through buffer loads), the ascending-k fmaf chain of
//            the separate GEMM, bit for bit.  bf16: v_mfma_f32_16x16x32_bf16, one staged B operand serving the R row blocks.
//   pipeline tile and image chunk are double-buffered: the fill of chunk c + 1 is issued before the product of chunk c, ONE barrier per
//            chunk.  (fill of c + 1 writes the buffer the product of c - 1 read: the barrier that ended chunk c - 1 lies between.)
//   epilogue once per tile, after the last chunk, from the D registers: + bias, ReLU, one store per element.
// No atomics, no scratch; every lane's address is a function of the arguments, and so is the result.
#include "sage_combine.cuh"

namespace gnnagg {
namespace {

constexpr int kWideLdsBytes = 160 * 1024;    // LDS of a CU
constexpr int kWideMaxFeat = 4096;
constexpr int kWideMaxOut = 256;
constexpr int kWidePerCu = 8;                // workgroups per CU the grid is capped at (fewer where the LDS of a workgroup allows fewer)
constexpr int kWideColBlocks = kWideMaxOut / 16 / (kSageThreads / 64);   // 4: the column blocks of a wavefront

// KC: a multiple of the MFMA's k block (4 fp32, 32 bf16).  fp32: 128 columns, 512-byte row pieces, the widest 16-byte lane group of 32;
// bf16: 64 columns -- the image chunk [256][64 + 8] is 36 KB, and two of them plus the tile must fit a CU twice.
__host__ __device__ constexpr int wide_kc(bool b16) { return b16 ? 64 : 128; }
__host__ __device__ constexpr int wide_kblk(bool b16) { return b16 ? 32 : 4; }
// pitch of the tile and of the image chunk: the narrow kernel's rule (rows 16-byte aligned, fp32 operand reads two per bank, the bf16
// pitch an odd number of 16-byte slots)
__host__ __device__ constexpr int wide_pitch(bool b16) { return wide_kc(b16) + (b16 ? 8 : 4); }
// R, the MFMA row blocks of a tile.  fp32 takes W from L1 / L2 per 16 rows as the narrow kernel does: R = 1.  bf16 pays the transposition
// of the image chunk per tile: R = 4 where two workgroups still fit a CU (n_out <= 128), else 1.
static int wide_r(int n_out, bool b16) { return b16 && n_out <= 128 ? 4 : 1; }

// The LDS of a launch: [tile_rows: 2 x ROWS ints][tile: 2 buffers of ROWS rows][bf16: 2 buffers of the image chunk]
__host__ __device__ constexpr int wide_tile_off(int rows) { return 2 * rows * (int)sizeof(int); }
static size_t wide_lds_bytes(int n_out, bool b16)
{
    const int rows = 16 * wide_r(n_out, b16);
    const size_t tile = (size_t)rows * wide_pitch(b16) * (b16 ? 2 : 4);
    const size_t wimg = b16 ? (size_t)((n_out + 15) & ~15) * wide_pitch(true) * 2 : 0;
    return wide_tile_off(rows) + 2 * (tile + wimg);
}

static bool wide_supported(int feat, int n_out, int x_dtype)
{
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return false;
    return feat >= 1 && feat <= kWideMaxFeat && n_out >= 1 && n_out <= kWideMaxOut;
}

static int wide_grid_cap(int n_out, int x_dtype)
{
    const size_t per_cu = (size_t)kWideLdsBytes / wide_lds_bytes(n_out, x_dtype == GNNAGG_DTYPE_BF16);
    return (int)std::min<size_t>(std::max<size_t>(per_cu, 1), kWidePerCu) * device_cu_count();
}

struct WideArgs {
    const int *ptr, *idx, *src, *eid;
    const float *val;
    const void *x, *wself, *wneigh;
    const float *bias;
    void *out;
    long long xpitch;   // elements between rows of x
    int num_dst, feat, n_out, ntiles, mean, relu, out_bf16, row_tiles;
};

template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, typename TX, int R>
__global__ __launch_bounds__(kSageThreads) void k_block_sage_wide(const WideArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int ROWS = 16 * R, KC = wide_kc(B16), KBLK = wide_kblk(B16), PITCH = wide_pitch(B16);
    constexpr int GPB = kSageThreads / GROUP, PASSES = ROWS / GPB;
    static_assert(PASSES >= 1 && PASSES * GPB == ROWS, "whole passes over the rows of a tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char wide_lds[];
    int *tile_rows = reinterpret_cast<int *>(wide_lds);
    TX *tiles = reinterpret_cast<TX *>(wide_lds + wide_tile_off(ROWS));
    const int F = a.feat, N = a.n_out, ncb = (N + 15) >> 4;
    const int wstride = ncb * 16 * PITCH;    // elements of one image chunk
    __bf16 *imgs = reinterpret_cast<__bf16 *>(tiles + 2 * ROWS * PITCH);
    const int lane = (int)threadIdx.x % GROUP, grp = (int)threadIdx.x / GROUP;
    const int wave = (int)threadIdx.x >> 6, wl = (int)threadIdx.x & 63, kq = wl >> 4;
    const bool with_self = a.wself != nullptr;
    const int nch = (F + KC - 1) / KC, nchunks = with_self ? 2 * nch : nch;   // chunks of a half, of a tile

    // chunk c of tile rt into buffer c & 1: (bf16) the image chunk, then the rows
    auto fill = [&](int rt, int c, int *trows) {
        const bool self = with_self && c < nch;
        const int k0 = (self || !with_self ? c : c - nch) * KC;
        const int kc = F - k0 < KC ? F - k0 : KC, kcp = (kc + KBLK - 1) & ~(KBLK - 1);
        TX *buf = tiles + (c & 1) * ROWS * PITCH;
        if constexpr (B16)
            stage_weight_half(imgs + (c & 1) * wstride, PITCH, kcp, static_cast<const __bf16 *>(self ? a.wself : a.wneigh) + (size_t)k0 * N, kc, N);
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int slot = pass * GPB + grp;
            const int row = rt * ROWS + slot;
            const bool live = row < a.num_dst;
            int beg = 0, end = 0;
            size_t srow = 0;
            if (live) {
                if (self) {
                    srow = (size_t)(a.src ? a.src[row] : row);
                } else {
                    beg = a.ptr[row];
                    end = a.ptr[row + 1];
                }
            }
            TX *trow = buf + slot * PITCH;
#pragma unroll 1
            for (int ct = 0; ct < a.ntiles; ++ct) {
                const int col = (ct * GROUP + lane) * VEC;
                const bool col_ok = col < kc;
                const TX *__restrict__ xcol = static_cast<const TX *>(a.x) + k0 + col;
                if (self) {   // a plain copy of x_dst's columns (a row past num_dst: zeros)
                    Pack<VEC, TX> s = {};
                    if (live && col_ok) s = load_pack<VEC>(xcol + srow * (size_t)a.xpitch);
                    if (col_ok) store_raw_pack<VEC, TX>(trow + col, s);
                    continue;
                }
                float acc[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = IS_MAX ? -INFINITY : 0.0f;
                chain_block_edges<VEC, GROUP, IS_MAX, MAPPED, kUnroll, TX>(acc, beg, end, lane, col_ok, a.idx, a.src, a.val, a.eid, xcol, a.xpitch);
                if (!col_ok) continue;
                if (beg == end) {  // no edges (or a row past num_dst): 0, whatever the reduce
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
                } else {
                    finish_gcn_row<VEC, IS_MAX>(acc, end - beg, row, nullptr, a.mean, 0, 0, nullptr);
                }
                if constexpr (B16) store_pack_bf16<VEC>(trow + col, acc, VEC);   // the conversion of a bf16 y store
                else store_pack<VEC>(trow + col, acc);
            }
            // the ragged last chunk of a half: zeros up to the k block (a full chunk's values may lie there; no row store reaches them)
            for (int cz = kc + lane; cz < kcp; cz += GROUP) trow[cz] = (TX)0.0f;
            if (c == 0 && lane == 0) trows[slot] = live ? row : -1;
        }
    };

    int parity = 0;
#pragma unroll 1
    for (int rt = (int)blockIdx.x; rt < a.row_tiles; rt += (int)gridDim.x, parity ^= 1) {
        int *trows = tile_rows + parity * ROWS;   // (two sets: the next tile's fill may pass this tile's epilogue)
        f32x4 acc[R][kWideColBlocks];
#pragma unroll
        for (int rb = 0; rb < R; ++rb)
#pragma unroll
            for (int j = 0; j < kWideColBlocks; ++j) acc[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int c = -1; c < nchunks; ++c) {   // (c = -1: the first fill alone)
            if (c + 1 < nchunks) fill(rt, c + 1, trows);
            if (c < 0) {
                __syncthreads();
                continue;
            }
            // ---- the product of chunk c
            const bool self = with_self && c < nch;
            const int k0 = (self || !with_self ? c : c - nch) * KC;
            const int kc = F - k0 < KC ? F - k0 : KC;
            const TX *buf = tiles + (c & 1) * ROWS * PITCH;
            if constexpr (B16) {
                const int kcp = (kc + KBLK - 1) & ~(KBLK - 1);
                const __bf16 *ap = buf + (wl & 15) * PITCH + 8 * kq;
                const __bf16 *bp = imgs + (c & 1) * wstride + (wl & 15) * PITCH + 8 * kq;
                for (int kb = 0; kb < kcp; kb += 32) {
                    sage_bf16x8 av[R];
#pragma unroll
                    for (int rb = 0; rb < R; ++rb) av[rb] = *reinterpret_cast<const sage_bf16x8 *>(ap + rb * 16 * PITCH + kb);
#pragma unroll
                    for (int j = 0; j < kWideColBlocks; ++j) {
                        const int cb = wave + j * (kSageThreads >> 6);
                        if (cb >= ncb) break;
                        const sage_bf16x8 bv = *reinterpret_cast<const sage_bf16x8 *>(bp + cb * 16 * PITCH + kb);
#pragma unroll
                        for (int rb = 0; rb < R; ++rb) acc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[rb], bv, acc[rb][j], 0, 0, 0);
                    }
                }
            } else {
                constexpr int KB = GROUP * VEC >= 128 ? 32 : GROUP * VEC / 4;
                const float *W = static_cast<const float *>(self ? a.wself : a.wneigh) + (size_t)k0 * N;
#pragma unroll
                for (int j = 0; j < kWideColBlocks; ++j) {
                    const int cb = wave + j * (kSageThreads >> 6);
                    if (cb >= ncb) break;
                    const int col = cb * 16 + (wl & 15);
#pragma unroll
                    for (int rb = 0; rb < R; ++rb)
                        half_times_weight<KB>(acc[rb][j], buf + (rb * 16 + (wl & 15)) * PITCH + kq, W, kc, N, col, col < N, kq);
                }
            }
            __syncthreads();   // chunk c + 1 is complete, chunk c is consumed
        }
        // ---- epilogue.  D layout: col = lane % 16, row = 4 * (lane / 16) + reg
#pragma unroll
        for (int j = 0; j < kWideColBlocks; ++j) {
            const int cb = wave + j * (kSageThreads >> 6);
            if (cb >= ncb) break;
            const int col = cb * 16 + (wl & 15);
            const bool cok = col < N;
            const float bias = (a.bias && cok) ? a.bias[col] : 0.0f;
#pragma unroll
            for (int rb = 0; rb < R; ++rb)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = trows[rb * 16 + 4 * kq + v];
                    if (r < 0 || !cok) continue;
                    float o = acc[rb][j][v];
                    if (a.bias) o += bias;
                    if (a.relu) o = o < 0.0f ? 0.0f : o;   // (a NaN stays a NaN: relu_pack)
                    if (a.out_bf16) static_cast<__bf16 *>(a.out)[(size_t)r * N + col] = (__bf16)o;
                    else static_cast<float *>(a.out)[(size_t)r * N + col] = o;
                }
        }
    }
}

template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, typename TX, int R>
static int launch_wide_inst(const WideArgs &a, int grid, size_t lds, hipStream_t st)
{
    static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (lds > 64 * 1024 && big_lds_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_block_sage_wide<VEC, GROUP, IS_MAX, MAPPED, TX, R>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kWideLdsBytes));
        big_lds_ok.done();
    }
    hipLaunchKernelGGL((k_block_sage_wide<VEC, GROUP, IS_MAX, MAPPED, TX, R>), dim3((unsigned)grid), dim3(kSageThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

template <int VEC, int GROUP, typename TX, int R>
static int launch_wide(const WideArgs &a, int is_max, int mapped, int grid, size_t lds, hipStream_t st)
{
    if constexpr (kSageThreads / GROUP > 16 * R) {
        return fail(GNNAGG_ERR_STATE, "internal: gnnagg_block_sage_wide_run runs no more lane groups than a tile has rows");
    } else {
        if (is_max) return mapped ? launch_wide_inst<VEC, GROUP, true, true, TX, R>(a, grid, lds, st) : launch_wide_inst<VEC, GROUP, true, false, TX, R>(a, grid, lds, st);
        return mapped ? launch_wide_inst<VEC, GROUP, false, true, TX, R>(a, grid, lds, st) : launch_wide_inst<VEC, GROUP, false, false, TX, R>(a, grid, lds, st);
    }
}

static int block_sage_wide_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const float *val, const int *eid, const void *x,
                               int x_dtype, long long x_pitch, int feat, const void *w_self, const void *w_neigh, const float *bias, int n_out,
                               void *out, int out_dtype, int reduce, int flags, void *stream)
{
    static const char *who = "gnnagg_block_sage_wide_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    if (num_dst < 0) return bad("num_dst = " + std::to_string(num_dst) + " is negative");
    if (feat < 1) return bad("feat = " + std::to_string(feat) + " must be >= 1");
    if (n_out < 1) return bad("n_out = " + std::to_string(n_out) + " must be >= 1");
    if (x_pitch < feat) return bad("x_pitch = " + std::to_string(x_pitch) + " is below feat = " + std::to_string(feat));
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (out_dtype != GNNAGG_DTYPE_F32 && out_dtype != GNNAGG_DTYPE_BF16) return bad("unknown out_dtype " + std::to_string(out_dtype));
    if (x_dtype == GNNAGG_DTYPE_F32 && out_dtype == GNNAGG_DTYPE_BF16) return bad("out_dtype: fp32 operands give a fp32 out, not a bf16 one");
    if (reduce != GNNAGG_REDUCE_SUM && reduce != GNNAGG_REDUCE_MEAN && reduce != GNNAGG_REDUCE_MAX)
        return bad("unknown reduce " + std::to_string(reduce));
    if (flags & ~GNNAGG_FLAG_RELU) return bad("flags = " + std::to_string(flags) + ": GNNAGG_FLAG_RELU is the only flag");
    if (eid && !val) return bad("d_eid needs d_val (d_eid indexes it)");
    if (!wide_supported(feat, n_out, x_dtype))
        return bad("feat = " + std::to_string(feat) + ", n_out = " + std::to_string(n_out) + " lie outside the range of gnnagg_block_sage_wide_supported");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!x) return bad("d_x is null");
        if (!w_neigh) return bad("d_w_neigh is null");
        if (!out) return bad("d_out is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: the rule of gnnagg_block_sage_run (a divisor of feat and of the pitch, no wider than x's alignment) on the columns
    // of ONE chunk, min(feat, KC): every chunk starts a multiple of KC elements into its row, so it has the row's alignment.  A tile of
    // 16 rows runs groups of 8 lanes as groups of 16 (16 groups are its 16 rows); a tile of 64 rows keeps them: a bf16 chunk of 64 columns
    // is 8 lanes of 16 bytes, and 32 groups walk 32 rows with every lane loading.
    const int fp = (int)gcd_ll(feat, x_pitch), cols = std::min(feat, wide_kc(x16));
    Geometry g = x16 ? typed_geometry(cols, x, 2, fp) : pick_geometry(cols, x, nullptr, nullptr, fp);
    const int r = wide_r(n_out, x16);
    if (g.group < 16 && r == 1) g.group = 16;
    WideArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.eid = eid; a.val = val;
    a.x = x; a.wself = w_self; a.wneigh = w_neigh; a.bias = bias; a.out = out; a.xpitch = x_pitch;
    a.num_dst = num_dst; a.feat = feat; a.n_out = n_out; a.ntiles = g.ntiles;
    a.mean = reduce == GNNAGG_REDUCE_MEAN; a.relu = (flags & GNNAGG_FLAG_RELU) != 0;
    a.out_bf16 = out_dtype == GNNAGG_DTYPE_BF16;
    a.row_tiles = ceil_div(num_dst, 16 * r);
    const int is_max = reduce == GNNAGG_REDUCE_MAX, mapped = src != nullptr || eid != nullptr;
    const int grid = std::min(a.row_tiles, wide_grid_cap(n_out, x_dtype));
    const size_t lds = wide_lds_bytes(n_out, x16);
    hipStream_t st = (hipStream_t)stream;
    int rc = GNNAGG_OK;
    if (!x16) {
        DISPATCH_GEOM(g, (rc = launch_wide<VEC, GROUP, float, 1>(a, is_max, mapped, grid, lds, st)))
    } else if (r == 4) {
        DISPATCH_GEOM_16BIT(g, (rc = launch_wide<VEC, GROUP, __bf16, 4>(a, is_max, mapped, grid, lds, st)))
    } else {
        DISPATCH_GEOM_16BIT(g, (rc = launch_wide<VEC, GROUP, __bf16, 1>(a, is_max, mapped, grid, lds, st)))
    }
    return rc;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_sage_wide_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const float *d_val, const int *d_eid,
                               const void *d_x, int x_dtype, long long x_pitch, int feat, const void *d_w_self, const void *d_w_neigh,
                               const float *d_bias, int n_out, void *d_out, int out_dtype, int reduce, int flags, void *hip_stream)
{
    return block_sage_wide_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_val, d_eid, d_x, x_dtype, x_pitch, feat, d_w_self, d_w_neigh, d_bias,
                               n_out, d_out, out_dtype, reduce, flags, hip_stream);
}

int gnnagg_block_sage_wide_supported(int feat, int n_out, int x_dtype) { return wide_supported(feat, n_out, x_dtype) ? 1 : 0; }

int gnnagg_block_sage_wide_grid_cap(int feat, int n_out, int x_dtype) { return wide_supported(feat, n_out, x_dtype) ? wide_grid_cap(n_out, x_dtype) : 0; }

int gnnagg_block_sage_wide_chunk(int x_dtype)
{
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return 0;
    return wide_kc(x_dtype == GNNAGG_DTYPE_BF16);
}

}  // extern "C"
#pragma GCC visibility pop
