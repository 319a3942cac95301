// agg_block_sage.hip -- a SAGE layer on ONE sampled block in one launch: gnnagg_block_sage_run (include/gnnagg.h section F, "Block SAGE layer").
//
//   out[i] = act( x_dst[i] . W_self + aggr_{p in row i}(x_src) . W_neigh + bias )
//
// The aggregation spreads the columns of a row over the lanes of a group while the matrix cores want rows across lanes, so the rows meet in
// LDS (the frame of k_gcn_plan_nn, agg_gcn.hip).  A workgroup of 256 threads owns tiles of kSageRows = 16 destination rows and walks the
// tiles blockIdx.x, blockIdx.x + gridDim.x, ...:
//   phase 1  one lane group per row (16 / (256 / GROUP) passes): the self row's load is issued, the chain of chain_block_edges runs in CSR
//            order -- the bits of k_block_gcn -- and the lane writes s to tile columns [0, feat) and a to [Fp, Fp + feat), Fp = feat
//            rounded up to the MFMA's k block.  A row wider than the group (narrow lanes: odd feat, odd pitch) is walked once per column
//            tile.  The padding columns are zeroed once per workgroup, the rows of a partial last tile per tile.
//   phase 2  after ONE barrier the 4 wavefronts take 16 x 16 output sub-tiles and run k over [W_self; W_neigh] in ONE fp32 accumulator:
//            fp32 operands on v_mfma_f32_16x16x4_f32, W through buffer loads from L1 / L2 (the ascending-k fmaf chain of the separate GEMM,
//            bit for bit; the zero columns between the halves add 0 * 0 to an accumulator that is never -0); bf16 operands on
//            v_mfma_f32_16x16x32_bf16 against an image wimg[n][k] of both weights, k contiguous, transposed into LDS ONCE per workgroup
//            -- which is what the persistent tile loop is for -- one ds_read_b128 per operand per MFMA.
//   epilogue from the D registers: + bias, ReLU, one store per element (a bf16 out: one round-to-nearest-even).
// The aggregate never reaches HBM, x_dst is never copied, nothing is concatenated.  No atomics, no scratch; every lane's address is a
// function of the arguments, and so is the result.
#include "sage_combine.cuh"

namespace gnnagg {
namespace {

constexpr int kSageRows = 16;                // destination rows of a tile: one MFMA row block
constexpr int kSageLdsBytes = 160 * 1024;    // LDS of a CU: the budget of tile + weight image
constexpr int kSageMaxDim = 256;             // feat and n_out
constexpr int kSagePerCu = 8;                // workgroups per CU the grid is capped at (fewer where the LDS of a workgroup allows fewer)

struct SageArgs {
    const int *ptr, *idx, *src, *eid;
    const float *val;
    const void *x, *wself, *wneigh;
    const float *bias;
    void *out;
    long long xpitch;   // elements between rows of x
    int num_dst, feat, n_out, ntiles, mean, relu, out_bf16, row_tiles;
};

// The LDS of a launch, kernel and launcher agree through these: [tile_rows: 16 ints][tile: 16 rows][bf16: the weight image].  Fp: feat
// rounded up to the MFMA's k block (4 fp32, 32 bf16).  The pitch of the tile and of the image is 2 Fp + 4 floats / 2 Fp + 8 bf16: rows stay
// 16-byte aligned, fp32 operand reads (row = lane % 16, k = lane / 16) fall two per bank, and the bf16 pitch is an odd number of 16-byte
// slots, so the 16 rows (columns) a b128 lane group reads fall on 16 different slots of the bank row.
__host__ __device__ constexpr int sage_fp(int feat, bool b16) { return b16 ? (feat + 31) & ~31 : (feat + 3) & ~3; }
__host__ __device__ constexpr int sage_pitch(int feat, bool b16) { return 2 * sage_fp(feat, b16) + (b16 ? 8 : 4); }
constexpr int kSageTileOff = kSageRows * (int)sizeof(int);
static size_t sage_lds_bytes(int feat, int n_out, bool b16)
{
    const size_t tile = (size_t)kSageRows * sage_pitch(feat, b16) * (b16 ? 2 : 4);
    const size_t wimg = b16 ? (size_t)((n_out + 15) & ~15) * sage_pitch(feat, true) * 2 : 0;
    return kSageTileOff + tile + wimg;
}

static bool sage_supported(int feat, int n_out, int x_dtype)
{
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return false;
    if (feat < 1 || feat > kSageMaxDim || n_out < 1 || n_out > kSageMaxDim) return false;
    return sage_lds_bytes(feat, n_out, x_dtype == GNNAGG_DTYPE_BF16) <= (size_t)kSageLdsBytes;
}

// workgroups a launch of this shape is capped at: as many per CU as their LDS allows, kSagePerCu at the most
static int sage_grid_cap(int feat, int n_out, int x_dtype)
{
    const size_t per_cu = (size_t)kSageLdsBytes / sage_lds_bytes(feat, n_out, x_dtype == GNNAGG_DTYPE_BF16);
    return (int)std::min<size_t>(std::max<size_t>(per_cu, 1), kSagePerCu) * device_cu_count();
}

template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, typename TX>
__global__ __launch_bounds__(kSageThreads) void k_block_sage(const SageArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int GPB = kSageThreads / GROUP, PASSES = kSageRows / GPB;
    static_assert(GROUP >= 16 && PASSES * GPB == kSageRows, "whole passes over the 16 rows of a tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char sage_lds[];
    int *tile_rows = reinterpret_cast<int *>(sage_lds);
    TX *tile = reinterpret_cast<TX *>(sage_lds + kSageTileOff);
    const int F = a.feat, N = a.n_out, Fp = sage_fp(F, B16), pitch = sage_pitch(F, B16);
    const int lane = (int)threadIdx.x % GROUP, grp = (int)threadIdx.x / GROUP;
    const bool with_self = a.wself != nullptr;

    // once per workgroup: the padding columns of both halves (no row store reaches them: a lane's VEC columns lie below feat) ...
    const int npad = Fp - F;
    for (int i = threadIdx.x; i < kSageRows * 2 * npad; i += kSageThreads) {
        const int r = i / (2 * npad), c = i % (2 * npad);
        tile[r * pitch + (c < npad ? F + c : Fp + F + c - npad)] = (TX)0.0f;
    }
    // ... and, bf16, the image of both weights: k over [W_self; zeros to Fp; W_neigh; zeros to 2 Fp]
    const __bf16 *wimg = nullptr;
    if constexpr (B16) {
        __bf16 *img = reinterpret_cast<__bf16 *>(tile) + kSageRows * pitch;
        if (with_self) stage_weight_half(img, pitch, Fp, static_cast<const __bf16 *>(a.wself), F, N);
        stage_weight_half(img + Fp, pitch, Fp, static_cast<const __bf16 *>(a.wneigh), F, N);
        wimg = img;
    }

#pragma unroll 1
    for (int rt = (int)blockIdx.x; rt < a.row_tiles; rt += (int)gridDim.x) {
        // ---- phase 1: rows into the tile
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int slot = pass * GPB + grp;
            const int row = rt * kSageRows + slot;
            const bool live = row < a.num_dst;
            int beg = 0, end = 0;
            size_t srow = 0;
            if (live) {
                beg = a.ptr[row];
                end = a.ptr[row + 1];
                if (with_self) srow = (size_t)(a.src ? a.src[row] : row);
            }
            TX *trow = tile + slot * pitch;
#pragma unroll 1
            for (int ct = 0; ct < a.ntiles; ++ct) {
                const int col = (ct * GROUP + lane) * VEC;
                const bool col_ok = col < F;
                const TX *__restrict__ xcol = static_cast<const TX *>(a.x) + col;
                Pack<VEC, TX> self = {};
                if (live && with_self && col_ok) self = load_pack<VEC>(xcol + srow * (size_t)a.xpitch);   // in flight over the chain
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
                if (with_self) store_raw_pack<VEC, TX>(trow + col, self);
                if constexpr (B16) store_pack_bf16<VEC>(trow + Fp + col, acc, VEC);   // the conversion of a bf16 y store
                else store_pack<VEC>(trow + Fp + col, acc);
            }
            if (lane == 0) tile_rows[slot] = live ? row : -1;
        }
        __syncthreads();   // the tile (and, the first time, its padding and the image) is complete

        // ---- phase 2: 16 x 16 output sub-tiles, one accumulator over both halves
        const int wave = (int)threadIdx.x >> 6, wl = (int)threadIdx.x & 63, kq = wl >> 4;
#pragma unroll 1
        for (int cb = wave; cb < (N + 15) >> 4; cb += kSageThreads >> 6) {
            const int col = cb * 16 + (wl & 15);
            const bool cok = col < N;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if constexpr (B16) {
                const __bf16 *ap = tile + (wl & 15) * pitch + 8 * kq;
                const __bf16 *bp = wimg + (size_t)col * pitch + 8 * kq;
                for (int k0 = with_self ? 0 : Fp; k0 < 2 * Fp; k0 += 32)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const sage_bf16x8 *>(ap + k0),
                                                                  *reinterpret_cast<const sage_bf16x8 *>(bp + k0), acc, 0, 0, 0);
            } else {
                constexpr int KB = GROUP * VEC >= 128 ? 32 : GROUP * VEC / 4;
                const float *arow = tile + (wl & 15) * pitch + kq;
                if (with_self) half_times_weight<KB>(acc, arow, static_cast<const float *>(a.wself), F, N, col, cok, kq);
                half_times_weight<KB>(acc, arow + Fp, static_cast<const float *>(a.wneigh), F, N, col, cok, kq);
            }
            // D layout: col = lane % 16, row = 4 * (lane / 16) + reg
            const float bias = (a.bias && cok) ? a.bias[col] : 0.0f;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = tile_rows[4 * kq + v];
                if (r < 0 || !cok) continue;
                float o = acc[v];
                if (a.bias) o += bias;
                if (a.relu) o = o < 0.0f ? 0.0f : o;   // (a NaN stays a NaN: relu_pack)
                if (a.out_bf16) static_cast<__bf16 *>(a.out)[(size_t)r * N + col] = (__bf16)o;
                else static_cast<float *>(a.out)[(size_t)r * N + col] = o;
            }
        }
        __syncthreads();   // before the next tile overwrites this one
    }
}

template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, typename TX>
static int launch_sage_inst(const SageArgs &a, int grid, size_t lds, hipStream_t st)
{
    static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (lds > 64 * 1024 && big_lds_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_block_sage<VEC, GROUP, IS_MAX, MAPPED, TX>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kSageLdsBytes));
        big_lds_ok.done();
    }
    hipLaunchKernelGGL((k_block_sage<VEC, GROUP, IS_MAX, MAPPED, TX>), dim3((unsigned)grid), dim3(kSageThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

template <int VEC, int GROUP, typename TX>
static int launch_sage(const SageArgs &a, int is_max, int mapped, int grid, size_t lds, hipStream_t st)
{
    if constexpr (GROUP < 16) {
        return fail(GNNAGG_ERR_STATE, "internal: gnnagg_block_sage_run runs groups of 16 lanes and more");
    } else {
        if (is_max) return mapped ? launch_sage_inst<VEC, GROUP, true, true, TX>(a, grid, lds, st) : launch_sage_inst<VEC, GROUP, true, false, TX>(a, grid, lds, st);
        return mapped ? launch_sage_inst<VEC, GROUP, false, true, TX>(a, grid, lds, st) : launch_sage_inst<VEC, GROUP, false, false, TX>(a, grid, lds, st);
    }
}

static int block_sage_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const float *val, const int *eid, const void *x,
                          int x_dtype, long long x_pitch, int feat, const void *w_self, const void *w_neigh, const float *bias, int n_out,
                          void *out, int out_dtype, int reduce, int flags, void *stream)
{
    static const char *who = "gnnagg_block_sage_run: ";
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
    if (!sage_supported(feat, n_out, x_dtype))
        return bad("feat = " + std::to_string(feat) + ", n_out = " + std::to_string(n_out) + " lie outside the range of gnnagg_block_sage_supported");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!x) return bad("d_x is null");
        if (!w_neigh) return bad("d_w_neigh is null");
        if (!out) return bad("d_out is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: the rule of gnnagg_block_gcn_run for x (a divisor of feat and of the pitch, no wider than x's alignment); the tile
    // rows in LDS are aligned for any lane.  Groups of 8 lanes run as groups of 16: 16 groups are the 16 rows of a tile.
    const int fp = (int)gcd_ll(feat, x_pitch);
    Geometry g = x16 ? typed_geometry(feat, x, 2, fp) : pick_geometry(feat, x, nullptr, nullptr, fp);
    if (g.group < 16) g.group = 16;
    SageArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.eid = eid; a.val = val;
    a.x = x; a.wself = w_self; a.wneigh = w_neigh; a.bias = bias; a.out = out; a.xpitch = x_pitch;
    a.num_dst = num_dst; a.feat = feat; a.n_out = n_out; a.ntiles = g.ntiles;
    a.mean = reduce == GNNAGG_REDUCE_MEAN; a.relu = (flags & GNNAGG_FLAG_RELU) != 0;
    a.out_bf16 = out_dtype == GNNAGG_DTYPE_BF16;
    a.row_tiles = ceil_div(num_dst, kSageRows);
    const int is_max = reduce == GNNAGG_REDUCE_MAX, mapped = src != nullptr || eid != nullptr;
    const int grid = std::min(a.row_tiles, sage_grid_cap(feat, n_out, x_dtype));
    const size_t lds = sage_lds_bytes(feat, n_out, x16);
    hipStream_t st = (hipStream_t)stream;
    int rc = GNNAGG_OK;
    if (x16) {
        DISPATCH_GEOM_16BIT(g, (rc = launch_sage<VEC, GROUP, __bf16>(a, is_max, mapped, grid, lds, st)))
    } else {
        DISPATCH_GEOM(g, (rc = launch_sage<VEC, GROUP, float>(a, is_max, mapped, grid, lds, st)))
    }
    return rc;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_sage_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const float *d_val, const int *d_eid,
                          const void *d_x, int x_dtype, long long x_pitch, int feat, const void *d_w_self, const void *d_w_neigh,
                          const float *d_bias, int n_out, void *d_out, int out_dtype, int reduce, int flags, void *hip_stream)
{
    return block_sage_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_val, d_eid, d_x, x_dtype, x_pitch, feat, d_w_self, d_w_neigh, d_bias, n_out,
                          d_out, out_dtype, reduce, flags, hip_stream);
}

int gnnagg_block_sage_supported(int feat, int n_out, int x_dtype) { return sage_supported(feat, n_out, x_dtype) ? 1 : 0; }

int gnnagg_block_sage_grid_cap(int feat, int n_out, int x_dtype) { return sage_supported(feat, n_out, x_dtype) ? sage_grid_cap(feat, n_out, x_dtype) : 0; }

}  // extern "C"
#pragma GCC visibility pop
