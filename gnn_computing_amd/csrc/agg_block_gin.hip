// agg_block_gin.hip -- a GIN layer on ONE sampled block in one launch: gnnagg_block_gin_run (include/gnnagg.h section F, "Block GIN layer").
//
//   h   = self_scale * x_dst + aggr_{p in row}(val_p * x_src(p))       [num_dst, feat]      self_scale = 1 + eps
//   z   = relu(h . W1 + b1)                                            [num_dst, hidden]
//   out = act(z . W2 + b2)                                             [num_dst, n_out]
//
// The frame is that of k_block_sage (agg_block_sage.hip): 256 threads, tiles of kGinRows = 16 destination rows, the tiles blockIdx.x,
// blockIdx.x + gridDim.x, ... per workgroup.  What is new is the MLP: TWO chained MFMA products per tile with the hidden tile held in LDS.
//   phase 1  one lane group per row: the self row's load is issued, the chain of chain_block_edges runs in CSR order -- the bits of
//            k_block_gcn -- and the lane forms h = a + self_scale * s (two fp32 roundings, no contraction) and stores it to its columns of
//            the h tile (bf16: one rounding).  ONE slot per row: self and neighbours share W1.
//   phase 2  after the first barrier the 4 wavefronts take the 16 x 16 sub-tiles of z, k ascending over the h tile and W1 in one fp32
//            accumulator; from the D registers + b1, ReLU, one LDS store per element into the z tile (bf16: one rounding).  Sub-tile
//            columns past `hidden` store 0: they are the k padding of phase 3, and 0 * NaN must not get there.
//   phase 3  after the second barrier the same over the sub-tiles of out, k over the z tile and W2; + b2, the optional ReLU, one global
//            store per element (a bf16 out: one rounding).
// fp32 operands run v_mfma_f32_16x16x4_f32 with W1 / W2 through buffer loads: the ascending-k fmaf chain of the separate GEMM, bit for bit.
// bf16 operands run v_mfma_f32_16x16x32_bf16 against images wimg1[n][k], wimg2[n][k] (k contiguous) of both weights, transposed into LDS
// once per workgroup, one ds_read_b128 per operand per MFMA.
// Two barriers per tile: the h tile and the z tile are separate regions, so a wavefront that has left phase 3 may start phase 1 of the
// workgroup's next tile (it writes h, which every wavefront stopped reading at the second barrier); the next tile's first barrier keeps
// its phase 2 off the z tile until every wavefront has left phase 3.  The one thing phase 1 writes and phase 3 reads is tile_rows, which
// therefore has two copies, indexed by the parity of the tile within the workgroup.
// Neither h nor z reaches HBM.  No atomics, no scratch; every lane's address is a function of the arguments, and so is the result.
#include "block_chain.cuh"

namespace gnnagg {
namespace {

constexpr int kGinThreads = 256;            // 4 wavefronts
constexpr int kGinRows = 16;                // destination rows of a tile: one MFMA row block
constexpr int kGinLdsBytes = 160 * 1024;    // LDS of a CU: the budget of both tiles + both weight images
constexpr int kGinMaxDim = 256;             // feat, hidden and n_out
constexpr int kGinPerCu = 8;                // workgroups per CU the grid is capped at (fewer where the LDS of a workgroup allows fewer)
constexpr int kGinKB = 16;                  // fp32: k quads whose operands are loaded before the first MFMA of a batch

struct GinArgs {
    const int *ptr, *idx, *src, *eid;
    const float *val;
    const void *x, *w1, *w2;
    const float *b1, *b2;
    void *out;
    long long xpitch;   // elements between rows of x
    float self_scale;
    int num_dst, feat, hidden, n_out, ntiles, mean, relu, out_bf16, row_tiles;
};

// The LDS of a launch, kernel and launcher agree through gin_lds:
//   [tile_rows: 2 x 16 ints][h tile: 16 rows of pitch_h][z tile: 16 rows of pitch_z][bf16: wimg1, roundup16(hidden) rows of pitch_h]
//   [bf16: wimg2, roundup16(n_out) rows of pitch_z]
// kp: K (feat / hidden) rounded up to the MFMA's k block (4 fp32, 32 bf16).  The pitch of a tile (and of the image read against it) is
// roundup8(K) + 4 floats -- the 16 rows of an A operand start on 8 different multiples of 4 banks, two lanes per bank -- or kp + 8 bf16: an
// odd number of 16-byte slots, so the 16 rows (columns) a b128 lane group reads fall on 16 different slots of the bank row.
struct GinLds {
    int fp, hp, pitch_h, pitch_z, h_off, z_off, w1_off, w2_off, bytes;
};
__host__ __device__ constexpr int gin_kp(int k, bool b16) { return b16 ? (k + 31) & ~31 : (k + 3) & ~3; }
__host__ __device__ constexpr int gin_pitch(int k, bool b16) { return b16 ? gin_kp(k, true) + 8 : ((k + 7) & ~7) + 4; }
__host__ __device__ constexpr GinLds gin_lds(int feat, int hidden, int n_out, bool b16)
{
    GinLds l = {};
    const int es = b16 ? 2 : 4;
    l.fp = gin_kp(feat, b16);
    l.hp = gin_kp(hidden, b16);
    l.pitch_h = gin_pitch(feat, b16);
    l.pitch_z = gin_pitch(hidden, b16);
    l.h_off = 2 * kGinRows * (int)sizeof(int);
    l.z_off = l.h_off + kGinRows * l.pitch_h * es;
    l.w1_off = l.z_off + kGinRows * l.pitch_z * es;
    l.w2_off = l.w1_off + (b16 ? ((hidden + 15) & ~15) * l.pitch_h * 2 : 0);
    l.bytes = l.w2_off + (b16 ? ((n_out + 15) & ~15) * l.pitch_z * 2 : 0);
    return l;
}

static bool gin_supported(int feat, int hidden, int n_out, int x_dtype)
{
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return false;
    if (feat < 1 || feat > kGinMaxDim || hidden < 1 || hidden > kGinMaxDim || n_out < 1 || n_out > kGinMaxDim) return false;
    return gin_lds(feat, hidden, n_out, x_dtype == GNNAGG_DTYPE_BF16).bytes <= kGinLdsBytes;
}

// workgroups a launch of this shape is capped at: as many per CU as their LDS allows, kGinPerCu at the most
static int gin_grid_cap(int feat, int hidden, int n_out, int x_dtype)
{
    const int per_cu = kGinLdsBytes / gin_lds(feat, hidden, n_out, x_dtype == GNNAGG_DTYPE_BF16).bytes;
    return std::min(std::max(per_cu, 1), kGinPerCu) * device_cu_count();
}

typedef __bf16 gin_bf16x8 __attribute__((ext_vector_type(8)));

// One weight into its image: wimg[n][0 .. kp) = W[0 .. K)[n] for the columns n < roundup16(N), zeros beyond K and N.  The two paths of
// stage_weight_bf16 (agg_gcn.hip): where N % 8 == 0 and W is 16-byte aligned one thread per 8 k x 8 columns -- eight 16-byte row pieces
// transposed in registers, one 16-byte LDS store per column; else one thread per (column, 8 k) with 2-byte loads.  Both write the same image.
__device__ __forceinline__ void stage_weight_image(__bf16 *wimg, int wpitch, int kp, const __bf16 *__restrict__ W, int K, int N)
{
    const unsigned short *Wu = reinterpret_cast<const unsigned short *>(W);
    const int ncols = (N + 15) & ~15;
    if ((N & 7) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
        const int nco = ncols >> 3;
        for (int i = threadIdx.x; i < nco * (kp >> 3); i += kGinThreads) {
            const int col = (i % nco) << 3, k = (i / nco) << 3;
            unsigned q[8][4];   // q[j]: row k + j, columns col .. col + 7
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint4 t = make_uint4(0u, 0u, 0u, 0u);
                if (k + j < K && col < N) t = *reinterpret_cast<const uint4 *>(Wu + (size_t)(k + j) * N + col);
                q[j][0] = t.x; q[j][1] = t.y; q[j][2] = t.z; q[j][3] = t.w;
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {   // column col + c: element c of every row, k pairs packed
                unsigned v[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const unsigned lo = q[2 * m][c >> 1], hi = q[2 * m + 1][c >> 1];
                    v[m] = (c & 1) ? ((lo >> 16) | (hi & 0xffff0000u)) : ((lo & 0xffffu) | (hi << 16));
                }
                *reinterpret_cast<uint4 *>(wimg + (size_t)(col + c) * wpitch + k) = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
        return;
    }
    for (int i = threadIdx.x; i < ncols * (kp >> 3); i += kGinThreads) {
        const int n = i % ncols, k = (i / ncols) << 3;
        unsigned q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (n < N && k + j < K) ? (unsigned)Wu[(size_t)(k + j) * N + n] : 0u;
        *reinterpret_cast<uint4 *>(wimg + (size_t)n * wpitch + k) =
            make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
    }
}

// fp32: acc = arow[0 .. K) . W[0 .. K)[col], k ascending from acc = +0 -- the fmaf chain of gnnagg_matmul_nn.  arow: this lane's tile row
// at its k offset kq = lane / 16 (A: row = lane % 16, k = lane / 16; B: k = lane / 16, col = lane % 16); the tile's columns
// [K, roundup4(K)) hold 0.  W operands as buffer loads: the per-lane byte offset in one VGPR (out of range for the padding columns, which
// then read 0), the k step in an SGPR.  k quads past K inside a batch are clamped loads with zeroed operands: 0 * 0 leaves the chain as
// it is (an accumulator that started at +0 is never -0).
__device__ __forceinline__ f32x4 tile_times_weight_f32(const float *arow, const float *W, int K, int N, int col, bool cok, int kq)
{
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int Kf = K & ~3;     // k covered by whole quads
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0, K * N * 4, 0x00020000);
    const int voff = cok ? (kq * N + col) * 4 : 0x7ffffff0;
#pragma unroll 1
    for (int k0 = 0; k0 < Kf; k0 += 4 * kGinKB) {
        float av[kGinKB], bv[kGinKB];
#pragma unroll
        for (int t = 0; t < kGinKB; ++t) {
            const int kk = k0 + 4 * t, kc = kk < Kf ? kk : Kf - 4;
            const float b = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrsrc, voff, kc * N * 4, 0));
            bv[t] = kk < Kf ? b : 0.f;
        }
#pragma unroll
        for (int t = 0; t < kGinKB; ++t) {
            const int kk = k0 + 4 * t, kc = kk < Kf ? kk : Kf - 4;
            const float v = arow[kc];
            av[t] = kk < Kf ? v : 0.f;
        }
#pragma unroll
        for (int t = 0; t < kGinKB; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[t], acc, 0, 0, 0);
    }
    if (K != Kf) {  // ragged last quad: k = Kf + kq valid only below K (the tile's padding columns hold 0)
        const float b = (cok && Kf + kq < K) ? W[(size_t)(Kf + kq) * N + col] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[Kf], b, acc, 0, 0, 0);
    }
    return acc;
}

// bf16: acc = arow[0 .. kp) . brow[0 .. kp), both in LDS with k contiguous and zeros in [K, kp); arow / brow: this lane's tile row /
// image column at its k offset 8 * (lane / 16)
__device__ __forceinline__ f32x4 tile_times_image_bf16(const __bf16 *arow, const __bf16 *brow, int kp)
{
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kp; k0 += 32)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const gin_bf16x8 *>(arow + k0),
                                                      *reinterpret_cast<const gin_bf16x8 *>(brow + k0), acc, 0, 0, 0);
    return acc;
}

// h = a + c * s with TWO roundings, the bits of torch's y + x_dst * c.  (__fadd_rn(a, __fmul_rn(c, s)) does not say that here: the
// header defines both as the plain operators, which the compiler's default contraction fuses into one fma.)
__device__ __forceinline__ float scaled_self_plus(float a, float c, float s)
{
#pragma clang fp contract(off)
    const float p = c * s;
    return a + p;
}

template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, typename TX>
__global__ __launch_bounds__(kGinThreads) void k_block_gin(const GinArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int GPB = kGinThreads / GROUP, PASSES = kGinRows / GPB;
    static_assert(GROUP >= 16 && PASSES * GPB == kGinRows, "whole passes over the 16 rows of a tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char gin_smem[];
    const int F = a.feat, H = a.hidden, N = a.n_out;
    const GinLds L = gin_lds(F, H, N, B16);
    const int Fp = L.fp, Hp = L.hp, pitch_h = L.pitch_h, pitch_z = L.pitch_z;
    int *tile_rows = reinterpret_cast<int *>(gin_smem);
    TX *htile = reinterpret_cast<TX *>(gin_smem + L.h_off);
    TX *ztile = reinterpret_cast<TX *>(gin_smem + L.z_off);
    const int lane = (int)threadIdx.x % GROUP, grp = (int)threadIdx.x / GROUP;

    // once per workgroup: the k padding of the h tile (no row store reaches it: a lane's VEC columns lie below feat), the k padding of the
    // z tile that no sub-tile of phase 2 covers (bf16: [roundup16(hidden), Hp)) ...
    const int npad = Fp - F;
    for (int i = threadIdx.x; i < kGinRows * npad; i += kGinThreads) htile[(i / npad) * pitch_h + F + i % npad] = (TX)0.0f;
    const int zcov = (H + 15) & ~15, zpad = Hp > zcov ? Hp - zcov : 0;
    for (int i = threadIdx.x; i < kGinRows * zpad; i += kGinThreads) ztile[(i / zpad) * pitch_z + zcov + i % zpad] = (TX)0.0f;
    // ... and, bf16, the images of both weights
    const __bf16 *wimg1 = nullptr, *wimg2 = nullptr;
    if constexpr (B16) {
        __bf16 *i1 = reinterpret_cast<__bf16 *>(gin_smem + L.w1_off), *i2 = reinterpret_cast<__bf16 *>(gin_smem + L.w2_off);
        stage_weight_image(i1, pitch_h, Fp, static_cast<const __bf16 *>(a.w1), F, H);
        stage_weight_image(i2, pitch_z, Hp, static_cast<const __bf16 *>(a.w2), H, N);
        wimg1 = i1;
        wimg2 = i2;
    }

    int par = 0;   // the copy of tile_rows this tile uses
#pragma unroll 1
    for (int rt = (int)blockIdx.x; rt < a.row_tiles; rt += (int)gridDim.x, par ^= kGinRows) {
        // ---- phase 1: h rows into the h tile
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int slot = pass * GPB + grp;
            const int row = rt * kGinRows + slot;
            const bool live = row < a.num_dst;
            int beg = 0, end = 0;
            size_t srow = 0;
            if (live) {
                beg = a.ptr[row];
                end = a.ptr[row + 1];
                srow = (size_t)(a.src ? a.src[row] : row);
            }
            TX *trow = htile + slot * pitch_h;
#pragma unroll 1
            for (int ct = 0; ct < a.ntiles; ++ct) {
                const int col = (ct * GROUP + lane) * VEC;
                const bool col_ok = col < F;
                const TX *__restrict__ xcol = static_cast<const TX *>(a.x) + col;
                Pack<VEC, TX> self = {};
                if (live && col_ok) self = load_pack<VEC>(xcol + srow * (size_t)a.xpitch);   // in flight over the chain
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
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = scaled_self_plus(acc[k], a.self_scale, self.at(k));
                if constexpr (B16) store_pack_bf16<VEC>(trow + col, acc, VEC);
                else store_pack<VEC>(trow + col, acc);
            }
            if (lane == 0) tile_rows[par + slot] = live ? row : -1;
        }
        __syncthreads();   // the h tile (and, the first time, the padding and the images) is complete; every wavefront has left phase 3

        const int wave = (int)threadIdx.x >> 6, wl = (int)threadIdx.x & 63, kq = wl >> 4;
        // ---- phase 2: z = relu(h . W1 + b1), 16 x 16 sub-tiles into the z tile
#pragma unroll 1
        for (int cb = wave; cb < (H + 15) >> 4; cb += kGinThreads >> 6) {
            const int col = cb * 16 + (wl & 15);
            const bool cok = col < H;
            f32x4 acc;
            if constexpr (B16) acc = tile_times_image_bf16(htile + (wl & 15) * pitch_h + 8 * kq, wimg1 + (size_t)col * pitch_h + 8 * kq, Fp);
            else acc = tile_times_weight_f32(htile + (wl & 15) * pitch_h + kq, static_cast<const float *>(a.w1), F, H, col, cok, kq);
            // D layout: col = lane % 16, row = 4 * (lane / 16) + reg
            const float bias = (a.b1 && cok) ? a.b1[col] : 0.0f;
            if (col < Hp) {   // (fp32: the pitch ends before roundup16(hidden))
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float o = acc[v];
                    if (a.b1) o += bias;
                    o = o < 0.0f ? 0.0f : o;   // (a NaN stays a NaN: relu_pack)
                    if (!cok) o = 0.0f;        // the k padding of phase 3, whatever h held
                    ztile[(4 * kq + v) * pitch_z + col] = (TX)o;
                }
            }
        }
        __syncthreads();   // the z tile is complete; every wavefront has left the h tile

        // ---- phase 3: out = act(z . W2 + b2)
#pragma unroll 1
        for (int cb = wave; cb < (N + 15) >> 4; cb += kGinThreads >> 6) {
            const int col = cb * 16 + (wl & 15);
            const bool cok = col < N;
            f32x4 acc;
            if constexpr (B16) acc = tile_times_image_bf16(ztile + (wl & 15) * pitch_z + 8 * kq, wimg2 + (size_t)col * pitch_z + 8 * kq, Hp);
            else acc = tile_times_weight_f32(ztile + (wl & 15) * pitch_z + kq, static_cast<const float *>(a.w2), H, N, col, cok, kq);
            const float bias = (a.b2 && cok) ? a.b2[col] : 0.0f;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = tile_rows[par + 4 * kq + v];
                if (r < 0 || !cok) continue;
                float o = acc[v];
                if (a.b2) o += bias;
                if (a.relu) o = o < 0.0f ? 0.0f : o;
                if (a.out_bf16) static_cast<__bf16 *>(a.out)[(size_t)r * N + col] = (__bf16)o;
                else static_cast<float *>(a.out)[(size_t)r * N + col] = o;
            }
        }
        // no third barrier: the next tile's phase 1 writes the h tile and the other copy of tile_rows only
    }
}

template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, typename TX>
static int launch_gin_inst(const GinArgs &a, int grid, size_t lds, hipStream_t st)
{
    static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (lds > 64 * 1024 && big_lds_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_block_gin<VEC, GROUP, IS_MAX, MAPPED, TX>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kGinLdsBytes));
        big_lds_ok.done();
    }
    hipLaunchKernelGGL((k_block_gin<VEC, GROUP, IS_MAX, MAPPED, TX>), dim3((unsigned)grid), dim3(kGinThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

template <int VEC, int GROUP, typename TX>
static int launch_gin(const GinArgs &a, int is_max, int mapped, int grid, size_t lds, hipStream_t st)
{
    if constexpr (GROUP < 16) {
        return fail(GNNAGG_ERR_STATE, "internal: gnnagg_block_gin_run runs groups of 16 lanes and more");
    } else {
        if (is_max) return mapped ? launch_gin_inst<VEC, GROUP, true, true, TX>(a, grid, lds, st) : launch_gin_inst<VEC, GROUP, true, false, TX>(a, grid, lds, st);
        return mapped ? launch_gin_inst<VEC, GROUP, false, true, TX>(a, grid, lds, st) : launch_gin_inst<VEC, GROUP, false, false, TX>(a, grid, lds, st);
    }
}

static int block_gin_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const float *val, const int *eid, const void *x,
                         int x_dtype, long long x_pitch, int feat, float self_scale, const void *w1, const float *b1, int hidden, const void *w2,
                         const float *b2, int n_out, void *out, int out_dtype, int reduce, int flags, void *stream)
{
    static const char *who = "gnnagg_block_gin_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    if (num_dst < 0) return bad("num_dst = " + std::to_string(num_dst) + " is negative");
    if (feat < 1) return bad("feat = " + std::to_string(feat) + " must be >= 1");
    if (hidden < 1) return bad("hidden = " + std::to_string(hidden) + " must be >= 1");
    if (n_out < 1) return bad("n_out = " + std::to_string(n_out) + " must be >= 1");
    if (x_pitch < feat) return bad("x_pitch = " + std::to_string(x_pitch) + " is below feat = " + std::to_string(feat));
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (out_dtype != GNNAGG_DTYPE_F32 && out_dtype != GNNAGG_DTYPE_BF16) return bad("unknown out_dtype " + std::to_string(out_dtype));
    if (x_dtype == GNNAGG_DTYPE_F32 && out_dtype == GNNAGG_DTYPE_BF16) return bad("out_dtype: fp32 operands give a fp32 out, not a bf16 one");
    if (reduce != GNNAGG_REDUCE_SUM && reduce != GNNAGG_REDUCE_MEAN && reduce != GNNAGG_REDUCE_MAX)
        return bad("unknown reduce " + std::to_string(reduce));
    if (flags & ~GNNAGG_FLAG_RELU) return bad("flags = " + std::to_string(flags) + ": GNNAGG_FLAG_RELU is the only flag");
    if (!std::isfinite(self_scale)) return bad("self_scale = " + std::to_string(self_scale) + " is not finite");
    if (eid && !val) return bad("d_eid needs d_val (d_eid indexes it)");
    if (!gin_supported(feat, hidden, n_out, x_dtype))
        return bad("feat = " + std::to_string(feat) + ", hidden = " + std::to_string(hidden) + ", n_out = " + std::to_string(n_out) +
                   " lie outside the range of gnnagg_block_gin_supported");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!x) return bad("d_x is null");
        if (!w1) return bad("d_w1 is null");
        if (!w2) return bad("d_w2 is null");
        if (!out) return bad("d_out is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: the rule of gnnagg_block_gcn_run for x (a divisor of feat and of the pitch, no wider than x's alignment); the tile
    // rows in LDS are aligned for any lane.  Groups of 8 lanes run as groups of 16: 16 groups are the 16 rows of a tile.
    const int fp = (int)gcd_ll(feat, x_pitch);
    Geometry g = x16 ? typed_geometry(feat, x, 2, fp) : pick_geometry(feat, x, nullptr, nullptr, fp);
    if (g.group < 16) g.group = 16;
    GinArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.eid = eid; a.val = val;
    a.x = x; a.w1 = w1; a.w2 = w2; a.b1 = b1; a.b2 = b2; a.out = out; a.xpitch = x_pitch; a.self_scale = self_scale;
    a.num_dst = num_dst; a.feat = feat; a.hidden = hidden; a.n_out = n_out; a.ntiles = g.ntiles;
    a.mean = reduce == GNNAGG_REDUCE_MEAN; a.relu = (flags & GNNAGG_FLAG_RELU) != 0;
    a.out_bf16 = out_dtype == GNNAGG_DTYPE_BF16;
    a.row_tiles = ceil_div(num_dst, kGinRows);
    const int is_max = reduce == GNNAGG_REDUCE_MAX, mapped = src != nullptr || eid != nullptr;
    const int grid = std::min(a.row_tiles, gin_grid_cap(feat, hidden, n_out, x_dtype));
    const size_t lds = (size_t)gin_lds(feat, hidden, n_out, x16).bytes;
    hipStream_t st = (hipStream_t)stream;
    int rc = GNNAGG_OK;
    if (x16) {
        DISPATCH_GEOM_16BIT(g, (rc = launch_gin<VEC, GROUP, __bf16>(a, is_max, mapped, grid, lds, st)))
    } else {
        DISPATCH_GEOM(g, (rc = launch_gin<VEC, GROUP, float>(a, is_max, mapped, grid, lds, st)))
    }
    return rc;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_gin_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const float *d_val, const int *d_eid,
                         const void *d_x, int x_dtype, long long x_pitch, int feat, float self_scale, const void *d_w1, const float *d_b1,
                         int hidden, const void *d_w2, const float *d_b2, int n_out, void *d_out, int out_dtype, int reduce, int flags,
                         void *hip_stream)
{
    return block_gin_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_val, d_eid, d_x, x_dtype, x_pitch, feat, self_scale, d_w1, d_b1, hidden,
                         d_w2, d_b2, n_out, d_out, out_dtype, reduce, flags, hip_stream);
}

int gnnagg_block_gin_supported(int feat, int hidden, int n_out, int x_dtype) { return gin_supported(feat, hidden, n_out, x_dtype) ? 1 : 0; }

int gnnagg_block_gin_grid_cap(int feat, int hidden, int n_out, int x_dtype)
{
    return gin_supported(feat, hidden, n_out, x_dtype) ? gin_grid_cap(feat, hidden, n_out, x_dtype) : 0;
}

}  // extern "C"
#pragma GCC visibility pop
