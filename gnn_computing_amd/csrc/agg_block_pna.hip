// agg_block_pna.hip -- a PNA layer on ONE sampled block in one launch: gnnagg_block_pna_run (include/gnnagg.h section F, "Block PNA layer").
//
//   out[i] = act( cat[x_dst[i], M[i]] . cat[W_self; W] + bias ),   M [num_dst, S * A * feat] = gnnagg_gcn_run_multi on the block
//
// PyG's PNAConv / MultiAggregation with a linear post-transform: A of sum / mean / min / max / var / std of the row's messages
// m_p = val_p * x_src(p), each times S of the degree scalers identity / amplification / attenuation.  The frame is that of k_block_sage
// (agg_block_sage.hip): 256 threads, tiles of kPnaRows = 16 destination rows, the tiles blockIdx.x, blockIdx.x + gridDim.x, ... per
// workgroup.  What is new: a scaler is ONE fp32 scalar per row, so the LDS tile holds only the A UNSCALED aggregates (1 + A slots of Fp
// columns) while the product runs over 1 + S * A weight slabs.
//   phase 1  one lane group per row: the self row's load is issued, the row's edges are walked ONCE through the block's maps (the window
//            prefetch and shuffle broadcast of chain_block_edges) into up to four accumulator sets per lane -- S1 the plain add chain, S2
//            the chain fmaf(m, m, S2), mn / mx skipping NaN: the arithmetic of multi_walk (agg_multi.hip), contraction off -- the A
//            selected aggregates are finished with the expressions of multi_store_row and stored to slots 1 .. A (bf16: one rounding of
//            the unscaled value); lane 0 stores the row's two scalars amp = logf(d + 1) / delta and att = delta / logf(d + 1) (0 and 0
//            for a row without edges: its slots hold +0, and 0 * 0 leaves them so where delta / logf(1) would have made a NaN).
//   phase 2  after ONE barrier the 4 wavefronts take 16 x 16 output sub-tiles.
//            fp32: ONE accumulator on v_mfma_f32_16x16x4_f32, k ascending over the self slab and then, scaler-major, the S * A slabs of W
//            through buffer loads.  In this MFMA's A layout a lane holds one row, so the A operand of slab (s, a) is the tile's slot a
//            times the lane's row scalar: the one v_mul_f32 the composition performs before it stores M, then the ascending-k fmaf chain
//            of gnnagg_matmul_nn over the same values -- bit for bit.  No multiply for identity.
//            bf16: v_mfma_f32_16x16x32_bf16 against an image wimg[n][k] of all 1 + S * A slabs, staged once per workgroup, one
//            ds_read_b128 per operand; one fp32 accumulator PER SELECTED SCALER, joined in the epilogue in fp32 with the row scalars read
//            per D-register row: out = acc_id(+ self) + amp * acc_amp + att * acc_att.  The scaler never passes a bf16 rounding.
//   epilogue + bias, ReLU, one store per element (a bf16 out: one round-to-nearest-even).
// A second barrier ends the tile: phase 1 of the next tile overwrites the tile, tile_rows and the row scalars, so ONE copy of each suffices.
// M never reaches HBM, x_dst is never copied, nothing is concatenated.  No atomics, no scratch; every lane's address is a function of the
// arguments, and so is the result.
#include "block_chain.cuh"

namespace gnnagg {
namespace {

constexpr int kPnaThreads = 256;            // 4 wavefronts
constexpr int kPnaRows = 16;                // destination rows of a tile: one MFMA row block
constexpr int kPnaLdsBytes = 160 * 1024;    // LDS of a CU: the budget of tile + weight image
constexpr int kPnaMaxDim = 256;             // feat and n_out
constexpr int kPnaPerCu = 8;                // workgroups per CU the grid is capped at (fewer where the LDS of a workgroup allows fewer)
constexpr int kPnaAggrBits = 6, kPnaScalerBits = 3;
constexpr int kPnaAllAggr = (1 << kPnaAggrBits) - 1, kPnaAllScalers = (1 << kPnaScalerBits) - 1;
constexpr int kPnaNeedS2 = GNNAGG_AGGR_VAR | GNNAGG_AGGR_STD, kPnaNeedMM = GNNAGG_AGGR_MIN | GNNAGG_AGGR_MAX;

struct PnaArgs {
    const int *ptr, *idx, *src, *eid;
    const float *val;
    const void *x, *wself, *w;
    const float *bias;
    void *out;
    long long xpitch;   // elements between rows of x
    float delta;
    int num_dst, feat, n_out, ntiles, relu, out_bf16, row_tiles, aggr_mask, scaler_mask, n_aggr, n_scaler;
};

// The LDS of a launch, kernel and launcher agree through pna_lds:
//   [tile_rows: 16 ints][row scalars: 16 x {amp, att}][tile: 16 rows of `pitch`][bf16: wimg, roundup16(n_out) rows of `wpitch`]
// fp: feat rounded up to the MFMA's k block (4 fp32, 32 bf16).  A tile row is 1 + A slots of fp columns (self, a_0 .. a_{A-1}), an image
// row 1 + S * A.  The pitches: roundup8(k) + 4 floats -- the 16 rows of an A operand start on 8 different multiples of 4 banks, two lanes
// per bank -- or k + 8 bf16: an odd number of 16-byte slots, so the 16 rows (columns) a b128 lane group reads fall on 16 different slots.
struct PnaLds {
    int fp, pitch, wpitch, tile_off, w_off, bytes;
};
constexpr int kPnaScalOff = kPnaRows * (int)sizeof(int);
__host__ __device__ constexpr PnaLds pna_lds(int feat, int n_out, int n_aggr, int n_scaler, bool b16)
{
    PnaLds l = {};
    l.fp = b16 ? (feat + 31) & ~31 : (feat + 3) & ~3;
    const int kt = (1 + n_aggr) * l.fp, kw = (1 + n_scaler * n_aggr) * l.fp;
    l.pitch = b16 ? kt + 8 : ((kt + 7) & ~7) + 4;
    l.wpitch = kw + 8;
    l.tile_off = kPnaScalOff + kPnaRows * 2 * (int)sizeof(float);
    l.w_off = l.tile_off + kPnaRows * l.pitch * (b16 ? 2 : 4);
    l.bytes = l.w_off + (b16 ? ((n_out + 15) & ~15) * l.wpitch * 2 : 0);
    return l;
}

static bool pna_supported(int feat, int n_out, int n_aggr, int n_scaler, int x_dtype)
{
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return false;
    if (feat < 1 || feat > kPnaMaxDim || n_out < 1 || n_out > kPnaMaxDim) return false;
    if (n_aggr < 1 || n_aggr > kPnaAggrBits || n_scaler < 1 || n_scaler > kPnaScalerBits) return false;
    return pna_lds(feat, n_out, n_aggr, n_scaler, x_dtype == GNNAGG_DTYPE_BF16).bytes <= kPnaLdsBytes;
}

// workgroups a launch of this shape is capped at: as many per CU as their LDS allows, kPnaPerCu at the most
static int pna_grid_cap(int feat, int n_out, int n_aggr, int n_scaler, int x_dtype)
{
    const int per_cu = kPnaLdsBytes / pna_lds(feat, n_out, n_aggr, n_scaler, x_dtype == GNNAGG_DTYPE_BF16).bytes;
    return std::min(std::max(per_cu, 1), kPnaPerCu) * device_cu_count();
}

typedef __bf16 pna_bf16x8 __attribute__((ext_vector_type(8)));

// One weight slab into its k range of the image: wimg[n][0 .. kp) = W[0 .. K)[n] for the columns n < roundup16(N), zeros beyond K and N (wimg
// already points at the slab's first k).  The two paths of stage_weight_half (agg_block_sage.hip): where N % 8 == 0 and W is 16-byte
// aligned one thread per 8 k x 8 columns -- eight 16-byte row pieces transposed in registers, one 16-byte LDS store per column; else one
// thread per (column, 8 k) with 2-byte loads.  Both write the same image.
__device__ __forceinline__ void stage_weight_slab(__bf16 *wimg, int wpitch, int kp, const __bf16 *__restrict__ W, int K, int N)
{
    const unsigned short *Wu = reinterpret_cast<const unsigned short *>(W);
    const int ncols = (N + 15) & ~15;
    if ((N & 7) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
        const int nco = ncols >> 3;
        for (int i = threadIdx.x; i < nco * (kp >> 3); i += kPnaThreads) {
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
    for (int i = threadIdx.x; i < ncols * (kp >> 3); i += kPnaThreads) {
        const int n = i % ncols, k = (i / ncols) << 3;
        unsigned q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (n < N && k + j < K) ? (unsigned)Wu[(size_t)(k + j) * N + n] : 0u;
        *reinterpret_cast<uint4 *>(wimg + (size_t)n * wpitch + k) =
            make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
    }
}

// fp32: acc += (sc * arow[0 .. K)) . W[0 .. K)[col], k ascending, for one slab: the branch-free batches of half_times_weight
// (agg_block_sage.hip) with the row scalar on the A operand (SCALED = false: the slot as it is, no multiply).  arow: this lane's tile row at
// its k offset kq = lane / 16 (A: row = lane % 16, k = lane / 16; B: k = lane / 16, col = lane % 16); the slot's columns [K, roundup4(K))
// hold 0.  W operands as buffer loads: the per-lane byte offset in one VGPR (out of range for the padding columns, which then read 0), the
// k step in an SGPR.  k quads past K inside a batch are clamped loads with zeroed operands: 0 * 0 leaves the chain as it is (an
// accumulator that started at +0 is never -0).
template <int KB, bool SCALED>
__device__ __forceinline__ void slab_times_weight(f32x4 &acc, const float *arow, float sc, const float *W, int K, int N, int col, bool cok, int kq)
{
#pragma clang fp contract(off)
    const int Kf = K & ~3;     // k covered by whole quads
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0, K * N * 4, 0x00020000);
    const int voff = cok ? (kq * N + col) * 4 : 0x7ffffff0;
#pragma unroll 1
    for (int k0 = 0; k0 < Kf; k0 += 4 * KB) {
        float av[KB], bv[KB];
#pragma unroll
        for (int t = 0; t < KB; ++t) {
            const int kk = k0 + 4 * t, kc = kk < Kf ? kk : Kf - 4;
            const float b = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrsrc, voff, kc * N * 4, 0));
            bv[t] = kk < Kf ? b : 0.f;
        }
#pragma unroll
        for (int t = 0; t < KB; ++t) {
            const int kk = k0 + 4 * t, kc = kk < Kf ? kk : Kf - 4;
            const float v = SCALED ? arow[kc] * sc : arow[kc];
            av[t] = kk < Kf ? v : 0.f;
        }
#pragma unroll
        for (int t = 0; t < KB; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[t], acc, 0, 0, 0);
    }
    if (K != Kf) {  // ragged last quad: k = Kf + kq valid only below K (the slot's padding columns hold 0)
        const float b = (cok && Kf + kq < K) ? W[(size_t)(Kf + kq) * N + col] : 0.f;
        const float v = Kf + kq < K ? (SCALED ? arow[Kf] * sc : arow[Kf]) : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v, b, acc, 0, 0, 0);
    }
}

// The four chains of one lane group over edges [beg, end) of its row, for the lane's VEC columns at xcol: the window of
// chain_block_edges (block_chain.cuh) -- lane j loads idx[p] of its edge and does the dependent loads through the block's maps, the next
// window's metadata is prefetched while this window's gathers run, ids and weights are broadcast inside the group, UNROLL gathers are
// issued before the first is consumed -- around the arithmetic of multi_walk (agg_multi.hip): the message is ONE fp32 multiply, S1 a plain
// add, S2 an fma, min and max skip NaN.  Lanes with col_ok == false still carry metadata.  Control flow is uniform over the group.
template <int VEC, int GROUP, bool MAPPED, int UNROLL, typename TX, bool S2, bool MM>
__device__ __forceinline__ void pna_walk(float (&s1)[VEC], float (&s2)[VEC], float (&mn)[VEC], float (&mx)[VEC], int beg, int end, int lane,
                                         bool col_ok, const int *__restrict__ idx, const int *__restrict__ src, const float *__restrict__ val,
                                         const int *__restrict__ eid, const TX *__restrict__ xcol, long long pitch)
{
#pragma clang fp contract(off)
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
    float my_w = 1.0f;   // (no val: x * 1.0f is x)
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
            // the batch's edges in CSR order
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if (j + u < n && col_ok) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float m = w[u] * xv[u].at(k);
                        s1[k] = s1[k] + m;
                        if constexpr (S2) s2[k] = __builtin_fmaf(m, m, s2[k]);
                        if constexpr (MM) {
                            mn[k] = m < mn[k] ? m : mn[k];
                            mx[k] = m > mx[k] ? m : mx[k];
                        }
                    }
                }
        }
        my_s = nx_s;
        my_w = nx_w;
    }
}

// A finished row piece (VEC columns) into the tile's aggregate slots, aslot = the lane's columns of slot 1: the selected aggregates in
// ascending bit order, each computed once with the expressions of multi_store_row (agg_multi.hip) and stored UNSCALED.  deg == 0: +0
// everywhere.  var and std keep a NaN, min and max of NaN messages alone are NaN, a NaN is stored as the quiet NaN.
template <int VEC, typename TX>
__device__ __forceinline__ void pna_store_slots(TX *aslot, int Fp, int aggr_mask, int deg, const float (&s1)[VEC], const float (&s2)[VEC],
                                                const float (&mn)[VEC], const float (&mx)[VEC])
{
#pragma clang fp contract(off)
    const float dg = (float)deg;
    for (int t = 0; t < kPnaAggrBits; ++t) {
        if (!((aggr_mask >> t) & 1)) continue;
        float v[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float r = 0.0f;
            if (deg > 0) {
                if (t == 0) r = s1[k];
                else if (t == 1) r = s1[k] / dg;
                else if (t == 2 || t == 3) {
                    r = mn[k] > mx[k] ? __builtin_nanf("") : t == 2 ? mn[k] : mx[k];   // the seeds survive NaN messages alone
                } else {
                    const float mu = s1[k] / dg;
                    const float q = s2[k] / dg;
                    const float d = q - mu * mu;    // the two-moment form, clamped: cancellation may leave it below zero
                    r = d < 0.0f ? 0.0f : d;        // (not fmaxf, which drops a NaN)
                    if (t == 5) r = sqrtf(r);
                }
            }
            v[k] = r != r ? __builtin_nanf("") : r;
        }
        if constexpr (std::is_same<TX, __bf16>::value) store_pack_bf16<VEC>(aslot, v, VEC);
        else store_pack<VEC>(aslot, v);
        aslot += Fp;
    }
}

template <int VEC, int GROUP, bool MAPPED, typename TX, bool S2, bool MM>
__global__ __launch_bounds__(kPnaThreads) void k_block_pna(const PnaArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int GPB = kPnaThreads / GROUP, PASSES = kPnaRows / GPB;
    static_assert(GROUP >= 16 && PASSES * GPB == kPnaRows, "whole passes over the 16 rows of a tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char pna_smem[];
    const int F = a.feat, N = a.n_out, A = a.n_aggr;
    const PnaLds L = pna_lds(F, N, A, a.n_scaler, B16);
    const int Fp = L.fp, pitch = L.pitch;
    int *tile_rows = reinterpret_cast<int *>(pna_smem);
    float *scal = reinterpret_cast<float *>(pna_smem + kPnaScalOff);   // [row]{amp, att}
    TX *tile = reinterpret_cast<TX *>(pna_smem + L.tile_off);
    const int lane = (int)threadIdx.x % GROUP, grp = (int)threadIdx.x / GROUP;
    const bool with_self = a.wself != nullptr;
    const bool scaled = (a.scaler_mask & ~GNNAGG_SCALER_IDENTITY) != 0;

    // once per workgroup: the k padding of every slot (no row store reaches it: a lane's VEC columns lie below feat) ...
    const int npad = Fp - F;
    for (int i = threadIdx.x; i < kPnaRows * (1 + A) * npad; i += kPnaThreads) {
        const int r = i / ((1 + A) * npad), c = i % ((1 + A) * npad);
        tile[r * pitch + (c / npad) * Fp + F + c % npad] = (TX)0.0f;
    }
    // ... and, bf16, the image of all weights: k over [W_self; zeros to Fp][W slab 0; zeros][W slab 1; zeros] ...
    const __bf16 *wimg = nullptr;
    if constexpr (B16) {
        __bf16 *img = reinterpret_cast<__bf16 *>(pna_smem + L.w_off);
        if (with_self) stage_weight_slab(img, L.wpitch, Fp, static_cast<const __bf16 *>(a.wself), F, N);
        for (int j = 0; j < a.n_scaler * A; ++j)
            stage_weight_slab(img + (1 + j) * Fp, L.wpitch, Fp, static_cast<const __bf16 *>(a.w) + (size_t)j * F * N, F, N);
        wimg = img;
    }

#pragma unroll 1
    for (int rt = (int)blockIdx.x; rt < a.row_tiles; rt += (int)gridDim.x) {
        // ---- phase 1: rows into the tile
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int slot = pass * GPB + grp;
            const int row = rt * kPnaRows + slot;
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
                if (live && with_self && col_ok) self = load_pack<VEC>(xcol + srow * (size_t)a.xpitch);   // in flight over the walk
                float s1[VEC], s2[VEC], mn[VEC], mx[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    s1[k] = 0.0f; s2[k] = 0.0f;
                    mn[k] = INFINITY; mx[k] = -INFINITY;
                }
                pna_walk<VEC, GROUP, MAPPED, kUnroll, TX, S2, MM>(s1, s2, mn, mx, beg, end, lane, col_ok, a.idx, a.src, a.val, a.eid, xcol, a.xpitch);
                if (!col_ok) continue;
                if (with_self) store_raw_pack<VEC, TX>(trow + col, self);
                pna_store_slots<VEC, TX>(trow + Fp + col, Fp, a.aggr_mask, end - beg, s1, s2, mn, mx);
            }
            if (lane == 0) {
#pragma clang fp contract(off)
                tile_rows[slot] = live ? row : -1;
                float amp = 0.0f, att = 0.0f;   // a row without edges: its slots are +0 and stay so
                if (end > beg && scaled) {
                    const float lg = logf((float)(end - beg) + 1.0f);
                    amp = lg / a.delta;
                    att = a.delta / lg;
                }
                scal[2 * slot] = amp;
                scal[2 * slot + 1] = att;
            }
        }
        __syncthreads();   // the tile and its rows' scalars (and, the first time, the padding and the image) are complete

        // ---- phase 2: 16 x 16 output sub-tiles
        const int wave = (int)threadIdx.x >> 6, wl = (int)threadIdx.x & 63, kq = wl >> 4;
#pragma unroll 1
        for (int cb = wave; cb < (N + 15) >> 4; cb += kPnaThreads >> 6) {
            const int col = cb * 16 + (wl & 15);
            const bool cok = col < N;
            const float bias = (a.bias && cok) ? a.bias[col] : 0.0f;
            float res[4];
            if constexpr (B16) {
#pragma clang fp contract(off)
                const __bf16 *ap = tile + (wl & 15) * pitch + 8 * kq;
                const __bf16 *bp = wimg + (size_t)col * L.wpitch + 8 * kq;
                f32x4 acc[kPnaScalerBits] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
                if (with_self)
                    for (int k0 = 0; k0 < Fp; k0 += 32)
                        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const pna_bf16x8 *>(ap + k0),
                                                                         *reinterpret_cast<const pna_bf16x8 *>(bp + k0), acc[0], 0, 0, 0);
                int wk = Fp;   // the image's k of the next slab
#pragma unroll
                for (int s = 0; s < kPnaScalerBits; ++s) {
                    if (!((a.scaler_mask >> s) & 1)) continue;
                    for (int k0 = Fp; k0 < (1 + A) * Fp; k0 += 32, wk += 32)
                        acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const pna_bf16x8 *>(ap + k0),
                                                                         *reinterpret_cast<const pna_bf16x8 *>(bp + wk), acc[s], 0, 0, 0);
                }
                // D layout: col = lane % 16, row = 4 * (lane / 16) + reg; the scalers join here, in fp32
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float o = acc[0][v];
                    if (a.scaler_mask & GNNAGG_SCALER_AMPLIFICATION) o = o + scal[2 * (4 * kq + v)] * acc[1][v];
                    if (a.scaler_mask & GNNAGG_SCALER_ATTENUATION) o = o + scal[2 * (4 * kq + v) + 1] * acc[2][v];
                    res[v] = o;
                }
            } else {
                constexpr int KB = GROUP * VEC >= 128 ? 32 : GROUP * VEC / 4;
                const float *arow = tile + (wl & 15) * pitch + kq;
                const float *W = static_cast<const float *>(a.w);
                const float amp = scal[2 * (wl & 15)], att = scal[2 * (wl & 15) + 1];   // A layout: this lane's row
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if (with_self) slab_times_weight<KB, false>(acc, arow, 1.0f, static_cast<const float *>(a.wself), F, N, col, cok, kq);
#pragma unroll 1
                for (int s = 0; s < kPnaScalerBits; ++s) {
                    if (!((a.scaler_mask >> s) & 1)) continue;
                    const float sc = s == 1 ? amp : att;
#pragma unroll 1
                    for (int j = 1; j <= A; ++j, W += (size_t)F * N) {
                        if (s == 0) slab_times_weight<KB, false>(acc, arow + j * Fp, 1.0f, W, F, N, col, cok, kq);
                        else slab_times_weight<KB, true>(acc, arow + j * Fp, sc, W, F, N, col, cok, kq);
                    }
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) res[v] = acc[v];
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = tile_rows[4 * kq + v];
                if (r < 0 || !cok) continue;
                float o = res[v];
                if (a.bias) o += bias;
                if (a.relu) o = o < 0.0f ? 0.0f : o;   // (a NaN stays a NaN: relu_pack)
                if (a.out_bf16) static_cast<__bf16 *>(a.out)[(size_t)r * N + col] = (__bf16)o;
                else static_cast<float *>(a.out)[(size_t)r * N + col] = o;
            }
        }
        __syncthreads();   // before the next tile overwrites this one, its tile_rows and its scalars
    }
}

template <int VEC, int GROUP, bool MAPPED, typename TX, bool S2, bool MM>
static int launch_pna_inst(const PnaArgs &a, int grid, size_t lds, hipStream_t st)
{
    static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (lds > 64 * 1024 && big_lds_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_block_pna<VEC, GROUP, MAPPED, TX, S2, MM>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kPnaLdsBytes));
        big_lds_ok.done();
    }
    hipLaunchKernelGGL((k_block_pna<VEC, GROUP, MAPPED, TX, S2, MM>), dim3((unsigned)grid), dim3(kPnaThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// the arm of the walk that keeps what the mask needs: S1 always, S2 for var / std, mn and mx for min / max
template <int VEC, int GROUP, typename TX>
static int launch_pna(const PnaArgs &a, int mapped, int grid, size_t lds, hipStream_t st)
{
    if constexpr (GROUP < 16) {
        return fail(GNNAGG_ERR_STATE, "internal: gnnagg_block_pna_run runs groups of 16 lanes and more");
    } else {
        const int arm = ((a.aggr_mask & kPnaNeedS2) ? 2 : 0) + ((a.aggr_mask & kPnaNeedMM) ? 1 : 0);
        if (mapped) {
            switch (arm) {
                case 0: return launch_pna_inst<VEC, GROUP, true, TX, false, false>(a, grid, lds, st);
                case 1: return launch_pna_inst<VEC, GROUP, true, TX, false, true>(a, grid, lds, st);
                case 2: return launch_pna_inst<VEC, GROUP, true, TX, true, false>(a, grid, lds, st);
                default: return launch_pna_inst<VEC, GROUP, true, TX, true, true>(a, grid, lds, st);
            }
        }
        switch (arm) {
            case 0: return launch_pna_inst<VEC, GROUP, false, TX, false, false>(a, grid, lds, st);
            case 1: return launch_pna_inst<VEC, GROUP, false, TX, false, true>(a, grid, lds, st);
            case 2: return launch_pna_inst<VEC, GROUP, false, TX, true, false>(a, grid, lds, st);
            default: return launch_pna_inst<VEC, GROUP, false, TX, true, true>(a, grid, lds, st);
        }
    }
}

static int block_pna_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const float *val, const int *eid, const void *x,
                         int x_dtype, long long x_pitch, int feat, int aggr_mask, int scaler_mask, float delta, const void *w_self, const void *w,
                         const float *bias, int n_out, void *out, int out_dtype, int flags, void *stream)
{
    static const char *who = "gnnagg_block_pna_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    if (num_dst < 0) return bad("num_dst = " + std::to_string(num_dst) + " is negative");
    if (feat < 1) return bad("feat = " + std::to_string(feat) + " must be >= 1");
    if (n_out < 1) return bad("n_out = " + std::to_string(n_out) + " must be >= 1");
    if (x_pitch < feat) return bad("x_pitch = " + std::to_string(x_pitch) + " is below feat = " + std::to_string(feat));
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (out_dtype != GNNAGG_DTYPE_F32 && out_dtype != GNNAGG_DTYPE_BF16) return bad("unknown out_dtype " + std::to_string(out_dtype));
    if (x_dtype == GNNAGG_DTYPE_F32 && out_dtype == GNNAGG_DTYPE_BF16) return bad("out_dtype: fp32 operands give a fp32 out, not a bf16 one");
    if (aggr_mask == 0 || (aggr_mask & ~kPnaAllAggr))
        return bad("aggr_mask = " + std::to_string(aggr_mask) + ": needs at least one and only GNNAGG_AGGR_* bits (1 .. " + std::to_string(kPnaAllAggr) + ")");
    if (scaler_mask == 0 || (scaler_mask & ~kPnaAllScalers))
        return bad("scaler_mask = " + std::to_string(scaler_mask) + ": needs at least one and only GNNAGG_SCALER_* bits (1 .. " +
                   std::to_string(kPnaAllScalers) + ")");
    if ((scaler_mask & ~GNNAGG_SCALER_IDENTITY) && !(std::isfinite(delta) && delta > 0.0f))
        return bad("delta = " + std::to_string(delta) + ": the amplification and attenuation scalers need a finite delta > 0");
    if (flags & ~GNNAGG_FLAG_RELU) return bad("flags = " + std::to_string(flags) + ": GNNAGG_FLAG_RELU is the only flag");
    if (eid && !val) return bad("d_eid needs d_val (d_eid indexes it)");
    const int n_aggr = __builtin_popcount((unsigned)aggr_mask), n_scaler = __builtin_popcount((unsigned)scaler_mask);
    if (!pna_supported(feat, n_out, n_aggr, n_scaler, x_dtype))
        return bad("feat = " + std::to_string(feat) + ", n_out = " + std::to_string(n_out) + " with " + std::to_string(n_aggr) + " aggregates x " +
                   std::to_string(n_scaler) + " scalers lie outside the range of gnnagg_block_pna_supported");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!x) return bad("d_x is null");
        if (!w) return bad("d_w is null");
        if (!out) return bad("d_out is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: the rule of gnnagg_block_gcn_run for x (a divisor of feat and of the pitch, no wider than x's alignment); the tile
    // rows in LDS are aligned for any lane.  Groups of 8 lanes run as groups of 16: 16 groups are the 16 rows of a tile.
    const int fp = (int)gcd_ll(feat, x_pitch);
    Geometry g = x16 ? typed_geometry(feat, x, 2, fp) : pick_geometry(feat, x, nullptr, nullptr, fp);
    if (g.group < 16) g.group = 16;
    PnaArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.eid = eid; a.val = val;
    a.x = x; a.wself = w_self; a.w = w; a.bias = bias; a.out = out; a.xpitch = x_pitch; a.delta = delta;
    a.num_dst = num_dst; a.feat = feat; a.n_out = n_out; a.ntiles = g.ntiles;
    a.relu = (flags & GNNAGG_FLAG_RELU) != 0; a.out_bf16 = out_dtype == GNNAGG_DTYPE_BF16;
    a.row_tiles = ceil_div(num_dst, kPnaRows);
    a.aggr_mask = aggr_mask; a.scaler_mask = scaler_mask; a.n_aggr = n_aggr; a.n_scaler = n_scaler;
    const int mapped = src != nullptr || eid != nullptr;
    const int grid = std::min(a.row_tiles, pna_grid_cap(feat, n_out, n_aggr, n_scaler, x_dtype));
    const size_t lds = (size_t)pna_lds(feat, n_out, n_aggr, n_scaler, x16).bytes;
    hipStream_t st = (hipStream_t)stream;
    int rc = GNNAGG_OK;
    if (x16) {
        DISPATCH_GEOM_16BIT(g, (rc = launch_pna<VEC, GROUP, __bf16>(a, mapped, grid, lds, st)))
    } else {
        DISPATCH_GEOM(g, (rc = launch_pna<VEC, GROUP, float>(a, mapped, grid, lds, st)))
    }
    return rc;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_pna_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const float *d_val, const int *d_eid,
                         const void *d_x, int x_dtype, long long x_pitch, int feat, int aggr_mask, int scaler_mask, float delta,
                         const void *d_w_self, const void *d_w, const float *d_bias, int n_out, void *d_out, int out_dtype, int flags,
                         void *hip_stream)
{
    return block_pna_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_val, d_eid, d_x, x_dtype, x_pitch, feat, aggr_mask, scaler_mask, delta,
                         d_w_self, d_w, d_bias, n_out, d_out, out_dtype, flags, hip_stream);
}

int gnnagg_block_pna_supported(int feat, int n_out, int n_aggr, int n_scaler, int x_dtype)
{
    return pna_supported(feat, n_out, n_aggr, n_scaler, x_dtype) ? 1 : 0;
}

int gnnagg_block_pna_grid_cap(int feat, int n_out, int n_aggr, int n_scaler, int x_dtype)
{
    return pna_supported(feat, n_out, n_aggr, n_scaler, x_dtype) ? pna_grid_cap(feat, n_out, n_aggr, n_scaler, x_dtype) : 0;
}

}  // extern "C"
#pragma GCC visibility pop
