// agg_block_rgcn_basis.hip -- a basis-decomposed relational GCN layer (RGCNConv(num_bases = B), RelGraphConv(regularizer = "basis")) on ONE
// sampled block in one launch: gnnagg_block_rgcn_basis_run (include/gnnagg.h section F, "Block R-GCN layer, basis decomposition").
//
//   W_r = sum_b comp[r][b] V_b, so the sum over relations moves in front of the matrix product:
//   out[i] = act( x_dst[i] . W_self + sum_{b < B} g_b[i] . V_b + bias )
//   g_b[i] = sum_{p in row i, 0 <= t_p < R} (comp[t_p][b] * s_p) x_src(p)        s_p = val_p (sum), val_p / n(i, t_p) (mean)
//
// The frame is k_block_rgcn's (agg_block_rgcn.hip): 256 threads, tiles of kBasisRows = 16 destination rows walked blockIdx.x,
// blockIdx.x + gridDim.x, ..., rows meeting in an LDS tile, one MFMA accumulator over stacked weights.  The tile row is
//   [ x_dst | g_0 | g_1 | ... | g_{B-1} ]          B + 1 slots of Fp columns WHATEVER R is (Fp = feat rounded up to the MFMA's k block)
//   once     comp [R][B] goes to LDS (the per-edge coefficient reads are broadcast reads of a lane group), the padding columns of the
//            slots are zeroed, bf16: the image of the stacked weights is transposed into LDS; one barrier.
//   phase 1  one lane group per row.  mean: the group first walks the row's TYPES only and counts them into its row of the [16][R] integer
//            table in LDS (integer adds: their order cannot change the result).  Then it walks the row's edges in CSR order with the window,
//            prefetch and broadcast of chain_block_edges, the type travelling with the id and the weight; the lane that loads an edge's
//            metadata does the one division s_p = val_p / (float) n.  Every lane holds BC x VEC fp32 accumulators -- BC bases, its VEC
//            columns -- and every gathered pack of x feeds BC fused multiply-adds: c = comp[t][b] * s_p (one fp32 multiply),
//            acc[b][k] = fmaf(x[k], c, acc[b][k]).  Nothing is stored or reloaded when the relation changes; at the end of a pass the lane
//            writes its finished sums ONCE into its own columns of the slots (bf16: rounded once, by the conversion of a bf16 y store;
//            there is no fp32 area beside a bf16 tile).  B > BC: further passes over the row take the next BC bases; a basis past B in the
//            last pass is not computed (never run with a zero coefficient: 0 * Inf would poison it).  A type outside [0, R) is skipped:
//            its row of x is never read, it is never counted.
//   phase 2  after ONE barrier the 4 wavefronts take 16 x 16 output sub-tiles; ONE fp32 accumulator runs k ascending over the self slot,
//            then b = 0 .. B-1: fp32 on v_mfma_f32_16x16x4_f32 with V through buffer loads, bf16 on v_mfma_f32_16x16x32_bf16 against the
//            image wimg[n][k] of the stacked [(B + 1) Fp, n_out] weights.
//   epilogue + bias, ReLU (a NaN stays a NaN), one store per element.
// BC (basis_chunk): the LDS of a workgroup -- 70 KB and more at the shapes the layer is for -- already leaves one to three workgroups
// per CU, three wavefronts per SIMD at the most and 168 VGPRs each, so a lane holds 64 accumulators beside its 8 gathers in flight: BC = 16
// for lanes of 1, 2 and 4 columns, 8 for the 8-column lanes of bf16 (profiles/block_rgcn_basis/kernel_resources.txt).
// Pitches as in agg_block_rgcn.hip with B for R.  No scratch, no floating-point atomics; the result is a function of the arguments alone.
#include "block_chain.cuh"

namespace gnnagg {
namespace {

constexpr int kBasisThreads = 256;            // 4 wavefronts
constexpr int kBasisRows = 16;                // destination rows of a tile: one MFMA row block
constexpr int kBasisLdsBytes = 160 * 1024;    // LDS of a CU: the budget of counts + comp + tile + weight image
constexpr int kBasisMaxDim = 256;             // feat and n_out
constexpr int kBasisMaxRel = 2560;            // (past it the counts alone are above the budget; keeps the sizes inside int)
constexpr int kBasisMaxBases = 640;           // (past it the fp32 tile of feat = 1 is alone above the budget)
constexpr int kBasisPerCu = 8;                // workgroups per CU the grid is capped at (fewer where the LDS of a workgroup allows fewer)

// bases a lane accumulates in one pass over a row: 64 accumulators for the widest lanes
constexpr int basis_chunk(int vec) { return vec == 8 ? 8 : 16; }

struct BasisArgs {
    const int *ptr, *idx, *src, *etype, *teid, *veid;   // teid / veid: the eid map of etype / val, or null
    const float *val, *comp;
    const void *x, *wself, *bases;
    const float *bias;
    void *out;
    long long xpitch;   // elements between rows of x
    int num_dst, feat, n_out, num_rel, num_bases, ntiles, mean, relu, out_bf16, row_tiles;
};

// The LDS of a launch, kernel and launcher agree through this:
//   [tile_rows: 16 ints][cnt: 16 x R ints][comp: R x B floats][tile: 16 rows of `pitch`][bf16: the weight image, roundup16(n_out) rows]
struct BasisLds {
    int fp, pitch, cnt_off, comp_off, tile_off, wimg_off, bytes;
};
__host__ __device__ inline BasisLds basis_lds(int feat, int n_out, int R, int B, bool b16)
{
    BasisLds l;
    l.fp = b16 ? (feat + 31) & ~31 : (feat + 3) & ~3;
    l.pitch = b16 ? (B + 1) * l.fp + 8 : (((B + 1) * l.fp + 7) & ~7) + 4;
    l.cnt_off = kBasisRows * (int)sizeof(int);
    l.comp_off = l.cnt_off + ((kBasisRows * R * (int)sizeof(int) + 15) & ~15);
    l.tile_off = l.comp_off + ((R * B * (int)sizeof(float) + 15) & ~15);
    l.wimg_off = l.tile_off + kBasisRows * l.pitch * (b16 ? 2 : 4);
    l.bytes = l.wimg_off + (b16 ? ((n_out + 15) & ~15) * l.pitch * 2 : 0);
    return l;
}

static bool basis_supported(int feat, int n_out, int num_rel, int num_bases, int x_dtype)
{
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return false;
    if (feat < 1 || feat > kBasisMaxDim || n_out < 1 || n_out > kBasisMaxDim) return false;
    if (num_rel < 1 || num_rel > kBasisMaxRel || num_bases < 1 || num_bases > kBasisMaxBases) return false;
    return basis_lds(feat, n_out, num_rel, num_bases, x_dtype == GNNAGG_DTYPE_BF16).bytes <= kBasisLdsBytes;
}

// workgroups a launch of this shape is capped at: as many per CU as their LDS allows, kBasisPerCu at the most
static int basis_grid_cap(int feat, int n_out, int num_rel, int num_bases, int x_dtype)
{
    const int per_cu = kBasisLdsBytes / basis_lds(feat, n_out, num_rel, num_bases, x_dtype == GNNAGG_DTYPE_BF16).bytes;
    return std::min(std::max(per_cu, 1), kBasisPerCu) * device_cu_count();
}

typedef __bf16 basis_bf16x8 __attribute__((ext_vector_type(8)));

// stage_weight_slot of agg_block_rgcn.hip (a copy: that object stays as it is).  One weight into its slot of the image:
// wimg[n][0 .. kp) = W[0 .. K)[n] for the columns n < roundup16(N), zeros beyond K and N.  Where N % 8 == 0 and W is 16-byte aligned one
// thread per 8 k x 8 columns, transposed in registers; else one thread per (column, 8 k) with 2-byte loads.  Both write the same image.
__device__ __forceinline__ void stage_basis_slot(__bf16 *wimg, int wpitch, int kp, const __bf16 *__restrict__ W, int K, int N)
{
    const unsigned short *Wu = reinterpret_cast<const unsigned short *>(W);
    const int ncols = (N + 15) & ~15;
    if ((N & 7) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
        const int nco = ncols >> 3;
        for (int i = threadIdx.x; i < nco * (kp >> 3); i += kBasisThreads) {
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
    for (int i = threadIdx.x; i < ncols * (kp >> 3); i += kBasisThreads) {
        const int n = i % ncols, k = (i / ncols) << 3;
        unsigned q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (n < N && k + j < K) ? (unsigned)Wu[(size_t)(k + j) * N + n] : 0u;
        *reinterpret_cast<uint4 *>(wimg + (size_t)n * wpitch + k) =
            make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
    }
}

// slot_times_weight of agg_block_rgcn.hip (a copy).  acc += arow[0 .. K) . W[0 .. K)[col], k ascending, for one slot of the tile, the
// accumulator carried in and out.  arow: this lane's tile row at its k offset kq = lane / 16; the slot's columns [K, roundup4(K)) hold 0.
// W operands as buffer loads (out of range for the padding columns, which then read 0); k-quads past K inside a batch are clamped loads
// with zeroed operands: 0 * 0 leaves the chain as it is.
template <int KB>
__device__ __forceinline__ void basis_slot_times_weight(f32x4 &acc, const float *arow, const float *W, int K, int N, int col, bool cok, int kq)
{
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
            const float v = arow[kc];
            av[t] = kk < Kf ? v : 0.f;
        }
#pragma unroll
        for (int t = 0; t < KB; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[t], acc, 0, 0, 0);
    }
    if (K != Kf) {  // ragged last quad: k = Kf + kq valid only below K (the slot's padding columns hold 0)
        const float b = (cok && Kf + kq < K) ? W[(size_t)(Kf + kq) * N + col] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[Kf], b, acc, 0, 0, 0);
    }
}

// what one lane of a group wrote to the group's LDS is what another lane of it reads next: a group lies inside one wavefront
__device__ __forceinline__ void basis_group_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// chain_block_edges with a type per edge and BC sums per lane.  acc[b]: this lane's VEC columns of g_{b0 + b}, zeroed by the caller;
// comp: the LDS copy of comp at column b0 (row pitch num_bases); cnt: the row's R counts (mean; read by the lane that loads an edge).
// FULL: all BC bases; else the first nb < BC, the others are not computed.  Lanes with col_ok == false carry metadata only.
template <int VEC, int GROUP, bool MAPPED, int BC, bool FULL, int UNROLL, typename TX>
__device__ __forceinline__ void chain_basis_edges(float (&acc)[BC][VEC], int nb, int beg, int end, int lane, bool col_ok, const BasisArgs &a,
                                                  const TX *__restrict__ xcol, const float *comp, const int *cnt)
{
    const unsigned R = (unsigned)a.num_rel;
    const int B = a.num_bases;
    auto edge_meta = [&](int p, int &s, float &w, int &t) {
        s = a.idx[p];
        if constexpr (MAPPED) {
            t = a.etype[a.teid ? a.teid[p] : p];
            if ((unsigned)t >= R) return;   // a skipped edge is not read through
            if (a.src) s = a.src[s];
            if (a.val) w = a.val[a.veid ? a.veid[p] : p];
        } else {
            t = a.etype[p];
            if ((unsigned)t >= R) return;
            if (a.val) w = a.val[p];
        }
        if (a.mean) w = w / (float)cnt[t];   // s_p: one IEEE division per edge (the edge itself is counted: n >= 1)
    };
    int my_s = 0, my_t = -1;
    float my_w = 1.0f;
    if (beg + lane < end) edge_meta(beg + lane, my_s, my_w, my_t);
    for (int cb = beg; cb < end; cb += GROUP) {
        int nx_s = 0, nx_t = -1;
        float nx_w = 1.0f;
        if (cb + GROUP + lane < end) edge_meta(cb + GROUP + lane, nx_s, nx_w, nx_t);
        const int nw = end - cb < GROUP ? end - cb : GROUP;
        for (int j = 0; j < nw; j += UNROLL) {
            int s[UNROLL], t[UNROLL];
            float w[UNROLL];
            Pack<VEC, TX> xv[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                s[u] = __shfl(my_s, j + u, GROUP);
                w[u] = __shfl(my_w, j + u, GROUP);
                t[u] = __shfl(my_t, j + u, GROUP);
                if (j + u >= nw) t[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if ((unsigned)t[u] < R && col_ok) xv[u] = load_pack<VEC>(xcol + (size_t)s[u] * (size_t)a.xpitch);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if ((unsigned)t[u] < R && col_ok) {
                    const float *cr = comp + t[u] * B;
#pragma unroll
                    for (int b = 0; b < BC; ++b)
                        if (FULL || b < nb) {
                            const float c = cr[b] * w[u];
#pragma unroll
                            for (int k = 0; k < VEC; ++k) acc[b][k] = __builtin_fmaf(xv[u].at(k), c, acc[b][k]);
                        }
                }
        }
        my_s = nx_s;
        my_w = nx_w;
        my_t = nx_t;
    }
}

template <int VEC, int GROUP, bool MAPPED, typename TX>
__global__ __launch_bounds__(kBasisThreads) void k_block_rgcn_basis(const BasisArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int BC = basis_chunk(VEC);
    constexpr int GPB = kBasisThreads / GROUP, PASSES = kBasisRows / GPB;
    static_assert(GROUP >= 16 && PASSES * GPB == kBasisRows, "whole passes over the 16 rows of a tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char basis_smem[];
    const int F = a.feat, N = a.n_out, R = a.num_rel, B = a.num_bases;
    const BasisLds L = basis_lds(F, N, R, B, B16);
    const int Fp = L.fp, pitch = L.pitch;
    int *tile_rows = reinterpret_cast<int *>(basis_smem);
    int *cnts = reinterpret_cast<int *>(basis_smem + L.cnt_off);
    float *comp = reinterpret_cast<float *>(basis_smem + L.comp_off);
    TX *tile = reinterpret_cast<TX *>(basis_smem + L.tile_off);
    const int lane = (int)threadIdx.x % GROUP, grp = (int)threadIdx.x / GROUP;
    const bool with_self = a.wself != nullptr;

    // once per workgroup: comp, the padding columns of every slot (no row store reaches them: a lane's VEC columns lie below feat) ...
    for (int i = threadIdx.x; i < R * B; i += kBasisThreads) comp[i] = a.comp[i];
    const int npad = Fp - F;
    for (int i = threadIdx.x; i < kBasisRows * (B + 1) * npad; i += kBasisThreads) {
        const int r = i / ((B + 1) * npad), c = i % ((B + 1) * npad);
        tile[r * pitch + (c / npad) * Fp + F + c % npad] = (TX)0.0f;
    }
    // ... and, bf16, the image of the stacked weights: k over [W_self; zeros to Fp; V_0; zeros; ...; V_{B-1}; zeros to (B + 1) Fp]
    const __bf16 *wimg = nullptr;
    if constexpr (B16) {
        __bf16 *img = reinterpret_cast<__bf16 *>(basis_smem + L.wimg_off);
        if (with_self) stage_basis_slot(img, pitch, Fp, static_cast<const __bf16 *>(a.wself), F, N);
        for (int b = 0; b < B; ++b)
            stage_basis_slot(img + (b + 1) * Fp, pitch, Fp, static_cast<const __bf16 *>(a.bases) + (size_t)b * F * N, F, N);
        wimg = img;
    }
    __syncthreads();   // every group reads comp in phase 1

#pragma unroll 1
    for (int rt = (int)blockIdx.x; rt < a.row_tiles; rt += (int)gridDim.x) {
        // ---- phase 1: rows into the tile
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int slot = pass * GPB + grp;
            const int row = rt * kBasisRows + slot;
            const bool live = row < a.num_dst;
            int beg = 0, end = 0;
            size_t srow = 0;
            if (live) {
                beg = a.ptr[row];
                end = a.ptr[row + 1];
                if (with_self) srow = (size_t)(a.src ? a.src[row] : row);
            }
            TX *trow = tile + slot * pitch;
            int *cnt = cnts + slot * R;
            if (a.mean) {   // n(row, t): a walk over the row's types only
                for (int i = lane; i < R; i += GROUP) cnt[i] = 0;
                basis_group_sync();
                for (int p = beg + lane; p < end; p += GROUP) {
                    const int t = a.etype[(MAPPED && a.teid) ? a.teid[p] : p];
                    if ((unsigned)t < (unsigned)R) __hip_atomic_fetch_add(cnt + t, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                basis_group_sync();
            }
#pragma unroll 1
            for (int ct = 0; ct < a.ntiles; ++ct) {
                const int col = (ct * GROUP + lane) * VEC;
                const bool col_ok = col < F;
                const TX *__restrict__ xcol = static_cast<const TX *>(a.x) + col;
                Pack<VEC, TX> self = {};
                if (live && with_self && col_ok) self = load_pack<VEC>(xcol + srow * (size_t)a.xpitch);   // in flight over the chains
#pragma unroll 1
                for (int b0 = 0; b0 < B; b0 += BC) {
                    const int nb = B - b0 < BC ? B - b0 : BC;
                    float acc[BC][VEC];
#pragma unroll
                    for (int b = 0; b < BC; ++b)
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[b][k] = 0.0f;
                    if (nb == BC) chain_basis_edges<VEC, GROUP, MAPPED, BC, true, kUnroll, TX>(acc, nb, beg, end, lane, col_ok, a, xcol, comp + b0, cnt);
                    else chain_basis_edges<VEC, GROUP, MAPPED, BC, false, kUnroll, TX>(acc, nb, beg, end, lane, col_ok, a, xcol, comp + b0, cnt);
                    if (!col_ok) continue;
#pragma unroll
                    for (int b = 0; b < BC; ++b)
                        if (b < nb) {   // a row without edges (or past num_dst) stores its +0
                            if constexpr (B16) store_pack_bf16<VEC>(trow + (b0 + b + 1) * Fp + col, acc[b], VEC);   // the conversion of a bf16 y store
                            else store_pack<VEC>(trow + (b0 + b + 1) * Fp + col, acc[b]);
                        }
                }
                if (col_ok && with_self) store_raw_pack<VEC, TX>(trow + col, self);
            }
            if (lane == 0) tile_rows[slot] = live ? row : -1;
        }
        __syncthreads();   // the tile (and, the first time, its padding and the image) is complete

        // ---- phase 2: 16 x 16 output sub-tiles, one accumulator over the B + 1 slots
        const int wave = (int)threadIdx.x >> 6, wl = (int)threadIdx.x & 63, kq = wl >> 4;
#pragma unroll 1
        for (int cb = wave; cb < (N + 15) >> 4; cb += kBasisThreads >> 6) {
            const int col = cb * 16 + (wl & 15);
            const bool cok = col < N;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if constexpr (B16) {
                const __bf16 *ap = tile + (wl & 15) * pitch + 8 * kq;
                const __bf16 *bp = wimg + (size_t)col * pitch + 8 * kq;
                for (int k0 = with_self ? 0 : Fp; k0 < (B + 1) * Fp; k0 += 32)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const basis_bf16x8 *>(ap + k0),
                                                                  *reinterpret_cast<const basis_bf16x8 *>(bp + k0), acc, 0, 0, 0);
            } else {
                constexpr int KB = GROUP * VEC >= 128 ? 32 : GROUP * VEC / 4;
                const float *arow = tile + (wl & 15) * pitch + kq;
                if (with_self) basis_slot_times_weight<KB>(acc, arow, static_cast<const float *>(a.wself), F, N, col, cok, kq);
#pragma unroll 1
                for (int b = 0; b < B; ++b)
                    basis_slot_times_weight<KB>(acc, arow + (b + 1) * Fp, static_cast<const float *>(a.bases) + (size_t)b * F * N, F, N, col, cok, kq);
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

template <int VEC, int GROUP, bool MAPPED, typename TX>
static int launch_basis_inst(const BasisArgs &a, int grid, size_t lds, hipStream_t st)
{
    static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (lds > 64 * 1024 && big_lds_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_block_rgcn_basis<VEC, GROUP, MAPPED, TX>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kBasisLdsBytes));
        big_lds_ok.done();
    }
    hipLaunchKernelGGL((k_block_rgcn_basis<VEC, GROUP, MAPPED, TX>), dim3((unsigned)grid), dim3(kBasisThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

template <int VEC, int GROUP, typename TX>
static int launch_basis(const BasisArgs &a, int mapped, int grid, size_t lds, hipStream_t st)
{
    if constexpr (GROUP < 16) {
        return fail(GNNAGG_ERR_STATE, "internal: gnnagg_block_rgcn_basis_run runs groups of 16 lanes and more");
    } else {
        return mapped ? launch_basis_inst<VEC, GROUP, true, TX>(a, grid, lds, st) : launch_basis_inst<VEC, GROUP, false, TX>(a, grid, lds, st);
    }
}

static int block_rgcn_basis_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const int *etype, const int *etype_eid,
                                const float *val, const int *val_eid, const void *x, int x_dtype, long long x_pitch, int feat,
                                const void *w_self, const void *bases, const float *comp, int num_rel, int num_bases, const float *bias,
                                int n_out, void *out, int out_dtype, int reduce, int flags, void *stream)
{
    static const char *who = "gnnagg_block_rgcn_basis_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    if (num_dst < 0) return bad("num_dst = " + std::to_string(num_dst) + " is negative");
    if (feat < 1) return bad("feat = " + std::to_string(feat) + " must be >= 1");
    if (n_out < 1) return bad("n_out = " + std::to_string(n_out) + " must be >= 1");
    if (num_rel < 1) return bad("num_rel = " + std::to_string(num_rel) + " must be >= 1");
    if (num_bases < 1) return bad("num_bases = " + std::to_string(num_bases) + " must be >= 1");
    if (x_pitch < feat) return bad("x_pitch = " + std::to_string(x_pitch) + " is below feat = " + std::to_string(feat));
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (out_dtype != GNNAGG_DTYPE_F32 && out_dtype != GNNAGG_DTYPE_BF16) return bad("unknown out_dtype " + std::to_string(out_dtype));
    if (x_dtype == GNNAGG_DTYPE_F32 && out_dtype == GNNAGG_DTYPE_BF16) return bad("out_dtype: fp32 operands give a fp32 out, not a bf16 one");
    if (reduce != GNNAGG_REDUCE_SUM && reduce != GNNAGG_REDUCE_MEAN)
        return bad("reduce " + std::to_string(reduce) + ": GNNAGG_REDUCE_SUM and GNNAGG_REDUCE_MEAN are the reduces of this layer");
    if (flags & ~GNNAGG_FLAG_RELU) return bad("flags = " + std::to_string(flags) + ": GNNAGG_FLAG_RELU is the only flag");
    if (val_eid && !val) return bad("d_val_eid needs d_val (d_val_eid indexes it)");
    if (etype_eid && !etype) return bad("d_etype_eid needs d_etype (d_etype_eid indexes it)");
    if (!basis_supported(feat, n_out, num_rel, num_bases, x_dtype))
        return bad("feat = " + std::to_string(feat) + ", n_out = " + std::to_string(n_out) + ", num_rel = " + std::to_string(num_rel) +
                   ", num_bases = " + std::to_string(num_bases) + " lie outside the range of gnnagg_block_rgcn_basis_supported");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!etype) return bad("d_etype is null");
        if (!x) return bad("d_x is null");
        if (!bases) return bad("d_bases is null");
        if (!comp) return bad("d_comp is null");
        if (!out) return bad("d_out is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: the rule of gnnagg_block_rgcn_run (a divisor of feat and of the pitch, no wider than x's alignment); the tile rows
    // in LDS are aligned for any lane.  Groups of 8 lanes run as groups of 16: 16 groups are the 16 rows of a tile.
    const int fp = (int)gcd_ll(feat, x_pitch);
    Geometry g = x16 ? typed_geometry(feat, x, 2, fp) : pick_geometry(feat, x, nullptr, nullptr, fp);
    if (g.group < 16) g.group = 16;
    BasisArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.etype = etype; a.teid = etype_eid; a.veid = val_eid; a.val = val; a.comp = comp;
    a.x = x; a.wself = w_self; a.bases = bases; a.bias = bias; a.out = out; a.xpitch = x_pitch;
    a.num_dst = num_dst; a.feat = feat; a.n_out = n_out; a.num_rel = num_rel; a.num_bases = num_bases; a.ntiles = g.ntiles;
    a.mean = reduce == GNNAGG_REDUCE_MEAN; a.relu = (flags & GNNAGG_FLAG_RELU) != 0;
    a.out_bf16 = out_dtype == GNNAGG_DTYPE_BF16;
    a.row_tiles = ceil_div(num_dst, kBasisRows);
    const int mapped = src != nullptr || etype_eid != nullptr || val_eid != nullptr;
    const int grid = std::min(a.row_tiles, basis_grid_cap(feat, n_out, num_rel, num_bases, x_dtype));
    const size_t lds = (size_t)basis_lds(feat, n_out, num_rel, num_bases, x16).bytes;
    hipStream_t st = (hipStream_t)stream;
    int rc = GNNAGG_OK;
    if (x16) {
        DISPATCH_GEOM_16BIT(g, (rc = launch_basis<VEC, GROUP, __bf16>(a, mapped, grid, lds, st)))
    } else {
        DISPATCH_GEOM(g, (rc = launch_basis<VEC, GROUP, float>(a, mapped, grid, lds, st)))
    }
    return rc;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_rgcn_basis_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const int *d_etype,
                                const int *d_etype_eid, const float *d_val, const int *d_val_eid, const void *d_x, int x_dtype,
                                long long x_pitch, int feat, const void *d_w_self, const void *d_bases, const float *d_comp, int num_rel,
                                int num_bases, const float *d_bias, int n_out, void *d_out, int out_dtype, int reduce, int flags,
                                void *hip_stream)
{
    return block_rgcn_basis_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_etype, d_etype_eid, d_val, d_val_eid, d_x, x_dtype, x_pitch, feat,
                                d_w_self, d_bases, d_comp, num_rel, num_bases, d_bias, n_out, d_out, out_dtype, reduce, flags, hip_stream);
}

int gnnagg_block_rgcn_basis_supported(int feat, int n_out, int num_rel, int num_bases, int x_dtype)
{
    return basis_supported(feat, n_out, num_rel, num_bases, x_dtype) ? 1 : 0;
}

int gnnagg_block_rgcn_basis_grid_cap(int feat, int n_out, int num_rel, int num_bases, int x_dtype)
{
    return basis_supported(feat, n_out, num_rel, num_bases, x_dtype) ? basis_grid_cap(feat, n_out, num_rel, num_bases, x_dtype) : 0;
}

}  // extern "C"
#pragma GCC visibility pop
