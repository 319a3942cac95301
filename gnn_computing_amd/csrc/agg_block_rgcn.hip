// agg_block_rgcn.hip -- a relational (typed-edge) GCN layer on ONE sampled block in one launch: gnnagg_block_rgcn_run (include/gnnagg.h
// section F, "Block R-GCN layer").
//
//   out[i] = act( x_dst[i] . W_self + sum_{r < R} aggr_{p in row i, etype(p) == r}(val(p) x_src(p)) . W_rel[r] + bias )
//
// The frame is k_block_sage's (agg_block_sage.hip): 256 threads, tiles of kRgcnRows = 16 destination rows walked blockIdx.x,
// blockIdx.x + gridDim.x, ..., rows meeting in an LDS tile, one MFMA accumulator over stacked weights.  What is new is the tile row
//   [ x_dst | a_0 | a_1 | ... | a_{R-1} ]          R + 1 slots of Fp columns, Fp = feat rounded up to the MFMA's k block (4 fp32, 32 bf16)
// and a walk that splits a row's neighbourhood by edge type while it reads it ONCE:
//   phase 1  one lane group per row walks the row's edges in CSR order with the window, prefetch and broadcast of chain_block_edges; the
//            type of an edge travels with its id and weight (the lane that loads idx[p] loads etype[eid ? eid[p] : p]).  The accumulator
//            of the CURRENT relation lives in the lane's registers.  When the next edge's relation differs the lane stores it to its own
//            fp32 columns of that relation's slot and loads the new relation's running value (and the group its running count): every
//            (row, relation) sum is the ascending fmaf chain from 0 in CSR order whatever the interleaving -- the chain
//            gnnagg_block_gcn_run runs on the relation-filtered sub-block -- and rows sorted by type run at register speed.  Only the
//            owning lane touches its columns: no atomics, no race.  A type outside [0, R) is skipped: its row of x is never read, it is
//            never counted.  The counts [16][R] lie beside the tile: every lane of a group writes the same value at the same
//            instruction and reads back what it wrote.  After the walk each slot is finished (the mean division of finish_gcn_row by
//            the relation's count in the row; an empty (row, relation) stays +0).
//            fp32 operands: the slots of the tile ARE the fp32 columns.  bf16 operands: the running values live in an fp32 area
//            [16][R][roundup4(feat)] beside the tile and are rounded ONCE into the bf16 tile by the conversion of a bf16 y store.
//   phase 2  after ONE barrier the 4 wavefronts take 16 x 16 output sub-tiles; ONE fp32 accumulator runs k ascending over the self slot,
//            then r = 0 .. R-1: fp32 on v_mfma_f32_16x16x4_f32 with W through buffer loads, the accumulator carried from slot to slot
//            (the zero columns that pad a slot add 0 * 0 to an accumulator that is never -0: the bits of matmul_nn over the
//            concatenation); bf16 on v_mfma_f32_16x16x32_bf16 against an image wimg[n][k] of the stacked [(R + 1) Fp, n_out] weights,
//            k contiguous, transposed into LDS ONCE per workgroup.
//   epilogue + bias, ReLU (a NaN stays a NaN), one store per element.
// Pitch of the tile (and of the image): fp32 roundup8((R + 1) Fp) + 4 floats -- 4 (2m + 1): the 16 rows of an A operand read (row =
// lane % 16, k = lane / 16) start on 8 different multiples of 4 banks and the 4 k offsets fill the gaps, two lanes per bank, as 2 Fp + 4
// does for the SAGE tile; bf16 (R + 1) Fp + 8 elements -- Fp is a multiple of 32, so a row is an odd number of 16-byte slots and the 16
// rows (columns) a b128 lane group reads fall on 16 different slots of the bank row.  R = 1 gives the SAGE tile.
// No scratch; every lane's address is a function of the arguments, and so is the result.
#include "block_chain.cuh"

namespace gnnagg {
namespace {

constexpr int kRgcnThreads = 256;            // 4 wavefronts
constexpr int kRgcnRows = 16;                // destination rows of a tile: one MFMA row block
constexpr int kRgcnLdsBytes = 160 * 1024;    // LDS of a CU: the budget of tile + counts + fp32 area + weight image
constexpr int kRgcnMaxDim = 256;             // feat and n_out
constexpr int kRgcnMaxRel = 640;             // (past it the fp32 tile of feat = 1 is alone above the budget; keeps the sizes inside int)
constexpr int kRgcnPerCu = 8;                // workgroups per CU the grid is capped at (fewer where the LDS of a workgroup allows fewer)

struct RgcnArgs {
    const int *ptr, *idx, *src, *etype, *teid, *veid;   // teid / veid: the eid map of etype / val, or null
    const float *val;
    const void *x, *wself, *wrel;
    const float *bias;
    void *out;
    long long xpitch;   // elements between rows of x
    int num_dst, feat, n_out, num_rel, ntiles, mean, relu, out_bf16, row_tiles;
};

// The LDS of a launch, kernel and launcher agree through this:
//   [tile_rows: 16 ints][cnt: 16 x R ints][tile: 16 rows of `pitch`][bf16: acc, 16 x R x fa floats][bf16: the weight image, roundup16(n_out) rows]
struct RgcnLds {
    int fp, pitch, fa, cnt_off, tile_off, acc_off, wimg_off, bytes;
};
__host__ __device__ inline RgcnLds rgcn_lds(int feat, int n_out, int R, bool b16)
{
    RgcnLds l;
    l.fp = b16 ? (feat + 31) & ~31 : (feat + 3) & ~3;
    l.pitch = b16 ? (R + 1) * l.fp + 8 : (((R + 1) * l.fp + 7) & ~7) + 4;
    l.fa = (feat + 3) & ~3;
    l.cnt_off = kRgcnRows * (int)sizeof(int);
    l.tile_off = l.cnt_off + ((kRgcnRows * R * (int)sizeof(int) + 15) & ~15);
    l.acc_off = l.tile_off + kRgcnRows * l.pitch * (b16 ? 2 : 4);
    l.wimg_off = l.acc_off + (b16 ? kRgcnRows * R * l.fa * 4 : 0);
    l.bytes = l.wimg_off + (b16 ? ((n_out + 15) & ~15) * l.pitch * 2 : 0);
    return l;
}

static bool rgcn_supported(int feat, int n_out, int num_rel, int x_dtype)
{
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return false;
    if (feat < 1 || feat > kRgcnMaxDim || n_out < 1 || n_out > kRgcnMaxDim || num_rel < 1 || num_rel > kRgcnMaxRel) return false;
    return rgcn_lds(feat, n_out, num_rel, x_dtype == GNNAGG_DTYPE_BF16).bytes <= kRgcnLdsBytes;
}

// workgroups a launch of this shape is capped at: as many per CU as their LDS allows, kRgcnPerCu at the most
static int rgcn_grid_cap(int feat, int n_out, int num_rel, int x_dtype)
{
    const int per_cu = kRgcnLdsBytes / rgcn_lds(feat, n_out, num_rel, x_dtype == GNNAGG_DTYPE_BF16).bytes;
    return std::min(std::max(per_cu, 1), kRgcnPerCu) * device_cu_count();
}

typedef __bf16 rgcn_bf16x8 __attribute__((ext_vector_type(8)));

// One weight into its slot of the image: wimg[n][0 .. kp) = W[0 .. K)[n] for the columns n < roundup16(N), zeros beyond K and N (wimg
// already points at the slot's first k).  The two paths of stage_weight_half (agg_block_sage.hip): where N % 8 == 0 and W is 16-byte
// aligned one thread per 8 k x 8 columns -- eight 16-byte row pieces transposed in registers, one 16-byte LDS store per column; else one
// thread per (column, 8 k) with 2-byte loads.  Both write the same image.
__device__ __forceinline__ void stage_weight_slot(__bf16 *wimg, int wpitch, int kp, const __bf16 *__restrict__ W, int K, int N)
{
    const unsigned short *Wu = reinterpret_cast<const unsigned short *>(W);
    const int ncols = (N + 15) & ~15;
    if ((N & 7) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
        const int nco = ncols >> 3;
        for (int i = threadIdx.x; i < nco * (kp >> 3); i += kRgcnThreads) {
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
    for (int i = threadIdx.x; i < ncols * (kp >> 3); i += kRgcnThreads) {
        const int n = i % ncols, k = (i / ncols) << 3;
        unsigned q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (n < N && k + j < K) ? (unsigned)Wu[(size_t)(k + j) * N + n] : 0u;
        *reinterpret_cast<uint4 *>(wimg + (size_t)n * wpitch + k) =
            make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
    }
}

// acc += arow[0 .. K) . W[0 .. K)[col], k ascending, for one slot of the tile: half_times_weight (agg_block_sage.hip), the accumulator
// carried in and out.  arow: this lane's tile row at its k offset kq = lane / 16 (A: row = lane % 16, k = lane / 16; B: k = lane / 16,
// col = lane % 16); the slot's columns [K, roundup4(K)) hold 0.  W operands as buffer loads: the per-lane byte offset in one VGPR (out of
// range for the padding columns, which then read 0), the k step in an SGPR.  k-quads past K inside a batch are clamped loads with zeroed
// operands: 0 * 0 leaves the chain as it is.
template <int KB>
__device__ __forceinline__ void slot_times_weight(f32x4 &acc, const float *arow, const float *W, int K, int N, int col, bool cok, int kq)
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

// chain_block_edges with a type per edge.  run: this lane's VEC fp32 columns of the row's R running sums (relation r at run + r * rstride),
// zeroed by the caller; cnt: the row's R running counts, zeroed too.  acc / n hold relation `cur` and go back to run / cnt when the
// relation changes and at the end of the row.  Lanes with col_ok == false carry metadata and counts and touch no column.
template <int VEC, int GROUP, bool MAPPED, int UNROLL, typename TX>
__device__ __forceinline__ void chain_typed_edges(int beg, int end, int lane, bool col_ok, const RgcnArgs &a, const TX *__restrict__ xcol,
                                                  float *run, int rstride, int *cnt)
{
    const unsigned R = (unsigned)a.num_rel;
    auto edge_meta = [&](int p, int &s, float &w, int &t) {
        s = a.idx[p];
        if constexpr (MAPPED) {
            t = a.etype[a.teid ? a.teid[p] : p];
            if ((unsigned)t >= R) return;   // a skipped edge is not read through
            if (a.src) s = a.src[s];
            if (a.val) w = a.val[a.veid ? a.veid[p] : p];
        } else {
            t = a.etype[p];
            if (a.val) w = a.val[p];
        }
    };
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
    int cur = -1, n = 0;
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
                if ((unsigned)t[u] < R) {
                    if (t[u] != cur) {   // the relation changes: this one's sum and count to LDS, the new one's from it
                        if (cur >= 0) {
                            if (col_ok) store_pack<VEC>(run + cur * rstride, acc);
                            cnt[cur] = n;
                        }
                        cur = t[u];
                        if (col_ok) {
                            const Pack<VEC> o = load_pack<VEC>(run + cur * rstride);
#pragma unroll
                            for (int k = 0; k < VEC; ++k) acc[k] = o.v[k];
                        }
                        n = cnt[cur];
                    }
                    ++n;
                    if (col_ok) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[k] = __builtin_fmaf(xv[u].at(k), w[u], acc[k]);
                    }
                }
        }
        my_s = nx_s;
        my_w = nx_w;
        my_t = nx_t;
    }
    if (cur >= 0) {
        if (col_ok) store_pack<VEC>(run + cur * rstride, acc);
        cnt[cur] = n;
    }
}

template <int VEC, int GROUP, bool MAPPED, typename TX>
__global__ __launch_bounds__(kRgcnThreads) void k_block_rgcn(const RgcnArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int GPB = kRgcnThreads / GROUP, PASSES = kRgcnRows / GPB;
    static_assert(GROUP >= 16 && PASSES * GPB == kRgcnRows, "whole passes over the 16 rows of a tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char rgcn_smem[];
    const int F = a.feat, N = a.n_out, R = a.num_rel;
    const RgcnLds L = rgcn_lds(F, N, R, B16);
    const int Fp = L.fp, pitch = L.pitch;
    int *tile_rows = reinterpret_cast<int *>(rgcn_smem);
    int *cnts = reinterpret_cast<int *>(rgcn_smem + L.cnt_off);
    TX *tile = reinterpret_cast<TX *>(rgcn_smem + L.tile_off);
    // the fp32 running sums of a tile row: the slots themselves (fp32), or the area beside the tile (bf16)
    float *runs = reinterpret_cast<float *>(rgcn_smem + (B16 ? L.acc_off : L.tile_off + Fp * 4));
    const int rstride = B16 ? L.fa : Fp, runpitch = B16 ? R * L.fa : pitch;
    const int lane = (int)threadIdx.x % GROUP, grp = (int)threadIdx.x / GROUP;
    const bool with_self = a.wself != nullptr;

    // once per workgroup: the padding columns of every slot (no row store reaches them: a lane's VEC columns lie below feat) ...
    const int npad = Fp - F;
    for (int i = threadIdx.x; i < kRgcnRows * (R + 1) * npad; i += kRgcnThreads) {
        const int r = i / ((R + 1) * npad), c = i % ((R + 1) * npad);
        tile[r * pitch + (c / npad) * Fp + F + c % npad] = (TX)0.0f;
    }
    // ... and, bf16, the image of the stacked weights: k over [W_self; zeros to Fp; W_rel[0]; zeros; ...; W_rel[R-1]; zeros to (R + 1) Fp]
    const __bf16 *wimg = nullptr;
    if constexpr (B16) {
        __bf16 *img = reinterpret_cast<__bf16 *>(rgcn_smem + L.wimg_off);
        if (with_self) stage_weight_slot(img, pitch, Fp, static_cast<const __bf16 *>(a.wself), F, N);
        for (int r = 0; r < R; ++r)
            stage_weight_slot(img + (r + 1) * Fp, pitch, Fp, static_cast<const __bf16 *>(a.wrel) + (size_t)r * F * N, F, N);
        wimg = img;
    }

#pragma unroll 1
    for (int rt = (int)blockIdx.x; rt < a.row_tiles; rt += (int)gridDim.x) {
        // ---- phase 1: rows into the tile
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int slot = pass * GPB + grp;
            const int row = rt * kRgcnRows + slot;
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
#pragma unroll 1
            for (int ct = 0; ct < a.ntiles; ++ct) {
                const int col = (ct * GROUP + lane) * VEC;
                const bool col_ok = col < F;
                const TX *__restrict__ xcol = static_cast<const TX *>(a.x) + col;
                float *run = runs + slot * runpitch + col;
                Pack<VEC, TX> self = {};
                if (live && with_self && col_ok) self = load_pack<VEC>(xcol + srow * (size_t)a.xpitch);   // in flight over the chain
                float acc[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
                for (int r = 0; r < R; ++r) {   // every (row, relation) starts at +0 with no edges (a row past num_dst stays there)
                    if (col_ok) store_pack<VEC>(run + r * rstride, acc);
                    cnt[r] = 0;
                }
                chain_typed_edges<VEC, GROUP, MAPPED, kUnroll, TX>(beg, end, lane, col_ok, a, xcol, run, rstride, cnt);
                if (!col_ok) continue;
                if (with_self) store_raw_pack<VEC, TX>(trow + col, self);
                if (B16 || a.mean) {
                    for (int r = 0; r < R; ++r) {
                        const int c = cnt[r];
                        if (!B16 && c == 0) continue;
                        const Pack<VEC> o = load_pack<VEC>(run + r * rstride);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[k] = o.v[k];
                        if (c > 0) finish_gcn_row<VEC, false>(acc, c, row, nullptr, a.mean, 0, 0, nullptr);
                        if constexpr (B16) store_pack_bf16<VEC>(trow + (r + 1) * Fp + col, acc, VEC);   // the conversion of a bf16 y store
                        else store_pack<VEC>(run + r * rstride, acc);
                    }
                }
            }
            if (lane == 0) tile_rows[slot] = live ? row : -1;
        }
        __syncthreads();   // the tile (and, the first time, its padding and the image) is complete

        // ---- phase 2: 16 x 16 output sub-tiles, one accumulator over the R + 1 slots
        const int wave = (int)threadIdx.x >> 6, wl = (int)threadIdx.x & 63, kq = wl >> 4;
#pragma unroll 1
        for (int cb = wave; cb < (N + 15) >> 4; cb += kRgcnThreads >> 6) {
            const int col = cb * 16 + (wl & 15);
            const bool cok = col < N;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if constexpr (B16) {
                const __bf16 *ap = tile + (wl & 15) * pitch + 8 * kq;
                const __bf16 *bp = wimg + (size_t)col * pitch + 8 * kq;
                for (int k0 = with_self ? 0 : Fp; k0 < (R + 1) * Fp; k0 += 32)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const rgcn_bf16x8 *>(ap + k0),
                                                                  *reinterpret_cast<const rgcn_bf16x8 *>(bp + k0), acc, 0, 0, 0);
            } else {
                constexpr int KB = GROUP * VEC >= 128 ? 32 : GROUP * VEC / 4;
                const float *arow = tile + (wl & 15) * pitch + kq;
                if (with_self) slot_times_weight<KB>(acc, arow, static_cast<const float *>(a.wself), F, N, col, cok, kq);
#pragma unroll 1
                for (int r = 0; r < R; ++r)
                    slot_times_weight<KB>(acc, arow + (r + 1) * Fp, static_cast<const float *>(a.wrel) + (size_t)r * F * N, F, N, col, cok, kq);
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
static int launch_rgcn_inst(const RgcnArgs &a, int grid, size_t lds, hipStream_t st)
{
    static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (lds > 64 * 1024 && big_lds_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_block_rgcn<VEC, GROUP, MAPPED, TX>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kRgcnLdsBytes));
        big_lds_ok.done();
    }
    hipLaunchKernelGGL((k_block_rgcn<VEC, GROUP, MAPPED, TX>), dim3((unsigned)grid), dim3(kRgcnThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

template <int VEC, int GROUP, typename TX>
static int launch_rgcn(const RgcnArgs &a, int mapped, int grid, size_t lds, hipStream_t st)
{
    if constexpr (GROUP < 16) {
        return fail(GNNAGG_ERR_STATE, "internal: gnnagg_block_rgcn_run runs groups of 16 lanes and more");
    } else {
        return mapped ? launch_rgcn_inst<VEC, GROUP, true, TX>(a, grid, lds, st) : launch_rgcn_inst<VEC, GROUP, false, TX>(a, grid, lds, st);
    }
}

static int block_rgcn_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const int *etype, const int *etype_eid,
                          const float *val, const int *val_eid, const void *x, int x_dtype, long long x_pitch, int feat, const void *w_self,
                          const void *w_rel, int num_rel, const float *bias, int n_out, void *out, int out_dtype, int reduce, int flags,
                          void *stream)
{
    static const char *who = "gnnagg_block_rgcn_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    if (num_dst < 0) return bad("num_dst = " + std::to_string(num_dst) + " is negative");
    if (feat < 1) return bad("feat = " + std::to_string(feat) + " must be >= 1");
    if (n_out < 1) return bad("n_out = " + std::to_string(n_out) + " must be >= 1");
    if (num_rel < 1) return bad("num_rel = " + std::to_string(num_rel) + " must be >= 1");
    if (x_pitch < feat) return bad("x_pitch = " + std::to_string(x_pitch) + " is below feat = " + std::to_string(feat));
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (out_dtype != GNNAGG_DTYPE_F32 && out_dtype != GNNAGG_DTYPE_BF16) return bad("unknown out_dtype " + std::to_string(out_dtype));
    if (x_dtype == GNNAGG_DTYPE_F32 && out_dtype == GNNAGG_DTYPE_BF16) return bad("out_dtype: fp32 operands give a fp32 out, not a bf16 one");
    if (reduce != GNNAGG_REDUCE_SUM && reduce != GNNAGG_REDUCE_MEAN)
        return bad("reduce " + std::to_string(reduce) + ": GNNAGG_REDUCE_SUM and GNNAGG_REDUCE_MEAN are the reduces of this layer");
    if (flags & ~GNNAGG_FLAG_RELU) return bad("flags = " + std::to_string(flags) + ": GNNAGG_FLAG_RELU is the only flag");
    if (val_eid && !val) return bad("d_val_eid needs d_val (d_val_eid indexes it)");
    if (etype_eid && !etype) return bad("d_etype_eid needs d_etype (d_etype_eid indexes it)");
    if (!rgcn_supported(feat, n_out, num_rel, x_dtype))
        return bad("feat = " + std::to_string(feat) + ", n_out = " + std::to_string(n_out) + ", num_rel = " + std::to_string(num_rel) +
                   " lie outside the range of gnnagg_block_rgcn_supported");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!etype) return bad("d_etype is null");
        if (!x) return bad("d_x is null");
        if (!w_rel) return bad("d_w_rel is null");
        if (!out) return bad("d_out is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: the rule of gnnagg_block_sage_run (a divisor of feat and of the pitch, no wider than x's alignment); the tile rows
    // and the fp32 area in LDS are aligned for any lane.  Groups of 8 lanes run as groups of 16: 16 groups are the 16 rows of a tile.
    const int fp = (int)gcd_ll(feat, x_pitch);
    Geometry g = x16 ? typed_geometry(feat, x, 2, fp) : pick_geometry(feat, x, nullptr, nullptr, fp);
    if (g.group < 16) g.group = 16;
    RgcnArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.etype = etype; a.teid = etype_eid; a.veid = val_eid; a.val = val;
    a.x = x; a.wself = w_self; a.wrel = w_rel; a.bias = bias; a.out = out; a.xpitch = x_pitch;
    a.num_dst = num_dst; a.feat = feat; a.n_out = n_out; a.num_rel = num_rel; a.ntiles = g.ntiles;
    a.mean = reduce == GNNAGG_REDUCE_MEAN; a.relu = (flags & GNNAGG_FLAG_RELU) != 0;
    a.out_bf16 = out_dtype == GNNAGG_DTYPE_BF16;
    a.row_tiles = ceil_div(num_dst, kRgcnRows);
    const int mapped = src != nullptr || etype_eid != nullptr || val_eid != nullptr;
    const int grid = std::min(a.row_tiles, rgcn_grid_cap(feat, n_out, num_rel, x_dtype));
    const size_t lds = (size_t)rgcn_lds(feat, n_out, num_rel, x16).bytes;
    hipStream_t st = (hipStream_t)stream;
    int rc = GNNAGG_OK;
    if (x16) {
        DISPATCH_GEOM_16BIT(g, (rc = launch_rgcn<VEC, GROUP, __bf16>(a, mapped, grid, lds, st)))
    } else {
        DISPATCH_GEOM(g, (rc = launch_rgcn<VEC, GROUP, float>(a, mapped, grid, lds, st)))
    }
    return rc;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_rgcn_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const int *d_etype,
                          const int *d_etype_eid, const float *d_val, const int *d_val_eid, const void *d_x, int x_dtype, long long x_pitch,
                          int feat, const void *d_w_self, const void *d_w_rel, int num_rel, const float *d_bias, int n_out, void *d_out,
                          int out_dtype, int reduce, int flags, void *hip_stream)
{
    return block_rgcn_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_etype, d_etype_eid, d_val, d_val_eid, d_x, x_dtype, x_pitch, feat,
                          d_w_self, d_w_rel, num_rel, d_bias, n_out, d_out, out_dtype, reduce, flags, hip_stream);
}

int gnnagg_block_rgcn_supported(int feat, int n_out, int num_rel, int x_dtype) { return rgcn_supported(feat, n_out, num_rel, x_dtype) ? 1 : 0; }

int gnnagg_block_rgcn_grid_cap(int feat, int n_out, int num_rel, int x_dtype)
{
    return rgcn_supported(feat, n_out, num_rel, x_dtype) ? rgcn_grid_cap(feat, n_out, num_rel, x_dtype) : 0;
}

}  // extern "C"
#pragma GCC visibility pop
