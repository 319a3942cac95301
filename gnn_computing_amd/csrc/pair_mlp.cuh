#pragma once
// pair_mlp.cuh -- the two-layer MLP over a tile of kPairRows rows held in LDS, shared by the kernels that run it per node pair
// (agg_pair_score.hip: k_pair_mlp, one row of out per pair) and per edge of a block (agg_block_edgeconv.hip: k_block_edgeconv, the rows
// reduced per destination): the LDS layout of the m and z tiles and of the bf16 weight images, the staging of an image, the two
// tile-times-weight chains and one MFMA phase with its three destinations.
#include "block_chain.cuh"

namespace gnnagg {
namespace {

constexpr int kPairThreads = 256;            // 4 wavefronts
constexpr int kPairRB = 2;                   // row blocks of 16 pairs per tile of k_pair_mlp (DESIGN.md "Pair scoring": why 2)
constexpr int kPairRows = 16 * kPairRB;      // pairs of a tile
constexpr int kPairKB = 16;                  // fp32: k quads whose B operands are loaded before the first MFMA of a batch

// The LDS of an mlp launch, kernel and launcher agree through pair_lds:
//   [m tile: kPairRows rows of pitch_m][z tile: kPairRows rows of pitch_z][bf16: wimg1, roundup16(hidden) rows of pitch_m]
//   [bf16: wimg2, roundup16(n_out) rows of pitch_z]
// k1 = feat (mul) or 2 feat (cat); kp: K rounded up to the MFMA's k block (4 fp32, 32 bf16).  The pitches are those of the block layers'
// tiles: roundup8(K) + 4 floats (the 16 rows of an A operand start on 8 different multiples of 4 banks) or kp + 8 bf16 (an odd number of
// 16-byte slots).
struct PairLds {
    int k1, kp1, hp, pitch_m, pitch_z, z_off, w1_off, w2_off, bytes;
};
__host__ __device__ constexpr int pair_kp(int k, bool b16) { return b16 ? (k + 31) & ~31 : (k + 3) & ~3; }
__host__ __device__ constexpr int pair_pitch(int k, bool b16) { return b16 ? pair_kp(k, true) + 8 : ((k + 7) & ~7) + 4; }
__host__ __device__ constexpr PairLds pair_lds(int feat, int hidden, int n_out, bool cat, bool b16)
{
    PairLds l = {};
    const int es = b16 ? 2 : 4;
    l.k1 = cat ? 2 * feat : feat;
    l.kp1 = pair_kp(l.k1, b16);
    l.hp = pair_kp(hidden, b16);
    l.pitch_m = pair_pitch(l.k1, b16);
    l.pitch_z = pair_pitch(hidden, b16);
    l.z_off = kPairRows * l.pitch_m * es;
    l.w1_off = l.z_off + kPairRows * l.pitch_z * es;
    l.w2_off = l.w1_off + (b16 ? ((hidden + 15) & ~15) * l.pitch_m * 2 : 0);
    l.bytes = l.w2_off + (b16 ? ((n_out + 15) & ~15) * l.pitch_z * 2 : 0);
    return l;
}

typedef __bf16 pair_bf16x8 __attribute__((ext_vector_type(8)));

// One weight into its image: wimg[n][0 .. kp) = W[0 .. K)[n] for the columns n < roundup16(N), zeros beyond K and N -- the layout and the
// two paths of stage_weight_image (agg_block_gin.hip): where N % 8 == 0 and W is 16-byte aligned one thread per 8 k x 8 columns, eight
// 16-byte row pieces transposed in registers; else one thread per (column, 8 k) with 2-byte loads.  Both write the same image.
__device__ __forceinline__ void pair_stage_weight(__bf16 *wimg, int wpitch, int kp, const __bf16 *__restrict__ W, int K, int N)
{
    const unsigned short *Wu = reinterpret_cast<const unsigned short *>(W);
    const int ncols = (N + 15) & ~15;
    if ((N & 7) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
        const int nco = ncols >> 3;
        for (int i = threadIdx.x; i < nco * (kp >> 3); i += kPairThreads) {
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
    for (int i = threadIdx.x; i < ncols * (kp >> 3); i += kPairThreads) {
        const int n = i % ncols, k = (i / ncols) << 3;
        unsigned q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (n < N && k + j < K) ? (unsigned)Wu[(size_t)(k + j) * N + n] : 0u;
        *reinterpret_cast<uint4 *>(wimg + (size_t)n * wpitch + k) =
            make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
    }
}

// fp32: acc[r] = arow[r][0 .. K) . W[0 .. K)[col] for NRB row blocks, k ascending from +0 -- per accumulator the fmaf chain of
// gnnagg_matmul_nn.  arow: this lane's row of the FIRST row block at its k offset kq = lane / 16 (A: row = lane % 16, k = lane / 16; B:
// k = lane / 16, col = lane % 16), the next row block 16 * pitch further; the tile's columns [K, roundup4(K)) hold 0.  ONE buffer load of
// W per k quad serves all NRB MFMAs: the per-lane byte offset in one VGPR (out of range for the padding columns, which then read 0), the
// k step in an SGPR.  k quads past K inside a batch are clamped loads with zeroed operands: 0 * 0 leaves a chain that started at +0 as
// it is.
template <int NRB>
__device__ __forceinline__ void tile_times_weight_f32(f32x4 (&acc)[NRB], const float *arow, int pitch, const float *W, int K, int N, int col,
                                                      bool cok, int kq)
{
    constexpr int KB = NRB > 1 ? kPairKB / 2 : kPairKB;
#pragma unroll
    for (int r = 0; r < NRB; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int Kf = K & ~3;     // k covered by whole quads
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0, K * N * 4, 0x00020000);
    const int voff = cok ? (kq * N + col) * 4 : 0x7ffffff0;
#pragma unroll 1
    for (int k0 = 0; k0 < Kf; k0 += 4 * KB) {
        float bv[KB];
#pragma unroll
        for (int t = 0; t < KB; ++t) {
            const int kk = k0 + 4 * t, kc = kk < Kf ? kk : Kf - 4;
            const float b = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrsrc, voff, kc * N * 4, 0));
            bv[t] = kk < Kf ? b : 0.f;
        }
#pragma unroll
        for (int t = 0; t < KB; ++t) {
            const int kk = k0 + 4 * t, kc = kk < Kf ? kk : Kf - 4;
#pragma unroll
            for (int r = 0; r < NRB; ++r) {
                const float v = arow[r * 16 * pitch + kc];
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(kk < Kf ? v : 0.f, bv[t], acc[r], 0, 0, 0);
            }
        }
    }
    if (K != Kf) {  // ragged last quad: k = Kf + kq valid only below K (the tile's padding columns hold 0)
        const float b = (cok && Kf + kq < K) ? W[(size_t)(Kf + kq) * N + col] : 0.f;
#pragma unroll
        for (int r = 0; r < NRB; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[r * 16 * pitch + Kf], b, acc[r], 0, 0, 0);
    }
}

// bf16: acc[r] = arow[r][0 .. kp) . brow[0 .. kp), both in LDS with k contiguous and zeros in [K, kp); arow / brow: this lane's tile row /
// image column at its k offset 8 * (lane / 16).  One read of the image per k block serves all NRB MFMAs.
template <int NRB>
__device__ __forceinline__ void tile_times_image_bf16(f32x4 (&acc)[NRB], const __bf16 *arow, int pitch, const __bf16 *brow, int kp)
{
#pragma unroll
    for (int r = 0; r < NRB; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kp; k0 += 32) {
        const pair_bf16x8 b = *reinterpret_cast<const pair_bf16x8 *>(brow + k0);
#pragma unroll
        for (int r = 0; r < NRB; ++r)
            acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const pair_bf16x8 *>(arow + r * 16 * pitch + k0), b, acc[r], 0, 0, 0);
    }
}

// where a phase's results go
constexpr int kPairToZ = 0;      // + bias, ReLU, into the z tile `zt` (columns in [N, np) store 0: the k padding of the next phase; columns
                                 // from np on are not stored)
constexpr int kPairToOut = 1;    // + bias, the optional ReLU (a.relu), to the rows p0 + row < a.P of a.out (a.out_bf16: its type)
constexpr int kPairToMsg = 2;    // + bias, as fp32 into the LDS tile `msg` of pitch `pitch_z` floats, columns below N: a message tile

// One MFMA phase of a tile: dst = epilogue(A tile [kPairRows x K] . W [K x N]) by work items of (16 columns) x (NRB row blocks), the
// items wave, wave + 4, ... of this wavefront.  ARGS: the launch's argument struct; only kPairToOut reads it.
template <int NRB, int DST, typename TX, typename ARGS>
__device__ __forceinline__ void pair_mlp_phase(const TX *atile, int pitch_a, int kp, const void *W, const __bf16 *wimg, int K, int N,
                                               const float *bias, TX *zt, int pitch_z, int np, const ARGS &a, int p0, float *msg = nullptr)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int SPLIT = kPairRB / NRB;   // items per column sub-tile
    const int wave = (int)threadIdx.x >> 6, wl = (int)threadIdx.x & 63, kq = wl >> 4;
    const int items = ((N + 15) >> 4) * SPLIT;
#pragma unroll 1
    for (int it = wave; it < items; it += kPairThreads >> 6) {
        const int cb = it / SPLIT, rb0 = (it % SPLIT) * NRB;
        const int col = cb * 16 + (wl & 15);
        const bool cok = col < N;
        f32x4 acc[NRB];
        if constexpr (B16)
            tile_times_image_bf16<NRB>(acc, atile + (rb0 * 16 + (wl & 15)) * pitch_a + 8 * kq, pitch_a, wimg + (size_t)col * pitch_a + 8 * kq, kp);
        else
            tile_times_weight_f32<NRB>(acc, atile + (rb0 * 16 + (wl & 15)) * pitch_a + kq, pitch_a, static_cast<const float *>(W), K, N, col, cok, kq);
        // D layout: col = lane % 16, row = 4 * (lane / 16) + reg
        const float bv = (bias && cok) ? bias[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < NRB; ++r) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = (rb0 + r) * 16 + 4 * kq + v;
                float o = acc[r][v];
                if (bias) o += bv;
                if constexpr (DST == kPairToZ) {
                    o = o < 0.0f ? 0.0f : o;   // (a NaN stays a NaN: relu_pack)
                    if (!cok) o = 0.0f;        // the k padding of phase 3, whatever m held
                    if (col < np) zt[row * pitch_z + col] = (TX)o;
                } else if constexpr (DST == kPairToOut) {
                    if (a.relu) o = o < 0.0f ? 0.0f : o;
                    const int p = p0 + row;
                    if (p < a.P && cok) {
                        if (a.out_bf16) static_cast<__bf16 *>(a.out)[(size_t)p * N + col] = (__bf16)o;
                        else static_cast<float *>(a.out)[(size_t)p * N + col] = o;
                    }
                } else {
                    if (cok) msg[row * pitch_z + col] = o;
                }
            }
        }
    }
}

}  // namespace
}  // namespace gnnagg
