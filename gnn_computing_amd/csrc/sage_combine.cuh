#pragma once
// sage_combine.cuh -- what the two kernels of the block SAGE layer share (agg_block_sage.hip: rows up to 256 features, the whole k in
// LDS; agg_block_sage_wide.hip: any width, k in chunks): the staging of a bf16 weight's k window into its LDS image and the fp32 product
// of a tile's k window with W through buffer loads.
#include "block_chain.cuh"

namespace gnnagg {
namespace {

constexpr int kSageThreads = 256;            // 4 wavefronts

typedef __bf16 sage_bf16x8 __attribute__((ext_vector_type(8)));

// One weight into its half of the image: wimg[n][0 .. kp) = W[0 .. K)[n] for the columns n < roundup16(N), zeros beyond K and N (wimg
// already points at the half's first k).  The two paths of stage_weight_bf16 (agg_gcn.hip): where N % 8 == 0 and W is 16-byte aligned one
// thread per 8 k x 8 columns -- eight 16-byte row pieces transposed in registers, one 16-byte LDS store per column; else one thread per
// (column, 8 k) with 2-byte loads.  Both write the same image.
__device__ __forceinline__ void stage_weight_half(__bf16 *wimg, int wpitch, int kp, const __bf16 *__restrict__ W, int K, int N)
{
    const unsigned short *Wu = reinterpret_cast<const unsigned short *>(W);
    const int ncols = (N + 15) & ~15;
    if ((N & 7) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
        const int nco = ncols >> 3;
        for (int i = threadIdx.x; i < nco * (kp >> 3); i += kSageThreads) {
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
    for (int i = threadIdx.x; i < ncols * (kp >> 3); i += kSageThreads) {
        const int n = i % ncols, k = (i / ncols) << 3;
        unsigned q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (n < N && k + j < K) ? (unsigned)Wu[(size_t)(k + j) * N + n] : 0u;
        *reinterpret_cast<uint4 *>(wimg + (size_t)n * wpitch + k) =
            make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
    }
}

// acc += arow[0 .. K) . W[0 .. K)[col], k ascending, for one half of the tile: the branch-free batches of tile_times_weight (agg_gcn.hip)
// with the accumulator carried in and out.  arow: this lane's tile row at its k offset kq = lane / 16 (A: row = lane % 16, k = lane / 16;
// B: k = lane / 16, col = lane % 16); the tile's columns [K, roundup4(K)) hold 0.  W operands as buffer loads: the per-lane byte offset
// in one VGPR (out of range for the padding columns, which then read 0), the k step in an SGPR.  k-quads past K inside a batch are
// clamped loads with zeroed operands: 0 * 0 leaves the chain as it is.
template <int KB>
__device__ __forceinline__ void half_times_weight(f32x4 &acc, const float *arow, const float *W, int K, int N, int col, bool cok, int kq)
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
    if (K != Kf) {  // ragged last quad: k = Kf + kq valid only below K (the tile's padding columns hold 0)
        const float b = (cok && Kf + kq < K) ? W[(size_t)(Kf + kq) * N + col] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[Kf], b, acc, 0, 0, 0);
    }
}

}  // namespace
}  // namespace gnnagg
