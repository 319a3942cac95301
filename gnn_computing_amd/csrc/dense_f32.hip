// dense_f32.hip -- the dense combine in fp32 (gnnagg_matmul_nn, the dense half of gnnagg_gcn_run_with_nn): C[M,N] = A[M,K] . B[K,N], all
// row-major fp32 -- the reference's matmul_NN (include/dense.h:4-23: cuBLAS Sgemm(T,T) + Sgeam transpose) and the dense half of aggr_gcn_nn
// (aggr_gcn.h:304-359).  The bf16 GEMM (dense_bf16.hip) is a separate kernel; the fused epilogue of the aggregation (k_gcn_plan_nn,
// k_dense_rows, tile_times_weight) lives in agg_gcn.hip.
//
// Regime: tall and skinny (M = |V|, K = feat_in, N = feat_out <= a few hundred) -- HBM-bound on reading A once.
//  * Every output element is ONE ascending-k chain of v_mfma_f32_32x32x2_f32 (k_dense_nn_tall: 16x16x4) steps, f32 in / f32 accumulate:
//    bit-for-bit an fmaf chain, so every kernel below equals the oracle's GEMM exactly, and they are interchangeable.
//  * launch_dense_nn (the end of this file) picks by shape, first match:
//      K in (64, 128], K % 4 == 0, M >= 500 000, 16-byte A   k_dense_nn_tall       W in registers, no workgroup barrier
//      N > 64 and M >= 1024 (wide outputs: persistent strips of 128 x 128 tiles, A read once whatever N is)
//        N % 128 == 0, 16-byte rows, K % 32 == 0             k_dense_nn_ahead<4>   chunks requested two periods ahead, hand-counted vmcnt
//        N % 128 == 0, 8-byte rows, K even                   k_dense_nn_ahead<2>   the same kernel text, two 8-byte loads per piece of A
//        N % 128 == 0, 16-byte rows, K % 32 != 0             k_dense_nn_lean<4>    descriptors rebased per chunk, the compiler's waits
//        anything else                                        k_dense_nn_strip<AV>  clamped addresses and masks: any N, K, alignment
//        (k_dense_nn_lean<2> is still instantiated; since the ahead kernels took its shapes no dispatch reaches it)
//      K = 32 / 64 / 96 / 128, 16-byte A                     k_dense_nn_up         all chunks of a tile requested up front
//      the rest                                              k_dense_nn            one chunk at a time
//  * The A/B switches these kernels grew up with (K chunk, workgroups per CU, lean against ahead, the operand pipeline of the burst, the
//    transposed accumulator, the per-phase timeline) are retired; their text is scripts/attic/gemm_switches_retired.patch.
#include "kernel_util.cuh"

#include <type_traits>

namespace gnnagg {

// ------------------------------------------------------------------- k_dense_nn: one chunk at a time
// One wavefront owns a 32x32 output tile.  A workgroup = 4 wavefronts = 128 rows x 32 columns; K is walked in chunks of 32 staged
// through LDS: A chunk with coalesced 128-byte row segments into a pitch-33 image (conflict-free operand reads: lane l reads row
// l&31, k = l>>5), B chunk as is (lane reads consecutive columns).
typedef float f32x16 __attribute__((ext_vector_type(16)));
static constexpr int kGemmRows = 128, kGemmCols = 32, kGemmKC = 32, kGemmPitch = 33;

__global__ __launch_bounds__(256) void k_dense_nn(const float *__restrict__ A, const float *__restrict__ B,
                                                  float *__restrict__ C, int M, int N, int K)
{
    __shared__ float As[kGemmRows * kGemmPitch];
    __shared__ float Bs[kGemmKC * kGemmCols];
    const int row0 = blockIdx.x * kGemmRows, col0 = blockIdx.y * kGemmCols;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kGemmKC) {
        // stage A[row0 .. +128, k0 .. +32): thread t loads rows t/8 + 32*j, floats (t%8)*4 .. +4
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = (threadIdx.x >> 3) + 32 * j, kq = (threadIdx.x & 7) * 4;
            const int gr = row0 + r, gk = k0 + kq;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (gr < M) {
                const float *src = A + (size_t)gr * K + gk;
                if (gk + 3 < K && ((uintptr_t)src & 15) == 0) {
                    const float4 t = *reinterpret_cast<const float4 *>(src);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (gk + q < K) v[q] = src[q];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) As[r * kGemmPitch + kq + q] = v[q];
        }
        // stage B[k0 .. +32, col0 .. +32): 1024 floats, 4 per thread
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = threadIdx.x + 256 * j, kk = e >> 5, cc = e & 31;
            Bs[e] = (k0 + kk < K && col0 + cc < N) ? B[(size_t)(k0 + kk) * N + col0 + cc] : 0.0f;
        }
        __syncthreads();
        // all 16 operand pairs of the chunk into registers first, then 16 back-to-back MFMAs
        float av[kGemmKC / 2], bv[kGemmKC / 2];
#pragma unroll
        for (int t = 0; t < kGemmKC / 2; ++t) {
            av[t] = As[(wave * 32 + (lane & 31)) * kGemmPitch + 2 * t + (lane >> 5)];
            bv[t] = Bs[(2 * t + (lane >> 5)) * kGemmCols + (lane & 31)];
        }
#pragma unroll
        for (int t = 0; t < kGemmKC / 2; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc, 0, 0, 0);
        __syncthreads();
    }
    // C/D layout of 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int col = col0 + (lane & 31);
    if (col < N) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = row0 + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (row < M) C[(size_t)row * N + col] = acc[reg];
        }
    }
}

// The narrow layers (K = 32 / 64 / 96 / 128 -> 32 or 64 columns) are one round of workgroups: 1323 tiles of 128 rows all resident at once,
// and in k_dense_nn each of them walks its K chunks one after the other -- request, wait, LDS, barrier, 16 MFMAs, barrier -- so a tile is
// NCH HBM latencies in a row and the launch is as long as that chain (27 us for 169 343 x 128 @ 128 x 32, half the HBM roofline, the same as
// rocBLAS).  Here ALL of a tile's chunks are requested before anything else happens, in straight-line code (NCH is a template parameter: no
// loop back-edge for the compiler's vmcnt bookkeeping to get lost at), and they are written to LDS and multiplied in order while the later
// ones are still in flight; the tile's whole B strip (K x 32 floats) goes to LDS once.  Same operand layout, same ascending-k chain per
// output as k_dense_nn: bit-exact.  16-byte aligned A rows, K = 32 NCH <= 128.
template <int NCH, int NCB>
__global__ __launch_bounds__(256) void k_dense_nn_up(const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C, int M, int N)
{
    // NCB = 32-column blocks per workgroup (1: N <= 32; 2: N <= 64 -- the tile of A is read once for both, not once per column block)
    constexpr int K = NCH * kGemmKC, BC = NCB * kGemmCols, NIMG = NCB == 1 ? 2 : 1;   // (two A images only where the LDS has room for them)
    __shared__ float As[NIMG][kGemmRows * kGemmPitch];
    __shared__ float Bs[K * BC];
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const int row0 = blockIdx.x * kGemmRows, col0 = blockIdx.y * BC;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // A through a descriptor rebased to the tile: rows beyond M are outside it (zeros)
    const size_t a_off = (size_t)row0 * K * sizeof(float), a_all = (size_t)M * K * sizeof(float);
    const size_t a_left = a_off < a_all ? a_all - a_off : 0;
    const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(A) + (size_t)row0 * K, 0,
                                                                            (int)(unsigned)(a_left < 0xfffffffcULL ? a_left : 0xfffffffcULL), 0x00020000);
    u4 ra[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            ra[c][j] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, ((((int)threadIdx.x >> 3) + 32 * j) * K + c * kGemmKC + ((int)threadIdx.x & 7) * 4) * (int)sizeof(float), 0, 0);
    // the B strip: K x BC floats, NCH x NCB x 4 per thread (column guard by clamp + select: no branch)
    constexpr int NBV = NCH * NCB * 4;
    float rb[NBV];
#pragma unroll
    for (int j = 0; j < NBV; ++j) {
        const int e = (int)threadIdx.x + 256 * j, kk = e / BC, cc = col0 + (e % BC);
        const float v = B[(size_t)kk * N + (cc < N ? cc : N - 1)];
        rb[j] = cc < N ? v : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < NBV; ++j) Bs[(int)threadIdx.x + 256 * j] = rb[j];
    f32x16 acc[NCB];
#pragma unroll
    for (int n = 0; n < NCB; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        float *as = As[NIMG == 2 ? (c & 1) : 0];
        if (NIMG == 1 && c > 0) __syncthreads();   // one image: every wavefront is done with chunk c - 1 before chunk c overwrites it
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float *d = as + (((int)threadIdx.x >> 3) + 32 * j) * kGemmPitch + ((int)threadIdx.x & 7) * 4;
            d[0] = __uint_as_float(ra[c][j][0]); d[1] = __uint_as_float(ra[c][j][1]); d[2] = __uint_as_float(ra[c][j][2]); d[3] = __uint_as_float(ra[c][j][3]);
        }
        __syncthreads();   // (two images: chunk c + 1 is written while chunk c is still being read by slower wavefronts)
        float av[kGemmKC / 2];
#pragma unroll
        for (int t = 0; t < kGemmKC / 2; ++t) av[t] = as[(wave * 32 + (lane & 31)) * kGemmPitch + 2 * t + (lane >> 5)];
#pragma unroll
        for (int n = 0; n < NCB; ++n) {
            float bv[kGemmKC / 2];
#pragma unroll
            for (int t = 0; t < kGemmKC / 2; ++t) bv[t] = Bs[(c * kGemmKC + 2 * t + (lane >> 5)) * BC + n * kGemmCols + (lane & 31)];
#pragma unroll
            for (int t = 0; t < kGemmKC / 2; ++t) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc[n], 0, 0, 0);
        }
    }
    // C/D layout of 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
        const int col = col0 + n * kGemmCols + (lane & 31);
        if (col < N) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = row0 + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                if (row < M) C[(size_t)row * N + col] = acc[n][reg];
            }
        }
    }
}

// Wide-N variant (N > 64: the 512 -> 128 layer of the 3-layer models): a workgroup owns a TM x 128 output tile (TM = 128 for the
// bulk), so A is read from HBM once whatever N is (k_dense_nn re-reads it per 32-column block); wavefront w owns the tile's columns
// [32 w, 32 w + 32) over all TM rows -- TM / 32 accumulators of 32 x 32: a k-step of 2 feeds TM / 32 MFMAs from TM / 32 + 1 operand
// reads (k_dense_nn: 1 MFMA from 2), which is what the matrix pipe needs to stay busy (k_dense_nn: 59 TFLOP/s on 169 343 x 512 @
// 512 x 128, rocBLAS 89).  K in chunks of 32 through a double-buffered LDS image (A: pitch 33, B: as is): the next chunk's global
// loads are in flight during the current chunk's MFMAs, one barrier per chunk.  Every accumulator is still one ascending-k chain of
// v_mfma_f32_32x32x2_f32 steps: bit-exact against the oracle's GEMM like the other two kernels.
// Tail: two workgroups fit a CU (LDS, 256 registers), so the chip runs 2 x CUs tiles at a time and 169 343 rows = 1323 tiles of 128
// are 2.58 rounds of 512 -- the third round 58 % full.  The rows beyond the last full round are cut into at most one round of
// SMALLER tiles instead (TMT = 32 / 64 / 96 rows: 2 rounds of 128 + 1 of 96 here, 2.75 round-times instead of 3).
// (K chunk 16 with 3 or 4 workgroups per CU, 8 with 4: 273-294 us on 169 343 x 512 @ 512 x 128 against 266 us for 32 with 2 --
// more wavefronts per SIMD buy nothing here)
static constexpr int kBigT = 128, kBigKC = 32, kBigPA = kBigKC + 1;
static constexpr int kBigWgs = 2;   // workgroups per CU (LDS: 66.6 KB each)

// AV: floats per aligned load of A (4: K % 4 == 0 and A 16-byte aligned; 2: K even, A 8-byte aligned -- the 602-wide layer; 1: any).
// AV > 1 also says N % 4 == 0 and B 16-byte aligned: every 4-float piece of B is one aligned load.
// (Round 3's k_dense_nn_big -- one 128-row tile per workgroup, a last round of smaller tiles -- is gone: the strips below do the same
// arithmetic without a partial last round; its text is in git history, its numbers in profiles/r03/gemm.txt.)
template <int AV>
__global__ __launch_bounds__(256, kBigWgs) void k_dense_nn_strip(const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C,
                                                                 int M, int N, int K, int nb32, int nstrips)
{
    extern __shared__ float lds[];
    constexpr int KQ = kBigKC / 4, NA = kBigT * KQ / 256, NB = kBigKC * (kBigT / 4) / 256, BV = AV > 1 ? 4 : 1;
    const int col0 = blockIdx.y * kBigT;
    const int q = nb32 / nstrips, extra = nb32 - q * nstrips, sidx = blockIdx.x;
    const int blk0 = sidx * q + (sidx < extra ? sidx : extra), nblk = q + (sidx < extra ? 1 : 0);
    if (nblk == 0) return;
    float *As0 = lds, *As1 = lds + kBigT * kBigPA, *Bs0 = lds + 2 * kBigT * kBigPA, *Bs1 = Bs0 + kBigKC * kBigT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    float4 ra[NA], rb[NB];
    auto load_a = [&](int r, int c) -> float4 {   // clamped (always valid) addresses; zeroing happens at the stash
        const int rc = r < M ? r : M - 1;
        const float *src = A + (size_t)rc * K;
        if constexpr (AV == 4) return *reinterpret_cast<const float4 *>(src + (c < K ? c : K - 4));
        else if constexpr (AV == 2) {
            const float2 lo = *reinterpret_cast<const float2 *>(src + (c < K ? c : K - 2)), hi = *reinterpret_cast<const float2 *>(src + (c + 2 < K ? c + 2 : K - 2));
            return make_float4(lo.x, lo.y, hi.x, hi.y);
        } else return make_float4(src[c < K ? c : K - 1], src[c + 1 < K ? c + 1 : K - 1], src[c + 2 < K ? c + 2 : K - 1], src[c + 3 < K ? c + 3 : K - 1]);
    };
    auto load_b = [&](int r, int c) -> float4 {
        const int rc = r < K ? r : K - 1;
        const float *src = B + (size_t)rc * N;
        if constexpr (BV == 4) return *reinterpret_cast<const float4 *>(src + (c < N ? c : N - 4));
        else return make_float4(src[c < N ? c : N - 1], src[c + 1 < N ? c + 1 : N - 1], src[c + 2 < N ? c + 2 : N - 1], src[c + 3 < N ? c + 3 : N - 1]);
    };
    auto keep4 = [](float4 v, bool k0, bool k1, bool k2, bool k3) -> float4 {   // bit masks, not selects
        v.x = __uint_as_float(__float_as_uint(v.x) & (k0 ? 0xffffffffu : 0u)); v.y = __uint_as_float(__float_as_uint(v.y) & (k1 ? 0xffffffffu : 0u));
        v.z = __uint_as_float(__float_as_uint(v.z) & (k2 ? 0xffffffffu : 0u)); v.w = __uint_as_float(__float_as_uint(v.w) & (k3 ? 0xffffffffu : 0u));
        return v;
    };
    auto fetch = [&](int row0, int k0) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int p = (int)threadIdx.x + 256 * j;
            ra[j] = load_a(row0 + p / KQ, k0 + (p % KQ) * 4);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) rb[j] = load_b(k0 + (threadIdx.x >> 5) + 8 * j, col0 + (threadIdx.x & 31) * 4);
    };
    auto stash = [&](float *As, float *Bs, int row0, int k0) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int p = (int)threadIdx.x + 256 * j;
            const int r = row0 + p / KQ, c = k0 + (p % KQ) * 4;
            const bool rok = r < M;
            const float4 v = AV == 4 ? keep4(ra[j], rok && c < K, rok && c < K, rok && c < K, rok && c < K)
                             : AV == 2 ? keep4(ra[j], rok && c < K, rok && c < K, rok && c + 2 < K, rok && c + 2 < K)
                                       : keep4(ra[j], rok && c < K, rok && c + 1 < K, rok && c + 2 < K, rok && c + 3 < K);
            float *da = As + (p / KQ) * kBigPA + (p % KQ) * 4;
            da[0] = v.x; da[1] = v.y; da[2] = v.z; da[3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int r = k0 + (threadIdx.x >> 5) + 8 * j, c = col0 + (threadIdx.x & 31) * 4;
            const bool rok = r < K;
            *reinterpret_cast<float4 *>(Bs + ((threadIdx.x >> 5) + 8 * j) * kBigT + (threadIdx.x & 31) * 4) =
                BV == 4 ? keep4(rb[j], rok && c < N, rok && c < N, rok && c < N, rok && c < N)
                        : keep4(rb[j], rok && c < N, rok && c + 1 < N, rok && c + 2 < N, rok && c + 3 < N);
        }
    };
    // rbk: 32-row blocks of the tile (workgroup-uniform): the blocks beyond it are skipped by scalar branches (one code path: four
    // unrolled variants of the chunk keep four operand sets alive and spill)
    auto mma = [&](int rbk, const float *As, const float *Bs) {
        const float *ap = As + (lane & 31) * kBigPA + (lane >> 5);
        const float *bp = Bs + (lane >> 5) * kBigT + 32 * wave + (lane & 31);
        // operands of k-step t + 1 are requested before the MFMAs of k-step t (4 x 64 pipe cycles cover the LDS latency); rows of the
        // image that belong to no block of the tile are read and never used
        float a_cur[4], a_nxt[4], b_cur, b_nxt;
#pragma unroll
        for (int i = 0; i < 4; ++i) a_cur[i] = ap[i * 32 * kBigPA];
        b_cur = bp[0];
        // (s_setprio around the burst -- so that the two wavefronts that share a SIMD's matrix pipe fall out of phase -- measured:
        // 201.1 against 202.2 us, nothing)
#pragma unroll
        for (int t = 0; t < kBigKC / 2; ++t) {
            if (t + 1 < kBigKC / 2) {
#pragma unroll
                for (int i = 0; i < 4; ++i) a_nxt[i] = ap[i * 32 * kBigPA + 2 * (t + 1)];
                b_nxt = bp[2 * (t + 1) * kBigT];
            }
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[0], b_cur, acc[0], 0, 0, 0);
            if (rbk > 1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[1], b_cur, acc[1], 0, 0, 0);
            if (rbk > 2) acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[2], b_cur, acc[2], 0, 0, 0);
            if (rbk > 3) acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[3], b_cur, acc[3], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) a_cur[i] = a_nxt[i];
            b_cur = b_nxt;
        }
    };
    const int nchunks = (K + kBigKC - 1) / kBigKC;
    const int ntiles = (nblk + 3) >> 2, total = ntiles * nchunks;   // the strip as ONE sequence of chunks g = tile * nchunks + c
    const int col = col0 + 32 * wave + (lane & 31);
    auto row_of = [&](int g) { return (blk0 + 4 * (g / nchunks)) * 32; };
    auto k_of = [&](int g) { return (g % nchunks) * kBigKC; };
    // While chunk g is multiplied out of LDS buffer g & 1, chunk g + 1 travels to registers; after the MFMAs it goes to the other LDS
    // buffer.  (A second register set -- chunk g + 2 requested during chunk g -- was built and measured: 206.7 against 201-205 us on the
    // 512 -> 128 layer; the loads are not what the matrix pipe waits for.  profiles/r04/gemm.txt)
    fetch(row_of(0), 0);
    stash(As0, Bs0, row_of(0), 0);
    __syncthreads();
    for (int g = 0; g < total; ++g) {
        const float *As = (g & 1) ? As1 : As0, *Bs = (g & 1) ? Bs1 : Bs0;
        const int tile = g / nchunks, c = g - tile * nchunks;
        const int row0 = (blk0 + 4 * tile) * 32;
        const int rbk = nblk - 4 * tile < 4 ? nblk - 4 * tile : 4;   // 32-row blocks of this tile (workgroup-uniform)
        // (unconditional: the last step re-requests the last chunk -- behind a branch the fetch registers meet in phi copies, and the
        // copies wait for the loads that were just issued)
        const int gn = g + 1 < total ? g + 1 : total - 1;
        fetch(row_of(gn), k_of(gn));
        mma(rbk, As, Bs);
        if (c + 1 == nchunks) {
            // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  Buffer stores: ONE
            // lane offset + a scalar offset per store (64 global addresses computed up front cost 128 registers while the next
            // tile's fetch is in flight), and rows beyond M fall off the end of the buffer -- the hardware drops them
            const size_t co = (size_t)row0 * N * sizeof(float), c_bytes = (size_t)M * N * sizeof(float);   // descriptor rebased to C[row0][0]
            const size_t cr = co < c_bytes ? c_bytes - co : 0;
            const __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(C + (size_t)row0 * N, 0, (int)(unsigned)(cr < 0xfffffffcULL ? cr : 0xfffffffcULL), 0x00020000);
            const unsigned voff = (unsigned)(((size_t)(4 * (lane >> 5)) * N + col) * sizeof(float));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < rbk && col < N) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[i][reg]), crsrc, voff,
                                                              (unsigned)((32 * i + (reg & 3) + 8 * (reg >> 2)) * N) * (unsigned)sizeof(float), 0);
                }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) acc[i][reg] = 0.0f;
            }
        }
        if (g + 1 < total) stash((g & 1) ? As0 : As1, (g & 1) ? Bs0 : Bs1, row_of(g + 1), k_of(g + 1));   // the other buffer: last read one chunk ago
        __syncthreads();
    }
}

// Round 4, second step: the LEAN form of the strip kernel.  A per-phase timeline (scripts/attic/exp_gemm_timeline.py, s_memtime stamps) showed
// where a chunk goes: issuing the 8 loads of the next chunk 20 % of the period, the 64 MFMAs 35 %, the stash 20 %, the barrier 12 % -- and the
// MFMA phase runs at 80 ticks per MFMA, i.e. the two wavefronts of a SIMD ALTERNATE: while one bursts, every other instruction of its
// neighbour (address arithmetic, clamps, masks, LDS writes: ~210 per chunk) trickles out between MFMAs at ~30 ticks apiece.  The matrix
// pipe is busy 2 x 35 %.  So everything that is not an MFMA or an operand read is made cheap in INSTRUCTIONS:
//   * A and B come through buffer descriptors REBASED per chunk in scalar registers (base = A + row0 * K + k0): the per-thread offsets are
//     computed once per kernel, a fetch is 8 buffer loads and a handful of scalar instructions, and rows beyond M / k beyond K are
//     out of range of the descriptor -- the hardware returns zeros, no clamps, no masks;
//   * only the ragged last K chunk (K % 32 != 0: the 602-wide layer) masks, behind a workgroup-uniform branch;
//   * the chunk / tile counters advance by addition (g / nchunks was an integer division per chunk).
// Needs N % 128 == 0, K even and 8-byte aligned rows; other shapes keep k_dense_nn_strip.  Same arithmetic: bit-exact.
template <int AV>
__global__ __launch_bounds__(256, kBigWgs) void k_dense_nn_lean(const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C,
                                                                int M, int N, int K, int nb32, int nstrips)
{
    static_assert(AV == 4 || AV == 2, "lean form: 16- or 8-byte loads of A");
    extern __shared__ float lds[];
    constexpr int KQ = kBigKC / 4, NA = kBigT * KQ / 256, NB = kBigKC * (kBigT / 4) / 256;
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    const int col0 = blockIdx.y * kBigT;
    const int q = nb32 / nstrips, extra = nb32 - q * nstrips, sidx = blockIdx.x;
    const int blk0 = sidx * q + (sidx < extra ? sidx : extra), nblk = q + (sidx < extra ? 1 : 0);
    if (nblk == 0) return;
    float *As0 = lds, *As1 = lds + kBigT * kBigPA, *Bs0 = lds + 2 * kBigT * kBigPA, *Bs1 = Bs0 + kBigKC * kBigT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    // per-thread constants: byte offsets of this thread's pieces inside a chunk (global) and inside the LDS images
    int voa[NA], vob[NB], la[NA], lb[NB];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int p = (int)threadIdx.x + 256 * j;
        voa[j] = ((p / KQ) * K + (p % KQ) * 4) * (int)sizeof(float);
        la[j] = (p / KQ) * kBigPA + (p % KQ) * 4;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        vob[j] = (((int)(threadIdx.x >> 5) + 8 * j) * N + (int)(threadIdx.x & 31) * 4) * (int)sizeof(float);
        lb[j] = ((int)(threadIdx.x >> 5) + 8 * j) * kBigT + (int)(threadIdx.x & 31) * 4;
    }
    const size_t a_bytes = (size_t)M * K * sizeof(float), b_bytes = (size_t)K * N * sizeof(float);
    float4 ra[NA], rb[NB];
    // chunk (row0, k0): descriptors whose first byte is A[row0][k0] / B[k0][col0] and whose size is what is left of the matrix (capped at
    // 4 GB - 4: a tile is 128 rows, the cap is never what decides a row of it)
    auto fetch = [&](int row0, int k0) {
        const size_t ao = ((size_t)row0 * K + k0) * sizeof(float), bo = ((size_t)k0 * N + col0) * sizeof(float);
        const size_t ar = ao < a_bytes ? a_bytes - ao : 0, br = bo < b_bytes ? b_bytes - bo : 0;
        const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(A) + ((size_t)row0 * K + k0), 0,
                                                                                (int)(unsigned)(ar < 0xfffffffcULL ? ar : 0xfffffffcULL), 0x00020000);
        const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(B) + ((size_t)k0 * N + col0), 0,
                                                                                (int)(unsigned)(br < 0xfffffffcULL ? br : 0xfffffffcULL), 0x00020000);
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            if constexpr (AV == 4) {
                const u4 v = __builtin_amdgcn_raw_buffer_load_b128(arsrc, voa[j], 0, 0);
                ra[j] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
            } else {
                const u2 lo = __builtin_amdgcn_raw_buffer_load_b64(arsrc, voa[j], 0, 0), hi = __builtin_amdgcn_raw_buffer_load_b64(arsrc, voa[j] + 8, 0, 0);
                ra[j] = make_float4(__uint_as_float(lo[0]), __uint_as_float(lo[1]), __uint_as_float(hi[0]), __uint_as_float(hi[1]));
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const u4 v = __builtin_amdgcn_raw_buffer_load_b128(brsrc, vob[j], 0, 0);
            rb[j] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
        }
    };
    auto stash = [&](float *As, float *Bs, int k0) {
        if (k0 + kBigKC > K) {   // the ragged last chunk (workgroup-uniform): A's k beyond K belongs to the next row, not to nothing
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int c = k0 + (((int)threadIdx.x + 256 * j) % KQ) * 4;
                const unsigned m0 = c < K ? 0xffffffffu : 0u, m1 = c + 1 < K ? 0xffffffffu : 0u, m2 = c + 2 < K ? 0xffffffffu : 0u, m3 = c + 3 < K ? 0xffffffffu : 0u;
                ra[j].x = __uint_as_float(__float_as_uint(ra[j].x) & m0); ra[j].y = __uint_as_float(__float_as_uint(ra[j].y) & m1);
                ra[j].z = __uint_as_float(__float_as_uint(ra[j].z) & m2); ra[j].w = __uint_as_float(__float_as_uint(ra[j].w) & m3);
            }
        }
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            float *da = As + la[j];
            da[0] = ra[j].x; da[1] = ra[j].y; da[2] = ra[j].z; da[3] = ra[j].w;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) *reinterpret_cast<float4 *>(Bs + lb[j]) = rb[j];
    };
    // RBK (32-row blocks of this tile: 4 except at the end of a strip) is a compile-time constant of the burst: with a run-time count every
    // MFMA sat in a basic block of its own behind a scalar branch (ISA of round 4's kernel: 64 one-MFMA blocks, ~190 branch instructions and
    // a wait per chunk), so nothing could be scheduled across them
    auto mma = [&](auto rbk_c, const float *As, const float *Bs) {
        constexpr int RBK = decltype(rbk_c)::value;
        const float *ap = As + (lane & 31) * kBigPA + (lane >> 5);
        const float *bp = Bs + (lane >> 5) * kBigT + 32 * wave + (lane & 31);
        float a_cur[RBK], a_nxt[RBK], b_cur, b_nxt;
#pragma unroll
        for (int i = 0; i < RBK; ++i) a_cur[i] = ap[i * 32 * kBigPA];
        b_cur = bp[0];
#pragma unroll
        for (int t = 0; t < kBigKC / 2; ++t) {
            if (t + 1 < kBigKC / 2) {
#pragma unroll
                for (int i = 0; i < RBK; ++i) a_nxt[i] = ap[i * 32 * kBigPA + 2 * (t + 1)];
                b_nxt = bp[2 * (t + 1) * kBigT];
            }
#pragma unroll
            for (int i = 0; i < RBK; ++i) {
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[i], b_cur, acc[i], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < RBK; ++i) a_cur[i] = a_nxt[i];
            b_cur = b_nxt;
        }
    };
    const int nchunks = (K + kBigKC - 1) / kBigKC;
    const int ntiles = (nblk + 3) >> 2, total = ntiles * nchunks;
    const int colc = (32 * wave + (lane & 31)) * (int)sizeof(float);
    fetch(blk0 * 32, 0);
    stash(As0, Bs0, 0);
    __syncthreads();
    int c = 0, row0 = blk0 * 32, left = nblk;   // chunk inside the tile, the tile's first row, 32-row blocks from this tile on
    for (int g = 0; g < total; ++g) {
        const float *As = (g & 1) ? As1 : As0, *Bs = (g & 1) ? Bs1 : Bs0;
        const int rbk = left < 4 ? left : 4;
        const bool last_c = c + 1 == nchunks;
        // the next chunk (the last step re-requests its own: unconditional, see k_dense_nn_strip)
        const int nrow0 = last_c && g + 1 < total ? row0 + kBigT : row0;
        const int nk0 = g + 1 < total ? (last_c ? 0 : (c + 1) * kBigKC) : c * kBigKC;
        fetch(nrow0, nk0);
        // (measured on this form and not kept, profiles/r04/gemm.txt: s_setprio low inside the burst / high outside -- the stash and barrier
        // phases shrink, the fetch phase grows, 191.8-205 against 194 us; a second register set with chunk g + 2 in flight -- 195.5; K chunks
        // of 16 with 3 / 4 workgroups per CU -- 193.6 / 207.5; the next chunk's stash folded into the second half of the burst -- the stash
        // phase goes from 19 % to 4 % of the period and the burst grows by as much: 200 against 194 us at the same ratio to rocBLAS)
        if (rbk == 4) mma(std::integral_constant<int, 4>{}, As, Bs);
        else if (rbk == 3) mma(std::integral_constant<int, 3>{}, As, Bs);
        else if (rbk == 2) mma(std::integral_constant<int, 2>{}, As, Bs);
        else mma(std::integral_constant<int, 1>{}, As, Bs);
        if (last_c) {
            // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); a descriptor rebased to
            // C[row0][col0]: one lane offset + a scalar offset per store, rows beyond M fall off its end
            const size_t co = ((size_t)row0 * N + col0) * sizeof(float), c_bytes = (size_t)M * N * sizeof(float);
            const size_t cr = co < c_bytes ? c_bytes - co : 0;
            const __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(C + ((size_t)row0 * N + col0), 0,
                                                                                    (int)(unsigned)(cr < 0xfffffffcULL ? cr : 0xfffffffcULL), 0x00020000);
            const int voff = 4 * (lane >> 5) * N * (int)sizeof(float) + colc;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < rbk) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[i][reg]), crsrc, voff,
                                                              (32 * i + (reg & 3) + 8 * (reg >> 2)) * N * (int)sizeof(float), 0);
                }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) acc[i][reg] = 0.0f;
            }
        }
        if (g + 1 < total) stash((g & 1) ? As0 : As1, (g & 1) ? Bs0 : Bs1, nk0);
        __syncthreads();
        if (last_c) { c = 0; row0 += kBigT; left -= 4; } else ++c;
    }
}

// k_dense_nn_lean with every chunk requested TWO periods before it is written to LDS, the wait for it counted by hand (round 5).
// Timing variants (profiles/r05/gemm_forms.txt) put the loss of the lean kernel against its compute-only rate on the HBM stream of A
// arriving late: with A served from L2 the same kernel runs at the compute-only rate.  A second register set alone does not buy a
// second period: hipcc's s_waitcnt bookkeeping does not survive the loop back-edge and the barrier -- it waits vmcnt(0) in front of the
// LDS writes, for the chunk requested a moment ago as well -- and a load whose destination is a compiler-visible value may be copied
// (v_mov) before it has landed.  So the producer side is inline assembly on FIXED registers the compiler never sees:
// `amdgpu_num_vgpr(192)` keeps its allocator below v192 (it needs 155), the two register sets are v192-v223 and v224-v255 (named as
// clobbers, so the kernel descriptor still says 256), and the loads, the one wait -- `s_waitcnt vmcnt(8)`: everything but the eight
// newest -- and the LDS writes are written out.  vmcnt also counts the C stores of a tile's last chunk; loads return in order among
// loads, so "at most 8 outstanding" always covers the 8 oldest loads.  Every iteration requests exactly 8 loads (past the end of the
// strip: the last chunk again), so the count is the same everywhere.  Chunk h travels in register set h & 1 and lands in LDS image
// h & 1.  Same arithmetic as k_dense_nn_lean: bit-exact.
// Measured (profiles/r05/gemm_forms.txt): 169 343 x 512 @ 512 x 128 204 -> 192 us (115.6 TF); THREE periods (three sets from v160, the
// compiler squeezed into 160 registers, the image of a chunk a run-time value) 198.6 us -- two is where it pays.
// AV = floats per aligned load of A, the only thing the two instantiations differ in:
//   4: 16-byte aligned A rows and K % 32 == 0.  A piece of A is one 16-byte load: 8 loads per chunk, the counts above.
//   2: A rows that are only 8-byte aligned and any even K (the 602-wide layer).  A piece is two 8-byte loads: 12 loads per chunk, the
//      wait is `s_waitcnt vmcnt(12)`, and the last chunk of a ragged K is masked in the registers before it goes to LDS (A's k beyond K
//      belongs to the next row, not to nothing; B's rows beyond K are outside its descriptor).
// Other shapes stay on k_dense_nn_lean.  One kernel text for both: a fix to the register sets or the counting lands in both.
#define GNNAGG_AHEAD_LOAD(REGS, C0, C1, C2, C3, OFF, RSRC) \
    asm volatile("buffer_load_dwordx4 " REGS ", %0, %1, 0 offen" :: "v"(OFF), "s"(RSRC) : "memory", C0, C1, C2, C3)
#define GNNAGG_AHEAD_LOAD_A(C0, C1, C2, C3, OFF, RSRC)                                                                             \
    if constexpr (AV == 4) GNNAGG_AHEAD_LOAD("v[" C0 ":" C3 "]", "v" C0, "v" C1, "v" C2, "v" C3, OFF, RSRC);                        \
    else asm volatile("buffer_load_dwordx2 v[" C0 ":" C1 "], %0, %1, 0 offen\n\tbuffer_load_dwordx2 v[" C2 ":" C3 "], %0, %1, 0 offen offset:8" \
                      :: "v"(OFF), "s"(RSRC) : "memory", "v" C0, "v" C1, "v" C2, "v" C3)
#define GNNAGG_AHEAD_MASK(C0, C1, C2, C3, CBASE)                                                                                    \
    {                                                                                                                              \
        const int c_ = (CBASE);                                                                                                    \
        const unsigned m0_ = c_ < K ? 0xffffffffu : 0u, m1_ = c_ + 1 < K ? 0xffffffffu : 0u, m2_ = c_ + 2 < K ? 0xffffffffu : 0u,   \
                       m3_ = c_ + 3 < K ? 0xffffffffu : 0u;                                                                         \
        asm volatile("v_and_b32 v" C0 ", %0, v" C0 "\n\tv_and_b32 v" C1 ", %1, v" C1 "\n\tv_and_b32 v" C2 ", %2, v" C2 "\n\tv_and_b32 v" C3 ", %3, v" C3 \
                     :: "v"(m0_), "v"(m1_), "v"(m2_), "v"(m3_) : "memory", "v" C0, "v" C1, "v" C2, "v" C3);                          \
    }
#define GNNAGG_AHEAD_STASH_A(R0, R1, R2, R3, ADDR) \
    asm volatile("ds_write2_b32 %0, " R0 ", " R1 " offset1:1\n\tds_write2_b32 %0, " R2 ", " R3 " offset0:2 offset1:3" :: "v"(ADDR) : "memory")
#define GNNAGG_AHEAD_STASH_B(REGS, ADDR) asm volatile("ds_write_b128 %0, " REGS :: "v"(ADDR) : "memory")
// everything but the newest chunk's loads has landed: 4 + 4 loads per chunk at AV = 4, 8 + 4 at AV = 2
#define GNNAGG_AHEAD_WAIT                                                  \
    if constexpr (AV == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); \
    else asm volatile("s_waitcnt vmcnt(12)" ::: "memory")
template <int AV>
__global__ __launch_bounds__(256, kBigWgs) __attribute__((amdgpu_num_vgpr(192))) void k_dense_nn_ahead(
    const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C, int M, int N, int K, int nb32, int nstrips)
{
    extern __shared__ float lds[];
    constexpr int KQ = kBigKC / 4, NA = kBigT * KQ / 256, NB = kBigKC * (kBigT / 4) / 256;
    static_assert(AV == 4 || AV == 2, "ahead form: 16- or 8-byte loads of A");
    static_assert(NA == 4 && NB == 4, "the register sets and the hand-counted wait assume 4 pieces of A (one 16-byte or two 8-byte loads each) + 4 of B per chunk");
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) float *lds_f;
    const int col0 = blockIdx.y * kBigT;
    const int q = nb32 / nstrips, extra = nb32 - q * nstrips, sidx = blockIdx.x;
    const int blk0 = sidx * q + (sidx < extra ? sidx : extra), nblk = q + (sidx < extra ? 1 : 0);
    if (nblk == 0) return;
    float *As0 = lds, *As1 = lds + kBigT * kBigPA, *Bs0 = lds + 2 * kBigT * kBigPA, *Bs1 = Bs0 + kBigKC * kBigT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    // per-thread constants: byte offsets of this thread's pieces inside a chunk (global) and LDS byte addresses inside image 0
    int voa[NA], vob[NB];
    unsigned la0[NA], lb0[NB];
    const unsigned img_a = kBigT * kBigPA * (unsigned)sizeof(float), img_b = kBigKC * kBigT * (unsigned)sizeof(float);   // image 1 = image 0 + this
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int p = (int)threadIdx.x + 256 * j;
        voa[j] = ((p / KQ) * K + (p % KQ) * 4) * (int)sizeof(float);
        la0[j] = (unsigned)(unsigned long long)(lds_f)(As0 + (p / KQ) * kBigPA + (p % KQ) * 4);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        vob[j] = (((int)(threadIdx.x >> 5) + 8 * j) * N + (int)(threadIdx.x & 31) * 4) * (int)sizeof(float);
        lb0[j] = (unsigned)(unsigned long long)(lds_f)(Bs0 + ((int)(threadIdx.x >> 5) + 8 * j) * kBigT + (int)(threadIdx.x & 31) * 4);
    }
    const size_t a_bytes = (size_t)M * K * sizeof(float), b_bytes = (size_t)K * N * sizeof(float);
    // a raw buffer descriptor by hand (base, stride 0, bytes, the flags __builtin_amdgcn_make_buffer_rsrc is given elsewhere in this file)
    auto rsrc_of = [](const float *base, size_t bytes) -> u4 {
        const unsigned long long a = (unsigned long long)base;
        u4 r;
        r[0] = (unsigned)a; r[1] = (unsigned)(a >> 32) & 0xffffu; r[2] = (unsigned)(bytes < 0xfffffffcULL ? bytes : 0xfffffffcULL); r[3] = 0x00020000u;
        return r;
    };
    const int nchunks = AV == 4 ? K / kBigKC : (K + kBigKC - 1) / kBigKC;   // (AV = 4: K % 32 == 0)
    const int ntiles = (nblk + 3) >> 2, total = ntiles * nchunks;
    // the next chunk to REQUEST: (fc, frow0), index fi; past the last chunk of the strip the last one is requested again
    int fc = 0, frow0 = blk0 * 32, fi = 0;
    [[maybe_unused]] int sc = 0;   // AV = 2: chunk-in-tile of the next chunk to WRITE to LDS (its k0 decides the ragged mask)
#define GNNAGG_AHEAD_FETCH(SET)                                                                                                                       \
    {                                                                                                                                                 \
        const int k0_ = fc * kBigKC;                                                                                                                  \
        const size_t ao_ = ((size_t)frow0 * K + k0_) * sizeof(float), bo_ = ((size_t)k0_ * N + col0) * sizeof(float);                                 \
        const u4 ar_ = rsrc_of(A + ((size_t)frow0 * K + k0_), ao_ < a_bytes ? a_bytes - ao_ : 0);                                                     \
        const u4 br_ = rsrc_of(B + ((size_t)k0_ * N + col0), bo_ < b_bytes ? b_bytes - bo_ : 0);                                                      \
        if (SET == 0) {                                                                                                                               \
            GNNAGG_AHEAD_LOAD_A("192", "193", "194", "195", voa[0], ar_);                                                                             \
            GNNAGG_AHEAD_LOAD_A("196", "197", "198", "199", voa[1], ar_);                                                                             \
            GNNAGG_AHEAD_LOAD_A("200", "201", "202", "203", voa[2], ar_);                                                                             \
            GNNAGG_AHEAD_LOAD_A("204", "205", "206", "207", voa[3], ar_);                                                                             \
            GNNAGG_AHEAD_LOAD("v[208:211]", "v208", "v209", "v210", "v211", vob[0], br_);                                                             \
            GNNAGG_AHEAD_LOAD("v[212:215]", "v212", "v213", "v214", "v215", vob[1], br_);                                                             \
            GNNAGG_AHEAD_LOAD("v[216:219]", "v216", "v217", "v218", "v219", vob[2], br_);                                                             \
            GNNAGG_AHEAD_LOAD("v[220:223]", "v220", "v221", "v222", "v223", vob[3], br_);                                                             \
        } else {                                                                                                                                      \
            GNNAGG_AHEAD_LOAD_A("224", "225", "226", "227", voa[0], ar_);                                                                             \
            GNNAGG_AHEAD_LOAD_A("228", "229", "230", "231", voa[1], ar_);                                                                             \
            GNNAGG_AHEAD_LOAD_A("232", "233", "234", "235", voa[2], ar_);                                                                             \
            GNNAGG_AHEAD_LOAD_A("236", "237", "238", "239", voa[3], ar_);                                                                             \
            GNNAGG_AHEAD_LOAD("v[240:243]", "v240", "v241", "v242", "v243", vob[0], br_);                                                             \
            GNNAGG_AHEAD_LOAD("v[244:247]", "v244", "v245", "v246", "v247", vob[1], br_);                                                             \
            GNNAGG_AHEAD_LOAD("v[248:251]", "v248", "v249", "v250", "v251", vob[2], br_);                                                             \
            GNNAGG_AHEAD_LOAD("v[252:255]", "v252", "v253", "v254", "v255", vob[3], br_);                                                             \
        }                                                                                                                                             \
        if (fi + 1 < total) { ++fi; if (fc + 1 == nchunks) { fc = 0; frow0 += kBigT; } else ++fc; }                                                   \
    }
    // set SET (landed: the caller waited) -> LDS image SET; then the LDS writes are drained so that the set can be requested into again
#define GNNAGG_AHEAD_STASH(SET, K0)                                                                                                                   \
    {                                                                                                                                                 \
        if constexpr (AV == 2) if ((K0) + kBigKC > K) {   /* the ragged last chunk (workgroup-uniform) */                                             \
            if (SET == 0) {                                                                                                                           \
            GNNAGG_AHEAD_MASK("192", "193", "194", "195", (K0) + (((int)threadIdx.x + 256 * 0) % KQ) * 4)                                             \
            GNNAGG_AHEAD_MASK("196", "197", "198", "199", (K0) + (((int)threadIdx.x + 256 * 1) % KQ) * 4)                                             \
            GNNAGG_AHEAD_MASK("200", "201", "202", "203", (K0) + (((int)threadIdx.x + 256 * 2) % KQ) * 4)                                             \
            GNNAGG_AHEAD_MASK("204", "205", "206", "207", (K0) + (((int)threadIdx.x + 256 * 3) % KQ) * 4)                                             \
            } else {                                                                                                                                  \
            GNNAGG_AHEAD_MASK("224", "225", "226", "227", (K0) + (((int)threadIdx.x + 256 * 0) % KQ) * 4)                                             \
            GNNAGG_AHEAD_MASK("228", "229", "230", "231", (K0) + (((int)threadIdx.x + 256 * 1) % KQ) * 4)                                             \
            GNNAGG_AHEAD_MASK("232", "233", "234", "235", (K0) + (((int)threadIdx.x + 256 * 2) % KQ) * 4)                                             \
            GNNAGG_AHEAD_MASK("236", "237", "238", "239", (K0) + (((int)threadIdx.x + 256 * 3) % KQ) * 4)                                             \
            }                                                                                                                                         \
        }                                                                                                                                             \
        if (SET == 0) {                                                                                                                               \
            GNNAGG_AHEAD_STASH_A("v192", "v193", "v194", "v195", la0[0]);                                                                             \
            GNNAGG_AHEAD_STASH_A("v196", "v197", "v198", "v199", la0[1]);                                                                             \
            GNNAGG_AHEAD_STASH_A("v200", "v201", "v202", "v203", la0[2]);                                                                             \
            GNNAGG_AHEAD_STASH_A("v204", "v205", "v206", "v207", la0[3]);                                                                             \
            GNNAGG_AHEAD_STASH_B("v[208:211]", lb0[0]);                                                                                               \
            GNNAGG_AHEAD_STASH_B("v[212:215]", lb0[1]);                                                                                               \
            GNNAGG_AHEAD_STASH_B("v[216:219]", lb0[2]);                                                                                               \
            GNNAGG_AHEAD_STASH_B("v[220:223]", lb0[3]);                                                                                               \
        } else {                                                                                                                                      \
            GNNAGG_AHEAD_STASH_A("v224", "v225", "v226", "v227", la0[0] + img_a);                                                                     \
            GNNAGG_AHEAD_STASH_A("v228", "v229", "v230", "v231", la0[1] + img_a);                                                                     \
            GNNAGG_AHEAD_STASH_A("v232", "v233", "v234", "v235", la0[2] + img_a);                                                                     \
            GNNAGG_AHEAD_STASH_A("v236", "v237", "v238", "v239", la0[3] + img_a);                                                                     \
            GNNAGG_AHEAD_STASH_B("v[240:243]", lb0[0] + img_b);                                                                                       \
            GNNAGG_AHEAD_STASH_B("v[244:247]", lb0[1] + img_b);                                                                                       \
            GNNAGG_AHEAD_STASH_B("v[248:251]", lb0[2] + img_b);                                                                                       \
            GNNAGG_AHEAD_STASH_B("v[252:255]", lb0[3] + img_b);                                                                                       \
        }                                                                                                                                             \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                                            \
    }
    auto mma = [&](auto rbk_c, const float *As, const float *Bs) __attribute__((always_inline)) {
        constexpr int RBK = decltype(rbk_c)::value;
        const float *ap = As + (lane & 31) * kBigPA + (lane >> 5);
        const float *bp = Bs + (lane >> 5) * kBigT + 32 * wave + (lane & 31);
        // two k-steps (a "pair": 2 RBK MFMAs) per stage; the operand reads of pair p + 1 are issued BEFORE the MFMAs of pair p (left to
        // itself the compiler issues them behind the pair's last MFMA and waits for them in front of the next one)
        float a[2][RBK][2], b[2][2];
#define GNNAGG_RD(BUF, PR)                                                                                                    \
        {                                                                                                                     \
            _Pragma("unroll") for (int i = 0; i < RBK; ++i) {                                                                 \
                a[BUF][i][0] = ap[i * 32 * kBigPA + 4 * (PR)]; a[BUF][i][1] = ap[i * 32 * kBigPA + 4 * (PR) + 2];             \
            }                                                                                                                 \
            b[BUF][0] = bp[4 * (PR) * kBigT]; b[BUF][1] = bp[(4 * (PR) + 2) * kBigT];                                         \
        }
        GNNAGG_RD(0, 0)
#pragma unroll
        for (int pr = 0; pr < kBigKC / 4; ++pr) {
            if (pr + 1 < kBigKC / 4) GNNAGG_RD((pr + 1) & 1, pr + 1)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < RBK; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[pr & 1][i][kk], b[pr & 1][kk], acc[i], 0, 0, 0);
            if (pr + 1 < kBigKC / 4) __builtin_amdgcn_sched_group_barrier(0x100, RBK + 1, 0);   // DS reads of the next pair first ...
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * RBK, 0);                              // ... then this pair's MFMAs
        }
#undef GNNAGG_RD
    };
    const int colc = (32 * wave + (lane & 31)) * (int)sizeof(float);
    int c = 0, row0 = blk0 * 32, left = nblk;   // the chunk being multiplied
    // prologue: chunks 0 and 1 requested, chunk 0 landed and written, chunk 2 requested
    GNNAGG_AHEAD_FETCH(0)
    GNNAGG_AHEAD_FETCH(1)
    GNNAGG_AHEAD_WAIT;
    GNNAGG_AHEAD_STASH(0, 0)
    if constexpr (AV == 2) sc = nchunks > 1 ? 1 : 0;
    GNNAGG_AHEAD_FETCH(0)
    __syncthreads();
    for (int g0 = 0; g0 < total; g0 += 2) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {   // unrolled: the register set and the LDS image of a chunk (h & 1) are compile-time constants
            const int g = g0 + half;
            if (g >= total) break;
            // ---- multiply chunk g (image g & 1)
            const float *As = half ? As1 : As0, *Bs = half ? Bs1 : Bs0;
            const int rbk = left < 4 ? left : 4;
            const bool last_c = c + 1 == nchunks;
            if (rbk == 4) mma(std::integral_constant<int, 4>{}, As, Bs);
            else if (rbk == 3) mma(std::integral_constant<int, 3>{}, As, Bs);
            else if (rbk == 2) mma(std::integral_constant<int, 2>{}, As, Bs);
            else mma(std::integral_constant<int, 1>{}, As, Bs);
            const int srow0 = row0, srbk = rbk;   // (the tile whose last chunk this is: its C stores go out BEHIND the request below)
            if (last_c) { c = 0; row0 += kBigT; left -= 4; } else ++c;
            // ---- chunk g + 1 (requested two periods ago; everything but the newest chunk's loads has landed) goes to the other image, and the
            //      set it frees takes the request of chunk g + 3 (past the end: the last chunk once more -- the count stays the same)
            GNNAGG_AHEAD_WAIT;
            if (half == 0) {
                if (g + 1 < total) { GNNAGG_AHEAD_STASH(1, sc * kBigKC) if constexpr (AV == 2) sc = sc + 1 == nchunks ? 0 : sc + 1; }
                GNNAGG_AHEAD_FETCH(1)
            } else {
                if (g + 1 < total) { GNNAGG_AHEAD_STASH(0, sc * kBigKC) if constexpr (AV == 2) sc = sc + 1 == nchunks ? 0 : sc + 1; }
                GNNAGG_AHEAD_FETCH(0)
            }
            if (last_c) {
                // The tile's C stores, behind the wait and the request: in front of the wait they were its 64 newest operations, and
                // "all but the 8 newest" then meant the stores just issued AND the chunk requested a period ago.  Here the next wait finds
                // them a whole period old.  (Still safe: at most 8 outstanding operations cannot be the 8 needed loads unless the 8
                // younger loads are outstanding too -- loads return in order.  AV = 2: 12 for 8.)
                // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); descriptor rebased to C[srow0][col0]
                const size_t co = ((size_t)srow0 * N + col0) * sizeof(float), c_bytes = (size_t)M * N * sizeof(float);
                const size_t cr = co < c_bytes ? c_bytes - co : 0;
                const __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(C + ((size_t)srow0 * N + col0), 0,
                                                                                        (int)(unsigned)(cr < 0xfffffffcULL ? cr : 0xfffffffcULL), 0x00020000);
                const int voff = 4 * (lane >> 5) * N * (int)sizeof(float) + colc;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < srbk) {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg)
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[i][reg]), crsrc, voff,
                                                                  (32 * i + (reg & 3) + 8 * (reg >> 2)) * N * (int)sizeof(float), 0);
                    }
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) acc[i][reg] = 0.0f;
                }
            }
            __syncthreads();
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
#undef GNNAGG_AHEAD_FETCH
#undef GNNAGG_AHEAD_STASH
#undef GNNAGG_AHEAD_LOAD
#undef GNNAGG_AHEAD_STASH_A
#undef GNNAGG_AHEAD_STASH_B
#undef GNNAGG_AHEAD_LOAD_A
#undef GNNAGG_AHEAD_WAIT
#undef GNNAGG_AHEAD_MASK

// Tall-skinny variant for the aggregation widths (K <= 128, K % 4 == 0): every wavefront keeps its B operands -- the
// whole W[K, 32] column block, 64 VGPRs -- in registers for the life of the kernel and walks 32-row tiles of A on its own:
// 16 coalesced 16-byte loads per lane fetch the NEXT tile while the current one is multiplied; the tile passes through a
// per-wavefront LDS image (pitch K + 4: aligned ds_write_b128, operand reads two per bank) only to turn rows-over-lanes
// into the MFMA operand layout; no workgroup barrier anywhere.  Four 16x16 sub-tiles per tile, each the full ascending-k
// chain on v_mfma_f32_16x16x4_f32 (bit-exact as k_dense_nn).
static constexpr int kTallWaves = 2;  // wavefronts per workgroup (one 16.9 KB LDS image each at K = 128)

__global__ __launch_bounds__(64 * kTallWaves) void k_dense_nn_tall(const float *__restrict__ A, const float *__restrict__ B,
                                                                   float *__restrict__ C, int M, int N, int K, int ntiles)
{
    extern __shared__ float lds[];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int pitch = K + 4, q4 = K >> 2;  // K % 4 == 0
    float *tile = lds + wave * 32 * pitch;
    const int col0 = blockIdx.y * 32;
    const int kq = lane >> 4, cl = lane & 15;
    // B operands: lane (c = lane % 16, k = lane / 16) of MFMA t holds W[4t + k][col]; two column halves
    float b0[32], b1[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const int k = 4 * t + kq;
        b0[t] = (k < K && col0 + cl < N) ? B[(size_t)k * N + col0 + cl] : 0.0f;
        b1[t] = (k < K && col0 + 16 + cl < N) ? B[(size_t)k * N + col0 + 16 + cl] : 0.0f;
    }
    const int wstride = gridDim.x * kTallWaves;
    int t_idx = blockIdx.x * kTallWaves + wave;
    float4 pre[16];
    // float4 number e = lane + 64 i of a tile is (row e / q4, quad e % q4); stepping e by 64 advances (row, quad) by
    // (64 / q4, 64 % q4) with one carry -- no division in the loops
    const int step_r = 64 / q4, step_c = 64 - step_r * q4;
    const int r0 = lane / q4, c0 = lane - r0 * q4;
    auto fetch = [&](int ti) {
        int r = r0, c4 = c0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = ti * 32 + r;
            pre[i] = (r < 32 && row < M) ? *reinterpret_cast<const float4 *>(A + (size_t)row * K + 4 * c4)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
            r += step_r; c4 += step_c;
            if (c4 >= q4) { c4 -= q4; ++r; }
        }
    };
    if (t_idx < ntiles) fetch(t_idx);
    for (; t_idx < ntiles; t_idx += wstride) {
        {
            int r = r0, c4 = c0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (r < 32) *reinterpret_cast<float4 *>(&tile[r * pitch + 4 * c4]) = pre[i];
                r += step_r; c4 += step_c;
                if (c4 >= q4) { c4 -= q4; ++r; }
            }
        }
        if (t_idx + wstride < ntiles) fetch(t_idx + wstride);  // travels during the MFMA chains below
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int rh = 0; rh < 2; ++rh) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            const float *arow = tile + (rh * 16 + cl) * pitch + kq;
            float av[32];
#pragma unroll
            for (int t = 0; t < 32; ++t) av[t] = 4 * t < K ? arow[4 * t] : 0.0f;
#pragma unroll
            for (int t = 0; t < 32; ++t) {
                if (4 * t < K) {  // wave-uniform
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], b0[t], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], b1[t], acc1, 0, 0, 0);
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {  // D layout: col = lane % 16, row = 4 * (lane / 16) + reg
                const int row = t_idx * 32 + rh * 16 + 4 * kq + v;
                if (row < M) {
                    if (col0 + cl < N) C[(size_t)row * N + col0 + cl] = acc0[v];
                    if (col0 + 16 + cl < N) C[(size_t)row * N + col0 + 16 + cl] = acc1[v];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();  // the image is rewritten next iteration
    }
}

int launch_dense_nn(const float *A, const float *B, float *C, int M, int N, int K, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    if (M <= 0 || N <= 0) return GNNAGG_OK;
    {
        // measured against k_dense_nn (N = 32): K = 128: M = 300 k 48.2 vs 46.4 us, 600 k 92.4 vs 99.9, 1.2 M 169 vs 184,
        // 2.45 M 307 vs 352; K = 100, M = 2.45 M: 268 vs 363 (torch.mm 427); K = 64 loses at every M -> large M, wide K only
        if (K > 64 && K <= 128 && (K & 3) == 0 && M >= 500000 && ((uintptr_t)A & 15) == 0) {
            const int ntiles = ceil_div(M, 32);
            const size_t lds = (size_t)kTallWaves * 32 * (K + 4) * sizeof(float);
            const int wgs = std::min(ceil_div(ntiles, kTallWaves), 256 * 4);
            hipLaunchKernelGGL(k_dense_nn_tall, dim3(wgs, ceil_div(N, 32)), dim3(64 * kTallWaves), lds, stream, A, B, C, M, N, K,
                               ntiles);
            HIP_TRY(hipGetLastError());
            return GNNAGG_OK;
        }
    }
    if (K <= 0) {
        return launch_zero_words(C, (size_t)M * N, stream);
    }
    {
        if (N > 64 && M >= 1024 && (size_t)kBigT * N * sizeof(float) < 0x7fffffffULL) {   // wide outputs: persistent strips of 128 x 128 tiles, A read once
            const size_t lds = (size_t)(2 * kBigT * kBigPA + 2 * kBigKC * kBigT) * sizeof(float);
            const bool bvec = (N & 3) == 0 && N >= 4 && ((uintptr_t)B & 15) == 0;
            const int av = !bvec ? 1 : ((K & 3) == 0 && K >= 4 && ((uintptr_t)A & 15) == 0) ? 4 : ((K & 1) == 0 && K >= 2 && ((uintptr_t)A & 7) == 0) ? 2 : 1;
            // the grid is what the chip holds at a time: kBigWgs workgroups per CU, shared by the column tiles
            const int ncol = ceil_div(N, kBigT), slots = std::max(1, kBigWgs * device_cu_count() / ncol);
            const int nb32 = ceil_div(M, 32), nstrips = std::min(slots, ceil_div(nb32, 2));
            const dim3 sgrid(nstrips, ncol);
#define WIDE_CALL(KERNEL_)                                                                                                              \
            {                                                                                                                           \
                static OncePerDevice attr_ok;                                                                                           \
                if (attr_ok.first()) {                                                                                                  \
                    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&KERNEL_), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                    attr_ok.done();                                                                                                     \
                }                                                                                                                       \
                hipLaunchKernelGGL(KERNEL_, sgrid, dim3(256), lds, stream, A, B, C, M, N, K, nb32, nstrips);                            \
            }
            // lean form: whole 128-column tiles, 16-byte aligned B rows, A rows 16- or 8-byte aligned, row pitches inside 32-bit offsets
            const bool lean = (N % kBigT) == 0 && bvec && av >= 2 && (size_t)kBigT * K * sizeof(float) < 0x7fffffffULL &&
                              (size_t)kBigKC * N * sizeof(float) < 0x7fffffffULL;
            if (lean && av == 4 && (K % kBigKC) == 0) WIDE_CALL(k_dense_nn_ahead<4>)
            else if (lean && av == 2) WIDE_CALL(k_dense_nn_ahead<2>)
            else if (lean && av == 4) WIDE_CALL(k_dense_nn_lean<4>)
            else if (lean) WIDE_CALL(k_dense_nn_lean<2>)
            else if (av == 4) WIDE_CALL(k_dense_nn_strip<4>)
            else if (av == 2) WIDE_CALL(k_dense_nn_strip<2>)
            else WIDE_CALL(k_dense_nn_strip<1>)
#undef WIDE_CALL
            HIP_TRY(hipGetLastError());
            return GNNAGG_OK;
        }
    }
    const dim3 grid(ceil_div(M, kGemmRows), ceil_div(N, kGemmCols));
    if (K % kGemmKC == 0 && K <= 4 * kGemmKC && ((uintptr_t)A & 15) == 0 && (size_t)kGemmRows * K * sizeof(float) < 0x7fffffffULL) {
        // every chunk of a tile requested up front (k_dense_nn_up); 33 .. 64 columns: both 32-column blocks in one workgroup
        const bool two = N > kGemmCols && N <= 2 * kGemmCols;
        const dim3 g(ceil_div(M, kGemmRows), two ? 1 : ceil_div(N, kGemmCols));
#define UP_CALL(NCH_) \
        { if (two) hipLaunchKernelGGL((k_dense_nn_up<NCH_, 2>), g, dim3(256), 0, stream, A, B, C, M, N); \
          else hipLaunchKernelGGL((k_dense_nn_up<NCH_, 1>), g, dim3(256), 0, stream, A, B, C, M, N); }
        switch (K / kGemmKC) {
            case 1: UP_CALL(1) break;
            case 2: UP_CALL(2) break;
            case 3: UP_CALL(3) break;
            default: UP_CALL(4) break;
        }
#undef UP_CALL
        HIP_TRY(hipGetLastError());
        return GNNAGG_OK;
    }
    hipLaunchKernelGGL(k_dense_nn, grid, dim3(256), 0, stream, A, B, C, M, N, K);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

}  // namespace gnnagg
