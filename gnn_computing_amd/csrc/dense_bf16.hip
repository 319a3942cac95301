// dense_bf16.hip -- the dense combine with 16-bit operands (gnnagg_matmul_nn_typed): C[M,N] = A[M,K] . B[K,N], A and B row-major bf16,
// C row-major fp32 or bf16, fp32 accumulation on v_mfma_f32_32x32x16_bf16.  The fp32 GEMM (dense_f32.hip) is a separate set of kernels.
//
// Regime: tall and skinny (M = |V|, K = 32 .. 602, N = 2 .. 128) -- the job is to stream A from HBM once; B is small.
//  * One wavefront owns 32 rows x (32 * NT) columns at a time: NT accumulator tiles of 32 x 32 (NT = 4: N up to 128 in one pass over A).
//  * A never passes through LDS.  The A operand of the MFMA wants 8 consecutive k of one row per lane (lane l: row l & 31, lane half
//    h = l >> 5), which in row-major A is one 16-byte load.  The sum runs over k, so k may be dealt to (step, lane half, element) in any
//    order as long as A and B agree: a "superstep" covers 64 k with FOUR MFMA steps, and lane half h takes k = 64 * ss + 32 * h + 8 * s + j
//    for step s, element j -- every lane reads 64 contiguous bytes of its row per superstep (the hardware's own order, 16 * s + 8 * h + j,
//    would interleave the halves at 16 bytes).
//  * B is transposed once per workgroup into LDS, bt[column][k] with k contiguous, so the B fragment of (step, half) is one 16-byte LDS
//    read at bt[column][64 * ss + 32 * h + 8 * s].  The image holds K rounded up to 8 plus ONE octet of zeros per column; the octets of
//    the last superstep that lie beyond it are all read from that one (A is zero there too).  So K = 602 fits the 160 KB of LDS at 128
//    columns (128 x 616 x 2 bytes) and A is read once.  The row pitch is an odd number of 16-byte units: the 16-byte reads of consecutive
//    columns walk the banks.  Padding (k >= K, column >= N) is written as zeros, and A octets beyond K or a wavefront's rows are zeros built
//    in registers -- nothing behind an operand is ever read.
//  * Workgroups are persistent and every wavefront streams ONE contiguous range of rows, ceil(M / wavefronts) of them, tile
//    after tile -- a share of the BYTES that is the same for every wavefront whatever M is (whole 32-row tiles dealt round-robin leave a
//    part of the chip a whole tile short: 5292 tiles on 2048 wavefronts is 3 against 2).  The last tile of a range is partial: its other
//    rows are the next wavefront's and are neither read nor stored here.
//  * A loads run kBfDepth supersteps ahead of the MFMAs through a register ring, across tile boundaries.  Every request is
//    unconditional and branch-free, and B is staged outside the loop, because a load the compiler cannot count turns its counted waits
//    (s_waitcnt vmcnt(12 .. 15)) into waits for everything outstanding.
//  * K wider than the image holds first narrows the column block (NT = 2, 1: A is read once per column block, the blocks of a row range
//    on one XCD at about the same time); beyond that (NT = 1, K > 2544) the image is restaged per chunk of 2048 k for every tile (MULTI):
//    correct, outside the regime, not tuned.
//  * Alignment classes of A: 16-byte rows (one aligned 16-byte load per octet), 4-byte rows (K even: the same load, dword-aligned, which
//    the hardware takes; the row's last partial octet is read shifted back and its dwords are moved into place), 2-byte rows (element
//    loads).  Every class runs this kernel.  B is read in 16-byte pieces where N % 8 == 0 and its address allow, else in elements.  C is
//    stored element by element: 32 consecutive columns of a row per half wavefront.
//  * bf16 C: the same accumulators, one round-to-nearest-even conversion (v_cvt_pk_bf16_f32: NaN kept, overflow to inf) at the store.
#include "kernel_util.cuh"

namespace gnnagg {
namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
struct __attribute__((aligned(4))) Dwords4 { unsigned x, y, z, w; };   // 16 bytes at a dword-aligned address

constexpr int kBfWaves = 8;                  // wavefronts per workgroup
constexpr int kBfThreads = 64 * kBfWaves;
constexpr int kBfStepK = 64;                 // k per superstep: 4 MFMA steps of 16
constexpr int kBfDepth = 4;                  // supersteps of A in flight per wavefront (16 registers each)
constexpr int kBfLdsBytes = 160 * 1024;      // LDS of a CU: the largest image
constexpr int kBfChunk = 2048;               // k per image where K needs several (MULTI)

// 8 consecutive k of one A row as the four dwords of an MFMA operand, in two halves.  AV = the row's alignment class in elements: 8
// (K % 8 == 0), 2 (K even, K >= 8) or 1.
//  * load_a_octet issues the loads, branch-free: an octet that ends beyond K is read from the row's LAST octet instead (AV = 1: element
//    by element from the last element), and the caller points rows it does not own at one it does, so nothing behind A is read.  (With
//    loads under branches the compiler waits for ALL outstanding loads at every superstep and the register ring holds nothing in flight.)
//  * fix_a_tail puts the dwords of such an octet where they belong and zeros the rest, where the MFMAs consume it -- a select at the
//    load would wait for it on the spot.
template <int AV>
__device__ __forceinline__ uint4 load_a_octet(const __bf16 *__restrict__ row, int k, int K)
{
    if constexpr (AV == 8) {
        return *reinterpret_cast<const uint4 *>(row + min(k, K - 8));
    } else if constexpr (AV == 2) {
        const Dwords4 t = *reinterpret_cast<const Dwords4 *>(row + min(k, K - 8));
        return make_uint4(t.x, t.y, t.z, t.w);
    } else {   // (the halves of a dword are packed here; their zeros are still dealt at the MFMAs)
        const unsigned short *p = reinterpret_cast<const unsigned short *>(row);
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (unsigned)p[min(k + 2 * j, K - 1)] | ((unsigned)p[min(k + 2 * j + 1, K - 1)] << 16);
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
}
template <int AV>
__device__ __forceinline__ uint4 fix_a_tail(uint4 v, int k, int K, bool ok)
{
    unsigned w[4] = {v.x, v.y, v.z, v.w};
    if constexpr (AV == 2) {   // the octet was read at K - 8 instead of k: its dword j is dword j + sh of what was read (K, k even)
        const int sh = max(k - (K - 8), 0) >> 1;
        const unsigned u[7] = {v.x, v.y, v.z, v.w, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = sh == 0 ? u[j] : sh == 1 ? u[j + 1] : sh == 2 ? u[j + 2] : u[j + 3];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (AV == 1) {
            const unsigned keep = (ok && k + 2 * j < K ? 0xffffu : 0u) | (ok && k + 2 * j + 1 < K ? 0xffff0000u : 0u);
            w[j] &= keep;
        } else {   // K is even: a dword lies inside or outside the row
            w[j] = (ok && k + 2 * j < K) ? w[j] : 0u;
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// grid: gx persistent workgroups per column block, column block = blockIdx.x / gx (x-fastest: the column blocks of a row range start
// together).  rpw = rows per wavefront; kimg = k of an LDS image (!MULTI: K rounded up to 8; MULTI: kBfChunk), pitch = its row pitch.
template <int NT, int AV, bool MULTI>
__global__ __launch_bounds__(kBfThreads) void k_dense_nn_bf16(const __bf16 *__restrict__ A, const __bf16 *__restrict__ B,
                                                                               void *__restrict__ C, int c_bf16, int M, int N, int K, int kimg,
                                                                               int pitch, int rpw, int gx, int b_vec)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bf16_lds[];
    __bf16 *bt = reinterpret_cast<__bf16 *>(bf16_lds);
    constexpr int NB = 32 * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int bx = blockIdx.x % gx, col0 = (blockIdx.x / gx) * NB;
    const int nss = (K + kBfStepK - 1) / kBfStepK, spc = MULTI ? kimg / kBfStepK : nss;
    const int zoct = kimg / 8;                        // !MULTI: the octet of zeros behind the image
    const int niter = (rpw + 31) / 32;                // tiles of a wavefront: the same for all, so the barriers of MULTI are uniform
    // supersteps of a wavefront, rounded up to the ring: the phantom ones lie beyond its rows (zero operands, nothing stored)
    const long total = ((long)niter * nss + kBfDepth - 1) / kBfDepth * kBfDepth;
    const long wrow0 = ((long)bx * kBfWaves + wave) * rpw, wrow1 = min(wrow0 + rpw, (long)M);   // this wavefront's rows
    const long wlast = max(min(wrow1, (long)M) - 1, 0L);                                         // a row inside A for every request

    auto fetch = [&](uint4(&buf)[4], int it, int ss) {
        const long row = min(wrow0 + 32L * it + r, wlast);
        const __bf16 *p = A + (size_t)row * K;
        const int kb = ss * kBfStepK + 32 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) buf[s] = load_a_octet<AV>(p, kb + 8 * s, K);
    };
    // bt[c][0 .. n_oct * 8) = B[k0 ..)[col0 + c], zeros beyond K and N.  One thread per 8 k x 8 columns: eight 16-byte row pieces
    // (b_vec: N % 8 == 0 and B 16-byte aligned, so a piece lies inside or outside a row) or 64 elements, transposed in registers and
    // written as one 16-byte LDS store per column.
    auto stage = [&](int chunk) {
        const unsigned short *Bu = reinterpret_cast<const unsigned short *>(B);
        const int k0 = chunk * kimg, n_item = (MULTI ? zoct : zoct + 1) * (NB / 8);
        for (int i = threadIdx.x; i < n_item; i += kBfThreads) {
            const int co = i % (NB / 8), ko = i / (NB / 8), k = k0 + 8 * ko, col = col0 + 8 * co;
            unsigned q[8][4];   // q[j]: row k + j, columns col .. col + 7
            if (b_vec) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    uint4 t = make_uint4(0u, 0u, 0u, 0u);
                    if (k + j < K && col < N) t = *reinterpret_cast<const uint4 *>(Bu + (size_t)(k + j) * N + col);
                    q[j][0] = t.x; q[j][1] = t.y; q[j][2] = t.z; q[j][3] = t.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const unsigned lo = (k + j < K && col + 2 * m < N) ? (unsigned)Bu[(size_t)(k + j) * N + col + 2 * m] : 0u;
                        const unsigned hi = (k + j < K && col + 2 * m + 1 < N) ? (unsigned)Bu[(size_t)(k + j) * N + col + 2 * m + 1] : 0u;
                        q[j][m] = lo | (hi << 16);
                    }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {   // column col + c: element c of every row, k pairs packed
                unsigned w[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const unsigned a = q[2 * m][c >> 1], b = q[2 * m + 1][c >> 1];
                    w[m] = (c & 1) ? ((a >> 16) | (b & 0xffff0000u)) : ((a & 0xffffu) | (b << 16));
                }
                *reinterpret_cast<uint4 *>(bt + (size_t)(8 * co + c) * pitch + 8 * ko) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };

    f32x16_t acc[NT];
    uint4 ring[kBfDepth][4];
    int f_it = 0, f_ss = 0;   // the next superstep to request
#pragma unroll
    for (int d = 0; d < kBfDepth; ++d) {
        fetch(ring[d], f_it, f_ss);
        if (++f_ss == nss) { f_ss = 0; ++f_it; }
    }
    int c_it = 0, c_ss = 0, c_in = 0;   // the superstep the MFMAs are at; c_in = its index inside the LDS image
    if constexpr (!MULTI) {   // all of K in one image: staged once, behind the first requests for A
        stage(0);
        __syncthreads();
    }
    // One flat sequence of supersteps, tile after tile, so that every ring slot is a real request.  c_it, c_ss, c_in are
    // workgroup-uniform, like everything that decides a branch around a barrier below.
    for (long w = 0; w < total; w += kBfDepth) {
#pragma unroll
        for (int d = 0; d < kBfDepth; ++d) {
            if constexpr (MULTI) {
                if (c_in == 0) {
                    __syncthreads();   // (the other wavefronts may still read the previous image)
                    stage(c_ss / spc);
                    __syncthreads();
                }
            }
            if (c_ss == 0) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[t][v] = 0.0f;
            }
            const long row0 = wrow0 + 32L * c_it;
            const __bf16 *bl = bt + (size_t)r * pitch;
            const bool a_ok = row0 + r < wrow1;
            const int a_k = c_ss * kBfStepK + 32 * h, b_oct = c_in * (kBfStepK / 8) + 4 * h;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bf16x8_t a = __builtin_bit_cast(bf16x8_t, fix_a_tail<AV>(ring[d][s], a_k + 8 * s, K, a_ok));
                const int oct = MULTI ? b_oct + s : min(b_oct + s, zoct);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const bf16x8_t b = *reinterpret_cast<const bf16x8_t *>(bl + (size_t)t * 32 * pitch + 8 * oct);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);
                }
            }
            if (c_ss == nss - 1) {   // D layout: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
                const bool whole = row0 + 32 <= wrow1 && col0 + NB <= N;   // wave-uniform: the tile needs no guards
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int col = col0 + 32 * t + r;
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const long row = row0 + (v & 3) + 8 * (v >> 2) + 4 * h;
                        if (whole || (row < wrow1 && col < N)) {
                            const size_t o = (size_t)row * N + col;
                            if (c_bf16) static_cast<__bf16 *>(C)[o] = (__bf16)acc[t][v];
                            else static_cast<float *>(C)[o] = acc[t][v];
                        }
                    }
                }
            }
            if (++c_in == spc) c_in = 0;
            if (++c_ss == nss) { c_ss = 0; c_in = 0; ++c_it; }
            // slot d is free: the superstep one ring ahead.  Behind the stores: the counter the waits count is shared with them and in
            // order, so loads requested before a tile's (branch-guarded) stores would be waited for together with everything else.
            fetch(ring[d], f_it, f_ss);
            if (++f_ss == nss) { f_ss = 0; ++f_it; }
        }
    }
}

// K == 0 with a bf16 C: +0 in every element (2-byte aligned ranges; the fp32 C goes through launch_zero_words)
__global__ __launch_bounds__(256) void k_zero_bf16(unsigned short *__restrict__ p, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// row pitch of an image of kext elements (kext % 8 == 0): at least one octet more, and an odd number of 16-byte units
static long image_pitch(long kext) { return kext + 8 + ((kext / 8) % 2 ? 8 : 0); }

template <int NT, int AV, bool MULTI>
int call_dense_nn_bf16(const __bf16 *A, const __bf16 *B, void *C, int c_bf16, int M, int N, int K, int kimg, int pitch, int rpw, int gx, int ncolb,
                       size_t lds, int b_vec, hipStream_t stream)
{
    static OncePerDevice attr_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (attr_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dense_nn_bf16<NT, AV, MULTI>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kBfLdsBytes));
        attr_ok.done();
    }
    hipLaunchKernelGGL((k_dense_nn_bf16<NT, AV, MULTI>), dim3((unsigned)gx * ncolb), dim3(kBfThreads), lds, stream, A, B, C, c_bf16, M, N, K, kimg,
                       pitch, rpw, gx, b_vec);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

}  // namespace

int launch_dense_nn_bf16(const void *A_v, const void *B_v, void *C, int c_bf16, int M, int N, int K, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    if (M <= 0 || N <= 0) return GNNAGG_OK;
    if (K <= 0) {
        if (!c_bf16) return launch_zero_words(C, (size_t)M * N, stream);
        const long n = (long)M * N;
        hipLaunchKernelGGL(k_zero_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, static_cast<unsigned short *>(C), n);
        HIP_TRY(hipGetLastError());
        return GNNAGG_OK;
    }
    const __bf16 *A = static_cast<const __bf16 *>(A_v), *B = static_cast<const __bf16 *>(B_v);
    const long k8 = ((long)K + 7) / 8 * 8;
    // the widest column block whose LDS image holds all of K (A is read once per column block); none at NT = 1: K in chunks
    int nt = N > 64 ? 4 : N > 32 ? 2 : 1;
    while (nt > 1 && 32 * nt * image_pitch(k8) * (long)sizeof(__bf16) > kBfLdsBytes) nt >>= 1;
    const bool multi = 32 * nt * image_pitch(k8) * (long)sizeof(__bf16) > kBfLdsBytes;   // (only at nt = 1)
    const int kimg = multi ? kBfChunk : (int)k8, pitch = (int)image_pitch(kimg);
    const size_t lds = (size_t)32 * nt * pitch * sizeof(__bf16);
    const int ncolb = ceil_div(N, 32 * nt);
    // persistent: what the chip holds at a time, shared by the column blocks -- one workgroup per CU (two wavefronts per SIMD: the ring and
    // the accumulators take 150 .. 170 registers; capped at 128 for a second workgroup the narrow kernels spill); every wavefront takes
    // the same number of rows
    const int gx = std::min(ceil_div(ceil_div(M, 32), kBfWaves), std::max(1, device_cu_count() / ncolb));
    const int rpw = ceil_div(M, (long)gx * kBfWaves);
    int av = align_class(K, A, (int)sizeof(__bf16), 8);
    if (av == 4) av = 2;            // 4-byte aligned rows: dword-aligned 16-byte loads
    if (av == 2 && K < 8) av = 1;   // (an octet of the row to fall back on)
    const int b_vec = align_class(N, B, (int)sizeof(__bf16), 8) == 8;
#define BF16_CALL(NT_, AV_, MULTI_) \
    return call_dense_nn_bf16<NT_, AV_, MULTI_>(A, B, C, c_bf16, M, N, K, kimg, pitch, rpw, gx, ncolb, lds, b_vec, stream);
#define BF16_CALL_NT(NT_, MULTI_)              \
    switch (av) {                              \
        case 8: BF16_CALL(NT_, 8, MULTI_)      \
        case 2: BF16_CALL(NT_, 2, MULTI_)      \
        default: BF16_CALL(NT_, 1, MULTI_)     \
    }
    switch (nt) {
        case 4: BF16_CALL_NT(4, false)
        case 2: BF16_CALL_NT(2, false)
        default:
            if (multi) BF16_CALL_NT(1, true)
            BF16_CALL_NT(1, false)
    }
#undef BF16_CALL_NT
#undef BF16_CALL
}

}  // namespace gnnagg
