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
//  * EPI = G (gnnagg_gat_project, launch_dense_nn_bf16_att): the GAT attention terms att[row, head, 0 / 1] = sum over the head's columns of
//    C AS STORED times a_dst / a_src, taken from the accumulators behind a tile's C stores.  One column block holds all of N; a_dst /
//    a_src lie in LDS behind the image as fp32 (zeros in padded columns), not in registers across the loop.  A lane holds column 32 t + r
//    of 16 rows: it adds the products of the tiles of one head (tph tiles where a head is wider than 32 columns), then the G = min(D, 32)
//    lanes of the head add up -- a halving exchange (every step hands half of the lane's rows to its partner: v_permlane16_swap across
//    the two 16-lane rows, then DPP row_mirror / row_half_mirror / quad_perm), 31 additions for 32 lanes x 32 values, a fixed order.  An even
//    lane ends up with the finished (dst, src) pairs of 32 / G rows and stores them under the C store's row guard.  EPI = 0 is the kernel as
//    it was: the same signature (the epilogue's arguments are a parameter pack, empty there) and the same instructions.
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

// ---- the attention-term epilogue (EPI != 0)
struct AttEpi {
    const __bf16 *a_dst, *a_src;   // [heads, D] = [N]
    float *att;                    // [M, heads, 2]
    int heads, tph;                // tph: tiles per head (EPI = 32; 1 otherwise)
};
struct __attribute__((aligned(4))) AttPair { float dst, src; };   // 8 bytes at a dword-aligned address
template <class... EP>
__device__ __forceinline__ const AttEpi &att_epi_of(const AttEpi &e, const EP &...) { return e; }
template <int CTRL>
__device__ __forceinline__ float att_dpp(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
// one halving step over lane pairs (i, partner(i)) that differ in the lane bit `up` tests: the lane keeps the upper (up) or lower N / 2
// of its N (dst, src) pairs and adds the partner's partial sums of the same ones
typedef float f32x2_t __attribute__((ext_vector_type(2)));
template <int N, int CTRL>
__device__ __forceinline__ void att_halve(f32x2_t (&u)[16], bool up)
{
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const f32x2_t keep = up ? u[j + N / 2] : u[j], send = up ? u[j] : u[j + N / 2];
        u[j].x = keep.x + att_dpp<CTRL>(send.x);
        u[j].y = keep.y + att_dpp<CTRL>(send.y);
    }
}
// u[v]: this lane's partial (dst, src) sums for row row0 + (v & 3) + 8 * (v >> 2) + 4 * h.  The G lanes of a head (aligned to G) add up; the
// even lane r then holds rows v = ((r >> 1) & (G / 2 - 1)) * (32 / G) + j, j < 32 / G, and stores them.
template <int G>
__device__ __forceinline__ void att_reduce_store(f32x2_t (&u)[16], int r, int h, long row0, long wrow1, int head, int heads, float *__restrict__ att)
{
    if constexpr (G == 32) {   // rows 8 .. 15 of the values to lanes 16 .. 31: odd 16-lane rows of lo <-> even ones of hi
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const auto d = __builtin_amdgcn_permlane16_swap(__float_as_uint(u[j].x), __float_as_uint(u[j + 8].x), false, false);
            const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(u[j].y), __float_as_uint(u[j + 8].y), false, false);
            u[j].x = __uint_as_float(d[0]) + __uint_as_float(d[1]);
            u[j].y = __uint_as_float(s[0]) + __uint_as_float(s[1]);
        }
    }
    constexpr int N0 = G == 32 ? 8 : 16;
    if constexpr (G >= 16) att_halve<N0, 0x140>(u, (r & 8) != 0);   // row_mirror: partner 15 - i
    constexpr int N1 = G >= 16 ? N0 / 2 : N0;
    att_halve<N1, 0x141>(u, (r & 4) != 0);      // row_half_mirror: partner i ^ 7
    att_halve<N1 / 2, 0x1b>(u, (r & 2) != 0);   // quad_perm [3, 2, 1, 0]: partner i ^ 3
    constexpr int NV = 32 / G;
#pragma unroll
    for (int j = 0; j < NV; ++j) {   // quad_perm [1, 0, 3, 2]: both lanes of a pair get the total
        u[j].x += att_dpp<0xb1>(u[j].x);
        u[j].y += att_dpp<0xb1>(u[j].y);
    }
    if ((r & 1) == 0 && head < heads) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = ((r >> 1) & (G / 2 - 1)) * NV + j;
            const long row = row0 + (v & 3) + 8 * (v >> 2) + 4 * h;
            if (row < wrow1) *reinterpret_cast<AttPair *>(att + ((size_t)row * heads + head) * 2) = AttPair{u[j].x, u[j].y};
        }
    }
}

// grid: gx persistent workgroups per column block, column block = blockIdx.x / gx (x-fastest: the column blocks of a row range start
// together).  rpw = rows per wavefront; kimg = k of an LDS image (!MULTI: K rounded up to 8; MULTI: kBfChunk), pitch = its row pitch.
// EPI = 8, 16, 32: the lanes that hold one head's columns of a tile; ep is one AttEpi (the grid is one column block: col0 = 0).
template <int NT, int AV, bool MULTI, int EPI = 0, class... EP>
__global__ __launch_bounds__(kBfThreads) void k_dense_nn_bf16(const __bf16 *__restrict__ A, const __bf16 *__restrict__ B,
                                                                               void *__restrict__ C, int c_bf16, int M, int N, int K, int kimg,
                                                                               int pitch, int rpw, int gx, int b_vec, EP... ep)
{
    static_assert(EPI == 0 ? sizeof...(EP) == 0 : (sizeof...(EP) == 1 && !MULTI), "the epilogue takes one AttEpi and a single image");
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
        if constexpr (EPI != 0) {   // behind the image: a_dst[0 .. NB), a_src[0 .. NB) as fp32, zeros beyond N
            const AttEpi &e = att_epi_of(ep...);
            float *al = reinterpret_cast<float *>(bf16_lds + (size_t)NB * pitch * sizeof(__bf16));
            for (int i = threadIdx.x; i < 2 * NB; i += kBfThreads) {
                const int c = i < NB ? i : i - NB;
                al[i] = c < N ? (float)(i < NB ? e.a_dst : e.a_src)[c] : 0.0f;
            }
        }
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
                if constexpr (EPI != 0) {   // the attention terms of the tile's rows, from C as stored; stores, so ahead of the request below
                    const AttEpi &e = att_epi_of(ep...);
                    const float *al = reinterpret_cast<const float *>(bf16_lds + (size_t)NB * pitch * sizeof(__bf16));
                    f32x2_t u[16] = {};
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        // (wave-uniform, like every branch here) nothing to do for a phantom tile beyond the wavefront's rows, nor for a
                        // tile of padded columns, which holds no head
                        if (row0 >= wrow1 || 32 * t >= N) continue;
                        const f32x2_t a2 = {al[32 * t + r], al[NB + 32 * t + r]};
                        // one head over several tiles (EPI = 32): its padded columns share the sum, and a NaN row has left NaN there
                        const bool pad = EPI == 32 && 32 * t + r >= N;
                        if (EPI < 32 || t % e.tph == 0) {
#pragma unroll
                            for (int v = 0; v < 16; ++v) {
                                const float c = c_bf16 ? (float)(__bf16)acc[t][v] : acc[t][v];
                                u[v] = a2 * (pad ? 0.0f : c);
                            }
                        } else {
#pragma unroll
                            for (int v = 0; v < 16; ++v) {
                                const float c = c_bf16 ? (float)(__bf16)acc[t][v] : acc[t][v];
                                u[v] += a2 * (pad ? 0.0f : c);
                            }
                        }
                        if (EPI < 32 || (t + 1) % e.tph == 0 || 32 * (t + 1) >= N)   // the head's last tile
                            att_reduce_store<EPI>(u, r, h, row0, wrow1, EPI == 32 ? t / e.tph : (32 * t + r) / EPI, e.heads, e.att);
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

template <int NT, int AV, bool MULTI, int EPI = 0, class... EP>
int call_dense_nn_bf16(const __bf16 *A, const __bf16 *B, void *C, int c_bf16, int M, int N, int K, int kimg, int pitch, int rpw, int gx, int ncolb,
                       size_t lds, int b_vec, hipStream_t stream, EP... ep)
{
    static OncePerDevice attr_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (attr_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dense_nn_bf16<NT, AV, MULTI, EPI, EP...>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kBfLdsBytes));
        attr_ok.done();
    }
    hipLaunchKernelGGL((k_dense_nn_bf16<NT, AV, MULTI, EPI, EP...>), dim3((unsigned)gx * ncolb), dim3(kBfThreads), lds, stream, A, B, C, c_bf16, M, N,
                       K, kimg, pitch, rpw, gx, b_vec, ep...);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// the launch geometry of (M, N, K): one rule for the plain product and the one with the attention epilogue, so both write the same C
struct BfGeometry {
    int nt, multi, kimg, pitch, ncolb, gx, rpw;
    size_t lds;
};
BfGeometry bf16_geometry(int M, int N, int K)
{
    BfGeometry g;
    const long k8 = ((long)K + 7) / 8 * 8;
    // the widest column block whose LDS image holds all of K (A is read once per column block); none at NT = 1: K in chunks
    g.nt = N > 64 ? 4 : N > 32 ? 2 : 1;
    while (g.nt > 1 && 32 * g.nt * image_pitch(k8) * (long)sizeof(__bf16) > kBfLdsBytes) g.nt >>= 1;
    g.multi = 32 * g.nt * image_pitch(k8) * (long)sizeof(__bf16) > kBfLdsBytes;   // (only at nt = 1)
    g.kimg = g.multi ? kBfChunk : (int)k8;
    g.pitch = (int)image_pitch(g.kimg);
    g.lds = (size_t)32 * g.nt * g.pitch * sizeof(__bf16);
    g.ncolb = ceil_div(N, 32 * g.nt);
    // persistent: what the chip holds at a time, shared by the column blocks -- one workgroup per CU (two wavefronts per SIMD: the ring and
    // the accumulators take 150 .. 170 registers; capped at 128 for a second workgroup the narrow kernels spill); every wavefront takes
    // the same number of rows
    g.gx = std::min(ceil_div(ceil_div(M, 32), kBfWaves), std::max(1, device_cu_count() / g.ncolb));
    g.rpw = ceil_div(M, (long)g.gx * kBfWaves);
    return g;
}

// the lane map of the epilogue for (N, heads) in a column block of nt tiles: false where it has none
bool att_lane_map(int N, int heads, int nt, int *gsz, int *tph)
{
    if (heads == 1) { *gsz = 32; *tph = nt; return true; }
    const int d = N / heads;
    if (d != 8 && d != 16 && d != 32 && d != 64) return false;
    *gsz = std::min(d, 32);
    *tph = std::max(d / 32, 1);
    return *tph <= nt;
}

}  // namespace

// Whether launch_dense_nn_bf16_att takes the attention terms of (M, N, K, heads) in the GEMM's epilogue.  What the kernel can do: all of N
// in one column block with all of K in its image (N <= 128 and K not beyond the 128-column image: 602 at N = 128), room for a_dst / a_src
// behind the image, and a head layout the lane map reduces (one head, or D = 8, 16, 32, 64).
int dense_nn_bf16_att_fuses(int M, int N, int K, int heads)
{
    if (M <= 0 || N <= 0 || K <= 0 || heads < 1 || N % heads != 0) return 0;
    const long k8 = ((long)K + 7) / 8 * 8;
    int nt = N > 64 ? 4 : N > 32 ? 2 : 1, gsz, tph;
    if (N > 32 * nt) return 0;
    if (32 * nt * image_pitch(k8) * (long)sizeof(__bf16) + 2 * 32 * nt * (long)sizeof(float) > kBfLdsBytes) return 0;
    return att_lane_map(N, heads, nt, &gsz, &tph);
}

// epi = NULL: C = A . B.  epi != NULL (dense_nn_bf16_att_fuses holds): the same launch with the attention epilogue behind every tile.
static int dense_nn_bf16(const void *A_v, const void *B_v, void *C, int c_bf16, int M, int N, int K, const AttEpi *epi, hipStream_t stream)
{
    if (M <= 0 || N <= 0) return GNNAGG_OK;
    if (K <= 0) {
        if (!c_bf16) return launch_zero_words(C, (size_t)M * N, stream);
        const long n = (long)M * N;
        hipLaunchKernelGGL(k_zero_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, static_cast<unsigned short *>(C), n);
        HIP_TRY(hipGetLastError());
        return GNNAGG_OK;
    }
    const __bf16 *A = static_cast<const __bf16 *>(A_v), *B = static_cast<const __bf16 *>(B_v);
    const BfGeometry g = bf16_geometry(M, N, K);
    const int nt = g.nt, multi = g.multi, kimg = g.kimg, pitch = g.pitch, ncolb = g.ncolb, gx = g.gx, rpw = g.rpw;
    const size_t lds = g.lds;
    int av = align_class(K, A, (int)sizeof(__bf16), 8);
    if (av == 4) av = 2;            // 4-byte aligned rows: dword-aligned 16-byte loads
    if (av == 2 && K < 8) av = 1;   // (an octet of the row to fall back on)
    const int b_vec = align_class(N, B, (int)sizeof(__bf16), 8) == 8;
#define BF16_CALL(NT_, AV_, MULTI_) \
    return call_dense_nn_bf16<NT_, AV_, MULTI_>(A, B, C, c_bf16, M, N, K, kimg, pitch, rpw, gx, ncolb, lds, b_vec, stream);
#define BF16_CALL_ATT(NT_, AV_, G_)                                                                                                          \
    if (gsz == G_)                                                                                                                           \
        return call_dense_nn_bf16<NT_, AV_, false, G_, AttEpi>(A, B, C, c_bf16, M, N, K, kimg, pitch, rpw, gx, ncolb, lds_att, b_vec, stream, e);
#define BF16_CALL_ATT_G(NT_, AV_, MULTI_) BF16_CALL_ATT(NT_, AV_, 32) BF16_CALL_ATT(NT_, AV_, 16) BF16_CALL_ATT(NT_, AV_, 8) break;
#define BF16_CALL_NT(CALL_, NT_, MULTI_)   \
    switch (av) {                          \
        case 8: CALL_(NT_, 8, MULTI_)      \
        case 2: CALL_(NT_, 2, MULTI_)      \
        default: CALL_(NT_, 1, MULTI_)     \
    }
    if (epi) {
        AttEpi e = *epi;
        int gsz = 0;
        const size_t lds_att = lds + (size_t)2 * 32 * nt * sizeof(float);
        if (multi || ncolb != 1 || lds_att > (size_t)kBfLdsBytes || !att_lane_map(N, e.heads, nt, &gsz, &e.tph))
            return fail(GNNAGG_ERR_STATE, "internal: attention epilogue on a shape it does not cover");
        switch (nt) {
            case 4: BF16_CALL_NT(BF16_CALL_ATT_G, 4, false) break;
            case 2: BF16_CALL_NT(BF16_CALL_ATT_G, 2, false) break;
            default: BF16_CALL_NT(BF16_CALL_ATT_G, 1, false) break;
        }
        return fail(GNNAGG_ERR_STATE, "internal: attention epilogue without a lane map");
    }
    switch (nt) {
        case 4: BF16_CALL_NT(BF16_CALL, 4, false)
        case 2: BF16_CALL_NT(BF16_CALL, 2, false)
        default:
            if (multi) BF16_CALL_NT(BF16_CALL, 1, true)
            BF16_CALL_NT(BF16_CALL, 1, false)
    }
#undef BF16_CALL_NT
#undef BF16_CALL_ATT_G
#undef BF16_CALL_ATT
#undef BF16_CALL
}

int launch_dense_nn_bf16(const void *A, const void *B, void *C, int c_bf16, int M, int N, int K, void *stream)
{
    return dense_nn_bf16(A, B, C, c_bf16, M, N, K, nullptr, (hipStream_t)stream);
}

// C = A . B as launch_dense_nn_bf16 writes it, and att[M, heads, 2] from C as stored (a_dst, a_src: bf16 [heads, N / heads]) in the same kernel.
// Only where dense_nn_bf16_att_fuses(M, N, K, heads) holds.
int launch_dense_nn_bf16_att(const void *A, const void *B, void *C, int c_bf16, const void *a_dst, const void *a_src, float *att, int M, int N, int K,
                             int heads, void *stream)
{
    if (!dense_nn_bf16_att_fuses(M, N, K, heads)) return fail(GNNAGG_ERR_STATE, "internal: attention epilogue on a shape it does not cover");
    const AttEpi e = {static_cast<const __bf16 *>(a_dst), static_cast<const __bf16 *>(a_src), att, heads, 0};
    return dense_nn_bf16(A, B, C, c_bf16, M, N, K, &e, (hipStream_t)stream);
}

}  // namespace gnnagg
