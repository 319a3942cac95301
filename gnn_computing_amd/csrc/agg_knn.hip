// agg_knn.hip -- the k-nearest-neighbour graph of a batch of point clouds: gnnagg_knn_run (include/gnnagg.h section I, "kNN graph").
// For every query row i the k candidates j of its segment with the smallest key (r_ij, j), r_ij = |y_j|^2 - 2 x_i . y_j; the [n, m]
// matrix of the r_ij lives in MFMA accumulators only.
//
// Frame.  256 threads own QT = 64 (32 where LDS forces it: knn_lds) consecutive query rows and the share blockIdx.y of the candidate
// range [y_ptr[seg of the first row], y_ptr[seg of the last row + 1]), walked in tiles of kKnnTile = 64 candidates.  A tile may straddle
// segments: a row keeps its own [lo, hi) in LDS (one bisection over x_ptr per row, once) and masks the rest.
//   stage    4 threads per row copy a row into LDS in 16-byte chunks (scalar loads where the row is not aligned: the same chunks) and
//            sum its squares -- chunk q, q + 4, ... ascending per thread, the four partials (p0 + p1) + (p2 + p3): a norm is a function
//            of the row alone.  Rows past the range and the k padding are zeros.  The query tile is staged once and stays; candidate
//            tiles alternate between two buffers where both fit, the next one staged while this one is multiplied.
//   product  both operands are row-major with k along the row.  Wavefront w takes the row block w % RBW (16 query rows) and the RBW
//            column blocks (w / RBW) RBW ... of the tile (RBW = QT / 16), one A fragment per RBW B fragments.  fp32: a lane reads a
//            float4 at k0 + 4 (lane / 16) of its row from BOTH operands and feeds element t to MFMA t of 4 (16x16x4): a permutation of k
//            common to A and B, 16-byte LDS reads.  bf16: 8 elements per lane and 16x16x32 MFMA.
//   select   D: candidate = lane % 16, query row = 4 (lane / 16) + reg.  key = (mono(r) << 32) | j with mono the monotone integer image
//            of the float bits (NaN: all ones).  A key in the row's segment, not the row itself (loop = 0), and below the row's threshold
//            tau (its k-th best key; all ones until k are known) is appended to the row's queue: one LDS atomic on the queue's count.
//   merge    a row whose queue holds >= 64 keys is merged by ONE wavefront (rows w, w + 4, ...): 64 queued keys sorted across the lanes by
//            a bitonic network of shuffles, min(best[l], sorted[63 - l]) is a bitonic sequence of the 64 smallest of both, six more
//            stages sort it.  best[k - 1] is the new tau.  A queue starts a tile below 64 and gains at most 64, so 128 slots serve.
// Keys are distinct (j is part of them), so neither the order of the queue nor the split changes a bit of the result.
// splits = 1: the wavefront that flushes a row writes idx / dist.  S > 1: it writes the row's k keys to the workspace [n][S][k] (|x_i|^2
// behind them) and k_knn_merge, one wavefront per row, merges the S lists with the same network and writes the row.
// LDS: [x tile QT x pitch][y tiles NBUF x 64 x pitch][y norms NBUF x 64][per row: lo, hi, |x|^2, count, tau][best QT x 64 keys]
// [queues QT x 128 keys].  Barriers per tile: (1) the queues are complete before the merge reads them; (2) merges (tau, counts) and the
// staging of the next tile are complete before the next product and select; with one buffer the next tile is staged between (2) and a third.
#include "kernel_util.cuh"

namespace gnnagg {
namespace {

constexpr int kKnnThreads = 256;
constexpr unsigned long long kKnnSentinel = ~0ull;   // above every key: a real j is below 2^31

typedef __bf16 knn_bf16x8 __attribute__((ext_vector_type(8)));

struct KnnArgs {
    const void *x, *y;
    const int *x_ptr, *y_ptr, *out_ptr;
    int *idx;
    float *dist;
    unsigned long long *work;   // S > 1: [n][S][k] keys, then n floats
    long long xpitch, ypitch;
    int n, m, feat, k, num_seg, excl_self, splits, xvec, yvec;
};

// kernel and launcher agree through knn_lds
struct KnnLds {
    int qt, nbuf, kp, pitch, ys_off, yy_off, meta_off, best_off, queue_off, bytes;
};
__host__ __device__ constexpr KnnLds knn_lds_for(int feat, bool b16, int qt, int nbuf)
{
    KnnLds l = {};
    const int es = b16 ? 2 : 4;
    l.qt = qt;
    l.nbuf = nbuf;
    l.kp = b16 ? (feat + 31) & ~31 : (feat + 15) & ~15;   // whole k steps of a lane's 16 bytes x 4
    l.pitch = b16 ? l.kp + 8 : l.kp + 4;                  // rows 16 bytes past a multiple of 64: the 16 rows of a fragment spread over the banks
    l.ys_off = qt * l.pitch * es;
    l.yy_off = l.ys_off + nbuf * kKnnTile * l.pitch * es;
    l.meta_off = l.yy_off + nbuf * kKnnTile * 4;
    l.best_off = l.meta_off + qt * 24;
    l.queue_off = l.best_off + qt * kKnnList * 8;
    l.bytes = l.queue_off + qt * kKnnQueue * 8;
    return l;
}
__host__ __device__ constexpr KnnLds knn_lds(int feat, bool b16)
{
    for (int qt = 64; qt >= 32; qt >>= 1)
        for (int nbuf = 2; nbuf >= 1; --nbuf) {
            const KnnLds l = knn_lds_for(feat, b16, qt, nbuf);
            if (l.bytes <= kKnnLdsBytes) return l;
        }
    return KnnLds{};   // qt = 0: no tile fits
}

static bool knn_supported(int feat, int k, int dtype)
{
    if (dtype != GNNAGG_DTYPE_F32 && dtype != GNNAGG_DTYPE_BF16) return false;
    if (feat < 1 || feat > kKnnMaxFeat || k < 1 || k > kKnnMaxK) return false;
    return knn_lds(feat, dtype == GNNAGG_DTYPE_BF16).qt > 0;
}

// the shares a candidate range is split into: enough workgroups for every CU, no share below one tile of the mean segment
static int knn_splits(int n, int m, int feat, int dtype, int num_seg, int splits)
{
    if (splits > 0) return splits;
    const int qtiles = ceil_div(n, knn_lds(feat, dtype == GNNAGG_DTYPE_BF16).qt);
    const int ctiles = ceil_div(ceil_div(m, std::max(num_seg, 1)), kKnnTile);
    return std::max(1, std::min(std::min(device_cu_count() / std::max(qtiles, 1), ctiles), kKnnMaxSplits));
}
static long long knn_work_bytes(int n, int k, int S) { return S > 1 ? (long long)n * S * k * 8 + (long long)n * 4 : 0; }

__device__ __forceinline__ unsigned knn_mono(float r)
{
    r = r + 0.0f;   // -0 orders as +0
    const unsigned u = __float_as_uint(r);
    if (r != r) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unmono(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__device__ __forceinline__ unsigned long long knn_shfl_xor(unsigned long long v, int mask)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, mask, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), mask, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long knn_shfl(unsigned long long v, int src)
{
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, 64);
    return ((unsigned long long)hi << 32) | lo;
}
// one compare-exchange stage across the wavefront: lane l and lane l ^ j order their keys, the lower lane takes the smaller where `up`
__device__ __forceinline__ unsigned long long knn_cx(unsigned long long v, int lane, int j, bool up)
{
    const unsigned long long p = knn_shfl_xor(v, j);
    const bool keep_min = ((lane & j) == 0) == up;
    return ((v < p) == keep_min) ? v : p;
}
// best: 64 keys ascending across the lanes; q: 64 keys in any order.  Returns the 64 smallest of both, ascending.
__device__ __forceinline__ unsigned long long knn_merge64(unsigned long long best, unsigned long long q, int lane)
{
#pragma unroll
    for (int ks = 2; ks <= 64; ks <<= 1)
#pragma unroll
        for (int j = ks >> 1; j > 0; j >>= 1) q = knn_cx(q, lane, j, (lane & ks) == 0);
    const unsigned long long qr = knn_shfl(q, 63 - lane);
    unsigned long long v = best < qr ? best : qr;
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) v = knn_cx(v, lane, j, true);
    return v;
}

// a row of the output from its sorted keys: lane l holds the l-th best
__device__ __forceinline__ void knn_write_row(const KnnArgs &a, int row, unsigned long long best, float xx, int lane)
{
    const int o0 = a.out_ptr[row], cnt = a.out_ptr[row + 1] - o0;
    if (lane < cnt && lane < a.k && best != kKnnSentinel) {
        a.idx[(size_t)o0 + lane] = (int)(unsigned)best;
        if (a.dist) a.dist[(size_t)o0 + lane] = fmaxf(knn_unmono((unsigned)(best >> 32)) + xx, 0.0f);
    }
}

// Rows g0 .. g0 + nrows - 1 of src (those below gend; zeros beyond) into dst [nrows x pitch], columns [0, kp), and their squared norms.
// 4 threads per row, 16-byte chunks q, q + 4, ...: see the header.  vec: rows are 16-byte aligned and feat is whole chunks.
template <typename TX>
__device__ __forceinline__ void knn_stage(TX *dst, int pitch, int kp, float *norms, const TX *__restrict__ src, long long spitch, int feat,
                                          long long g0, long long gend, int nrows, bool vec)
{
    constexpr int V = 16 / (int)sizeof(TX);
    const int q = (int)threadIdx.x & 3;
    for (int row = (int)threadIdx.x >> 2; row < nrows; row += kKnnThreads / 4) {
        const long long g = g0 + row;
        const bool ok = g < gend;
        const TX *s = src + (size_t)(ok ? g : 0) * (size_t)spitch;
        float sum = 0.0f;
        for (int c = q * V; c < kp; c += 4 * V) {
            unsigned w[4] = {0u, 0u, 0u, 0u};
            if (ok && c < feat) {
                if (vec) {
                    const uint4 t = *reinterpret_cast<const uint4 *>(s + c);
                    w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
                } else if constexpr (sizeof(TX) == 4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < feat) w[e] = __float_as_uint(reinterpret_cast<const float *>(s)[c + e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (c + e < feat) w[e >> 1] |= (unsigned)reinterpret_cast<const unsigned short *>(s)[c + e] << (16 * (e & 1));
                }
            }
            if constexpr (sizeof(TX) == 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sum = fmaf(__uint_as_float(w[e]), __uint_as_float(w[e]), sum);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = __uint_as_float(w[e] << 16), hi = __uint_as_float(w[e] & 0xffff0000u);
                    sum = fmaf(lo, lo, sum);
                    sum = fmaf(hi, hi, sum);
                }
            }
            uint2 *d = reinterpret_cast<uint2 *>(dst + (size_t)row * pitch + c);   // two 8-byte stores (scripts/check_store_hazard.py)
            d[0] = make_uint2(w[0], w[1]);
            d[1] = make_uint2(w[2], w[3]);
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        if (q == 0) norms[row] = sum;
    }
}

template <int RBW, typename TX>
__global__ __launch_bounds__(kKnnThreads) void k_knn(const KnnArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int QT = 16 * RBW;
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
    const KnnLds L = knn_lds(a.feat, B16);   // the launcher instantiates RBW = L.qt / 16
    const int pitch = L.pitch, kp = L.kp, nbuf = L.nbuf;
    TX *xs = reinterpret_cast<TX *>(knn_smem);
    TX *ys = reinterpret_cast<TX *>(knn_smem + L.ys_off);
    float *yy = reinterpret_cast<float *>(knn_smem + L.yy_off);
    int *row_lo = reinterpret_cast<int *>(knn_smem + L.meta_off), *row_hi = row_lo + QT, *qcnt = row_hi + QT;
    float *row_xx = reinterpret_cast<float *>(qcnt + QT);
    unsigned long long *tau = reinterpret_cast<unsigned long long *>(row_xx + QT);
    unsigned long long *best = reinterpret_cast<unsigned long long *>(knn_smem + L.best_off);
    unsigned long long *queue = reinterpret_cast<unsigned long long *>(knn_smem + L.queue_off);
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
    const int r0 = (int)blockIdx.x * QT, s = (int)blockIdx.y;
    const TX *__restrict__ x = static_cast<const TX *>(a.x);
    const TX *__restrict__ y = static_cast<const TX *>(a.y);

    // ---- once: the query tile, every row's candidate range, empty lists
    knn_stage<TX>(xs, pitch, kp, row_xx, x, a.xpitch, a.feat, r0, a.n, QT, a.xvec != 0);
    if (tid < QT) {
        const int g = r0 + tid;
        int lo = 0, hi = 0;
        if (g < a.n) {
            if (a.x_ptr) {
                int b = 0, e = a.num_seg;   // the largest b < num_seg with x_ptr[b] <= g
                while (e - b > 1) {
                    const int mid = (b + e) >> 1;
                    if (a.x_ptr[mid] <= g) b = mid;
                    else e = mid;
                }
                lo = a.y_ptr[b];
                hi = a.y_ptr[b + 1];
            } else {
                hi = a.m;
            }
            lo = lo < 0 ? 0 : (lo > a.m ? a.m : lo);
            hi = hi < lo ? lo : (hi > a.m ? a.m : hi);
        }
        row_lo[tid] = lo;
        row_hi[tid] = hi;
        qcnt[tid] = 0;
        tau[tid] = kKnnSentinel;
    }
    for (int i = tid; i < QT * kKnnList; i += kKnnThreads) best[i] = kKnnSentinel;
    __syncthreads();
    const int nvalid = a.n - r0 < QT ? a.n - r0 : QT;
    int c0 = row_lo[0], c1 = c0;
    for (int r = 0; r < nvalid; ++r) {   // pointers that break the contract may descend: the walk covers what the rows ask for
        c0 = row_lo[r] < c0 ? row_lo[r] : c0;
        c1 = row_hi[r] > c1 ? row_hi[r] : c1;
    }
    const int ntiles = (c1 - c0 + kKnnTile - 1) / kKnnTile;
    const int t_beg = (int)((long long)ntiles * s / a.splits), t_end = (int)((long long)ntiles * (s + 1) / a.splits);

    const int rbw = wave % RBW, cg = wave / RBW;   // this wavefront's row block and group of RBW column blocks
    int my_lo[4], my_hi[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        my_lo[v] = row_lo[rbw * 16 + 4 * kq + v];
        my_hi[v] = row_hi[rbw * 16 + 4 * kq + v];
    }
    const TX *arow = xs + (size_t)(rbw * 16 + l16) * pitch + (B16 ? 8 : 4) * kq;

    if (t_beg < t_end) knn_stage<TX>(ys, pitch, kp, yy, y, a.ypitch, a.feat, (long long)c0 + (long long)t_beg * kKnnTile, c1, kKnnTile, a.yvec != 0);
    __syncthreads();
#pragma unroll 1
    for (int t = t_beg; t < t_end; ++t) {
        const int buf = nbuf == 2 ? (t - t_beg) & 1 : 0;
        const TX *yb = ys + (size_t)buf * kKnnTile * pitch;
        const float *yyb = yy + buf * kKnnTile;
        if (nbuf == 2 && t + 1 < t_end)
            knn_stage<TX>(ys + (size_t)(buf ^ 1) * kKnnTile * pitch, pitch, kp, yy + (buf ^ 1) * kKnnTile, y, a.ypitch, a.feat,
                          (long long)c0 + (long long)(t + 1) * kKnnTile, c1, kKnnTile, a.yvec != 0);
        // ---- product: acc[cb][v] = x[row 4 kq + v of the row block] . y[column l16 of column block cb]
        f32x4 acc[RBW];
#pragma unroll
        for (int cb = 0; cb < RBW; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const TX *brow = yb + (size_t)(cg * RBW * 16 + l16) * pitch + (B16 ? 8 : 4) * kq;
        if constexpr (B16) {
            for (int k0 = 0; k0 < kp; k0 += 32) {
                const knn_bf16x8 av = *reinterpret_cast<const knn_bf16x8 *>(arow + k0);
#pragma unroll
                for (int cb = 0; cb < RBW; ++cb)
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, *reinterpret_cast<const knn_bf16x8 *>(brow + (size_t)cb * 16 * pitch + k0),
                                                                      acc[cb], 0, 0, 0);
            }
        } else {
            for (int k0 = 0; k0 < kp; k0 += 16) {
                const float4 av = *reinterpret_cast<const float4 *>(arow + k0);
#pragma unroll
                for (int cb = 0; cb < RBW; ++cb) {
                    const float4 bv = *reinterpret_cast<const float4 *>(brow + (size_t)cb * 16 * pitch + k0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[cb], 0, 0, 0);
                }
            }
        }
        // ---- select
        unsigned long long my_tau[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) my_tau[v] = tau[rbw * 16 + 4 * kq + v];
#pragma unroll
        for (int cb = 0; cb < RBW; ++cb) {
            const int jl = (cg * RBW + cb) * 16 + l16;
            const int j = c0 + t * kKnnTile + jl;
            const float ny = yyb[jl];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = rbw * 16 + 4 * kq + v;
                const unsigned long long key = ((unsigned long long)knn_mono(fmaf(-2.0f, acc[cb][v], ny)) << 32) | (unsigned)j;
                const bool in = j >= my_lo[v] && j < my_hi[v] && !(a.excl_self && j == r0 + row);
                if (in && key < my_tau[v]) {
                    const int slot = atomicAdd(&qcnt[row], 1);
                    if (slot < kKnnQueue) queue[row * kKnnQueue + slot] = key;
                }
            }
        }
        __syncthreads();   // (1) the queues of this tile are complete
        for (int row = wave; row < QT; row += kKnnThreads / 64) {
            const int cnt = qcnt[row] < kKnnQueue ? qcnt[row] : kKnnQueue;
            if (cnt < kKnnList) continue;
            unsigned long long b = best[row * kKnnList + lane];
            for (int base = 0; base < cnt; base += 64)
                b = knn_merge64(b, base + lane < cnt ? queue[row * kKnnQueue + base + lane] : kKnnSentinel, lane);
            best[row * kKnnList + lane] = b;
            const unsigned long long kth = knn_shfl(b, a.k - 1);
            if (lane == 0) {
                tau[row] = kth;
                qcnt[row] = 0;
            }
        }
        __syncthreads();   // (2) tau and the counts are settled; the other buffer holds the next tile
        if (nbuf == 1 && t + 1 < t_end) {
            knn_stage<TX>(ys, pitch, kp, yy, y, a.ypitch, a.feat, (long long)c0 + (long long)(t + 1) * kKnnTile, c1, kKnnTile, a.yvec != 0);
            __syncthreads();
        }
    }
    // ---- flush what the queues still hold and write the rows
    for (int row = wave; row < nvalid; row += kKnnThreads / 64) {
        const int cnt = qcnt[row] < kKnnQueue ? qcnt[row] : kKnnQueue;
        unsigned long long b = best[row * kKnnList + lane];
        for (int base = 0; base < cnt; base += 64)
            b = knn_merge64(b, base + lane < cnt ? queue[row * kKnnQueue + base + lane] : kKnnSentinel, lane);
        const int g = r0 + row;
        if (a.splits == 1) {
            knn_write_row(a, g, b, row_xx[row], lane);
        } else {
            if (lane < a.k) a.work[((size_t)g * a.splits + s) * a.k + lane] = b;
            if (s == 0 && lane == 0) reinterpret_cast<float *>(a.work + (size_t)a.n * a.splits * a.k)[g] = row_xx[row];
        }
    }
}

// S > 1: one wavefront per row merges the S lists of k keys that the workgroups (tile, s) left
__global__ __launch_bounds__(kKnnThreads) void k_knn_merge(const KnnArgs a)
{
    const int lane = (int)threadIdx.x & 63;
    const int g = (int)blockIdx.x * (kKnnThreads / 64) + ((int)threadIdx.x >> 6);
    if (g >= a.n) return;
    const unsigned long long *w = a.work + (size_t)g * a.splits * a.k;
    const int cnt = a.splits * a.k;
    unsigned long long b = kKnnSentinel;
    for (int base = 0; base < cnt; base += 64) b = knn_merge64(b, base + lane < cnt ? w[base + lane] : kKnnSentinel, lane);
    knn_write_row(a, g, b, reinterpret_cast<const float *>(a.work + (size_t)a.n * a.splits * a.k)[g], lane);
}

template <int RBW, typename TX>
static int launch_knn(const KnnArgs &a, size_t lds, hipStream_t st)
{
    static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
    if (lds > 64 * 1024 && big_lds_ok.first()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_knn<RBW, TX>), hipFuncAttributeMaxDynamicSharedMemorySize, kKnnLdsBytes));
        big_lds_ok.done();
    }
    hipLaunchKernelGGL((k_knn<RBW, TX>), dim3((unsigned)ceil_div(a.n, 16 * RBW), (unsigned)a.splits), dim3(kKnnThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    if (a.splits > 1) {
        hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)ceil_div(a.n, kKnnThreads / 64)), dim3(kKnnThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return GNNAGG_OK;
}

// the checks that knn_run and knn_work_bytes share; 0: fine
static int knn_check_shape(const char *who, int n, int m, int feat, int k, int dtype, int num_seg, int splits)
{
    auto bad = [&](const std::string &msg) { return fail(GNNAGG_ERR_ARG, who + msg); };
    if (n < 0) return bad("n = " + std::to_string(n) + " is negative");
    if (m < 0) return bad("m = " + std::to_string(m) + " is negative");
    if (feat < 1 || feat > kKnnMaxFeat) return bad("feat = " + std::to_string(feat) + " lies outside 1.." + std::to_string(kKnnMaxFeat));
    if (k < 1 || k > kKnnMaxK) return bad("k = " + std::to_string(k) + " lies outside 1.." + std::to_string(kKnnMaxK));
    if (dtype != GNNAGG_DTYPE_F32 && dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(dtype));
    if (num_seg < 0) return bad("num_seg = " + std::to_string(num_seg) + " is negative");
    if (splits < 0 || splits > kKnnMaxSplits) return bad("splits = " + std::to_string(splits) + " lies outside 0.." + std::to_string(kKnnMaxSplits));
    if (!knn_supported(feat, k, dtype)) return bad("feat = " + std::to_string(feat) + ", k = " + std::to_string(k) + " lie outside the range of gnnagg_knn_supported");
    return GNNAGG_OK;
}

static int knn_run(const void *x, const void *y, int dtype, long long x_pitch, long long y_pitch, int n, int m, int feat, int k, const int *x_ptr,
                   const int *y_ptr, int num_seg, int loop, const int *out_ptr, int *idx, float *dist, void *work, long long work_bytes, int splits,
                   void *stream)
{
    static const char *who = "gnnagg_knn_run: ";
    auto bad = [&](const std::string &msg) { return fail(GNNAGG_ERR_ARG, who + msg); };
    if (int rc = knn_check_shape(who, n, m, feat, k, dtype, (x_ptr || y_ptr) ? num_seg : 0, splits)) return rc;
    if (x_pitch < feat) return bad("x_pitch = " + std::to_string(x_pitch) + " is below feat = " + std::to_string(feat));
    if (!y) {
        if (m != n) return bad("d_y is null (the candidates are the queries) but m = " + std::to_string(m) + " is not n = " + std::to_string(n));
        y = x;
        y_pitch = x_pitch;
        y_ptr = x_ptr;
    } else {
        if (y_pitch < feat) return bad("y_pitch = " + std::to_string(y_pitch) + " is below feat = " + std::to_string(feat));
        if (!x_ptr != !y_ptr) return bad(std::string(x_ptr ? "d_y_ptr" : "d_x_ptr") + " is null and the other pointer array is not");
        loop = 1;
    }
    if (x_ptr && num_seg < 1) return bad("num_seg = " + std::to_string(num_seg) + " must be >= 1 with segment pointers");
    if (n > 0) {
        if (!x) return bad("d_x is null");
        if (!out_ptr) return bad("d_out_ptr is null");
        if (!idx) return bad("d_idx is null");
    }
    if (n == 0) return GNNAGG_OK;
    const int S = knn_splits(n, m, feat, dtype, x_ptr ? num_seg : 1, splits);
    const long long need = knn_work_bytes(n, k, S);
    if (S > 1 && !work) return bad("d_work is null with " + std::to_string(S) + " splits");
    if (S > 1 && work_bytes < need) return bad("work_bytes = " + std::to_string(work_bytes) + " is below gnnagg_knn_work_bytes = " + std::to_string(need));

    const bool b16 = dtype == GNNAGG_DTYPE_BF16;
    const int V = b16 ? 8 : 4;
    auto vec_ok = [&](const void *p, long long pitch) { return feat % V == 0 && pitch % V == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    KnnArgs a;
    a.x = x; a.y = y; a.x_ptr = x_ptr; a.y_ptr = y_ptr; a.out_ptr = out_ptr; a.idx = idx; a.dist = dist;
    a.work = static_cast<unsigned long long *>(work); a.xpitch = x_pitch; a.ypitch = y_pitch;
    a.n = n; a.m = m; a.feat = feat; a.k = k; a.num_seg = num_seg; a.excl_self = !loop; a.splits = S;
    a.xvec = vec_ok(x, x_pitch); a.yvec = vec_ok(y, y_pitch);
    const KnnLds L = knn_lds(feat, b16);
    hipStream_t st = (hipStream_t)stream;
    switch ((L.qt / 16) * 2 + (b16 ? 1 : 0)) {
        case 8: return launch_knn<4, float>(a, (size_t)L.bytes, st);
        case 9: return launch_knn<4, __bf16>(a, (size_t)L.bytes, st);
        case 4: return launch_knn<2, float>(a, (size_t)L.bytes, st);
        case 5: return launch_knn<2, __bf16>(a, (size_t)L.bytes, st);
        default: return fail(GNNAGG_ERR_STATE, "internal: gnnagg_knn_run has no query tile for this shape");
    }
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_knn_run(const void *d_x, const void *d_y, int x_dtype, long long x_pitch, long long y_pitch, int n, int m, int feat, int k,
                   const int *d_x_ptr, const int *d_y_ptr, int num_seg, int loop, const int *d_out_ptr, int *d_idx, float *d_dist, void *d_work,
                   long long work_bytes, int splits, void *hip_stream)
{
    return knn_run(d_x, d_y, x_dtype, x_pitch, y_pitch, n, m, feat, k, d_x_ptr, d_y_ptr, num_seg, loop, d_out_ptr, d_idx, d_dist, d_work, work_bytes,
                   splits, hip_stream);
}

int gnnagg_knn_supported(int feat, int k, int x_dtype) { return knn_supported(feat, k, x_dtype) ? 1 : 0; }

long long gnnagg_knn_work_bytes(int n, int m, int feat, int k, int x_dtype, int num_seg, int splits)
{
    if (knn_check_shape("gnnagg_knn_work_bytes: ", n, m, feat, k, x_dtype, num_seg, splits)) return -1;
    if (n == 0) return 0;
    return knn_work_bytes(n, k, knn_splits(n, m, feat, x_dtype, std::max(num_seg, 1), splits));
}

}  // extern "C"
#pragma GCC visibility pop
