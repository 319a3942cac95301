// sample.hip -- neighbour sampling on the device (include/gnnagg.h, section "Neighbour sampling"): seeds + fanout -> a message-flow block.
//
// A seed row r with d edges at positions p in [ptr[r], ptr[r+1]) keeps all of them (fanout = -1 or d <= fanout) or the `fanout` edges with
// the smallest key(seed, p); kept edges stay in CSR order.  key is a bijection of p for a fixed seed (sample_key.h), so the fanout-th
// smallest key T of a row is unique and "key <= T" names the kept set: a SELECT of one threshold per row, then one ordered emission.
//
//   k_sample_counts   min(d, fanout) per seed                                  -> prims::scan -> blk_ptr
//   k_sample_select   a wavefront (sixteen per workgroup) takes 64 consecutive seeds; rows that keep everything and have <= 64 edges are copied by 8-lane groups,
//                     every other row by the whole wavefront: d <= 64 keys in registers, T by a 32-step radix select over ballots (ONE key
//                     evaluation per edge); d > 64 four passes of 8-bit digit histograms in this wavefront's 1 KB of LDS, then the
//                     emission in rounds of 64 edges (FIVE key evaluations per edge); rows above kHubEdges edges are queued and walked by
//                     the whole workgroup, their candidate keys buffered in LDS (TWO evaluations per edge: select_threshold_hub).  The
//                     four passes are radix_select, whoever walks and wherever the keys come from (a position, or the LDS buffer); the
//                     emission is emit_row for a wavefront and for the workgroup.  Output positions are ballot prefix ranks: no atomics
//                     touch the output, and nothing is loaded but ptr and the kept idx entries.
//   relabelling       the sampler's num_v-entry map is kUnseen between calls.  Seeds atomicMin (i - num_seeds) < 0, kept edges atomicMin
//                     their block position >= 0: the lowest seed index / first appearance wins whatever the order of the atomics.  An
//                     edge whose entry equals its position is a first appearance; a scan of those flags numbers the new source rows; one
//                     pass relabels and writes src_nodes; a last pass puts kUnseen back at the entries src_nodes names: O(batch).
//                     The scans read one buffer and write another.
//   weights           gnnagg_sampler_set_weights: the <true> instantiations of the counts and select kernels.  The key is sample_wkey (the
//                     bits of E / w, E the integer -log2 of the uniform key; no bijection), a row's count is min(eligible edges, fanout) from a per-row count made
//                     once per weight vector, and the emission keeps key < T plus the first `quota` edges with key == T in position order
//                     (the uniform rule, key <= T, is that rule without ties).  A weighted hub row takes the four walks: the candidate
//                     buffer rests on the distribution of the uniform keys.
#include <hip/hip_runtime.h>

#include <climits>
#include <mutex>
#include <set>

// prims.cuh as it is (tests/plan_census.py pins its text).  Its scan is a template; its two sort kernels are plain __global__ functions of a
// header that plan_gpu.hip includes as well, so this translation unit gives its (unused) copies names of their own for the linker.
#define k_sort_hist k_sort_hist_in_sample
#define k_sort_scatter k_sort_scatter_in_sample
#include "prims.cuh"
#undef k_sort_hist
#undef k_sort_scatter
#include "sample_key.h"

namespace gnnagg {
namespace {

constexpr int kUnseen = INT_MAX;     // (a block position is < cap_e <= INT_MAX - 1)
constexpr int kSelBlock = 1024;      // k_sample_select: sixteen wavefronts of 64 seeds each
constexpr int kHubEdges = 2048;      // rows above it are walked by the whole workgroup, not by one wavefront

// edges [beg, beg + d) of row r; a row id or a ptr pair that does not lie inside the CSR counts as a row without edges
__device__ __forceinline__ void row_extent(const int *__restrict__ ptr, int num_v, int num_e, int r, int &beg, int &d)
{
    beg = 0;
    d = 0;
    if ((unsigned)r < (unsigned)num_v) {
        const int b = ptr[r], e = ptr[r + 1];
        if (b >= 0 && e >= b && e <= num_e) { beg = b; d = e - b; }
    }
}

// WEIGHTED: d is the row's number of eligible edges, counted once per weight vector (k_sample_eligible)
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_sample_counts(const int *__restrict__ ptr, int num_v, int num_e, const int *__restrict__ seeds, int num_seeds,
                                                       int fanout, int *__restrict__ cnt /* [num_seeds + 1] */, const int *__restrict__ elig /* [num_v] */)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > num_seeds) return;
    int c = 0;
    if (i < num_seeds) {
        int beg, d;
        if (WEIGHTED) {
            const int r = seeds[i];
            d = (unsigned)r < (unsigned)num_v ? elig[r] : 0;
        } else row_extent(ptr, num_v, num_e, seeds[i], beg, d);
        c = fanout < 0 ? d : (d < fanout ? d : fanout);
    }
    cnt[i] = c;
}

// ---- the eligible edges of every row, once per weight vector: flags, one scan over the edges, a difference at the row boundaries (a hub
// row costs what its edges cost anywhere else)
__global__ __launch_bounds__(256) void k_sample_wflags(const float *__restrict__ w, long long num_e, int *__restrict__ flag /* [num_e + 1] */)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p <= num_e) flag[p] = p < num_e && w[p] > 0.0f;
}

__global__ __launch_bounds__(256) void k_sample_eligible(const int *__restrict__ ptr, int num_v, int num_e, const int *__restrict__ before /* [num_e + 1] */,
                                                         int *__restrict__ elig)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= num_v) return;
    int beg, d;
    row_extent(ptr, num_v, num_e, r, beg, d);
    elig[r] = before[beg + d] - before[beg];
}

// the key the select orders a row by: the uniform key, or the weighted key built from it and the edge's weight
template <bool WEIGHTED>
__device__ __forceinline__ unsigned edge_key(unsigned p, unsigned s, const float *__restrict__ w)
{
    const unsigned u = sample_key(p, s);
    if (!WEIGHTED) return u;
    return sample_wkey(u, w[p]);
}

// LDS traffic of ONE wavefront (its own histogram): orders the wavefront's LDS atomics and loads for the compiler; the hardware runs a
// wavefront's LDS instructions in order
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_bcast(int v, int src) { return __builtin_amdgcn_readfirstlane(__shfl(v, src, 64)); }

struct SampleOut {
    int *idx;         // [cap]
    int *eid;         // nullptr or [cap]
    long long cap;
};

__device__ __forceinline__ void emit(const SampleOut &o, const int *__restrict__ idx, long long q, int p)
{
    if (q >= 0 && q < o.cap) {   // (q < 0: a total past 2^31 wrapped -- nothing is written)
        o.idx[q] = idx[p];
        if (o.eid) o.eid[q] = p;
    }
}

// the digit whose bin holds the k-th smallest of the keys counted in hist[256] (1 <= k <= their number); k becomes the rank inside that bin.
// Every wavefront that calls it reads the same bins and comes to the same answer.
__device__ __forceinline__ int pick_digit(const int *hist, int lane, int &k)
{
    int h[4], sum = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) { h[b] = hist[lane * 4 + b]; sum += h[b]; }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const int excl = incl - sum;
    const unsigned long long hit = __ballot(excl < k && k <= incl);   // exactly one lane
    const int src = __ffsll((long long)hit) - 1;
    int digit = lane * 4, c = excl, knew = k;
    bool found = false;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (!found && k <= c + h[b]) { digit = lane * 4 + b; knew = k - c; found = true; }
        c += h[b];
    }
    k = wave_bcast(knew, src);
    return wave_bcast(digit, src);
}

// the k-th smallest (k >= 1) of the n keys key_at(0 .. n - 1): four passes of 8-bit digit histograms, most significant digit first.
// BLOCK = false: one wavefront and its own histogram; BLOCK = true: the whole workgroup on one shared histogram (every wavefront reads the
// same bins and comes to the same digit).  `tid` is the thread's index in the group of `GROUP` threads that walks the keys.  On return k is
// the rank of the k-th smallest among the keys EQUAL to it: 1 for the uniform keys, the number of tied edges to keep for the weighted ones.
template <bool BLOCK, class KeyAt>
__device__ unsigned radix_select(unsigned n, KeyAt key_at, int &k, int *hist /* [256] */, int tid, int lane)
{
    constexpr unsigned GROUP = BLOCK ? kSelBlock : 64;
    unsigned prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 64) {
#pragma unroll
            for (int b = 0; b < 4; ++b) hist[tid * 4 + b] = 0;
        }
        if (BLOCK) __syncthreads(); else wave_lds_sync();
        for (unsigned t = (unsigned)tid; t < n; t += GROUP) {
            const unsigned key = key_at(t);
            if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        if (BLOCK) __syncthreads(); else wave_lds_sync();
        const int digit = pick_digit(hist, lane, k);
        prefix = (prefix << 8) | (unsigned)digit;
        if (BLOCK) __syncthreads(); else wave_lds_sync();
    }
    return prefix;
}

// the k-th smallest key of positions [beg, beg + d), every key evaluated in each of the four passes
template <bool BLOCK, bool WEIGHTED>
__device__ unsigned select_threshold_lds(int beg, int d, int &k, unsigned s, const float *__restrict__ w, int *hist /* [256] */, int tid, int lane)
{
    return radix_select<BLOCK>((unsigned)d, [=](unsigned t) { return edge_key<WEIGHTED>((unsigned)beg + t, s, w); }, k, hist, tid, lane);
}

// Hub rows (the whole workgroup): a row much longer than k is walked ONCE for the select.  The keys below 2^(32 - c), c chosen so that
// 1024 .. 2047 of them are expected, are buffered in LDS (their order there does not matter: only the k-th smallest is taken from them), and
// the radix select runs over the buffer.  Fewer than k candidates, or more than the buffer holds: the four walks of select_threshold_lds.
// (Uniform keys only: the prefilter rests on their distribution.  Weighted hub rows take the four walks.)
constexpr int kCand = (kSelBlock / 64) * 256;   // the wavefronts' own histograms, idle by then, are the buffer
__device__ unsigned select_threshold_hub(int beg, int d, int k, unsigned s, int *hist /* shared [256] */, int *buf /* shared [kCand] */, int *cand_n,
                                         int tid, int lane)
{
    int c = 1;
    while (c < 24 && (d >> (c + 1)) >= 1024) ++c;
    if (tid == 0) *cand_n = 0;
    __syncthreads();
    for (unsigned t = (unsigned)tid; t < (unsigned)d; t += kSelBlock) {
        const unsigned key = sample_key((unsigned)beg + t, s);
        if ((key >> (32 - c)) == 0u) {
            const int pos = atomicAdd(cand_n, 1);
            if (pos < kCand) buf[pos] = (int)key;
        }
    }
    __syncthreads();
    const int n = *cand_n;
    __syncthreads();
    if (n < k || n > kCand) return select_threshold_lds<true, false>(beg, d, k, s, nullptr, hist, tid, lane);   // (the same for every thread)
    return radix_select<true>((unsigned)n, [=](unsigned j) { return (unsigned)buf[j]; }, k, hist, tid, lane);
}

// The ordered emission of row [b, b + dd) under its threshold T, to out[o ..], in rounds of one edge per thread.  BLOCK = false: one
// wavefront (tid = lane); BLOCK = true: the whole workgroup, whose wavefronts exchange their counts of a round through wcount[kWaves].  dd, T
// and quota are the same for every thread that enters, so the loop and its barriers are uniform.
// Uniform keys: an edge is kept when key <= T, at o + (kept edges before it).  WEIGHTED: when key < T, or key == T and fewer than `quota`
// edges equal to T lie before it; at o + (keys < T before it) + min(keys == T before it, quota).  "Before it" is the rounds so far (run,
// ties), the wavefronts below this one in the round (their counts packed as lt | eq << 16: both <= 64 a wavefront, <= 1024 a round) and
// the lanes below this one (ballot ranks).
template <bool BLOCK, bool WEIGHTED>
__device__ __forceinline__ void emit_row(const SampleOut &out, const int *__restrict__ idx, int b, int dd, int o, unsigned T, int quota, unsigned s,
                                         const float *__restrict__ w, int *wcount, int tid, int lane, int wave)
{
    constexpr unsigned GROUP = BLOCK ? kSelBlock : 64;
    constexpr int kWaves = kSelBlock / 64;
    const unsigned long long below = (1ull << lane) - 1ull;
    int run = 0, ties = 0;
    for (unsigned base = 0; base < (unsigned)dd; base += GROUP) {
        const unsigned t = base + (unsigned)tid;
        unsigned key = 0;
        bool keep = false;
        unsigned long long lt, eq = 0;
        if (WEIGHTED) {
            // (no weight is read past the row; T is an eligible edge's key, below kSampleIneligible -- unless the weights changed under
            // the sampler, hence t < dd in eq)
            key = t < (unsigned)dd ? edge_key<true>((unsigned)b + t, s, w) : kSampleIneligible;
            lt = __ballot(key < T);
            eq = __ballot(t < (unsigned)dd && key == T);
        } else {
            keep = t < (unsigned)dd && sample_key((unsigned)b + t, s) <= T;
            lt = __ballot(keep);
        }
        int before = 0, total = WEIGHTED ? __popcll(lt) | (__popcll(eq) << 16) : __popcll(lt);
        if (BLOCK) {
            if (lane == 0) wcount[wave] = total;
            __syncthreads();
            total = 0;
#pragma unroll
            for (int v = 0; v < kWaves; ++v) {
                const int c = wcount[v];
                if (v < wave) before += c;
                total += c;
            }
        }
        if (WEIGHTED) {
            const int tied = ties + (before >> 16) + __popcll(eq & below);
            if (key < T || (((eq >> lane) & 1ull) && tied < quota))
                emit(out, idx, (long long)o + run + (before & 0xffff) + __popcll(lt & below) + (tied < quota ? tied : quota), b + (int)t);
            run += total & 0xffff;
            ties += total >> 16;
        } else {
            if (keep) emit(out, idx, (long long)o + run + before + __popcll(lt & below), b + (int)t);
            run += total;
        }
        if (BLOCK) __syncthreads();
    }
}

// WEIGHTED: keys are edge_key<true> (no bijection), a row's count is min(d+, fanout) and may be 0 .. d, and `quota` is what the select leaves
// of k inside T's bin.  An ineligible edge's key is above every T.
template <bool WEIGHTED>
__global__ __launch_bounds__(kSelBlock) void k_sample_select(const int *__restrict__ ptr, const int *__restrict__ idx, int num_v, int num_e,
                                                             const int *__restrict__ seeds, int num_seeds, unsigned s,
                                                             const int *__restrict__ blk_ptr, SampleOut out, const float *__restrict__ w)
{
    constexpr int kWaves = kSelBlock / 64;
    __shared__ int hist_all[kWaves][256];
    __shared__ int hub_hist[256], hub_list[kSelBlock], hub_n, cand_n, wcount[kWaves];
    __shared__ int s_beg[kSelBlock], s_d[kSelBlock], s_out0[kSelBlock], s_cnt[kSelBlock];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *hist = hist_all[wave];
    if (tid == 0) hub_n = 0;
    const long long i = (long long)blockIdx.x * kSelBlock + tid;
    int beg = 0, d = 0, out0 = 0, cnt = 0;
    if (i < num_seeds) {
        row_extent(ptr, num_v, num_e, seeds[i], beg, d);
        out0 = blk_ptr[i];
        cnt = blk_ptr[i + 1] - out0;
        if (cnt < 0 || cnt > d) { cnt = 0; d = 0; }   // (a wrapped total: the row is skipped)
    }
    s_beg[tid] = beg; s_d[tid] = d; s_out0[tid] = out0; s_cnt[tid] = cnt;
    __syncthreads();   // (hub_n = 0 is seen by everyone before the first append)
    const bool small_copy = d > 0 && cnt == d && d <= 64;
    const bool some = !WEIGHTED || cnt > 0;   // (a weighted row may keep nothing)
    const bool hub = d > kHubEdges && some;
    const bool by_wave = d > 0 && !small_copy && !(d > kHubEdges) && some;
    const unsigned long long m_small = __ballot(small_copy);
    unsigned long long m_wave = __ballot(by_wave);
    const unsigned long long m_hub = __ballot(hub);
    if (m_hub) {   // hub rows wait for the whole workgroup (their order in the list does not reach the output)
        int base = 0;
        if (lane == 0) base = atomicAdd(&hub_n, __popcll(m_hub));
        base = wave_bcast(base, 0);
        if (hub) hub_list[base + __popcll(m_hub & ((1ull << lane) - 1ull))] = tid;
    }

    // rows that keep every edge and have at most 64: eight rows at a time, eight lanes each
    const int sub = lane >> 3, sl = lane & 7;
    for (int round = 0; round < 8; ++round) {
        if (((m_small >> (round * 8)) & 0xffull) == 0) continue;
        const int j = round * 8 + sub;
        const int b = __shfl(beg, j, 64), dd = __shfl(d, j, 64), o = __shfl(out0, j, 64);
        if ((m_small >> j) & 1ull)
            for (int t = sl; t < dd; t += 8) emit(out, idx, (long long)o + t, b + t);
    }

    // every other row of up to kHubEdges edges: the whole wavefront
    while (m_wave) {
        const int j = __ffsll((long long)m_wave) - 1;
        m_wave &= m_wave - 1;
        const int b = wave_bcast(beg, j), dd = wave_bcast(d, j), o = wave_bcast(out0, j), k = wave_bcast(cnt, j);
        if (k == dd) {   // a long row kept whole
            for (int t = lane; t < dd; t += 64) emit(out, idx, (long long)o + t, b + t);
            continue;
        }
        if (dd <= 64) {   // keys in registers; the k-th smallest bit by bit, most significant first
            const bool valid = lane < dd;
            unsigned key;
            if (WEIGHTED) key = valid ? edge_key<true>((unsigned)(b + lane), s, w) : kSampleIneligible;   // (no weight is read past the row)
            else key = sample_key((unsigned)(b + lane), s);
            unsigned long long cand = __ballot(valid);
            int kk = k;
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned long long ones = __ballot((key >> bit) & 1u);
                const unsigned long long zeros = cand & ~ones;
                const int c0 = __popcll(zeros);
                if (kk <= c0) cand = zeros;
                else { kk -= c0; cand &= ones; }
            }
            // cand is the single lane that holds the k-th smallest key (WEIGHTED: every lane that holds it, kk of them to keep)
            const unsigned T = (unsigned)wave_bcast((int)key, __ffsll((long long)cand) - 1);
            const unsigned long long below = (1ull << lane) - 1ull;
            bool keep;
            if (WEIGHTED) keep = valid && (key < T || (((cand >> lane) & 1ull) && __popcll(cand & below) < kk));
            else keep = valid && key <= T;
            const unsigned long long bal = __ballot(keep);
            if (keep) emit(out, idx, (long long)o + __popcll(bal & below), b + lane);
            continue;
        }
        int quota = k;
        const unsigned T = select_threshold_lds<false, WEIGHTED>(b, dd, quota, s, w, hist, lane, lane);
        emit_row<false, WEIGHTED>(out, idx, b, dd, o, T, quota, s, w, nullptr, lane, lane, 0);
    }

    // hub rows (more than kHubEdges edges): the whole workgroup per row, one after the other
    __syncthreads();
    const int n_hub = hub_n;   // (the same for every thread: the loop and its barriers are uniform)
    for (int h = 0; h < n_hub; ++h) {
        const int j = hub_list[h];
        const int b = s_beg[j], dd = s_d[j], o = s_out0[j], k = s_cnt[j];
        if (k == dd) {
            for (unsigned t = (unsigned)tid; t < (unsigned)dd; t += kSelBlock) emit(out, idx, (long long)o + t, b + (int)t);
            continue;
        }
        int quota = k;
        const unsigned T = WEIGHTED ? select_threshold_lds<true, true>(b, dd, quota, s, w, hub_hist, tid, lane)
                                    : select_threshold_hub(b, dd, k, s, hub_hist, &hist_all[0][0], &cand_n, tid, lane);
        emit_row<true, WEIGHTED>(out, idx, b, dd, o, T, quota, s, w, wcount, tid, lane, wave);
    }
}

// ---- relabelling
__device__ __forceinline__ int kept_edges(const int *__restrict__ blk_ptr, int num_seeds, long long cap)
{
    const int total = blk_ptr[num_seeds];
    return total < 0 ? 0 : (int)(total < cap ? total : cap);
}

__global__ __launch_bounds__(256) void k_sample_mark_seeds(const int *__restrict__ seeds, int num_seeds, int num_v, int *__restrict__ map,
                                                           int *__restrict__ src_nodes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_seeds) return;
    const int r = seeds[i];
    src_nodes[i] = r;
    if ((unsigned)r < (unsigned)num_v) atomicMin(&map[r], i - num_seeds);
}

__global__ __launch_bounds__(256) void k_sample_mark_edges(const int *__restrict__ blk_ptr, int num_seeds, long long cap, const int *__restrict__ blk_idx,
                                                           int num_v, int *__restrict__ map)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= kept_edges(blk_ptr, num_seeds, cap)) return;
    const int v = blk_idx[q];
    if ((unsigned)v < (unsigned)num_v) atomicMin(&map[v], (int)q);
}

// flag[q] = 1 where edge q is the first appearance of a row that is no seed; flag[n] = 0 closes the scan
__global__ __launch_bounds__(256) void k_sample_flags(const int *__restrict__ blk_ptr, int num_seeds, long long cap, const int *__restrict__ blk_idx,
                                                      int num_v, const int *__restrict__ map, long long n, int *__restrict__ flag)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q > n) return;
    int f = 0;
    if (q < kept_edges(blk_ptr, num_seeds, cap)) {
        const int v = blk_idx[q];
        f = (unsigned)v < (unsigned)num_v && map[v] == (int)q;
    }
    flag[q] = f;
}

__global__ __launch_bounds__(256) void k_sample_relabel(const int *__restrict__ blk_ptr, int num_seeds, long long cap, int *__restrict__ blk_idx, int num_v,
                                                        const int *__restrict__ map, const int *__restrict__ first_rank, int *__restrict__ src_nodes)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= kept_edges(blk_ptr, num_seeds, cap)) return;
    const int v = blk_idx[q];
    int local = -1;   // (an id outside the CSR's rows: an invalid graph)
    if ((unsigned)v < (unsigned)num_v) {
        const int m = map[v];
        if (m < 0) local = m + num_seeds;
        else {
            local = num_seeds + first_rank[m];
            if (m == (int)q) src_nodes[local] = v;
        }
    }
    blk_idx[q] = local;
}

__global__ __launch_bounds__(256) void k_sample_restore(const int *__restrict__ src_nodes, int num_seeds, const int *__restrict__ first_rank, long long n,
                                                        int num_v, int *__restrict__ map)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= (long long)num_seeds + first_rank[n]) return;
    const int v = src_nodes[j];
    if ((unsigned)v < (unsigned)num_v) map[v] = kUnseen;
}

__global__ void k_sample_finish(const int *__restrict__ blk_ptr, int num_seeds, const int *__restrict__ first_rank, long long n, int num_v,
                                int *__restrict__ counts)
{
    counts[0] = blk_ptr[num_seeds];
    counts[1] = first_rank ? num_seeds + first_rank[n] : num_v;
}

__global__ __launch_bounds__(256) void k_sample_fill(int *__restrict__ p, long long n, int v)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

struct Sampler {
    const int *d_ptr = nullptr, *d_idx = nullptr;
    int V = 0, E = 0;
    hipStream_t stream = nullptr;
    DevBuf<int> map, cnt, flag, rank, scan_tmp;
    const float *d_w = nullptr;     // gnnagg_sampler_set_weights: borrowed [E], nullptr = uniform sampling
    DevBuf<int> elig;               // [V] eligible edges (w > 0) of every row, of d_w
};

std::mutex g_sampler_mu;
std::set<Sampler *> g_samplers;

Sampler *lookup_sampler(gnnagg_sampler h)
{
    std::lock_guard<std::mutex> lk(g_sampler_mu);
    Sampler *s = reinterpret_cast<Sampler *>(h);
    return g_samplers.count(s) ? s : nullptr;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

int sampler_sample(Sampler *c, const int *d_seeds, int num_seeds, int fanout, unsigned long long seed, int *d_blk_ptr, int *d_blk_idx, int *d_blk_eid,
                   long long cap_e, int *d_src_nodes, int *d_counts)
{
    if (num_seeds < 0) return fail(GNNAGG_ERR_ARG, "sample: num_seeds < 0");
    if (fanout == 0 || fanout < -1) return fail(GNNAGG_ERR_ARG, "sample: fanout must be -1 (every edge) or >= 1");
    if (cap_e < 0) return fail(GNNAGG_ERR_ARG, "sample: cap_e < 0");
    if ((long long)num_seeds + cap_e >= (1ll << 31)) return fail(GNNAGG_ERR_ARG, "sample: num_seeds + cap_e must stay below 2^31");
    if (!d_blk_ptr || !d_counts || (num_seeds > 0 && !d_seeds) || (cap_e > 0 && !d_blk_idx))
        return fail(GNNAGG_ERR_ARG, "sample: null pointer (d_seeds, d_blk_ptr, d_blk_idx, d_counts)");
    const bool relabel = d_src_nodes != nullptr;
    // positions the relabelling passes are launched over (they guard with blk_ptr[num_seeds], read on the device)
    const long long n = fanout > 0 ? std::min<long long>(cap_e, (long long)num_seeds * fanout) : cap_e;
    int rc;
    if ((rc = c->cnt.reserve((size_t)num_seeds + 1))) return rc;
    if (relabel && ((rc = c->flag.reserve((size_t)n + 1)) || (rc = c->rank.reserve((size_t)n + 1)))) return rc;
    const long long m = (long long)num_seeds + n;   // (src_nodes has at most that many entries)
    hipStream_t st = c->stream;
    const unsigned s = sample_seed_mix(seed);

    // (the <true> instantiations under a weight vector; <false> reads neither elig nor w)
    const auto counts = c->d_w ? k_sample_counts<true> : k_sample_counts<false>;
    const auto select = c->d_w ? k_sample_select<true> : k_sample_select<false>;
    hipLaunchKernelGGL(counts, dim3(blocks_of((long long)num_seeds + 1)), dim3(256), 0, st, c->d_ptr, c->V, c->E, d_seeds, num_seeds, fanout, c->cnt.p,
                       c->d_w ? c->elig.p : nullptr);
    if ((rc = prims::scan<prims::OpSum, true>(c->cnt.p, d_blk_ptr, (long)num_seeds + 1, c->scan_tmp, st))) return rc;
    if (num_seeds > 0) {
        const SampleOut out{d_blk_idx, d_blk_eid, cap_e};
        const dim3 grid((unsigned)((num_seeds + kSelBlock - 1) / kSelBlock));
        hipLaunchKernelGGL(select, grid, dim3(kSelBlock), 0, st, c->d_ptr, c->d_idx, c->V, c->E, d_seeds, num_seeds, s, d_blk_ptr, out, c->d_w);
    }
    if (relabel) {
        if (num_seeds > 0)
            hipLaunchKernelGGL(k_sample_mark_seeds, dim3(blocks_of(num_seeds)), dim3(256), 0, st, d_seeds, num_seeds, c->V, c->map.p, d_src_nodes);
        if (n > 0)
            hipLaunchKernelGGL(k_sample_mark_edges, dim3(blocks_of(n)), dim3(256), 0, st, d_blk_ptr, num_seeds, cap_e, d_blk_idx, c->V, c->map.p);
        hipLaunchKernelGGL(k_sample_flags, dim3(blocks_of(n + 1)), dim3(256), 0, st, d_blk_ptr, num_seeds, cap_e, d_blk_idx, c->V, c->map.p, n, c->flag.p);
        if ((rc = prims::scan<prims::OpSum, true>(c->flag.p, c->rank.p, (long)n + 1, c->scan_tmp, st))) return rc;
        if (n > 0)
            hipLaunchKernelGGL(k_sample_relabel, dim3(blocks_of(n)), dim3(256), 0, st, d_blk_ptr, num_seeds, cap_e, d_blk_idx, c->V, c->map.p, c->rank.p,
                               d_src_nodes);
        if (m > 0)
            hipLaunchKernelGGL(k_sample_restore, dim3(blocks_of(m)), dim3(256), 0, st, d_src_nodes, num_seeds, c->rank.p, n, c->V, c->map.p);
    }
    hipLaunchKernelGGL(k_sample_finish, dim3(1), dim3(1), 0, st, d_blk_ptr, num_seeds, relabel ? c->rank.p : nullptr, n, c->V, d_counts);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// the eligible count of every row for the weights d_w, on the sampler's stream; the sampler changes only once everything has succeeded
int sampler_set_weights(Sampler *c, const float *d_w)
{
    if (!d_w) {
        c->d_w = nullptr;   // (elig keeps its room for the next weight vector)
        return GNNAGG_OK;
    }
    DevBuf<int> elig, before, tmp;   // (scratch of num_e + 1 ints, released before the call returns)
    int rc;
    if ((rc = elig.alloc((size_t)c->V)) || (rc = before.alloc((size_t)c->E + 1))) return rc;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_sample_wflags, dim3(blocks_of((long long)c->E + 1)), dim3(256), 0, st, d_w, (long long)c->E, before.p);
    if ((rc = prims::scan<prims::OpSum, true>(before.p, before.p, (long)c->E + 1, tmp, st))) return rc;
    if (c->V > 0) hipLaunchKernelGGL(k_sample_eligible, dim3(blocks_of(c->V)), dim3(256), 0, st, c->d_ptr, c->V, c->E, before.p, elig.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the scratch goes away with this scope, and a sample in flight may still read the old counts)
    c->elig.swap(elig);
    c->d_w = d_w;
    return GNNAGG_OK;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_sampler_create(const int *d_ptr, const int *d_idx, int num_v, int num_e, gnnagg_sampler *out)
{
    if (!out) return fail(GNNAGG_ERR_ARG, "null output handle");
    *out = 0;
    if (num_v < 0 || num_e < 0) return fail(GNNAGG_ERR_ARG, "negative graph size");
    if (!d_ptr || (num_e > 0 && !d_idx)) return fail(GNNAGG_ERR_ARG, "null CSR pointer");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GNNAGG_ERR_HIP, "no HIP device available: libgnnagg has no CPU fallback (gnnagg_sample_block_host is the host sampler)");
    Sampler *c = new Sampler;
    c->d_ptr = d_ptr; c->d_idx = d_idx; c->V = num_v; c->E = num_e;
    int rc = c->map.alloc((size_t)num_v);
    if (!rc && num_v > 0) {
        hipLaunchKernelGGL(k_sample_fill, dim3(blocks_of(num_v)), dim3(256), 0, nullptr, c->map.p, (long long)num_v, kUnseen);
        const hipError_t e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) rc = fail(GNNAGG_ERR_HIP, std::string("sampler map: ") + hipGetErrorString(e));
    }
    if (rc) { delete c; return rc; }
    {
        std::lock_guard<std::mutex> lk(g_sampler_mu);
        g_samplers.insert(c);
    }
    *out = reinterpret_cast<gnnagg_sampler>(c);
    return GNNAGG_OK;
}

int gnnagg_sampler_destroy(gnnagg_sampler h)
{
    Sampler *c;
    {
        std::lock_guard<std::mutex> lk(g_sampler_mu);
        c = reinterpret_cast<Sampler *>(h);
        if (!g_samplers.count(c)) return fail(GNNAGG_ERR_ARG, "invalid or destroyed sampler");
        g_samplers.erase(c);
    }
    (void)hipStreamSynchronize(c->stream);
    delete c;
    return GNNAGG_OK;
}

int gnnagg_sampler_set_stream(gnnagg_sampler h, void *hip_stream)
{
    Sampler *c = lookup_sampler(h);
    if (!c) return fail(GNNAGG_ERR_ARG, "invalid or destroyed sampler");
    c->stream = (hipStream_t)hip_stream;
    return GNNAGG_OK;
}

int gnnagg_sampler_set_weights(gnnagg_sampler h, const float *d_w)
{
    Sampler *c = lookup_sampler(h);
    if (!c) return fail(GNNAGG_ERR_ARG, "invalid or destroyed sampler");
    return sampler_set_weights(c, d_w);
}

int gnnagg_sampler_sample(gnnagg_sampler h, const int *d_seeds, int num_seeds, int fanout, unsigned long long seed, int *d_blk_ptr, int *d_blk_idx,
                          int *d_blk_eid, long long cap_e, int *d_src_nodes, int *d_counts)
{
    Sampler *c = lookup_sampler(h);
    if (!c) return fail(GNNAGG_ERR_ARG, "invalid or destroyed sampler");
    return sampler_sample(c, d_seeds, num_seeds, fanout, seed, d_blk_ptr, d_blk_idx, d_blk_eid, cap_e, d_src_nodes, d_counts);
}

}  // extern "C"
#pragma GCC visibility pop
