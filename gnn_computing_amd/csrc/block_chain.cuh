#pragma once
// block_chain.cuh -- what the kernels over ONE sampled block share (agg_block.hip: the aggregation; agg_block_sage.hip: the aggregation
// with the SAGE combine behind it): the chain over a row's edges through the block's two maps, and the raw copy of a lane's elements.
#include "kernel_util.cuh"

namespace gnnagg {
namespace {

// chain_edges with the two maps of a block: the row of x of edge p is src[idx[p]] (src given) and its weight val[eid[p]] (eid
// given).  Lane j of the group loads idx[p] of its edge of the window and then does the dependent loads; the next window's
// metadata -- maps applied -- is prefetched while this window's gathers and FMAs run.  Ids and weights are broadcast inside the
// group, UNROLL row gathers are issued before the first FMA, lanes with col_ok == false still carry metadata, and no padding
// lane ever multiplies a real source row by zero.  MAPPED = false: neither map, and no test for one.
template <int VEC, int GROUP, bool IS_MAX, bool MAPPED, int UNROLL, typename TX>
__device__ __forceinline__ void chain_block_edges(float (&acc)[VEC], int beg, int end, int lane, bool col_ok,
                                                  const int *__restrict__ idx, const int *__restrict__ src,
                                                  const float *__restrict__ val, const int *__restrict__ eid,
                                                  const TX *__restrict__ xcol, long long pitch)
{
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
    float my_w = 1.0f;
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
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if (j + u < n && col_ok) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        if (IS_MAX) {
                            const float p = xv[u].at(k) * w[u];
                            acc[k] = p > acc[k] ? p : acc[k];
                        } else {
                            acc[k] = __builtin_fmaf(xv[u].at(k), w[u], acc[k]);
                        }
                    }
                }
        }
        my_s = nx_s;
        my_w = nx_w;
    }
}

// a lane's loaded elements back to memory as they are (x_dst; the launch picks lanes no wider than x_dst's alignment)
template <int VEC, typename TX>
__device__ __forceinline__ void store_raw_pack(TX *p, const Pack<VEC, TX> &v)
{
    if constexpr (std::is_same<TX, __bf16>::value) {
        if constexpr (VEC == 8) *reinterpret_cast<uint4 *>(p) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
        else if constexpr (VEC == 4) *reinterpret_cast<uint2 *>(p) = make_uint2(v.w[0], v.w[1]);
        else if constexpr (VEC == 2) *reinterpret_cast<unsigned *>(p) = v.w[0];
        else *reinterpret_cast<unsigned short *>(p) = (unsigned short)v.w[0];
    } else {
        store_pack<VEC>(p, v.v);
    }
}

// the widest lane divides feat AND the pitch of x: every row of x then has the alignment of the first
static long long gcd_ll(long long a, long long b)
{
    while (b) { const long long t = a % b; a = b; b = t; }
    return a;
}

}  // namespace
}  // namespace gnnagg
