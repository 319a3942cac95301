// gat_project.hip -- the GAT attention terms from a finished projection (gnnagg_gat_project, path 2):
//   att[r, h, 0] = sum_c feat[r, h D + c] . a_dst[h, c],   att[r, h, 1] = the same with a_src,   feat[M, heads . D] fp32 or bf16 AS STORED.
// Row-major feat[M, heads . D] is feat[M . heads, D] and att is [M . heads, 2]: one "unit" per (row, head), D contiguous elements each.
//  * A unit is read by a group of 2^j lanes (j = 0 .. 6: the smallest group whose lanes cover D in one pass, 64 lanes at most, then
//    in passes), VEC elements per lane and pass.  VEC = the widest of 8, 4, 2, 1 (16 bytes at most) that divides D and that the addresses
//    of feat, a_dst and a_src allow, so a lane's load lies inside one head and nothing behind an operand is read.
//  * Products and sums are fp32: a lane adds its products in ascending column order, the group adds up by an xor butterfly (a fixed
//    association: the same bits on every call), lane 0 of the group stores the pair.
//  * Units are dealt to consecutive groups: the lanes of a wavefront read one contiguous piece of feat.  The kernel is a single pass over
//    feat from memory (or from the L2 / MALL the GEMM in front of it has just filled); a_dst / a_src stay in cache.
#include "kernel_util.cuh"

namespace gnnagg {
namespace {

template <class T>
__device__ __forceinline__ float widen(T v);
template <>
__device__ __forceinline__ float widen<float>(float v) { return v; }
template <>
__device__ __forceinline__ float widen<__bf16>(__bf16 v) { return (float)v; }

template <class T, int VEC>
struct __attribute__((aligned(sizeof(T) * VEC))) Pack { T e[VEC]; };

template <class FT, class AT, int VEC>
__global__ __launch_bounds__(256) void k_gat_rowdot(const FT *__restrict__ feat, const AT *__restrict__ a_dst, const AT *__restrict__ a_src,
                                                    float *__restrict__ att, long units, int heads, int D, int group)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long unit = g / group;
    const int l = (int)(g - unit * group);
    float sd = 0.0f, ss = 0.0f;
    if (unit < units) {
        const int head = (int)(unit % heads);
        const FT *f = feat + (size_t)unit * D;
        const AT *ad = a_dst + (size_t)head * D, *as = a_src + (size_t)head * D;
        for (int c = l * VEC; c < D; c += group * VEC) {   // D % VEC == 0: c + VEC <= D
            const Pack<FT, VEC> fv = *reinterpret_cast<const Pack<FT, VEC> *>(f + c);
            const Pack<AT, VEC> dv = *reinterpret_cast<const Pack<AT, VEC> *>(ad + c), sv = *reinterpret_cast<const Pack<AT, VEC> *>(as + c);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float x = widen<FT>(fv.e[j]);
                sd += x * widen<AT>(dv.e[j]);
                ss += x * widen<AT>(sv.e[j]);
            }
        }
    }
    for (int m = group >> 1; m > 0; m >>= 1) {   // every lane of the wavefront takes part; groups are aligned to their size
        sd += __shfl_xor(sd, m, 64);
        ss += __shfl_xor(ss, m, 64);
    }
    if (unit < units && l == 0) {
        att[(size_t)unit * 2] = sd;
        att[(size_t)unit * 2 + 1] = ss;
    }
}

template <class FT, class AT>
int call_rowdot(const void *feat, const void *a_dst, const void *a_src, float *att, long units, int heads, int D, hipStream_t stream)
{
    constexpr int maxvec = 16 / (int)sizeof(FT);
    int vec = align_class(D, feat, (int)sizeof(FT), maxvec);
    vec = std::min(vec, std::min(align_class(D, a_dst, (int)sizeof(AT), maxvec), align_class(D, a_src, (int)sizeof(AT), maxvec)));
    int group = 1;
    while (group < 64 && group * vec < D) group <<= 1;
    const long lanes = units * group;
    const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
    const FT *f = static_cast<const FT *>(feat);
    const AT *ad = static_cast<const AT *>(a_dst), *as = static_cast<const AT *>(a_src);
    switch (vec) {
        case 8:
            if constexpr (maxvec >= 8) { hipLaunchKernelGGL((k_gat_rowdot<FT, AT, 8>), grid, block, 0, stream, f, ad, as, att, units, heads, D, group); break; }
        case 4: hipLaunchKernelGGL((k_gat_rowdot<FT, AT, 4>), grid, block, 0, stream, f, ad, as, att, units, heads, D, group); break;
        case 2: hipLaunchKernelGGL((k_gat_rowdot<FT, AT, 2>), grid, block, 0, stream, f, ad, as, att, units, heads, D, group); break;
        default: hipLaunchKernelGGL((k_gat_rowdot<FT, AT, 1>), grid, block, 0, stream, f, ad, as, att, units, heads, D, group); break;
    }
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

}  // namespace

// att[M, heads, 2] from feat[M, N] (fp32, or bf16 with feat_bf16) and a_dst / a_src[heads, N / heads] (fp32, or bf16 with a_bf16; a bf16 feat
// comes with bf16 a).  M, N > 0, N % heads == 0.
int launch_gat_rowdot(const void *feat, int feat_bf16, const void *a_dst, const void *a_src, int a_bf16, float *att, int M, int N, int heads,
                      void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    const long units = (long)M * heads;
    const int D = N / heads;
    if (units * 64 / 256 + 1 > 0x7fffffffL) return fail(GNNAGG_ERR_ARG, "gnnagg_gat_project: m . heads beyond the grid of the row-dot kernel");
    if (feat_bf16) {
        if (!a_bf16) return fail(GNNAGG_ERR_STATE, "internal: a bf16 feat with fp32 attention vectors");
        return call_rowdot<__bf16, __bf16>(feat, a_dst, a_src, att, units, heads, D, stream);
    }
    if (a_bf16) return call_rowdot<float, __bf16>(feat, a_dst, a_src, att, units, heads, D, stream);
    return call_rowdot<float, float>(feat, a_dst, a_src, att, units, heads, D, stream);
}

}  // namespace gnnagg
