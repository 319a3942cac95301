// gatv2_shared.cuh -- what the two online-softmax attention kernels share (agg_gatv2.hip: GATv2; agg_dot.hip: scaled dot-product): the kernel
// arguments, the row-fragment load and the typed store, the lane geometry, the ordered merge of a long row's segments, and the launch: the
// common members of the arguments (attn_fill_args) and the one pair of dispatch switches both kernels are launched through
// (attn_launch_inst: none / BIAS / BIAS + WEIGHTS and the merge; attn_launch_typed: the lane geometries).
#pragma once
#include "kernel_util.cuh"

namespace gnnagg {

struct Gatv2Args {
    const int *ptr, *idx;
    const int4 *seg;    // {beg, end, row, slot}: slot < 0 = the row's only segment (stored directly)
    const int4 *mrow;   // {row, first slot, end slot, -} per row of several segments
    const void *xs, *xd;
    const float *a;
    void *y;
    float *scratch;     // [n_slots][m: NF * GROUP | den: NF * GROUP | acc: NF * GROUP * VEC]
    int V, n_seg, n_mrows, nblocks_short, feat, heads, dhead, lph, y_bf16, yvec, x_aligned, slot_stride;
    float slope;
    const float *bias;  // [num_e, bias_heads] fp32 added to the scores, or null (the BIAS arm of the walks runs exactly when it is not)
    int bias_heads;     // 1 (one value per edge serves every head) or heads
    float *alpha;       // [num_e, heads] the finished scores go here raw (the WEIGHTS arm of the walks runs exactly when it is not null) ...
    float *stat;        // ... with [V, heads, 2] = every (row, head)'s final (maximum, denominator); launch_attn_finish makes weights of them
};

// Whether fragment f of this lane starts its head (column hf * dhead): the one lane that stores the head's score and (m, den)
__device__ __forceinline__ bool gatv2_head_owner(const Gatv2Args &a, int col, int hf) { return hf >= 0 && col == hf * a.dhead; }

// (row, head)'s final pair, as it stands (not a log-sum-exp: gnnagg.h "weights")
__device__ __forceinline__ void gatv2_store_stat(const Gatv2Args &a, int row, int h, float m, float den)
{
    float *st = a.stat + ((size_t)row * (size_t)a.heads + (size_t)h) * 2;
    st[0] = m;
    st[1] = den;
}

// The bias of edge p for the head of each of this lane's fragments, bias_heads == heads (hf[f]: the fragment's head, -1 past F: nothing is
// loaded).  A direct per-lane load: the lanes of a head share the address, the heads of an edge and the edges of a batch are consecutive
// floats.  (bias_heads == 1 is read by the walks as a window of one value per lane, like the ids.)
template <int NF>
__device__ __forceinline__ void gatv2_load_bias(const Gatv2Args &a, int p, const int (&hf)[NF], float (&b)[NF])
{
    const float *__restrict__ bp = a.bias + (size_t)p * (size_t)a.bias_heads;
#pragma unroll
    for (int f = 0; f < NF; ++f)
        if (hf[f] >= 0) b[f] = bp[hf[f]];
}

// VEC elements of a row at p: one 16-byte (or narrower) load, or element by element where the row is not aligned for it
template <int VEC, typename TX>
__device__ __forceinline__ Pack<VEC, TX> gatv2_load(const TX *p, int aligned)
{
    if constexpr (VEC == 1) {
        return load_pack<1, TX>(p);
    } else {
        if (aligned) return load_pack<VEC, TX>(p);
        Pack<VEC, TX> r;
        if constexpr (std::is_same<TX, __bf16>::value) {
            const unsigned short *q = reinterpret_cast<const unsigned short *>(p);
#pragma unroll
            for (int k = 0; k < VEC / 2; ++k) r.w[k] = (unsigned)q[2 * k] | ((unsigned)q[2 * k + 1] << 16);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) r.v[k] = p[k];
        }
        return r;
    }
}

// gatv2_load for the per-edge feature rows (the EDGE arm of the walks): a stream read once, in order, beside gathered rows that are
// re-read and mostly cache hits.  The aligned 16-byte load is marked non-temporal: 13 - 40 us faster at fp32 and for the bf16 dot-product,
// even for bf16 GATv2 (profiles/attn_edge/nontemporal_ab.jsonl).  Same bytes as the plain load it was measured against
// (scripts/attic/ab_switches_retired.patch has the switch): the bits do not depend on it.
template <int VEC, typename TX>
__device__ __forceinline__ Pack<VEC, TX> gatv2_load_once(const TX *p, int aligned)
{
    if constexpr (VEC * sizeof(TX) == 16) {
        if (aligned) {
            typedef unsigned u4 __attribute__((ext_vector_type(4)));
            const u4 t = __builtin_nontemporal_load(reinterpret_cast<const u4 *>(p));
            Pack<VEC, TX> r;
            __builtin_memcpy(&r, &t, 16);
            return r;
        }
    }
    return gatv2_load<VEC, TX>(p, aligned);
}

// acc / den of a finished row piece, stored in Y's type
template <int VEC>
__device__ __forceinline__ void gatv2_store(const Gatv2Args &a, size_t off, const float (&acc)[VEC], float den, bool has_edges)
{
    float o[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) o[k] = has_edges ? acc[k] / den : 0.0f;
    store_y_typed<VEC>(a.y, a.y_bf16, a.yvec, 0, 0u, off, o);
}

// Rows of several segments: one lane group folds the row's triples in ascending slot order.
template <int VEC, int GROUP, int NF, bool WEIGHTS = false>
__global__ __launch_bounds__(block_of<GROUP>()) void k_gatv2_merge(const Gatv2Args a)
{
    constexpr int GPB = block_of<GROUP>() / GROUP;
    const int F = a.feat;
    const int lane = threadIdx.x & (GROUP - 1);
    const int mi = blockIdx.x * GPB + (int)threadIdx.x / GROUP;
    if (mi >= a.n_mrows) return;
    const int4 d = a.mrow[mi];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int col = (f * GROUP + lane) * VEC;
        if (col >= F) continue;
        const int i = f * GROUP + lane;
        float M = -INFINITY;
        for (int s = d.y; s < d.z; ++s) M = fmaxf(M, a.scratch[(size_t)s * a.slot_stride + i]);
        float dn = 0.0f, o[VEC] = {};
        for (int s = d.y; s < d.z; ++s) {
            const float *sl = a.scratch + (size_t)s * a.slot_stride;
            // (every segment has edges: its m is a score, or -inf with den = acc = 0.  A row masked whole has M = -inf too and NaN factors:
            // y is NaN either way, but the WEIGHTS form owes (-inf, +0) to stat and takes the factor 0 of the LDS fold)
            const float sc = WEIGHTS && sl[i] == -INFINITY ? 0.0f : expf(sl[i] - M);
            dn = __builtin_fmaf(sl[NF * GROUP + i], sc, dn);
#pragma unroll
            for (int k = 0; k < VEC; ++k) o[k] = __builtin_fmaf(sl[2 * NF * GROUP + i * VEC + k], sc, o[k]);
        }
        gatv2_store<VEC>(a, (size_t)d.x * F + col, o, dn, true);
        if constexpr (WEIGHTS) {
            if (gatv2_head_owner(a, col, col / a.dhead)) gatv2_store_stat(a, d.x, col / a.dhead, M, dn);
        }
    }
}

struct Gatv2Geom {
    int vec, group, nf, lph;
    bool segred;
};

static bool gatv2_geometry(int F, int heads, int esize, Gatv2Geom &g)
{
    if (F < 1 || heads < 1 || F % heads != 0 || F > kGatv2MaxFeat) return false;
    const int D = F / heads, vec = 16 / esize;
    if (D % vec == 0) {
        const int lph = D / vec;
        if ((lph & (lph - 1)) == 0 && lph <= 64) {
            const int lanes = F / vec;
            int group = 8;
            while (group < 64 && group < lanes) group <<= 1;
            const int nf = (lanes + group - 1) / group;
            g = {vec, group, nf <= 1 ? 1 : nf <= 2 ? 2 : 4, lph, true};   // (F <= 1024: at most 256 16-byte lanes)
            return true;
        }
    }
    const int nf = (F + 63) / 64;
    g = {1, 64, nf <= 1 ? 1 : nf <= 2 ? 2 : nf <= 4 ? 4 : nf <= 10 ? 10 : 16, 0, false};
    return true;
}

// ------------------------------------------------------------------------------------------------ launch
// The members of Gatv2Args that both attentions fill alike from the common part of their launch structs (common.h: AttnLaunch); the
// operands (xs, xd, a, slope, x_aligned, and what a derived argument struct adds) are the entry point's own.
static void attn_fill_args(Gatv2Args &a, const AttnLaunch &L, const Gatv2Geom &g)
{
    a.ptr = L.ptr; a.idx = L.idx; a.seg = reinterpret_cast<const int4 *>(L.seg); a.mrow = reinterpret_cast<const int4 *>(L.mrow);
    a.y = L.y; a.scratch = L.scratch;
    a.V = L.V; a.n_seg = L.n_seg; a.n_mrows = L.n_mrows; a.nblocks_short = 0; a.feat = L.feat; a.heads = L.heads; a.dhead = L.feat / L.heads;
    a.lph = g.lph; a.y_bf16 = L.y_dtype == GNNAGG_DTYPE_BF16 ? 1 : 0;
    a.yvec = align_class(L.feat, L.y, L.y_dtype == GNNAGG_DTYPE_BF16 ? 2 : 4, g.vec);
    a.slot_stride = g.nf * g.group * (g.vec + 2);
    a.bias = L.bias; a.bias_heads = L.bias_heads;
    a.alpha = L.alpha; a.stat = L.stat;
}

// One lane geometry of kernel K (a struct whose get<...>() names the __global__ function: Gatv2Kernel, DotKernel) and the merge behind it.
template <typename K, int VEC, int GROUP, int NF, typename TX, bool SEGRED, typename ARGS>
static int attn_launch_inst(const ARGS &a, hipStream_t stream)
{
    constexpr int BLOCK = block_of<GROUP>(), GPB = BLOCK / GROUP;
    const int grid = a.n_seg + a.nblocks_short;
    if (grid > 0) {
        // the BIAS arm only where there is a bias: a call without one launches the kernel it always launched
        // ... and the WEIGHTS arm only where the scores are asked for: ONE more instantiation, with or without a bias (the walks: has_b)
        if (a.alpha) hipLaunchKernelGGL((K::template get<VEC, GROUP, NF, TX, SEGRED, true, true>()), dim3(grid), dim3(BLOCK), 0, stream, a);
        else if (a.bias) hipLaunchKernelGGL((K::template get<VEC, GROUP, NF, TX, SEGRED, true, false>()), dim3(grid), dim3(BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((K::template get<VEC, GROUP, NF, TX, SEGRED, false, false>()), dim3(grid), dim3(BLOCK), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (a.n_mrows > 0) {
        const Gatv2Args &base = a;   // (what the merge and the store read is the base)
        if (a.alpha) hipLaunchKernelGGL((k_gatv2_merge<VEC, GROUP, NF, true>), dim3(ceil_div(a.n_mrows, GPB)), dim3(BLOCK), 0, stream, base);
        else hipLaunchKernelGGL((k_gatv2_merge<VEC, GROUP, NF>), dim3(ceil_div(a.n_mrows, GPB)), dim3(BLOCK), 0, stream, base);
        HIP_TRY(hipGetLastError());
    }
    return GNNAGG_OK;
}

// The instantiations: 6 segmented (GROUP, NF) cases and 5 general fragment counts per element type (no_inst: the caller's message for a
// geometry outside them, which gatv2_geometry never returns).
template <typename K, int VEC, typename TX, typename ARGS>
static int attn_launch_typed(ARGS &a, const Gatv2Geom &g, hipStream_t stream, const char *no_inst)
{
    a.nblocks_short = ceil_div(a.V, block_for(g.group) / g.group);
    if (g.segred) {
        switch (g.group * 10 + g.nf) {
            case 81:  return attn_launch_inst<K, VEC, 8, 1, TX, true>(a, stream);
            case 161: return attn_launch_inst<K, VEC, 16, 1, TX, true>(a, stream);
            case 321: return attn_launch_inst<K, VEC, 32, 1, TX, true>(a, stream);
            case 641: return attn_launch_inst<K, VEC, 64, 1, TX, true>(a, stream);
            case 642: return attn_launch_inst<K, VEC, 64, 2, TX, true>(a, stream);
            case 644:
                if constexpr (VEC == 4) return attn_launch_inst<K, VEC, 64, 4, TX, true>(a, stream);   // (bf16: at most 128 lanes)
                break;
        }
    } else {
        switch (g.nf) {
            case 1:  return attn_launch_inst<K, 1, 64, 1, TX, false>(a, stream);
            case 2:  return attn_launch_inst<K, 1, 64, 2, TX, false>(a, stream);
            case 4:  return attn_launch_inst<K, 1, 64, 4, TX, false>(a, stream);
            case 10: return attn_launch_inst<K, 1, 64, 10, TX, false>(a, stream);
            case 16: return attn_launch_inst<K, 1, 64, 16, TX, false>(a, stream);
        }
    }
    return fail(GNNAGG_ERR_STATE, no_inst);
}

}  // namespace gnnagg
