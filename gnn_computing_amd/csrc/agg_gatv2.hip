// agg_gatv2.hip -- GATv2 ("dynamic attention"): edge score, online edge softmax and weighted aggregation in one pass over the gathered rows.
//
//     e_j = sum_c a[h, c] * leaky(xd[r, hD + c] + xs[j, hD + c]),   y[r] = sum_j softmax_j(e_j) * xs[j]          (gnnagg_gatv2_run)
//
// The score needs the gathered source row itself (the non-linearity sits inside the dot product), so the softmax runs ONLINE: every lane
// keeps a running (m, den, acc) per column fragment and one gather feeds both the score and the sum.
//
// Geometry (gatv2_geometry: a function of (F, heads, element size) only, never of a pointer):
//   * segmented: D * elemsize is a multiple of 16 bytes and a head spans a power-of-two number (<= 64) of 16-byte lanes.  A lane group of
//     8 .. 64 lanes covers the row, NF = 1, 2 or 4 fragments per lane when F / VEC > 64; the per-head reduction is an xor butterfly over the
//     head's lanes (every lane of the head ends with the same bits).
//   * general: any other (heads, D).  One-element lanes, 64-lane groups, NF = ceil(F / 64) fragments per lane; one masked 64-lane
//     reduction per head.  Slower, and covers heads narrower than a lane and D that no lane width divides.
// Where X is not 16-byte aligned the segmented geometry stays and a lane loads its elements one by one: same arithmetic, same bits.
//
// Order of a row (DESIGN.md "GATv2"): edges in CSR order in batches of kGatv2Batch.  Per batch and fragment: the scores; if the batch
// maximum exceeds m, ONE rescale of (den, acc) by expf(m - new m) (skipped as 0 while m = -inf: no inf - inf); then, edge by edge,
// w = expf(e - m), den += w, acc = fma(x, w, acc) -- with 0 for m while m is still -inf, so that a -inf score (a masked edge) is a
// weight of +0 wherever it stands and an all-masked chunk leaves (-inf, 0, 0) (gnnagg.h "non-finite").
// Rows above kGatv2LongEdges edges are cut into segments of kGatv2SegEdges edges, one workgroup each: its lane groups walk contiguous
// chunks, and group 0 folds the (m, den, acc) triples through LDS in ascending chunk order (M = max m; den = sum den_g * expf(m_g - M)).
// A row of several segments leaves one triple per segment in scratch and k_gatv2_merge folds them the same way, ascending.  No atomics;
// the same bits on every call.
//
// Score bias (gnnagg_gatv2_run_bias; the BIAS arm of gatv2_walk / k_gatv2, chosen in attn_launch_inst (gatv2_shared.cuh) from
// a.bias != nullptr): one fp32 per edge position, or per (edge position, head), added to the finished score -- after the head's reduction,
// before the batch maximum.  A -inf bias is a masked edge by the rules above.  BIAS = false is the kernel without the operand, instruction
// for instruction.
//
// Weights out (gnnagg_gatv2_run_weights; the WEIGHTS arm, on top of BIAS, chosen in attn_launch_inst from a.alpha != nullptr): the finished
// score of every (edge, head) is stored raw to alpha[p, h] by the lane and fragment that start the head, and the row's final (maximum,
// denominator) to stat[row, h] from wherever the row is finished -- the short-row store, group 0 after the LDS fold, k_gatv2_merge.
// launch_attn_finish (aux_kernels.hip), behind this launch on the same stream, makes weights of the scores.  y is computed as without.
//
// Edge features (gnnagg_gatv2_run_edge; k_gatv2_edge, the EDGE arm of gatv2_walk / k_gatv2): a row ef[p] of F elements per edge POSITION,
// added to the gathered row inside the score only -- z = xd + (xs[j] + ef[p]), the inner add first -- while the summed row stays xs[j].
// The rows of a batch are consecutive (p = cb + j + u): a lane reads its fragments of them with the loads of the gather, behind the gathers,
// and keeps them packed (TX) until the add.  EDGE = false is k_gatv2, instruction for instruction.
#include "gatv2_shared.cuh"

namespace gnnagg {

struct Gatv2EdgeArgs : Gatv2Args {   // what the merge and the store read is the base
    const void *ef;                  // [num_e, feat] elements of the operands' type, row p at p * ef_pitch
    long long ef_pitch;
};

// The online-softmax walk of one lane group over edges [beg, end) of its row, into (m, den, acc).  Control flow is uniform over the group.
template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS, bool EDGE = false, typename ARGS = Gatv2Args>
__device__ __forceinline__ void gatv2_walk(const ARGS &a, int beg, int end, int lane, const float (&xdv)[NF][VEC],
                                           const float (&av)[NF][VEC], const int (&hf)[NF], float (&m)[NF], float (&den)[NF],
                                           float (&acc)[NF][VEC])
{
    constexpr int U = kGatv2Batch;
    const int F = a.feat;
    const TX *__restrict__ xs = static_cast<const TX *>(a.xs) + lane * VEC;
    const int *__restrict__ idx = a.idx;
    [[maybe_unused]] const TX *__restrict__ ef = nullptr;
    [[maybe_unused]] size_t ef_pitch = 0;
    if constexpr (EDGE) {
        ef = static_cast<const TX *>(a.ef) + lane * VEC;
        ef_pitch = (size_t)a.ef_pitch;
    }
    // BIAS.  bias_heads == heads: the value of (edge, hf[f]) is loaded per (edge, fragment) with the batch's rows.
    // bias_heads == 1: one value per edge, so the group reads a window of GROUP values beside its ids and shuffles them out (my_b, nx_b).
    // WEIGHTS (BIAS arm only, one instantiation for both): a null bias runs as a per-edge bias of +0.0 that is never loaded -- the unbiased
    // bits (gnnagg.h "no bias").  has_b is a constant without WEIGHTS: the BIAS arm alone is the kernel it was.
    [[maybe_unused]] const bool has_b = !WEIGHTS || a.bias != nullptr;             // (group-uniform)
    [[maybe_unused]] const bool per_edge = BIAS && (a.bias_heads == 1 || !has_b);   // (group-uniform)
    [[maybe_unused]] float my_b = 0.0f;
    if constexpr (BIAS) {
        if (per_edge && has_b && beg + lane < end) my_b = a.bias[beg + lane];
    }
    int my_s = 0;
    if (beg + lane < end) my_s = idx[beg + lane];
    for (int cb = beg; cb < end; cb += GROUP) {
        int nx_s = 0;
        if (cb + GROUP + lane < end) nx_s = idx[cb + GROUP + lane];
        [[maybe_unused]] float nx_b = 0.0f;
        if constexpr (BIAS) {
            if (per_edge && has_b && cb + GROUP + lane < end) nx_b = a.bias[cb + GROUP + lane];
        }
        const int n = end - cb < GROUP ? end - cb : GROUP;
        for (int j = 0; j < n; j += U) {
            int s[U];
            Pack<VEC, TX> xv[U][NF];
            float e[U][NF];
            [[maybe_unused]] float bv[U][NF];
            [[maybe_unused]] Pack<VEC, TX> ev[EDGE ? U : 1][EDGE ? NF : 1];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = __shfl(my_s, j + u, GROUP);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (j + u < n) {
#pragma unroll
                    for (int f = 0; f < NF; ++f)
                        if ((f * GROUP + lane) * VEC < F) xv[u][f] = gatv2_load<VEC, TX>(xs + (size_t)s[u] * F + f * GROUP * VEC, a.x_aligned);
                }
            // the batch's edge rows, consecutive in memory and read once: behind the gathers, kept packed until the add
            if constexpr (EDGE) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j + u < n) {
#pragma unroll
                        for (int f = 0; f < NF; ++f)
                            if ((f * GROUP + lane) * VEC < F)
                                ev[u][f] = gatv2_load_once<VEC, TX>(ef + (size_t)(cb + j + u) * ef_pitch + f * GROUP * VEC, a.x_aligned);
                    }
            }
            // the batch's biases, one per (edge, head): in flight with the rows (one per edge: already in the window)
            if constexpr (BIAS) {
                if (!per_edge) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j + u < n) gatv2_load_bias<NF>(a, cb + j + u, hf, bv[u]);
                }
            }
            // this lane's part of every score
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    float p = 0.0f;
                    if (j + u < n && (f * GROUP + lane) * VEC < F) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) {
                            float xe = xv[u][f].at(k);
                            if constexpr (EDGE) xe += ev[u][f].at(k);   // (the inner add first; the summed row below is xv alone)
                            const float z = xdv[f][k] + xe;
                            const float zs = z * a.slope;
                            p = __builtin_fmaf(av[f][k], z > zs ? z : zs, p);
                        }
                    }
                    e[u][f] = p;
                }
            // ... summed over the lanes (and fragments) of its head
            if constexpr (SEGRED) {
                const int lph = a.lph;
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int f = 0; f < NF; ++f) {
                        float v = e[u][f];
                        if (lph > 1) v += __shfl_xor(v, 1, GROUP);
                        if (lph > 2) v += __shfl_xor(v, 2, GROUP);
                        if (lph > 4) v += __shfl_xor(v, 4, GROUP);
                        if constexpr (GROUP > 8) { if (lph > 8) v += __shfl_xor(v, 8, GROUP); }
                        if constexpr (GROUP > 16) { if (lph > 16) v += __shfl_xor(v, 16, GROUP); }
                        if constexpr (GROUP > 32) { if (lph > 32) v += __shfl_xor(v, 32, GROUP); }
                        e[u][f] = v;
                    }
            } else {
                for (int h = 0; h < a.heads; ++h) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float t = 0.0f;
#pragma unroll
                        for (int f = 0; f < NF; ++f) t += hf[f] == h ? e[u][f] : 0.0f;
                        t = group_sum<GROUP>(t);
#pragma unroll
                        for (int f = 0; f < NF; ++f)
                            if (hf[f] == h) e[u][f] = t;   // (a fragment belongs to one head: nothing read later was overwritten)
                    }
                }
            }
            // the bias: one fp32 add to the finished score (-inf: a masked edge)
            if constexpr (BIAS) {
                if (per_edge) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j + u < n) {
                            const float b = __shfl(my_b, j + u, GROUP);
#pragma unroll
                            for (int f = 0; f < NF; ++f)
                                if (hf[f] >= 0) e[u][f] += b;
                        }
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j + u < n) {
#pragma unroll
                            for (int f = 0; f < NF; ++f)
                                if (hf[f] >= 0) e[u][f] += bv[u][f];
                        }
                }
            }
            // WEIGHTS: the finished score of every (edge, head), raw, from the one lane and fragment that starts the head (idle fragments
            // have hf = -1); launch_attn_finish turns it into the weight once the row's (maximum, denominator) are final
            if constexpr (WEIGHTS) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j + u < n) {
#pragma unroll
                        for (int f = 0; f < NF; ++f)
                            if (gatv2_head_owner(a, (f * GROUP + lane) * VEC, hf[f]))
                                a.alpha[(size_t)(cb + j + u) * (size_t)a.heads + (size_t)hf[f]] = e[u][f];
                    }
            }
            // online softmax: at most one rescale per batch, then the batch's edges in CSR order
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                if ((f * GROUP + lane) * VEC >= F) continue;
                float bm = e[0][f];
#pragma unroll
                for (int u = 1; u < U; ++u)
                    if (j + u < n) bm = fmaxf(bm, e[u][f]);
                if (bm > m[f]) {
                    const float sc = m[f] == -INFINITY ? 0.0f : expf(m[f] - bm);   // first batch: nothing to rescale, and no -inf - -inf
                    den[f] *= sc;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[f][k] *= sc;
                    m[f] = bm;
                }
                // m still -inf: every score so far was -inf (or NaN).  The shift is then 0, not m: expf(-inf - 0) is the weight +0 of a
                // masked edge where -inf - -inf would be NaN.  Any other m is the shift itself: finite rows keep their bits.
                const float ms = m[f] == -INFINITY ? 0.0f : m[f];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j + u < n) {
                        const float w = expf(e[u][f] - ms);
                        den[f] += w;
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[f][k] = __builtin_fmaf(xv[u][f].at(k), w, acc[f][k]);
                    }
            }
        }
        my_s = nx_s;
        if constexpr (BIAS) my_b = nx_b;
    }
}

// Workgroups [0, n_seg): one segment of a long row each.  The others: block_of<GROUP>() / GROUP short rows each, one lane group per row.
// (k_gatv2: EDGE = false; k_gatv2_edge: EDGE = true)
template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS = false, bool EDGE = false, typename ARGS = Gatv2Args>
__global__ __launch_bounds__(block_of<GROUP>()) void k_gatv2(const ARGS a)
{
    constexpr int BLOCK = block_of<GROUP>(), GPB = BLOCK / GROUP;
    __shared__ float s_m[BLOCK * NF], s_den[BLOCK * NF], s_acc[BLOCK * NF * VEC];
    const int F = a.feat;
    const int lane = threadIdx.x & (GROUP - 1);
    const int grp = (int)threadIdx.x / GROUP;
    const bool seg_block = (int)blockIdx.x < a.n_seg;   // workgroup-uniform
    int beg, end, row, slot = -1;
    if (seg_block) {
        const int4 d = a.seg[blockIdx.x];
        row = d.z; slot = d.w;
        int chunk = (d.y - d.x + GPB - 1) / GPB;
        chunk = (chunk + kGatv2Batch - 1) / kGatv2Batch * kGatv2Batch;
        beg = d.x + grp * chunk < d.y ? d.x + grp * chunk : d.y;
        end = beg + chunk < d.y ? beg + chunk : d.y;
    } else {
        int b = (int)blockIdx.x - a.n_seg;
        if (a.nblocks_short >= 64) b = xcd_remap(b, a.nblocks_short);
        row = b * GPB + grp;
        if (row >= a.V) return;
        beg = a.ptr[row]; end = a.ptr[row + 1];
        if (end - beg > kGatv2LongEdges) return;   // a long row: the segment workgroups' work
    }
    float xdv[NF][VEC], av[NF][VEC], m[NF], den[NF], acc[NF][VEC];
    int hf[NF];
    const TX *__restrict__ xd = static_cast<const TX *>(a.xd) + (size_t)row * F + lane * VEC;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int col = (f * GROUP + lane) * VEC;
        const bool ok = col < F;
        hf[f] = ok ? col / a.dhead : -1;
        m[f] = -INFINITY;
        den[f] = 0.0f;
        Pack<VEC, TX> xr;
        if (ok && beg < end) xr = gatv2_load<VEC, TX>(xd + f * GROUP * VEC, a.x_aligned);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            acc[f][k] = 0.0f;
            xdv[f][k] = ok && beg < end ? xr.at(k) : 0.0f;
            av[f][k] = ok ? a.a[col + k] : 0.0f;   // a is [heads, D]: element (h, c) sits at column h D + c
        }
    }
    if (beg < end) gatv2_walk<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS, EDGE, ARGS>(a, beg, end, lane, xdv, av, hf, m, den, acc);
    if (!seg_block) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int col = (f * GROUP + lane) * VEC;
            if (col < F) gatv2_store<VEC>(a, (size_t)row * F + col, acc[f], den[f], beg < end);
            if constexpr (WEIGHTS) {
                if (gatv2_head_owner(a, col, hf[f])) gatv2_store_stat(a, row, hf[f], m[f], den[f]);   // (no edges: (-inf, +0) as initialised)
            }
        }
        return;
    }
    // fold of the lane groups' triples, ascending chunk order, by group 0
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int i = (grp * NF + f) * GROUP + lane;
        s_m[i] = m[f];
        s_den[i] = den[f];
#pragma unroll
        for (int k = 0; k < VEC; ++k) s_acc[i * VEC + k] = acc[f][k];
    }
    __syncthreads();
    if (grp != 0) return;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int col = (f * GROUP + lane) * VEC;
        if (col >= F) continue;
        float M = -INFINITY;
        for (int g = 0; g < GPB; ++g) M = fmaxf(M, s_m[(g * NF + f) * GROUP + lane]);
        float d = 0.0f, o[VEC] = {};
        for (int g = 0; g < GPB; ++g) {
            const int i = (g * NF + f) * GROUP + lane;
            const float mg = s_m[i];
            const float sc = mg == -INFINITY ? 0.0f : expf(mg - M);   // a chunk without edges, or all masked (M = -inf too)
            d = __builtin_fmaf(s_den[i], sc, d);
#pragma unroll
            for (int k = 0; k < VEC; ++k) o[k] = __builtin_fmaf(s_acc[i * VEC + k], sc, o[k]);
        }
        if (slot < 0) {
            gatv2_store<VEC>(a, (size_t)row * F + col, o, d, true);
            if constexpr (WEIGHTS) {
                if (gatv2_head_owner(a, col, hf[f])) gatv2_store_stat(a, row, hf[f], M, d);
            }
        } else {
            float *sl = a.scratch + (size_t)slot * a.slot_stride;
            const int i = f * GROUP + lane;
            sl[i] = M;
            sl[NF * GROUP + i] = d;
#pragma unroll
            for (int k = 0; k < VEC; ++k) sl[2 * NF * GROUP + i * VEC + k] = o[k];
        }
    }
}

struct Gatv2Kernel {   // names the kernel for the launch switches (gatv2_shared.cuh)
    template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS>
    static constexpr auto get() { return &k_gatv2<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>; }
};

// k_gatv2_edge<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>: the kernel with the EDGE arm, a sibling instantiation of the same template (a
// wrapper around a shared body would reorder the instructions of k_gatv2; as a defaulted parameter it leaves them as they were)
template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS>
constexpr auto k_gatv2_edge = &k_gatv2<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS, true, Gatv2EdgeArgs>;

struct Gatv2EdgeKernel {
    template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS>
    static constexpr auto get() { return k_gatv2_edge<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>; }
};

// ------------------------------------------------------------------------------------------------ geometry and launch
size_t gatv2_slot_floats(int feat, int heads, int x_dtype)
{
    Gatv2Geom g;
    if (!gatv2_geometry(feat, heads, x_dtype == GNNAGG_DTYPE_BF16 ? 2 : 4, g)) return 0;
    return (size_t)g.nf * g.group * (g.vec + 2);
}

int launch_gatv2(const Gatv2Launch &L, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    Gatv2Geom g;
    if (!gatv2_geometry(L.feat, L.heads, L.x_dtype == GNNAGG_DTYPE_BF16 ? 2 : 4, g))
        return fail(GNNAGG_ERR_ARG, "internal: GATv2 launch outside the kernel's shapes");
    if (L.V <= 0) return GNNAGG_OK;
    constexpr const char *no_inst = "internal: GATv2 lane geometry without an instantiation";
    if (L.ef) {   // the edge call: the alignment flag also covers the ef base and its row pitch
        const int esize = L.x_dtype == GNNAGG_DTYPE_BF16 ? 2 : 4;
        Gatv2EdgeArgs a;
        attn_fill_args(a, L, g);
        a.xs = L.xs; a.xd = L.xd; a.a = L.a;
        a.x_aligned = ((uintptr_t)L.xs % 16 == 0 && (uintptr_t)L.xd % 16 == 0 && (uintptr_t)L.ef % 16 == 0 && (L.ef_pitch * esize) % 16 == 0) ? 1 : 0;
        a.slope = L.slope;
        a.ef = L.ef; a.ef_pitch = L.ef_pitch;
        if (L.x_dtype == GNNAGG_DTYPE_BF16) return attn_launch_typed<Gatv2EdgeKernel, 8, __bf16>(a, g, stream, no_inst);
        return attn_launch_typed<Gatv2EdgeKernel, 4, float>(a, g, stream, no_inst);
    }
    Gatv2Args a;
    attn_fill_args(a, L, g);
    a.xs = L.xs; a.xd = L.xd; a.a = L.a;
    a.x_aligned = ((uintptr_t)L.xs % 16 == 0 && (uintptr_t)L.xd % 16 == 0) ? 1 : 0;   // (segmented: F * esize is a multiple of 16)
    a.slope = L.slope;
    if (L.x_dtype == GNNAGG_DTYPE_BF16) return attn_launch_typed<Gatv2Kernel, 8, __bf16>(a, g, stream, no_inst);
    return attn_launch_typed<Gatv2Kernel, 4, float>(a, g, stream, no_inst);
}

}  // namespace gnnagg
