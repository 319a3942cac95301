// agg_dot.hip -- scaled dot-product attention over a graph's edges (graph-transformer attention): score, online edge softmax and weighted
// aggregation in one pass over two gathered rows per edge.
//
//     e_j = scale * sum_c q[r, hD + c] * k[j, hD + c],   y[r] = sum_j softmax_j(e_j) * v[j]          (gnnagg_dot_attn_run)
//
// A sibling of k_gatv2 (agg_gatv2.hip) on the same frame (gatv2_shared.cuh): the lane geometry of (F, heads, element size), the batches
// of edges with one guarded rescale, the segments of long rows folded in ascending order through LDS and, for rows of several segments,
// through scratch by k_gatv2_merge.  What differs is the walk: a lane group keeps its row's q fragments in registers, MULTIPLIED BY scale
// ONCE (so the score is the fp32 FMA chain over (scale * q) and k; a power-of-two scale commutes with every rounding), and every batch
// gathers the k fragments (scored) and the v fragments (summed) of its edges; the v loads are issued before the score reduction.
//
// Batch (dot_batch): kGatv2Batch edges, halved where a lane holds 2 or more fragments -- a batch holds k AND v fragments, twice GATv2's
// gather registers; measured against batches of 4 and of 1 (DESIGN.md "Dot-product attention", profiles/dot_attn/batch_ab.jsonl).
//
// q rows are q_pitch elements apart, k and v rows kv_pitch: column views of one [n, 3F] projection serve as the three operands.  Where a
// pointer or a pitch is not 16-byte aligned the geometry stays and a lane loads its elements one by one: same arithmetic, same bits.
//
// Score bias (gnnagg_dot_attn_run_bias): the BIAS arm of dot_walk / k_dot_attn, as in agg_gatv2.hip -- one fp32 add to the finished score.
// Weights out (gnnagg_dot_attn_run_weights): the WEIGHTS arm, as in agg_gatv2.hip -- raw scores to alpha, (maximum, denominator) to stat.
// Edge features (gnnagg_dot_attn_run_edge; k_dot_attn_edge, the EDGE arm of dot_walk / k_dot_attn): a row ef[p] per edge POSITION, added to
// the gathered k row where it is scored and to the gathered v row where it is summed -- one fp32 add each, at the point of use; the rows
// of a batch are consecutive and read once, packed, behind the gathers.  The batch stays dot_batch (the edge call owes the bits of
// k_dot_attn on the expanded graph, and the batches are part of the arithmetic).
#include "gatv2_shared.cuh"

namespace gnnagg {

struct DotArgs : Gatv2Args {   // q is xd, k is xs (a and slope are unused); what the merge and the store read is the base
    const void *v;
    long long q_pitch, kv_pitch;
    float scale;
};

// the batch of the geometries with kDotWideNf or more fragments per lane
static constexpr int kDotWideBatch = kGatv2Batch / 2;
static constexpr int kDotWideNf = 2;
template <int NF>
constexpr int dot_batch() { return NF >= kDotWideNf ? kDotWideBatch : kGatv2Batch; }
static_assert(kGatv2Batch % dot_batch<kDotWideNf>() == 0, "a segment's chunks are cut at multiples of kGatv2Batch");

struct DotEdgeArgs : DotArgs {
    const void *ef;   // [num_e, feat] elements of the operands' type, row p at p * ef_pitch
    long long ef_pitch;
};

// The online-softmax walk of one lane group over edges [beg, end) of its row, into (m, den, acc).  Control flow is uniform over the group.
// (EDGE keeps dot_batch: the batches are part of the arithmetic, and the edge call owes the bits of k_dot_attn on the expanded graph)
template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS, bool EDGE = false, typename ARGS = DotArgs>
__device__ __forceinline__ void dot_walk(const ARGS &a, int beg, int end, int lane, const float (&qv)[NF][VEC], const int (&hf)[NF],
                                         float (&m)[NF], float (&den)[NF], float (&acc)[NF][VEC])
{
    constexpr int U = dot_batch<NF>();
    const int F = a.feat;
    const size_t pitch = (size_t)a.kv_pitch;
    const TX *__restrict__ kp = static_cast<const TX *>(a.xs) + lane * VEC;
    const TX *__restrict__ vp = static_cast<const TX *>(a.v) + lane * VEC;
    const int *__restrict__ idx = a.idx;
    [[maybe_unused]] const TX *__restrict__ ef = nullptr;
    [[maybe_unused]] size_t ef_pitch = 0;
    if constexpr (EDGE) {
        ef = static_cast<const TX *>(a.ef) + lane * VEC;
        ef_pitch = (size_t)a.ef_pitch;
    }
    // BIAS, as in gatv2_walk: per (edge, head) loaded with the batch's rows, per edge (bias_heads == 1) read as a window beside the ids
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
            Pack<VEC, TX> kx[U][NF], vx[U][NF];
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
                        if ((f * GROUP + lane) * VEC < F) kx[u][f] = gatv2_load<VEC, TX>(kp + (size_t)s[u] * pitch + f * GROUP * VEC, a.x_aligned);
                }
            // the rows to sum: in flight under the score and its reduction
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (j + u < n) {
#pragma unroll
                    for (int f = 0; f < NF; ++f)
                        if ((f * GROUP + lane) * VEC < F) vx[u][f] = gatv2_load<VEC, TX>(vp + (size_t)s[u] * pitch + f * GROUP * VEC, a.x_aligned);
                }
            // the batch's edge rows, consecutive in memory and read once: behind the gathers, kept packed until the adds
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
                            if constexpr (EDGE) p = __builtin_fmaf(qv[f][k], kx[u][f].at(k) + ev[u][f].at(k), p);   // k' = k + ef: one fp32 add
                            else p = __builtin_fmaf(qv[f][k], kx[u][f].at(k), p);
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
                        for (int k = 0; k < VEC; ++k) {
                            if constexpr (EDGE) acc[f][k] = __builtin_fmaf(vx[u][f].at(k) + ev[u][f].at(k), w, acc[f][k]);   // v' = v + ef
                            else acc[f][k] = __builtin_fmaf(vx[u][f].at(k), w, acc[f][k]);
                        }
                    }
            }
        }
        my_s = nx_s;
        if constexpr (BIAS) my_b = nx_b;
    }
}

// Workgroups [0, n_seg): one segment of a long row each.  The others: block_of<GROUP>() / GROUP short rows each, one lane group per row.
// (k_dot_attn: EDGE = false; k_dot_attn_edge: EDGE = true)
template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS = false, bool EDGE = false, typename ARGS = DotArgs>
__global__ __launch_bounds__(block_of<GROUP>()) void k_dot_attn(const ARGS a)
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
    float qv[NF][VEC], m[NF], den[NF], acc[NF][VEC];
    int hf[NF];
    const TX *__restrict__ q = static_cast<const TX *>(a.xd) + (size_t)row * (size_t)a.q_pitch + lane * VEC;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int col = (f * GROUP + lane) * VEC;
        const bool ok = col < F;
        hf[f] = ok ? col / a.dhead : -1;
        m[f] = -INFINITY;
        den[f] = 0.0f;
        Pack<VEC, TX> qr;
        if (ok && beg < end) qr = gatv2_load<VEC, TX>(q + f * GROUP * VEC, a.x_aligned);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            acc[f][k] = 0.0f;
            qv[f][k] = ok && beg < end ? qr.at(k) * a.scale : 0.0f;   // the scale goes on q, once per row
        }
    }
    if (beg < end) dot_walk<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS, EDGE, ARGS>(a, beg, end, lane, qv, hf, m, den, acc);
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

struct DotKernel {   // names the kernel for the launch switches (gatv2_shared.cuh)
    template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS>
    static constexpr auto get() { return &k_dot_attn<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>; }
};

// k_dot_attn_edge<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>: the kernel with the EDGE arm, a sibling instantiation of the same template (a
// wrapper around a shared body would reorder the instructions of k_dot_attn; as a defaulted parameter it leaves them as they were)
template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS>
constexpr auto k_dot_attn_edge = &k_dot_attn<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS, true, DotEdgeArgs>;

struct DotEdgeKernel {
    template <int VEC, int GROUP, int NF, typename TX, bool SEGRED, bool BIAS, bool WEIGHTS>
    static constexpr auto get() { return k_dot_attn_edge<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>; }
};

// ------------------------------------------------------------------------------------------------ launch
int launch_dot_attn(const DotAttnLaunch &L, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    const int esize = L.x_dtype == GNNAGG_DTYPE_BF16 ? 2 : 4;
    Gatv2Geom g;
    if (!gatv2_geometry(L.feat, L.heads, esize, g)) return fail(GNNAGG_ERR_ARG, "internal: dot-product attention launch outside the kernel's shapes");
    if (L.V <= 0) return GNNAGG_OK;
    constexpr const char *no_inst = "internal: dot-product attention lane geometry without an instantiation";
    if (L.ef) {   // the edge call: the alignment flag also covers the ef base and its row pitch
        DotEdgeArgs a;
        attn_fill_args(a, L, g);
        a.xs = L.k; a.xd = L.q; a.a = nullptr;
        a.x_aligned = ((uintptr_t)L.q % 16 == 0 && (uintptr_t)L.k % 16 == 0 && (uintptr_t)L.v % 16 == 0 && (uintptr_t)L.ef % 16 == 0 &&
                       (L.q_pitch * esize) % 16 == 0 && (L.kv_pitch * esize) % 16 == 0 && (L.ef_pitch * esize) % 16 == 0) ? 1 : 0;
        a.slope = 0.0f;
        a.v = L.v; a.q_pitch = L.q_pitch; a.kv_pitch = L.kv_pitch; a.scale = L.scale;
        a.ef = L.ef; a.ef_pitch = L.ef_pitch;
        if (L.x_dtype == GNNAGG_DTYPE_BF16) return attn_launch_typed<DotEdgeKernel, 8, __bf16>(a, g, stream, no_inst);
        return attn_launch_typed<DotEdgeKernel, 4, float>(a, g, stream, no_inst);
    }
    DotArgs a;
    attn_fill_args(a, L, g);
    a.xs = L.k; a.xd = L.q; a.a = nullptr;
    // (segmented: F * esize is a multiple of 16, so a lane's 16 bytes are aligned exactly when the base and the row pitch are)
    a.x_aligned = ((uintptr_t)L.q % 16 == 0 && (uintptr_t)L.k % 16 == 0 && (uintptr_t)L.v % 16 == 0 && (L.q_pitch * esize) % 16 == 0 &&
                   (L.kv_pitch * esize) % 16 == 0) ? 1 : 0;
    a.slope = 0.0f;
    a.v = L.v; a.q_pitch = L.q_pitch; a.kv_pitch = L.kv_pitch; a.scale = L.scale;
    if (L.x_dtype == GNNAGG_DTYPE_BF16) return attn_launch_typed<DotKernel, 8, __bf16>(a, g, stream, no_inst);
    return attn_launch_typed<DotKernel, 4, float>(a, g, stream, no_inst);
}

}  // namespace gnnagg
