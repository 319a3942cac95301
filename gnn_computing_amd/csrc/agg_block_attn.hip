// agg_block_attn.hip -- GATv2 / scaled dot-product attention on ONE sampled block in one launch: gnnagg_block_attn_run (include/gnnagg.h
// section F, "Block attention").
//
//     dot     e_p = scale * q[d(i)] . (k[s(p)] (+ ef[t(p)])) (+ bias[t(p)(, h)]),   y[i] = sum_p softmax_p(e) * (v[s(p)] (+ ef[t(p)]))
//     GATv2   e_p = a[h] . leaky(xd[d(i)] + xs[s(p)] (+ ef[t(p)])) (+ bias[t(p)(, h)]),   y[i] = sum_p softmax_p(e) * xs[s(p)]
//     s(p) = src_nodes ? src_nodes[idx[p]] : idx[p],   d(i) = src_nodes ? src_nodes[i] : i,   t(p) = eid ? eid[p] : p
//
// A handle's attention plan (the segments of long rows, their scratch slots, the merge) is amortised over thousands of runs on a fixed
// graph; a block is used once and its rows hold at most `fanout` edges.  k_block_attn therefore has the short-row path of k_dot_attn /
// k_gatv2 and nothing else: one lane group per destination row over the lane geometry of gatv2_geometry(F, heads, element size),
// block_of<GROUP>() / GROUP rows per workgroup, the block's own CSR for a plan.  No handle, no segment workgroups, no LDS, no scratch,
// no atomics, no second launch: the result is a function of the arguments and the call is capturable.
//
// The walk (block_attn_walk) is the online-softmax frame of dot_walk / gatv2_walk with the arithmetic untouched -- the same batches
// (kGatv2Batch; dot_batch<NF>() for the dot product), at most one guarded rescale per batch, the -inf shift rule, the head reduction
// (segmented xor butterfly or the general masked sum), CSR order -- so a row of at most kGatv2LongEdges edges has the bits of the handle's
// call on the gathered operands.  A LONGER row (fanout = -1 on a hub) is walked by its one lane group too, as in k_block_gcn: it differs
// from the handle's segmented fold in the last bits and is held to the float64 bound of the call instead.
//
// What is new is where the operands come from.  The lane that loads edge p's id for the group's window applies the block's maps there,
// once per edge, as chain_block_edges does (block_chain.cuh): the id goes through src_nodes, the edge position through eid, and a
// per-edge bias is fetched through the mapped position.  The next window's metadata -- maps applied -- is prefetched under this window's
// gathers; ids, positions and biases then travel by group shuffle.  q, k, v, ef and the bias are read where they live: per row and per
// edge of the full graph, never gathered into per-block copies.  The maps are run-time tests on group-uniform pointers.
//
// Arms: none / BIAS / EDGE.  Inside EDGE the bias is a run-time test (has_b), as it is inside the WEIGHTS arm of the handle's kernels.
// The ef rows of a batch are consecutive only without eid; they are read with the plain load of the gathers (gatv2_load), not the
// non-temporal one of gatv2_load_once: through eid the rows are scattered, and nothing was measured for either layout on a block.
// Unaligned bases or pitches keep the geometry and load element by element: same arithmetic, same bits.
#include "gatv2_shared.cuh"

namespace gnnagg {
namespace {

enum { kArmNone = 0, kArmBias = 1, kArmEdge = 2 };

struct BlockAttnArgs {
    const int *ptr, *idx, *src, *eid;
    const void *q, *k, *v, *ef;   // GATv2: q is xd, k is xs (v unused: the summed row is the scored one)
    const float *a, *bias;
    void *y;
    long long q_pitch, kv_pitch, ef_pitch;   // elements between rows
    int num_dst, nblocks, remap, feat, heads, dhead, lph, bias_heads, y_bf16, yvec, x_aligned;
    float scale, slope;
};

// The online-softmax walk of one lane group over edges [beg, end) of its row, into (m, den, acc).  Control flow is uniform over the group.
// qv: the row's q fragments times scale (dot) or its xd fragments (GATv2); av: GATv2's a fragments.
template <bool DOT, int VEC, int GROUP, int NF, typename TX, bool SEGRED, int ARM>
__device__ __forceinline__ void block_attn_walk(const BlockAttnArgs &a, int beg, int end, int lane, const float (&qv)[NF][VEC],
                                                const float (&av)[NF][VEC], const int (&hf)[NF], float (&m)[NF], float (&den)[NF],
                                                float (&acc)[NF][VEC])
{
    constexpr bool BIAS = ARM != kArmNone, EDGE = ARM == kArmEdge;
    constexpr int U = DOT ? dot_batch<NF>() : kGatv2Batch;
    const int F = a.feat;
    const size_t pitch = (size_t)a.kv_pitch;
    const TX *__restrict__ kp = static_cast<const TX *>(a.k) + lane * VEC;
    [[maybe_unused]] const TX *__restrict__ vp = static_cast<const TX *>(a.v) + lane * VEC;
    const int *__restrict__ idx = a.idx;
    const int *__restrict__ src = a.src;
    [[maybe_unused]] const int *__restrict__ eid = a.eid;
    [[maybe_unused]] const float *__restrict__ bias = a.bias;
    [[maybe_unused]] const TX *__restrict__ ef = nullptr;
    [[maybe_unused]] size_t ef_pitch = 0;
    if constexpr (EDGE) {
        ef = static_cast<const TX *>(a.ef) + lane * VEC;
        ef_pitch = (size_t)a.ef_pitch;
    }
    // BIAS, as in the handle's walks: per (edge, head) loaded with the batch's rows, per edge (bias_heads == 1) read as a window beside
    // the ids.  Inside EDGE a null bias is a run-time test and adds nothing: the unbiased bits.
    [[maybe_unused]] const bool has_b = ARM == kArmBias || (EDGE && bias != nullptr);   // (group-uniform)
    [[maybe_unused]] const bool per_edge = has_b && a.bias_heads == 1;                   // (group-uniform)
    // edge p's metadata, maps applied: the row s(p) to gather, the position t(p) of its per-edge operands, its per-edge bias
    auto edge_meta = [&](int p, int &s, int &t, float &b) {
        s = idx[p];
        if (src) s = src[s];
        if constexpr (BIAS) {
            t = eid ? eid[p] : p;
            if (per_edge) b = bias[t];
        }
    };
    int my_s = 0;
    [[maybe_unused]] int my_t = 0;
    [[maybe_unused]] float my_b = 0.0f;
    if (beg + lane < end) edge_meta(beg + lane, my_s, my_t, my_b);
    for (int cb = beg; cb < end; cb += GROUP) {
        int nx_s = 0;
        [[maybe_unused]] int nx_t = 0;
        [[maybe_unused]] float nx_b = 0.0f;
        if (cb + GROUP + lane < end) edge_meta(cb + GROUP + lane, nx_s, nx_t, nx_b);
        const int n = end - cb < GROUP ? end - cb : GROUP;
        for (int j = 0; j < n; j += U) {
            int s[U];
            [[maybe_unused]] int t[U];
            Pack<VEC, TX> kx[U][NF];
            [[maybe_unused]] Pack<VEC, TX> vx[DOT ? U : 1][DOT ? NF : 1];
            float e[U][NF];
            [[maybe_unused]] float bv[U][NF];
            [[maybe_unused]] Pack<VEC, TX> ev[EDGE ? U : 1][EDGE ? NF : 1];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = __shfl(my_s, j + u, GROUP);
            if constexpr (BIAS) {
                if (EDGE || !per_edge) {
#pragma unroll
                    for (int u = 0; u < U; ++u) t[u] = __shfl(my_t, j + u, GROUP);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (j + u < n) {
#pragma unroll
                    for (int f = 0; f < NF; ++f)
                        if ((f * GROUP + lane) * VEC < F) kx[u][f] = gatv2_load<VEC, TX>(kp + (size_t)s[u] * pitch + f * GROUP * VEC, a.x_aligned);
                }
            // dot: the rows to sum, in flight under the score and its reduction
            if constexpr (DOT) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j + u < n) {
#pragma unroll
                        for (int f = 0; f < NF; ++f)
                            if ((f * GROUP + lane) * VEC < F) vx[u][f] = gatv2_load<VEC, TX>(vp + (size_t)s[u] * pitch + f * GROUP * VEC, a.x_aligned);
                    }
            }
            // the batch's edge rows at their mapped positions: behind the gathers, kept packed until the adds
            if constexpr (EDGE) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j + u < n) {
#pragma unroll
                        for (int f = 0; f < NF; ++f)
                            if ((f * GROUP + lane) * VEC < F)
                                ev[u][f] = gatv2_load<VEC, TX>(ef + (size_t)t[u] * ef_pitch + f * GROUP * VEC, a.x_aligned);
                    }
            }
            // the batch's biases, one per (edge, head): in flight with the rows (one per edge: already in the window)
            if constexpr (BIAS) {
                if (has_b && !per_edge) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j + u < n) {
                            const float *__restrict__ bp = bias + (size_t)t[u] * (size_t)a.bias_heads;
#pragma unroll
                            for (int f = 0; f < NF; ++f)
                                if (hf[f] >= 0) bv[u][f] = bp[hf[f]];
                        }
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
                            if constexpr (DOT) {
                                if constexpr (EDGE) p = __builtin_fmaf(qv[f][k], kx[u][f].at(k) + ev[u][f].at(k), p);   // k' = k + ef: one fp32 add
                                else p = __builtin_fmaf(qv[f][k], kx[u][f].at(k), p);
                            } else {
                                float xe = kx[u][f].at(k);
                                if constexpr (EDGE) xe += ev[u][f].at(k);   // (the inner add first; the summed row below is kx alone)
                                const float z = qv[f][k] + xe;
                                const float zs = z * a.slope;
                                p = __builtin_fmaf(av[f][k], z > zs ? z : zs, p);
                            }
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
                        float t2 = 0.0f;
#pragma unroll
                        for (int f = 0; f < NF; ++f) t2 += hf[f] == h ? e[u][f] : 0.0f;
                        t2 = group_sum<GROUP>(t2);
#pragma unroll
                        for (int f = 0; f < NF; ++f)
                            if (hf[f] == h) e[u][f] = t2;   // (a fragment belongs to one head: nothing read later was overwritten)
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
                } else if (has_b) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j + u < n) {
#pragma unroll
                            for (int f = 0; f < NF; ++f)
                                if (hf[f] >= 0) e[u][f] += bv[u][f];
                        }
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
                            if constexpr (!DOT) acc[f][k] = __builtin_fmaf(kx[u][f].at(k), w, acc[f][k]);
                            else if constexpr (EDGE) acc[f][k] = __builtin_fmaf(vx[u][f].at(k) + ev[u][f].at(k), w, acc[f][k]);   // v' = v + ef
                            else acc[f][k] = __builtin_fmaf(vx[u][f].at(k), w, acc[f][k]);
                        }
                    }
            }
        }
        my_s = nx_s;
        if constexpr (BIAS) {
            my_t = nx_t;
            my_b = nx_b;
        }
    }
}

// block_of<GROUP>() / GROUP destination rows per workgroup, one lane group per row, rows of any length
template <bool DOT, int VEC, int GROUP, int NF, typename TX, bool SEGRED, int ARM>
__global__ __launch_bounds__(block_of<GROUP>()) void k_block_attn(const BlockAttnArgs a)
{
    constexpr int GPB = block_of<GROUP>() / GROUP;
    const int F = a.feat;
    const int lane = threadIdx.x & (GROUP - 1);
    const int grp = (int)threadIdx.x / GROUP;
    int b = (int)blockIdx.x;
    if (a.remap) b = xcd_remap(b, a.nblocks);
    const int row = b * GPB + grp;
    if (row >= a.num_dst) return;
    const int beg = a.ptr[row], end = a.ptr[row + 1];
    float qv[NF][VEC], av[NF][VEC], m[NF], den[NF], acc[NF][VEC];
    int hf[NF];
    const bool has_edges = beg < end;
    const TX *__restrict__ q = static_cast<const TX *>(a.q) + lane * VEC;
    if (has_edges) q += (size_t)(a.src ? a.src[row] : row) * (size_t)a.q_pitch;   // d(i): the row's own id goes through the map too
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int col = (f * GROUP + lane) * VEC;
        const bool ok = col < F;
        hf[f] = ok ? col / a.dhead : -1;
        m[f] = -INFINITY;
        den[f] = 0.0f;
        Pack<VEC, TX> qr;
        if (ok && has_edges) qr = gatv2_load<VEC, TX>(q + f * GROUP * VEC, a.x_aligned);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            acc[f][k] = 0.0f;
            if constexpr (DOT) {
                qv[f][k] = ok && has_edges ? qr.at(k) * a.scale : 0.0f;   // the scale goes on q, once per row
                av[f][k] = 0.0f;
            } else {
                qv[f][k] = ok && has_edges ? qr.at(k) : 0.0f;
                av[f][k] = ok && has_edges ? a.a[col + k] : 0.0f;   // a is [heads, D]: element (h, c) sits at column h D + c
            }
        }
    }
    if (has_edges) block_attn_walk<DOT, VEC, GROUP, NF, TX, SEGRED, ARM>(a, beg, end, lane, qv, av, hf, m, den, acc);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int col = (f * GROUP + lane) * VEC;
        if (col >= F) continue;
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = has_edges ? acc[f][k] / den[f] : 0.0f;   // a row without edges: exactly +0
        store_y_typed<VEC>(a.y, a.y_bf16, a.yvec, 0, 0u, (size_t)row * F + col, o);
    }
}

// ------------------------------------------------------------------------------------------------ launch
template <bool DOT, int VEC, int GROUP, int NF, typename TX, bool SEGRED>
static void block_attn_launch_inst(const BlockAttnArgs &a, hipStream_t st)
{
    const dim3 grid((unsigned)a.nblocks), block(block_of<GROUP>());
    if (a.ef) hipLaunchKernelGGL((k_block_attn<DOT, VEC, GROUP, NF, TX, SEGRED, kArmEdge>), grid, block, 0, st, a);
    else if (a.bias) hipLaunchKernelGGL((k_block_attn<DOT, VEC, GROUP, NF, TX, SEGRED, kArmBias>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_block_attn<DOT, VEC, GROUP, NF, TX, SEGRED, kArmNone>), grid, block, 0, st, a);
}

// the geometries of attn_launch_typed (gatv2_shared.cuh): 6 segmented (GROUP, NF) cases and 5 general fragment counts per element type
template <bool DOT, int VEC, typename TX>
static bool block_attn_launch_typed(const BlockAttnArgs &a, const Gatv2Geom &g, hipStream_t st)
{
    if (g.segred) {
        switch (g.group * 10 + g.nf) {
            case 81:  block_attn_launch_inst<DOT, VEC, 8, 1, TX, true>(a, st); return true;
            case 161: block_attn_launch_inst<DOT, VEC, 16, 1, TX, true>(a, st); return true;
            case 321: block_attn_launch_inst<DOT, VEC, 32, 1, TX, true>(a, st); return true;
            case 641: block_attn_launch_inst<DOT, VEC, 64, 1, TX, true>(a, st); return true;
            case 642: block_attn_launch_inst<DOT, VEC, 64, 2, TX, true>(a, st); return true;
            case 644:
                if constexpr (VEC == 4) { block_attn_launch_inst<DOT, VEC, 64, 4, TX, true>(a, st); return true; }   // (bf16: at most 128 lanes)
                break;
        }
    } else {
        switch (g.nf) {
            case 1:  block_attn_launch_inst<DOT, 1, 64, 1, TX, false>(a, st); return true;
            case 2:  block_attn_launch_inst<DOT, 1, 64, 2, TX, false>(a, st); return true;
            case 4:  block_attn_launch_inst<DOT, 1, 64, 4, TX, false>(a, st); return true;
            case 10: block_attn_launch_inst<DOT, 1, 64, 10, TX, false>(a, st); return true;
            case 16: block_attn_launch_inst<DOT, 1, 64, 16, TX, false>(a, st); return true;
        }
    }
    return false;
}

static int block_attn_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const int *eid, int kind, const void *q,
                          long long q_pitch, const void *k, const void *v, long long kv_pitch, const float *av, float slope, float scale,
                          const float *bias, int bias_heads, const void *ef, long long ef_pitch, int x_dtype, void *y, int y_dtype, int feat,
                          int heads, void *stream)
{
    static const char *who = "gnnagg_block_attn_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    auto known = [](int t) { return t == GNNAGG_DTYPE_F32 || t == GNNAGG_DTYPE_BF16; };
    const bool dot = kind == GNNAGG_ATTN_DOT;
    if (num_dst < 0) return bad("num_dst = " + std::to_string(num_dst) + " is negative");
    if (kind != GNNAGG_ATTN_DOT && kind != GNNAGG_ATTN_GATV2)
        return bad("unknown kind " + std::to_string(kind) + ": GNNAGG_ATTN_DOT (0) or GNNAGG_ATTN_GATV2 (1)");
    if (!known(x_dtype)) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (!known(y_dtype)) return bad("unknown y_dtype " + std::to_string(y_dtype));
    if (feat < 1 || heads < 1 || feat % heads != 0)
        return bad("feat = " + std::to_string(feat) + ", heads = " + std::to_string(heads) + ": needs feat >= 1, heads >= 1 and feat % heads == 0");
    if (feat > kGatv2MaxFeat)
        return bad("feat = " + std::to_string(feat) + " is above the kernel's limit of " + std::to_string(kGatv2MaxFeat) + " columns");
    if (q_pitch < feat) return bad("q_pitch = " + std::to_string(q_pitch) + " is below feat = " + std::to_string(feat));
    if (kv_pitch < feat) return bad("kv_pitch = " + std::to_string(kv_pitch) + " is below feat = " + std::to_string(feat));
    if (ef && ef_pitch < feat) return bad("ef_pitch = " + std::to_string(ef_pitch) + " is below feat = " + std::to_string(feat));
    if (dot && !std::isfinite(scale)) return bad("scale = " + std::to_string(scale) + " is not finite");
    if (!dot && !(slope >= 0.0f && slope <= 1.0f))
        return bad("slope = " + std::to_string(slope) + " is outside [0, 1] (the leaky form max(z, z * slope))");
    if (bias && bias_heads != 1 && bias_heads != heads)
        return bad("bias_heads = " + std::to_string(bias_heads) + " is neither 1 nor heads = " + std::to_string(heads));
    if (eid && !bias && !ef) return bad("d_eid needs d_bias or d_ef (d_eid indexes them)");
    if (!dot && v) return bad("d_v is given: GATv2 sums the rows it scores (d_k)");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!q) return bad(dot ? "d_q is null" : "d_q (xd) is null");
        if (!k) return bad(dot ? "d_k is null" : "d_k (xs) is null");
        if (dot && !v) return bad("d_v is null: the dot product sums a second gathered row");
        if (!dot && !av) return bad("d_a is null");
        if (!y) return bad("d_y is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16, y16 = y_dtype == GNNAGG_DTYPE_BF16;
    const int esize = x16 ? 2 : 4;
    Gatv2Geom g;
    if (!gatv2_geometry(feat, heads, esize, g)) return bad("internal: a shape outside the kernel's geometries");
    BlockAttnArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.eid = eid;
    a.q = q; a.k = k; a.v = dot ? v : k; a.ef = ef; a.a = av; a.bias = bias; a.y = y;
    a.q_pitch = q_pitch; a.kv_pitch = kv_pitch; a.ef_pitch = ef ? ef_pitch : 0;
    a.num_dst = num_dst; a.nblocks = ceil_div(num_dst, block_for(g.group) / g.group);
    a.remap = a.nblocks >= 64;   // the rule of the handle's kernels (not re-measured on a block-sized grid; it does not touch the bits)
    a.feat = feat; a.heads = heads; a.dhead = feat / heads; a.lph = g.lph; a.bias_heads = bias ? bias_heads : 1;
    a.y_bf16 = y16; a.yvec = align_class(feat, y, y16 ? 2 : 4, g.vec);
    // (segmented: F * esize is a multiple of 16, so a lane's 16 bytes are aligned exactly when every base and every row pitch is)
    const uintptr_t bases = (uintptr_t)q | (uintptr_t)k | (uintptr_t)a.v | (uintptr_t)ef;
    const long long pitches = q_pitch | kv_pitch | a.ef_pitch;
    a.x_aligned = (bases % 16 == 0 && ((unsigned long long)pitches * esize) % 16 == 0) ? 1 : 0;
    a.scale = scale; a.slope = slope;
    hipStream_t st = (hipStream_t)stream;
    bool ok;
    if (dot) ok = x16 ? block_attn_launch_typed<true, 8, __bf16>(a, g, st) : block_attn_launch_typed<true, 4, float>(a, g, st);
    else     ok = x16 ? block_attn_launch_typed<false, 8, __bf16>(a, g, st) : block_attn_launch_typed<false, 4, float>(a, g, st);
    if (!ok) return fail(GNNAGG_ERR_STATE, std::string(who) + "internal: lane geometry without an instantiation");
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_attn_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const int *d_eid, int kind,
                          const void *d_q, long long q_pitch, const void *d_k, const void *d_v, long long kv_pitch, const float *d_a,
                          float slope, float scale, const float *d_bias, int bias_heads, const void *d_ef, long long ef_pitch, int x_dtype,
                          void *d_y, int y_dtype, int feat, int heads, void *hip_stream)
{
    return block_attn_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_eid, kind, d_q, q_pitch, d_k, d_v, kv_pitch, d_a, slope, scale, d_bias,
                          bias_heads, d_ef, ef_pitch, x_dtype, d_y, y_dtype, feat, heads, hip_stream);
}

}  // extern "C"
#pragma GCC visibility pop
