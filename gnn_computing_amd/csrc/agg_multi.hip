// agg_multi.hip -- multi-aggregation (the aggregation stage of PNA; PyG's MultiAggregation, DGL's PNAConv): sum, mean, min, max, var and
// std of a row's messages from ONE gather of the neighbour rows, times the degree scalers (gnnagg_gcn_run_multi).
//
//     m_p = val[p] * x[idx[p]]      S1 = sum m    S2 = sum m * m    mn = min m    mx = max m            (per column, fp32)
//
// The frame is the attention kernels' (gatv2_shared.cuh; the walk is modelled on dot_walk / k_dot_attn of agg_dot.hip): a lane group per
// row, an id (and value) window shuffled across the group, batches of gathers issued before the first is consumed, the segment
// workgroups of the long rows first in the grid, the fold of a segment's lane groups by group 0 in ascending chunk order through LDS, and
// scratch slots plus a merge kernel for rows of several segments (the plan is gatv2_build_plan's: it needs only ptr).  What differs: no
// heads (multi_geometry: 16-byte lanes where feat is a multiple of the lane's elements, scalar lanes otherwise), nothing to rescale
// (the batch is no part of the arithmetic: multi_batch only bounds the registers in flight), and four accumulators per column of which
// the kernel keeps those the mask needs -- S1 always, S2 for var / std (template S2), mn and mx for min / max (template MM).  The masks
// themselves are kernel arguments: which blocks are stored, and with which scalers, is decided where the finished row is written.
//
// S1 is the plain chain s = s + m in CSR order (contraction off: the multiply that forms m and the add stay two roundings), S2 the FMA
// chain fma(m, m, s).  A block's bits depend on neither template arm nor on the masks: every arm runs the same chain for what it keeps.
#include "gatv2_shared.cuh"

namespace gnnagg {

struct MultiArgs {
    const int *ptr, *idx;
    const float *val;   // null: m = x[idx[p]]
    const int4 *seg;    // {beg, end, row, slot}: slot < 0 = the row's only segment (stored directly)
    const int4 *mrow;   // {row, first slot, end slot, -} per row of several segments
    const void *x;
    void *y;
    float *scratch;     // [n_slots][S1 | S2 | mn | mx][NF * VEC][GROUP]
    long long ypitch;   // S * A * feat: elements between rows of y
    int V, n_seg, n_mrows, nblocks_short, feat, y_bf16, yvec, x_aligned, slot_stride;
    int aggr_mask, scaler_mask, n_aggr;
    float delta;
};

static constexpr int kMultiNeedS2 = GNNAGG_AGGR_VAR | GNNAGG_AGGR_STD, kMultiNeedMM = GNNAGG_AGGR_MIN | GNNAGG_AGGR_MAX;
static constexpr int kMultiAggrBits = 6, kMultiScalerBits = 3;

// gathers in flight per lane group: kGatv2Batch edges, halved where a lane holds kMultiWideNf or more fragments (the scalar geometries of
// wide odd feat: 10 or 16 loads per edge and lane)
static constexpr int kMultiWideNf = 10;
template <int NF>
constexpr int multi_batch() { return NF >= kMultiWideNf ? kGatv2Batch / 2 : kGatv2Batch; }

// The chains of one lane group over edges [beg, end) of its row.  Control flow is uniform over the group.
template <int VEC, int GROUP, int NF, typename TX, bool S2, bool MM>
__device__ __forceinline__ void multi_walk(const MultiArgs &a, int beg, int end, int lane, float (&s1)[NF][VEC], float (&s2)[NF][VEC],
                                           float (&mn)[NF][VEC], float (&mx)[NF][VEC])
{
#pragma clang fp contract(off)
    constexpr int U = multi_batch<NF>();
    const int F = a.feat;
    const TX *__restrict__ xp = static_cast<const TX *>(a.x) + lane * VEC;
    const int *__restrict__ idx = a.idx;
    const float *__restrict__ val = a.val;
    int my_s = 0;
    float my_w = 1.0f;   // (no val: x * 1.0f is x)
    if (beg + lane < end) {
        my_s = idx[beg + lane];
        if (val) my_w = val[beg + lane];
    }
    for (int cb = beg; cb < end; cb += GROUP) {
        int nx_s = 0;
        float nx_w = 1.0f;
        if (cb + GROUP + lane < end) {
            nx_s = idx[cb + GROUP + lane];
            if (val) nx_w = val[cb + GROUP + lane];
        }
        const int n = end - cb < GROUP ? end - cb : GROUP;
        for (int j = 0; j < n; j += U) {
            int s[U];
            float w[U];
            Pack<VEC, TX> xv[U][NF];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = __shfl(my_s, j + u, GROUP);
                w[u] = __shfl(my_w, j + u, GROUP);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (j + u < n) {
#pragma unroll
                    for (int f = 0; f < NF; ++f)
                        if ((f * GROUP + lane) * VEC < F) xv[u][f] = gatv2_load<VEC, TX>(xp + (size_t)s[u] * (size_t)F + f * GROUP * VEC, a.x_aligned);
                }
            // the batch's edges in CSR order
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (j + u < n) {
#pragma unroll
                    for (int f = 0; f < NF; ++f)
                        if ((f * GROUP + lane) * VEC < F) {
#pragma unroll
                            for (int k = 0; k < VEC; ++k) {
                                const float m = w[u] * xv[u][f].at(k);   // the message: ONE fp32 multiply
                                s1[f][k] = s1[f][k] + m;                 // ... and a plain add
                                if constexpr (S2) s2[f][k] = __builtin_fmaf(m, m, s2[f][k]);
                                if constexpr (MM) {
                                    mn[f][k] = m < mn[f][k] ? m : mn[f][k];
                                    mx[f][k] = m > mx[f][k] ? m : mx[f][k];
                                }
                            }
                        }
                }
        }
        my_s = nx_s;
        my_w = nx_w;
    }
}

// A finished row piece (VEC columns from col) into every selected block of y: the aggregates in ascending bit order, each computed once
// and multiplied by the row's scalers (one fp32 scalar each; identity stores the aggregate itself).  deg == 0: +0 everywhere.
// Non-finite messages (gnnagg.h): var and std keep a NaN, min and max of NaN messages alone are NaN, a NaN is stored as the quiet NaN.
template <int VEC>
__device__ __forceinline__ void multi_store_row(const MultiArgs &a, int row, int col, int deg, const float (&s1)[VEC], const float (&s2)[VEC],
                                                const float (&mn)[VEC], const float (&mx)[VEC])
{
#pragma clang fp contract(off)
    const size_t base = (size_t)row * (size_t)a.ypitch + (size_t)col;
    const size_t F = (size_t)a.feat;
    const float dg = (float)deg;
    float amp = 0.0f, att = 0.0f;
    if (deg > 0 && (a.scaler_mask & ~GNNAGG_SCALER_IDENTITY)) {
        const float lg = logf(dg + 1.0f);
        amp = lg / a.delta;
        att = a.delta / lg;
    }
    int ap = 0;
    for (int t = 0; t < kMultiAggrBits; ++t) {
        if (!((a.aggr_mask >> t) & 1)) continue;
        float v[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float r = 0.0f;
            if (deg > 0) {
                if (t == 0) r = s1[k];
                else if (t == 1) r = s1[k] / dg;
                else if (t == 2 || t == 3) {
                    // mn > mx: the seeds, which with deg > 0 only a (row, column) of NaN messages alone keeps (the walk, the folds and the
                    // merge skip NaN and carry the seeds through) -- NaN, never a value no message had
                    r = mn[k] > mx[k] ? __builtin_nanf("") : t == 2 ? mn[k] : mx[k];
                } else {
                    const float mu = s1[k] / dg;
                    const float q = s2[k] / dg;
                    const float d = q - mu * mu;    // the two-moment form, clamped: cancellation may leave it below zero
                    r = d < 0.0f ? 0.0f : d;        // (not fmaxf, which drops a NaN: an Inf or NaN message is a NaN var and std)
                    if (t == 5) r = sqrtf(r);
                }
            }
            // a NaN is stored as THE quiet NaN: which of two NaN operands an add hands on (the sign and payload of x's NaN, or of the one an
            // Inf - Inf made) is the compiler's choice per instantiation, and a block's bits depend on no arm
            v[k] = r != r ? __builtin_nanf("") : r;
        }
        int sp = 0;
        for (int s = 0; s < kMultiScalerBits; ++s) {
            if (!((a.scaler_mask >> s) & 1)) continue;
            float o[VEC];
            const float sc = s == 1 ? amp : att;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o[k] = (s == 0 || deg == 0) ? v[k] : v[k] * sc;
            store_y_typed<VEC>(a.y, a.y_bf16, a.yvec, 0, 0u, base + (size_t)(sp * a.n_aggr + ap) * F, o);
            ++sp;
        }
        ++ap;
    }
}

// One quantity of a segment's lane groups through LDS, folded by group 0 in ascending chunk order (OP 0: sum from +0, 1: min, 2: max);
// group 0 keeps the result.  Every thread of the workgroup calls it.
template <int OP, int VEC, int GROUP, int NF>
__device__ __forceinline__ void multi_fold(float *s_buf, int grp, int lane, float (&v)[NF][VEC])
{
#pragma clang fp contract(off)
    constexpr int GPB = block_of<GROUP>() / GROUP;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int k = 0; k < VEC; ++k) s_buf[((grp * NF + f) * VEC + k) * GROUP + lane] = v[f][k];
    __syncthreads();
    if (grp == 0) {
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float o = OP == 0 ? 0.0f : OP == 1 ? INFINITY : -INFINITY;
                for (int g = 0; g < GPB; ++g) {
                    const float t = s_buf[((g * NF + f) * VEC + k) * GROUP + lane];
                    o = OP == 0 ? o + t : OP == 1 ? (t < o ? t : o) : (t > o ? t : o);
                }
                v[f][k] = o;
            }
    }
    __syncthreads();
}

// Workgroups [0, n_seg): one segment of a long row each.  The others: block_of<GROUP>() / GROUP short rows each, one lane group per row.
template <int VEC, int GROUP, int NF, typename TX, bool S2, bool MM>
__global__ __launch_bounds__(block_of<GROUP>()) void k_multi_aggr(const MultiArgs a)
{
    constexpr int BLOCK = block_of<GROUP>(), GPB = BLOCK / GROUP;
    __shared__ float s_buf[BLOCK * NF * VEC];
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
    float s1[NF][VEC], s2[NF][VEC], mn[NF][VEC], mx[NF][VEC];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            s1[f][k] = 0.0f; s2[f][k] = 0.0f;
            mn[f][k] = INFINITY; mx[f][k] = -INFINITY;
        }
    if (beg < end) multi_walk<VEC, GROUP, NF, TX, S2, MM>(a, beg, end, lane, s1, s2, mn, mx);
    if (!seg_block) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int col = (f * GROUP + lane) * VEC;
            if (col < F) multi_store_row<VEC>(a, row, col, end - beg, s1[f], s2[f], mn[f], mx[f]);
        }
        return;
    }
    // fold of the lane groups' chunks, ascending chunk order, by group 0: one quantity at a time through the one LDS buffer
    multi_fold<0, VEC, GROUP, NF>(s_buf, grp, lane, s1);
    if constexpr (S2) multi_fold<0, VEC, GROUP, NF>(s_buf, grp, lane, s2);
    if constexpr (MM) {
        multi_fold<1, VEC, GROUP, NF>(s_buf, grp, lane, mn);
        multi_fold<2, VEC, GROUP, NF>(s_buf, grp, lane, mx);
    }
    if (grp != 0) return;
    const int deg = a.ptr[row + 1] - a.ptr[row];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int col = (f * GROUP + lane) * VEC;
        if (col >= F) continue;
        if (slot < 0) {
            multi_store_row<VEC>(a, row, col, deg, s1[f], s2[f], mn[f], mx[f]);
        } else {
            float *sl = a.scratch + (size_t)slot * a.slot_stride;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int i = (f * VEC + k) * GROUP + lane;
                sl[i] = s1[f][k];
                if constexpr (S2) sl[NF * VEC * GROUP + i] = s2[f][k];
                if constexpr (MM) {
                    sl[2 * NF * VEC * GROUP + i] = mn[f][k];
                    sl[3 * NF * VEC * GROUP + i] = mx[f][k];
                }
            }
        }
    }
}

// Rows of several segments: one lane group folds the row's slots in ascending order (what the mask needs of them) and stores the row.
template <int VEC, int GROUP, int NF>
__global__ __launch_bounds__(block_of<GROUP>()) void k_multi_merge(const MultiArgs a)
{
#pragma clang fp contract(off)
    constexpr int GPB = block_of<GROUP>() / GROUP, Q = NF * VEC * GROUP;
    const int F = a.feat;
    const int lane = threadIdx.x & (GROUP - 1);
    const int mi = blockIdx.x * GPB + (int)threadIdx.x / GROUP;
    if (mi >= a.n_mrows) return;
    const int4 d = a.mrow[mi];
    const bool need_s2 = (a.aggr_mask & kMultiNeedS2) != 0, need_mm = (a.aggr_mask & kMultiNeedMM) != 0;
    const int deg = a.ptr[d.x + 1] - a.ptr[d.x];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int col = (f * GROUP + lane) * VEC;
        if (col >= F) continue;
        float s1[VEC], s2[VEC], mn[VEC], mx[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            s1[k] = 0.0f; s2[k] = 0.0f;
            mn[k] = INFINITY; mx[k] = -INFINITY;
        }
        for (int s = d.y; s < d.z; ++s) {
            const float *sl = a.scratch + (size_t)s * a.slot_stride;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int i = (f * VEC + k) * GROUP + lane;
                s1[k] = s1[k] + sl[i];
                if (need_s2) s2[k] = s2[k] + sl[Q + i];
                if (need_mm) {
                    const float lo = sl[2 * Q + i], hi = sl[3 * Q + i];
                    mn[k] = lo < mn[k] ? lo : mn[k];
                    mx[k] = hi > mx[k] ? hi : mx[k];
                }
            }
        }
        multi_store_row<VEC>(a, d.x, col, deg, s1, s2, mn, mx);
    }
}

// ------------------------------------------------------------------------------------------------ geometry
// 16-byte lanes (4 fp32 / 8 bf16 elements) where feat is a multiple of them, scalar lanes otherwise; 8 to 64 lanes per row, and the
// fragments per lane rounded up to an instantiated count.
struct MultiGeom {
    int vec, group, nf;
};

static bool multi_geometry(int F, int esize, MultiGeom &g)
{
    if (F < 1 || F > kGatv2MaxFeat) return false;
    int vec = 16 / esize;
    if (F % vec != 0) vec = 1;
    const int lanes = F / vec;
    int group = 8;
    while (group < 64 && group < lanes) group <<= 1;
    const int nf = (lanes + group - 1) / group;
    g = {vec, group, nf <= 1 ? 1 : nf <= 2 ? 2 : nf <= 4 ? 4 : nf <= 10 ? 10 : 16};   // (F <= 1024: at most 16 fragments of 64 scalar lanes)
    return true;
}

size_t multi_aggr_slot_floats(int feat, int x_dtype)
{
    MultiGeom g;
    if (!multi_geometry(feat, x_dtype == GNNAGG_DTYPE_BF16 ? 2 : 4, g)) return 0;
    return (size_t)4 * g.nf * g.vec * g.group;
}

// ------------------------------------------------------------------------------------------------ launch
// One lane geometry: the arm of the walk that keeps what the mask needs, and the merge behind it.
template <int VEC, int GROUP, int NF, typename TX>
static int multi_launch_inst(const MultiArgs &a, hipStream_t stream)
{
    constexpr int BLOCK = block_of<GROUP>(), GPB = BLOCK / GROUP;
    const bool s2 = (a.aggr_mask & kMultiNeedS2) != 0, mm = (a.aggr_mask & kMultiNeedMM) != 0;
    const int grid = a.n_seg + a.nblocks_short;
    if (grid > 0) {
        if (s2 && mm) hipLaunchKernelGGL((k_multi_aggr<VEC, GROUP, NF, TX, true, true>), dim3(grid), dim3(BLOCK), 0, stream, a);
        else if (s2) hipLaunchKernelGGL((k_multi_aggr<VEC, GROUP, NF, TX, true, false>), dim3(grid), dim3(BLOCK), 0, stream, a);
        else if (mm) hipLaunchKernelGGL((k_multi_aggr<VEC, GROUP, NF, TX, false, true>), dim3(grid), dim3(BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((k_multi_aggr<VEC, GROUP, NF, TX, false, false>), dim3(grid), dim3(BLOCK), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (a.n_mrows > 0) {
        hipLaunchKernelGGL((k_multi_merge<VEC, GROUP, NF>), dim3(ceil_div(a.n_mrows, GPB)), dim3(BLOCK), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return GNNAGG_OK;
}

// The instantiations per element type, by (16-byte lanes ? 10000 : 0) + GROUP * 100 + NF: 8 scalar and 6 packed geometries (VECW: the
// elements of a 16-byte lane of TX).
template <int VECW, typename TX>
static int multi_launch_typed(MultiArgs &a, const MultiGeom &g, hipStream_t stream)
{
    a.nblocks_short = ceil_div(a.V, block_for(g.group) / g.group);
    switch ((g.vec > 1 ? 10000 : 0) + g.group * 100 + g.nf) {
        case 801:   return multi_launch_inst<1, 8, 1, TX>(a, stream);
        case 1601:  return multi_launch_inst<1, 16, 1, TX>(a, stream);
        case 3201:  return multi_launch_inst<1, 32, 1, TX>(a, stream);
        case 6401:  return multi_launch_inst<1, 64, 1, TX>(a, stream);
        case 6402:  return multi_launch_inst<1, 64, 2, TX>(a, stream);
        case 6404:  return multi_launch_inst<1, 64, 4, TX>(a, stream);
        case 6410:  return multi_launch_inst<1, 64, 10, TX>(a, stream);
        case 6416:  return multi_launch_inst<1, 64, 16, TX>(a, stream);
        case 10801: return multi_launch_inst<VECW, 8, 1, TX>(a, stream);
        case 11601: return multi_launch_inst<VECW, 16, 1, TX>(a, stream);
        case 13201: return multi_launch_inst<VECW, 32, 1, TX>(a, stream);
        case 16401: return multi_launch_inst<VECW, 64, 1, TX>(a, stream);
        case 16402: return multi_launch_inst<VECW, 64, 2, TX>(a, stream);
        case 16404:
            if constexpr (VECW == 4) return multi_launch_inst<VECW, 64, 4, TX>(a, stream);   // (bf16: at most 128 lanes)
            break;
    }
    return fail(GNNAGG_ERR_STATE, "internal: multi-aggregation lane geometry without an instantiation");
}

int launch_multi_aggr(const MultiAggrLaunch &L, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    const int esize = L.x_dtype == GNNAGG_DTYPE_BF16 ? 2 : 4, ysize = L.y_dtype == GNNAGG_DTYPE_BF16 ? 2 : 4;
    MultiGeom g;
    if (!multi_geometry(L.feat, esize, g)) return fail(GNNAGG_ERR_ARG, "internal: multi-aggregation launch outside the kernel's shapes");
    if (L.V <= 0) return GNNAGG_OK;
    MultiArgs a;
    a.ptr = L.ptr; a.idx = L.idx; a.val = L.val;
    a.seg = reinterpret_cast<const int4 *>(L.seg); a.mrow = reinterpret_cast<const int4 *>(L.mrow);
    a.x = L.x; a.y = L.y; a.scratch = L.scratch;
    a.V = L.V; a.n_seg = L.n_seg; a.n_mrows = L.n_mrows; a.nblocks_short = 0; a.feat = L.feat;
    a.aggr_mask = L.aggr_mask; a.scaler_mask = L.scaler_mask; a.delta = L.delta;
    a.n_aggr = __builtin_popcount((unsigned)L.aggr_mask);
    a.ypitch = (long long)a.n_aggr * __builtin_popcount((unsigned)L.scaler_mask) * L.feat;
    a.y_bf16 = L.y_dtype == GNNAGG_DTYPE_BF16 ? 1 : 0;
    // (rows of y are S * A * feat elements apart and a block starts at a multiple of feat: both keep the class of (feat, y))
    a.yvec = align_class(L.feat, L.y, ysize, g.vec);
    // (plain stores: write-through ones, which serve the one-block y of k_gcn_plan, measured no faster here -- profiles/multi_aggr/store_ab.jsonl)
    // (packed lanes: feat * esize is a multiple of 16, so a lane's 16 bytes are aligned exactly when the base is)
    a.x_aligned = (uintptr_t)L.x % 16 == 0 ? 1 : 0;
    a.slot_stride = 4 * g.nf * g.vec * g.group;
    if (L.x_dtype == GNNAGG_DTYPE_BF16) return multi_launch_typed<8, __bf16>(a, g, stream);
    return multi_launch_typed<4, float>(a, g, stream);
}

}  // namespace gnnagg
