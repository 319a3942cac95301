// aux_kernels.hip -- everything beside the two aggregation families: CSR -> edge list, the unfused edge-softmax stages,
// the edge-wise and naive SpMM baselines, validators, the CSR check, the halo pack, the column-tiled images of the 2-D blocked mode, the
// zero fill and the row-gather probe.  (The dense combine GEMMs have files of their own: dense_f32.hip, dense_bf16.hip.)
#include "kernel_util.cuh"

namespace gnnagg {

// ------------------------------------------------------------------------- CSR -> edge list
// A lane group strides over the edges of one row; group size follows the average degree so short
// rows do not idle a whole wavefront.
static int edge_group(int avg_deg)
{
    int g = 8;
    while (g < 64 && g < avg_deg) g <<= 1;
    return g;
}


// reference convertCSRToEdgelist, aggregator.h:11-23 ((src,dst) written as one 8-byte store)
template <int GROUP>
__global__ __launch_bounds__(kBlock) void k_csr2edgelist(const int *__restrict__ ptr, const int *__restrict__ idx,
                                                        int2 *__restrict__ edgelist, int V)
{
    const int row = blockIdx.x * (kBlock / GROUP) + threadIdx.x / GROUP;
    const int lane = threadIdx.x & (GROUP - 1);
    if (row >= V) return;
    for (int e = ptr[row] + lane; e < ptr[row + 1]; e += GROUP) edgelist[e] = make_int2(idx[e], row);
}

#define DISPATCH_EDGE_GROUP(G, CALL)                      \
    switch (G) {                                          \
        case 8:  { constexpr int GROUP = 8;  CALL; } break;  \
        case 16: { constexpr int GROUP = 16; CALL; } break;  \
        case 32: { constexpr int GROUP = 32; CALL; } break;  \
        default: { constexpr int GROUP = 64; CALL; } break;  \
    }

int launch_csr2edgelist(const int *ptr, const int *idx, int *edgelist, int V, int avg_deg, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    if (V <= 0) return GNNAGG_OK;
    const int G = edge_group(avg_deg);
    const int nb = ceil_div(V, kBlock / G);
    DISPATCH_EDGE_GROUP(G, hipLaunchKernelGGL((k_csr2edgelist<GROUP>), dim3(nb), dim3(kBlock), 0, stream, ptr, idx,
                                              reinterpret_cast<int2 *>(edgelist), V))
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// ------------------------------------------------- edge kernels on chunked work items (hub-safe)
// Giving one lane group a whole row (the reference's warp-per-row attGat / u_add_v / add_to_center / each_div,
// aggr_gat.h:5-92) serialises on a 15 k-edge hub row: 860 us for attGat on the arxiv-shaped graph in the first
// version of this file.  These kernels run on the work items of the balanced
// neighbor grouping (<= chunk edges each): pass 1 writes the edge values and per-item sums (straight to
// den[row] when the row has one item, to partial_den[slot] otherwise), an ordered combine finishes the
// split rows, pass 2 normalises.  Lanes walk the flattened (edge, head) pairs of an item, so out[e,h]
// stores are fully coalesced and a lane keeps one head when GROUP % H == 0.
struct EdgeItemArgs {
    const int *ptr_s, *target, *slot, *empty_rows, *idx;
    const float *att;   // [V,H,2]
    const float *in;    // per-edge input (add_to_center) / per-row divisor (div)
    float *out;         // per-edge output [E,H]
    float *den;         // per-row sums [V,H]
    float *partial_den; // [n_slots,H]
    int n_items, n_empty, H;
    float slope;
};

// OP 0: attGat pass 1 (w = exp(leaky(a_dst + a_src)) -> out, item sums)   aggr_gat.h:13-19
// OP 1: add_to_center (item sums of in[e])                                 aggr_gat.h:62-73
template <int GROUP, int OP>
__global__ __launch_bounds__(kBlock) void k_edge_items_sum(const EdgeItemArgs a)
{
    const int item = blockIdx.x * (kBlock / GROUP) + (int)threadIdx.x / GROUP;
    const int lane = threadIdx.x & (GROUP - 1);
    const int H = a.H;
    if (item >= a.n_items + a.n_empty) return;
    if (item >= a.n_items) {  // rows without edges: sum = 0
        const int row = a.empty_rows[item - a.n_items];
        for (int h = lane; h < H; h += GROUP) a.den[(size_t)row * H + h] = 0.0f;
        return;
    }
    const int beg = a.ptr_s[item], end = a.ptr_s[item + 1];
    const int row = a.target[item];
    const int sl = a.slot[item];
    float *dst = sl >= 0 ? a.partial_den + (size_t)sl * H : a.den + (size_t)row * H;
    const int n = (end - beg) * H;
    if (H <= GROUP && (GROUP % H) == 0) {
        const int h = lane % H;  // fixed head per lane: the stride GROUP is a multiple of H
        const float a_dst = OP == 0 ? a.att[((size_t)row * H + h) * 2] : 0.0f;
        float part = 0.0f;
        for (int j = lane; j < n; j += GROUP) {
            const int e = beg + j / H;
            float w;
            if (OP == 0) {
                w = edge_weight(a_dst, a.att[((size_t)a.idx[e] * H + h) * 2 + 1], a.slope);
                a.out[(size_t)beg * H + j] = w;
            } else {
                w = a.in[(size_t)beg * H + j];
            }
            part += w;
        }
        for (int msk = GROUP / 2; msk >= H; msk >>= 1) part += __shfl_xor(part, msk, GROUP);
        if (lane < H) dst[lane] = part;
    } else {
        for (int h = 0; h < H; ++h) {  // odd head counts: one head at a time
            const float a_dst = OP == 0 ? a.att[((size_t)row * H + h) * 2] : 0.0f;
            float part = 0.0f;
            for (int e = beg + lane; e < end; e += GROUP) {
                float w;
                if (OP == 0) {
                    w = edge_weight(a_dst, a.att[((size_t)a.idx[e] * H + h) * 2 + 1], a.slope);
                    a.out[(size_t)e * H + h] = w;
                } else {
                    w = a.in[(size_t)e * H + h];
                }
                part += w;
            }
            part = group_sum<GROUP>(part);
            if (lane == 0) dst[h] = part;
        }
    }
}

// ordered sum of the item sums of split rows
__global__ void k_den_combine(const int *__restrict__ mrow_id, const int *__restrict__ mrow_ptr,
                              const float *__restrict__ partial_den, float *__restrict__ den, int n_mrows, int H)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_mrows * H) return;
    const int m = t / H, h = t % H;
    // ascending order kept; the loads of 16 partials are issued together (a hub has hundreds: one dependent load per
    // step made this 16 us on the arxiv-shaped input)
    float s = 0.0f;
    const int p1 = mrow_ptr[m + 1];
    for (int p = mrow_ptr[m]; p < p1; p += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = p + u < p1 ? partial_den[(size_t)(p + u) * H + h] : 0.0f;
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (p + u < p1) s += v[u];
    }
    den[(size_t)mrow_id[m] * H + h] = s;
}

// OP 0: out[e,h] /= den[row,h]   (attGat pass 2 aggr_gat.h:26-29, each_div aggr_gat.h:84-90)
// OP 1: out[e] = att[row,0] + att[idx[e],1]   (u_add_v aggr_gat.h:44-46)
template <int GROUP, int OP>
__global__ __launch_bounds__(kBlock) void k_edge_items_map(const EdgeItemArgs a)
{
    const int item = blockIdx.x * (kBlock / GROUP) + (int)threadIdx.x / GROUP;
    const int lane = threadIdx.x & (GROUP - 1);
    if (item >= a.n_items) return;
    const int beg = a.ptr_s[item], end = a.ptr_s[item + 1];
    const int row = a.target[item];
    const int H = a.H;
    if (OP == 0) {
        const int n = (end - beg) * H;
        for (int j = lane; j < n; j += GROUP) a.out[(size_t)beg * H + j] /= a.in[(size_t)row * H + j % H];
    } else {
        const float a_dst = a.att[(size_t)row * 2];
        for (int e = beg + lane; e < end; e += GROUP) a.out[e] = a_dst + a.att[(size_t)a.idx[e] * 2 + 1];
    }
}

static int edge_item_group(long avg_pairs)
{
    return avg_pairs <= 8 ? 8 : (avg_pairs <= 32 ? 32 : 64);
}

#define DISPATCH_EIG(G, CALL)                               \
    switch (G) {                                            \
        case 8:  { constexpr int GROUP = 8;  CALL; } break; \
        case 32: { constexpr int GROUP = 32; CALL; } break; \
        default: { constexpr int GROUP = 64; CALL; } break; \
    }

static void fill_edge_args(EdgeItemArgs &a, const EdgeItemLaunch &L)
{
    a.ptr_s = L.wl.ptr; a.target = L.wl.target; a.slot = L.wl.slot; a.empty_rows = L.wl.empty_rows; a.idx = L.idx;
    a.att = L.att; a.in = L.in; a.out = L.out; a.den = L.den; a.partial_den = L.partial_den;
    a.n_items = L.wl.n_items; a.n_empty = L.wl.n_empty; a.H = L.heads; a.slope = L.slope;
}

// sums: op 0 = attGat weights + row sums, op 1 = add_to_center
int launch_edge_items_sum(const EdgeItemLaunch &L, int op, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    EdgeItemArgs a;
    fill_edge_args(a, L);
    const int total = a.n_items + a.n_empty;
    if (total > 0) {
        const int G = edge_item_group((long)L.avg_item_edges * L.heads);
        const int nb = ceil_div(total, kBlock / G);
        if (op == 0) { DISPATCH_EIG(G, hipLaunchKernelGGL((k_edge_items_sum<GROUP, 0>), dim3(nb), dim3(kBlock), 0, stream, a)) }
        else         { DISPATCH_EIG(G, hipLaunchKernelGGL((k_edge_items_sum<GROUP, 1>), dim3(nb), dim3(kBlock), 0, stream, a)) }
        HIP_TRY(hipGetLastError());
    }
    if (L.wl.n_mrows > 0) {
        const int n = L.wl.n_mrows * L.heads;
        hipLaunchKernelGGL(k_den_combine, dim3(ceil_div(n, 256)), dim3(256), 0, stream, L.wl.mrow_id, L.wl.mrow_ptr,
                           L.partial_den, L.den, L.wl.n_mrows, L.heads);
        HIP_TRY(hipGetLastError());
    }
    return GNNAGG_OK;
}

// maps: op 0 = divide by the row value, op 1 = u_add_v
int launch_edge_items_map(const EdgeItemLaunch &L, int op, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    EdgeItemArgs a;
    fill_edge_args(a, L);
    if (a.n_items <= 0) return GNNAGG_OK;
    const int G = edge_item_group((long)L.avg_item_edges * L.heads);
    const int nb = ceil_div(a.n_items, kBlock / G);
    if (op == 0) { DISPATCH_EIG(G, hipLaunchKernelGGL((k_edge_items_map<GROUP, 0>), dim3(nb), dim3(kBlock), 0, stream, a)) }
    else         { DISPATCH_EIG(G, hipLaunchKernelGGL((k_edge_items_map<GROUP, 1>), dim3(nb), dim3(kBlock), 0, stream, a)) }
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// ------------------------------------------------------------------------ edge-wise variant
// reference aggr_gcn_edgewise, aggr_gcn.h:291-302 (which covers only 32 columns and reads one edge
// past the end, :296); here one 64-lane wavefront per edge strides over all F columns.
__global__ __launch_bounds__(kBlock) void k_edgewise(const int2 *__restrict__ edgelist, const float *__restrict__ val,
                                                    const float *__restrict__ x, float *__restrict__ y, int E,
                                                    int F)
{
    const int e = blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (e >= E) return;
    const int2 sd = edgelist[e];
    const float w = val ? val[e] : 1.0f;
    for (int c = lane; c < F; c += 64) atomicAdd(&y[(size_t)sd.y * F + c], x[(size_t)sd.x * F + c] * w);
}

int launch_edgewise(const int *edgelist, const float *val, const float *x, float *y, int E, int V, int feat,
                    void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    { const int rcz = launch_zero_words(y, (size_t)V * feat, stream); if (rcz) return rcz; }  // aggr_gcn.h:448
    if (E <= 0) return GNNAGG_OK;
    hipLaunchKernelGGL(k_edgewise, dim3(ceil_div(E, kBlock / 64)), dim3(kBlock), 0, stream,
                       reinterpret_cast<const int2 *>(edgelist), val, x, y, E, feat);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// --------------------------------------------------------------------- naive SpMM + validators
// reference spmm<L>, spmm.h:223-265: thread per row, first edge a plain product, the rest FMAs,
// empty rows left untouched.  Columns are walked in register tiles of 8 (any F, not a template).
__global__ __launch_bounds__(128) void k_spmm_naive(const int *__restrict__ ptr, const int *__restrict__ idx,
                                                   const float *__restrict__ val, const float *__restrict__ x,
                                                   float *__restrict__ y, int V, int F)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= V) return;
    const int beg = ptr[r], end = ptr[r + 1];
    if (beg == end) return;
    for (int c0 = 0; c0 < F; c0 += 8) {
        float ans[8];
        const int n = F - c0 < 8 ? F - c0 : 8;
        {
            const float v = val[beg];
            const float *xr = x + (size_t)idx[beg] * F + c0;
            for (int j = 0; j < n; ++j) ans[j] = v * xr[j];
        }
        for (int e = beg + 1; e < end; ++e) {
            const float v = val[e];
            const float *xr = x + (size_t)idx[e] * F + c0;
            for (int j = 0; j < n; ++j) ans[j] = __builtin_fmaf(v, xr[j], ans[j]);
        }
        for (int j = 0; j < n; ++j) y[(size_t)r * F + c0 + j] = ans[j];
    }
}

int launch_spmm_naive(const int *ptr, const int *idx, const float *val, const float *x, float *y, int V, int feat,
                      void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    if (V <= 0) return GNNAGG_OK;
    hipLaunchKernelGGL(k_spmm_naive, dim3(ceil_div(V, 128)), dim3(128), 0, stream, ptr, idx, val, x, y, V, feat);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// reference validate2, spmm.h:11-21
__global__ void k_validate(const float *__restrict__ ref, const float *__restrict__ ans, int num, int *diff)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < num && fabsf((ref[t] - ans[t]) / ref[t]) > 1e-2f) atomicAdd(diff, 1);
}

// reference validateReordered, spmm.h:23-33
__global__ void k_validate_reordered(const float *__restrict__ ref, const float *__restrict__ ans,
                                     const int *__restrict__ map, int V, int F, int *diff)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (long)V * F && fabsf(ref[t] - ans[(size_t)map[t / F] * F + t % F]) > 1e-2f) atomicAdd(diff, 1);
}

int launch_validate(const float *ref, const float *ans, int num, int *d_diff, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipMemsetAsync(d_diff, 0, sizeof(int), stream));
    if (num > 0) hipLaunchKernelGGL(k_validate, dim3(ceil_div(num, 256)), dim3(256), 0, stream, ref, ans, num, d_diff);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

int launch_validate_reordered(const float *ref, const float *ans, const int *map, int V, int feat, int *d_diff,
                              void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipMemsetAsync(d_diff, 0, sizeof(int), stream));
    if ((long)V * feat > 0)
        hipLaunchKernelGGL(k_validate_reordered, dim3(ceil_div((long)V * feat, 256)), dim3(256), 0, stream, ref, ans,
                           map, V, feat, d_diff);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// --------------------------------------------------------------------------------- CSR check
// The reference trusts its inputs (an out-of-range neighbor id is a silent out-of-bounds gather).  counts[0] = rows with
// ptr[r] > ptr[r+1], counts[1] = neighbor ids outside [0, num_cols).
__global__ void k_check_csr(const int *__restrict__ ptr, const int *__restrict__ idx, int V, int E, int num_cols, int *counts)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < V && ptr[t] > ptr[t + 1]) atomicAdd(&counts[0], 1);
    if (t < E && (idx[t] < 0 || idx[t] >= num_cols)) atomicAdd(&counts[1], 1);
}

int launch_check_csr(const int *ptr, const int *idx, int V, int E, int num_cols, int *d_counts, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(int), stream));
    const long n = std::max<long>(V, E);
    if (n > 0) hipLaunchKernelGGL(k_check_csr, dim3(ceil_div(n, 256)), dim3(256), 0, stream, ptr, idx, V, E, num_cols, d_counts);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// ----------------------------------------------------------------------------- halo packing
// out[i,:] = x[ids[i],:]  -- send buffer of the halo all-to-all (gnnagg.h Section D)
template <int VEC, int GROUP>
__global__ __launch_bounds__(kBlock) void k_pack_rows(const float *__restrict__ x, const int *__restrict__ ids, int n,
                                                     int F, int ntiles, float *__restrict__ out)
{
    const int tile = blockIdx.x % ntiles;
    const int i = (blockIdx.x / ntiles) * (kBlock / GROUP) + threadIdx.x / GROUP;
    const int col = (tile * GROUP + (threadIdx.x & (GROUP - 1))) * VEC;
    if (i >= n || col >= F) return;
    const Pack<VEC> p = load_pack<VEC>(x + (size_t)ids[i] * F + col);
    store_pack<VEC>(out + (size_t)i * F + col, p.v);
}

int launch_pack_rows(const float *x, const int *ids, int n, int feat, float *out, void *stream_v)
{
    hipStream_t stream = (hipStream_t)stream_v;
    if (n <= 0) return GNNAGG_OK;
    const Geometry g = pick_geometry(feat, x, out, nullptr, feat);
    const int nb = ceil_div(n, kBlock / g.group) * g.ntiles;
#define CALL_PACK hipLaunchKernelGGL((k_pack_rows<VEC, GROUP>), dim3(nb), dim3(kBlock), 0, stream, x, ids, n, feat, g.ntiles, out);
    DISPATCH_GEOM(g, CALL_PACK)
#undef CALL_PACK
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// GAT halo rows: one exchange carries the feature row AND the attention terms of every requested row.
// out[i, 0 .. F) = x[ids[i], :], out[i, F .. F + A) = att[ids[i], :]   (A = 2 * heads)
__global__ __launch_bounds__(256) void k_pack_rows2(const float *__restrict__ x, const float *__restrict__ att, const int *__restrict__ ids,
                                                    long n, int F, int A, float *__restrict__ out)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int W = F + A;
    if (t >= n * W) return;
    const long i = t / W;
    const int c = (int)(t - i * W);
    const size_t r = (size_t)ids[i];
    out[t] = c < F ? x[r * F + c] : att[r * A + (c - F)];
}

// the receiving side: in[i, :] -> x_out[i, 0 .. F), att_out[i, 0 .. A)   (the halo tails of X_ext / att_ext)
__global__ __launch_bounds__(256) void k_unpack_rows2(const float *__restrict__ in, long n, int F, int A, float *__restrict__ x_out,
                                                      float *__restrict__ att_out)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int W = F + A;
    if (t >= n * W) return;
    const long i = t / W;
    const int c = (int)(t - i * W);
    if (c < F) x_out[(size_t)i * F + c] = in[t];
    else att_out[(size_t)i * A + (c - F)] = in[t];
}

int launch_pack_rows2(const float *x, const float *att, const int *ids, int n, int feat, int att_w, float *out, void *stream_v)
{
    if (n <= 0) return GNNAGG_OK;
    const long total = (long)n * (feat + att_w);
    hipLaunchKernelGGL(k_pack_rows2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, x, att, ids, (long)n, feat,
                       att_w, out);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

int launch_unpack_rows2(const float *in, int n, int feat, int att_w, float *x_out, float *att_out, void *stream_v)
{
    if (n <= 0) return GNNAGG_OK;
    const long total = (long)n * (feat + att_w);
    hipLaunchKernelGGL(k_unpack_rows2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, in, (long)n, feat, att_w,
                       x_out, att_out);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// ------------------------------------------------------------------ column-tiled image of X (2-D blocked mode)
// xt[t][r][0 .. tile_w) = x[r][t * tile_w ..], zero beyond feat.  Rows of x whose pitch is not a multiple of a 128-byte
// line (F = 602: 2408 B) make every 256-byte tile segment of a gather straddle three lines -- 1.5x the L2 footprint and
// traffic; the tiled image is line-aligned whatever the caller's pitch is, and costs one streaming pass over X.
// One thread per (row, 4-column quad): reads are coalesced along the row, writes are 16-byte stores.
__global__ __launch_bounds__(256) void k_tile_x(const float *__restrict__ x, float *__restrict__ xt, int rows, int feat, int tile_w,
                                                int quads_per_row)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)rows * quads_per_row;
    if (i >= total) return;
    const int r = (int)(i / quads_per_row), q = (int)(i - (long)r * quads_per_row);
    const int c = q * 4;
    const float *src = x + (size_t)r * feat + c;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c + 3 < feat) {
        if ((((uintptr_t)src) & 15) == 0) v = *reinterpret_cast<const float4 *>(src);
        else if ((((uintptr_t)src) & 7) == 0) {
            const float2 a = *reinterpret_cast<const float2 *>(src), b = *reinterpret_cast<const float2 *>(src + 2);
            v = make_float4(a.x, a.y, b.x, b.y);
        } else v = make_float4(src[0], src[1], src[2], src[3]);
    } else {
        if (c < feat) v.x = src[0];
        if (c + 1 < feat) v.y = src[1];
        if (c + 2 < feat) v.z = src[2];
    }
    const int t = c / tile_w, ct = c - t * tile_w;
    *reinterpret_cast<float4 *>(xt + ((size_t)t * rows + r) * tile_w + ct) = v;
}

int launch_tile_x(const float *x, float *xt, int rows, int feat, int tile_w, void *stream_v)
{
    if (rows <= 0) return GNNAGG_OK;
    const int ntiles = (feat + tile_w - 1) / tile_w;
    const int quads = ntiles * tile_w / 4;
    const long total = (long)rows * quads;
    hipLaunchKernelGGL(k_tile_x, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, x, xt, rows, feat, tile_w, quads);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// n 4-byte words at p = 0.  A kernel rather than hipMemsetAsync: a memset NODE of a captured HIP graph did its work on the first
// replay only (ROCm 7.2: replays 2 and 3 of the chained rows mode started from the previous replay's Yt;
// tests/test_gpu_blocked.py::test_rows_mode_on_the_blocked_order_with_the_dense_combine_behind_it).  Every fill on a path that a
// caller may capture goes through here.
__global__ __launch_bounds__(256) void k_zero_f32x4(float4 *__restrict__ p, long n4)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ __launch_bounds__(256) void k_zero_u32(unsigned *__restrict__ p, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

int launch_zero_words(void *p, size_t n, void *stream_v)
{
    if (n == 0) return GNNAGG_OK;
    if (((uintptr_t)p & 3) != 0) return fail(GNNAGG_ERR_STATE, "internal: zero fill of an unaligned range");
    if ((n & 3) == 0 && ((uintptr_t)p & 15) == 0) {
        const long n4 = (long)(n / 4);
        hipLaunchKernelGGL(k_zero_f32x4, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, reinterpret_cast<float4 *>(p), n4);
    } else {
        hipLaunchKernelGGL(k_zero_u32, dim3((unsigned)(((long)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, reinterpret_cast<unsigned *>(p), (long)n);
    }
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// The finishing pass of gnnagg_gatv2_run_weights / gnnagg_dot_attn_run_weights: the walks left the raw fp32 score of every (edge, head) in
// alpha and every (row, head)'s final (maximum M, denominator) in stat; here alpha[p, h] = expf(e - ms) / den with ms = M, or 0 where M is
// -inf (the walks' own shift rule: a masked edge is +0, an all-masked (row, head) 0 / 0).  Edge-parallel, so a row of any length costs what
// its edges cost and no lane group sweeps a hub: a wavefront takes 64 consecutive edges.  Each lane finds the row of ONE of them -- the last
// r with ptr[r] <= p (rows without edges share their successor's ptr and are stepped over), a bisection over ptr whose upper levels the
// whole workgroup shares in cache -- and the wavefront then sweeps the 64 * heads floats of its edges in `heads` steps of 64 consecutive
// floats, every lane taking the row of its element's edge from the lane that found it: the [E, heads] array is read once and written once
// in whole coalesced lines, and the bisection runs once per edge, not once per element (one per element measured 108-127 us of a 330-450
// us call at 8 heads on the arxiv-shaped graph).  A launch of its own behind the walk and the merge on the same
// stream: the scores and the pairs it reads are ordered before it by the stream.
__global__ __launch_bounds__(256) void k_attn_finish(const int *__restrict__ ptr, int V, int E, int heads, float *alpha,
                                                     const float *__restrict__ stat)
{
    const int lane = threadIdx.x & 63;
    const long e0 = (long)blockIdx.x * 256 + (threadIdx.x & ~63);   // the wavefront's first edge
    int row = 0;
    if (e0 + lane < E) {
        const int p = (int)(e0 + lane);
        int lo = 0, hi = V;   // ptr[lo] <= p < ptr[hi] throughout (ptr[0] = 0, ptr[V] = E > p)
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (ptr[mid] <= p) lo = mid; else hi = mid;
        }
        row = lo;
    }
    for (int t = 0; t < heads; ++t) {       // (uniform over the wavefront: every lane takes part in the shuffle)
        const int k = t * 64 + lane;        // this lane's element among the wavefront's 64 * heads
        const int src = k / heads, h = k - src * heads;
        const int r = __shfl(row, src, 64);
        if (e0 + src >= E) continue;
        const float *st = stat + ((size_t)r * (size_t)heads + (size_t)h) * 2;
        const float M = st[0], den = st[1];
        const float ms = M == -INFINITY ? 0.0f : M;
        float *ap = alpha + (size_t)(e0 + src) * (size_t)heads + (size_t)h;
        *ap = expf(*ap - ms) / den;
    }
}

int launch_attn_finish(const int *ptr, int V, int E, int heads, float *alpha, const float *stat, void *stream_v)
{
    if (E <= 0 || V <= 0 || heads <= 0) return GNNAGG_OK;
    hipLaunchKernelGGL(k_attn_finish, dim3((unsigned)(((long)E + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, ptr, V, E, heads, alpha, stat);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// The inverse for the canonical rows mode on the blocked order: Yt[tile][row][tile_w] -> y[row][feat], finishing the row on the way
// (mean: / degree as finish_gcn_row does; ReLU).  One thread per (row, 4-column quad); the caller's rows may be 4-byte aligned only.
__global__ __launch_bounds__(256) void k_untile_y(const float *__restrict__ yt, float *__restrict__ y, const int *__restrict__ row_ptr,
                                                  const unsigned char *__restrict__ skip, int rows, int feat, int tile_w, int quads_per_row, int mean,
                                                  int relu, const float *__restrict__ den_t = nullptr, int ht = 1, int dhead = 1)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)rows * quads_per_row;
    if (i >= total) return;
    const int r = (int)(i / quads_per_row), q = (int)(i - (long)r * quads_per_row);
    if (skip && skip[r]) return;   // (rows another kernel writes)
    const int c = q * 4;
    const int t = c / tile_w, ct = c - t * tile_w;
    const float4 v4 = *reinterpret_cast<const float4 *>(yt + ((size_t)t * rows + r) * tile_w + ct);
    float v[4] = {v4.x, v4.y, v4.z, v4.w};
    if (den_t && row_ptr[r + 1] > row_ptr[r]) {   // GAT: the one division of aggr_gat (aggr_gat.h:163), unguarded like the row kernels' -- a
        // zero denominator is 0 / 0 = NaN (include/gnnagg.h, "Attention logits"); rows without edges keep the image's +0.  A quad lies
        // inside one head (head width % 4 == 0)
        const float d = den_t[((size_t)t * rows + r) * ht + (ht > 1 ? ct / dhead : 0)];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] / d;
    }
    if (mean) {
        const float dg = (float)(row_ptr[r + 1] - row_ptr[r]);
        if (dg > 0.0f) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = v[k] / dg;
        }
    }
    if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] < 0.0f ? 0.0f : v[k];   // (a NaN stays a NaN: relu_pack, kernel_util.cuh)
    }
    float *dst = y + (size_t)r * feat + c;
    if (c + 3 < feat && (((uintptr_t)dst) & 15) == 0) *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else if (c + 3 < feat && (((uintptr_t)dst) & 7) == 0) {
        *reinterpret_cast<float2 *>(dst) = make_float2(v[0], v[1]);
        *reinterpret_cast<float2 *>(dst + 2) = make_float2(v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c + k < feat) dst[k] = v[k];
    }
}

int launch_untile_y(const float *yt, float *y, const int *row_ptr, const unsigned char *skip, int rows, int feat, int tile_w, int mean, int relu,
                    void *stream_v)
{
    if (rows <= 0 || feat <= 0) return GNNAGG_OK;
    const int quads = (feat + 3) / 4;
    const long total = (long)rows * quads;
    hipLaunchKernelGGL(k_untile_y, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, yt, y, row_ptr, skip, rows, feat,
                       tile_w, quads, mean, relu);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

int launch_untile_y_gat(const float *yt, const float *den_t, float *y, const int *row_ptr, const unsigned char *skip, int rows, int feat, int tile_w,
                        int ht, int dhead, void *stream_v)
{
    if (rows <= 0 || feat <= 0) return GNNAGG_OK;
    const int quads = (feat + 3) / 4;
    const long total = (long)rows * quads;
    hipLaunchKernelGGL(k_untile_y, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, yt, y, row_ptr, skip, rows, feat, tile_w,
                       quads, 0, 0, den_t, ht, dhead);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// ------------------------------------------------------------------ compact attention terms (2-D blocked GAT)
// att is [V, H, 2] (centre term, source term interleaved per head): a tile of the span kernel needs the source terms of its
// HT heads per EDGE -- HT four-byte loads that each touch a different 64-byte att row per lane.  The compact image keeps
// them per head group hg = first head / HT as as_t[hg][v][0 .. HT) (and the centre terms as ac_t likewise): one HT * 4-byte
// load per edge, rows 16x denser in the L2 / L1 than att's.  Heads beyond H replicate head H - 1 (never stored).
__global__ __launch_bounds__(256) void k_tile_att(const float *__restrict__ att, float *__restrict__ as_t, float *__restrict__ ac_t,
                                                  int rows, int heads, int ht, int n_hg)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_hg = (long)rows * ht;
    if (i >= per_hg * n_hg) return;
    const int hg = (int)(i / per_hg);
    const long rem = i - (long)hg * per_hg;
    const int v = (int)(rem / ht), k = (int)(rem - (long)v * ht);
    int h = hg * ht + k;
    h = h < heads ? h : heads - 1;
    const float *cs = att + ((size_t)v * heads + h) * 2;  // (scalar loads: the caller's att may be 4-byte aligned only)
    ac_t[i] = cs[0];
    as_t[i] = cs[1];
}

int launch_tile_att(const float *att, float *as_t, float *ac_t, int rows, int heads, int ht, void *stream_v)
{
    if (rows <= 0) return GNNAGG_OK;
    const int n_hg = (heads + ht - 1) / ht;
    const long total = (long)rows * ht * n_hg;
    hipLaunchKernelGGL(k_tile_att, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, att, as_t, ac_t, rows, heads,
                       ht, n_hg);
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

// ------------------------------------------------------------------------- row-gather ceiling probe (measurement aid)
// What the memory system delivers to ROW GATHERS in the aggregation kernels' own access shape, by where the gathered rows live
// (one XCD's L2, the Infinity Cache, HBM): the caller chooses the window through the ids it passes.  A lane group of LANES lanes
// reads `per_group` ids (one coalesced load per LANES ids, broadcast lane to lane), gathers `active` x 16 B of row id at
// rows + id * pitch with 8 gathers in flight, XOR-consumes them and never stores (gnnagg_probe_row_gather; bench.py divides the
// bytes of its gather model by this launch's time to get the ceiling each roofline fraction is quoted against).
template <int LANES>
__global__ __launch_bounds__(256) void k_probe_row_gather(const int *__restrict__ ids, const char *__restrict__ rows, long pitch, int active,
                                                          int per_group, unsigned *sink)
{
    constexpr int U = 8, GPB = 256 / LANES;
    const int lane = threadIdx.x & (LANES - 1), grp = threadIdx.x / LANES;
    const int *my = ids + ((long)blockIdx.x * GPB + grp) * per_group;
    const char *col = rows + lane * 16;
    const bool on = lane < active;
    uint4 acc = {0, 0, 0, 0};
    int cur = my[lane];
    for (int cb = 0; cb < per_group; cb += LANES) {
        int nxt = 0;
        if (cb + LANES < per_group) nxt = my[cb + LANES + lane];
#pragma unroll 1
        for (int j = 0; j < LANES; j += U) {
            uint4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = __shfl(cur, j + u, LANES);
                v[u] = on ? *reinterpret_cast<const uint4 *>(col + (long)s * pitch) : uint4{0, 0, 0, 0};
            }
#pragma unroll
            for (int u = 0; u < U; ++u) { acc.x ^= v[u].x; acc.y ^= v[u].y; acc.z ^= v[u].z; acc.w ^= v[u].w; }
        }
        cur = nxt;
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9e3779b9U) sink[0] = acc.x;  // practically never: keeps the loads alive
}

int launch_probe_row_gather(const void *rows, long pitch, int seg_bytes, const int *ids, long n_ids, int per_group, void *stream_v)
{
    if (!rows || !ids || pitch < 16 || (pitch & 15) || seg_bytes < 16 || seg_bytes > 1024 || (seg_bytes & 15) || n_ids <= 0)
        return fail(GNNAGG_ERR_ARG, "probe_row_gather: rows / ids null, or pitch / seg_bytes not multiples of 16 (seg_bytes in 16 .. 1024)");
    const int active = seg_bytes / 16;
    int lanes = 8;
    while (lanes < active) lanes <<= 1;
    const int gpb = 256 / lanes;
    if (per_group <= 0 || per_group % lanes || n_ids % ((long)per_group * gpb))
        return fail(GNNAGG_ERR_ARG, "probe_row_gather: ids_per_group must be a multiple of the lane-group width and n_ids a multiple of ids_per_group x groups per 256-thread block");
    unsigned *sink = device_probe_sink();
    if (!sink) return fail(GNNAGG_ERR_HIP, "probe: no sink");
    const long nb = n_ids / ((long)per_group * gpb);
    if (nb > 0x7fffffffL) return fail(GNNAGG_ERR_ARG, "probe_row_gather: too many ids for one launch");
    hipStream_t stream = (hipStream_t)stream_v;
    const char *r = (const char *)rows;
    switch (lanes) {
        case 8:  hipLaunchKernelGGL((k_probe_row_gather<8>), dim3((unsigned)nb), dim3(256), 0, stream, ids, r, pitch, active, per_group, sink); break;
        case 16: hipLaunchKernelGGL((k_probe_row_gather<16>), dim3((unsigned)nb), dim3(256), 0, stream, ids, r, pitch, active, per_group, sink); break;
        case 32: hipLaunchKernelGGL((k_probe_row_gather<32>), dim3((unsigned)nb), dim3(256), 0, stream, ids, r, pitch, active, per_group, sink); break;
        default: hipLaunchKernelGGL((k_probe_row_gather<64>), dim3((unsigned)nb), dim3(256), 0, stream, ids, r, pitch, active, per_group, sink); break;
    }
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

}  // namespace gnnagg
