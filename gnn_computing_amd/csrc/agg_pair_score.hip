// agg_pair_score.hip -- one value (or one row of n_out values) per node PAIR in one launch: gnnagg_pair_score_run (include/gnnagg.h
// section G, "Pair scoring").  The decoders of link prediction, edge classification and knowledge-graph completion:
//
//   dot       out[p] = sum_f hu[u_p][f] * hv[v_p][f]                       (with rel / etype DistMult: ... * rel[t_p][f] * ...)
//   mlp       out[p] = act(relu(m_p . W1 + b1) . W2 + b2),   m_p = hu[u_p] (*) hv[v_p]  (mul)  or  [hu[u_p], hv[v_p]]  (cat)
//
// The pairs come as COO (u[P], v[P]) or as CSR (ptr[n + 1], idx[P]: u_p = the row that owns position p, found by the lane that needs it
// with a binary search over ptr -- no expanded row array exists anywhere); an optional src map is applied to both ids.
//
// The work unit is a PAIR, not a destination row: there is no edge chain to walk, a pair costs two row gathers and nothing else.
//   k_pair_dot   no LDS, no MFMA.  A lane group takes a window of GROUP consecutive pairs: lane j loads the ids of pair j (CSR: searches
//                its row), the window is then walked in batches of kPairBatch pairs -- ids broadcast in the group, BOTH rows (and the
//                relation's row) of every pair of the batch loaded before the first FMA, the hu row loaded once per run of equal u in the
//                batch (consecutive pairs of a CSR row share it).  Per lane fmaf over its columns in ascending f, then the fixed xor
//                butterfly of group_sum; lane j keeps the sum of pair j, and the window is stored with one coalesced store.
//   k_pair_mlp   256 threads, tiles of kPairRows = 16 * kPairRB pairs, the tiles blockIdx.x, blockIdx.x + gridDim.x, ... per workgroup.
//     phase 1    one lane group per pair slot, the gathers of up to 4 slots in flight: both rows loaded, m formed in registers (mul:
//                one fp32 product, for bf16 exact and rounded to bf16 once; cat: the raw elements, hv's half at column feat) and stored to
//                the m tile.  Slots past P store zeros.
//     phase 2    z = relu(m . W1 + b1) into the z tile.  A wavefront's work item is a 16-column sub-tile of z over NRB row blocks of 16
//                pairs: ONE B operand (fp32: a buffer load of W1; bf16: a ds_read_b128 of its LDS image) feeds NRB MFMAs, one fp32
//                accumulator per (row block, element), k ascending -- for fp32 the fmaf chain of gnnagg_matmul_nn, bit for bit.  With at
//                least 4 sub-tiles NRB = kPairRB (every operand of W1 is read once per tile); with fewer the row blocks are spread over
//                the wavefronts instead (NRB = 1), so that hidden <= 48 or n_out = 1 does not leave three wavefronts idle.
//     phase 3    the same over the z tile and W2; + b2, the optional ReLU, one global store per element.
//   Two barriers per tile, as in k_block_gin: the m tile and the z tile are separate regions, a wavefront that has left phase 3 may
//   start phase 1 of the workgroup's next tile.  Neither m nor z reaches HBM.  No atomics, no scratch.
//   The LDS layout, the image staging and the MFMA phases live in pair_mlp.cuh, which k_block_edgeconv shares.
#include "pair_mlp.cuh"

namespace gnnagg {
namespace {

constexpr int kPairLdsBytes = 160 * 1024;    // LDS of a CU: the budget of both tiles + both weight images
constexpr int kPairMaxDim = 256;             // feat, hidden and n_out of the mlp
constexpr int kPairPerCu = 8;                // workgroups per CU the grid is capped at (fewer where the LDS of a workgroup allows fewer)
constexpr int kPairBatch = 4;                // dot: pairs whose rows are in flight per lane group before the first FMA

struct PairArgs {
    const int *u, *v, *ptr, *idx, *src, *etype;
    const float *rel;
    const void *hu, *hv, *w1, *w2;
    const float *b1, *b2;
    void *out;
    long long upitch, vpitch;   // elements between rows of hu / hv
    int P, nrows, feat, num_rel, hidden, n_out, ntiles, cat, relu, out_bf16, tiles;
};

static bool pair_supported(int kind, int combine, int feat, int hidden, int n_out, int dtype)
{
    if (dtype != GNNAGG_DTYPE_F32 && dtype != GNNAGG_DTYPE_BF16) return false;
    if (combine != GNNAGG_PAIR_MUL && combine != GNNAGG_PAIR_CAT) return false;
    if (kind == GNNAGG_PAIR_DOT) return feat >= 1;
    if (kind != GNNAGG_PAIR_MLP) return false;
    if (feat < 1 || feat > kPairMaxDim || hidden < 1 || hidden > kPairMaxDim || n_out < 1 || n_out > kPairMaxDim) return false;
    return pair_lds(feat, hidden, n_out, combine == GNNAGG_PAIR_CAT, dtype == GNNAGG_DTYPE_BF16).bytes <= kPairLdsBytes;
}

// workgroups an mlp launch of this shape is capped at: as many per CU as their LDS allows, kPairPerCu at the most
static int pair_grid_cap(int combine, int feat, int hidden, int n_out, int dtype)
{
    const int per_cu = kPairLdsBytes / pair_lds(feat, hidden, n_out, combine == GNNAGG_PAIR_CAT, dtype == GNNAGG_DTYPE_BF16).bytes;
    return std::min(std::max(per_cu, 1), kPairPerCu) * device_cu_count();
}

// The rows of hu and hv pair p reads.  CSR: the largest row r with ptr[r] <= p -- ptr[r + 1] > p then, so r is never an empty row,
// wherever the empty rows lie; r stays inside [0, nrows) whatever ptr holds.
__device__ __forceinline__ void pair_rows(const PairArgs &a, int p, int &ur, int &vr)
{
    int u, v;
    if (a.ptr) {
        int lo = 0, hi = a.nrows;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.ptr[mid] <= p) lo = mid;
            else hi = mid;
        }
        u = lo;
        v = a.idx[p];
    } else {
        u = a.u[p];
        v = a.v[p];
    }
    if (a.src) {
        u = a.src[u];
        v = a.src[v];
    }
    ur = u;
    vr = v;
}

// ------------------------------------------------------------------------------------------------------------------ dot / DistMult
template <int VEC, int GROUP, bool REL, typename TX>
__global__ __launch_bounds__(kPairThreads) void k_pair_dot(const PairArgs a)
{
    constexpr int GPB = kPairThreads / GROUP, U = kPairBatch;
    const int lane = (int)threadIdx.x % GROUP, grp = (int)threadIdx.x / GROUP;
    const long long base_ll = ((long long)blockIdx.x * GPB + grp) * GROUP;
    if (base_ll >= a.P) return;   // the whole lane group
    const int base = (int)base_ll, p = base + lane, F = a.feat;
    int my_u = 0, my_v = 0, my_t = 0;
    if (p < a.P) {
        pair_rows(a, p, my_u, my_v);
        if constexpr (REL) my_t = a.etype[p];
    }
    float my_out = 0.0f;
    const int n = a.P - base < GROUP ? a.P - base : GROUP;
    const TX *__restrict__ hu = static_cast<const TX *>(a.hu);
    const TX *__restrict__ hv = static_cast<const TX *>(a.hv);
#pragma unroll 1
    for (int j = 0; j < n; j += U) {
        int ur[U], vr[U], tr[U];
        bool ok[U], same[U];
        float acc[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            ur[t] = __shfl(my_u, j + t, GROUP);
            vr[t] = __shfl(my_v, j + t, GROUP);
            tr[t] = REL ? __shfl(my_t, j + t, GROUP) : 0;
            ok[t] = j + t < n && (!REL || (unsigned)tr[t] < (unsigned)a.num_rel);   // a type outside [0, R): no load, the score stays +0
            acc[t] = 0.0f;
        }
        same[0] = false;
#pragma unroll
        for (int t = 1; t < U; ++t) same[t] = ok[t] && ok[t - 1] && ur[t] == ur[t - 1];
#pragma unroll 1
        for (int ct = 0; ct < a.ntiles; ++ct) {
            const int col = (ct * GROUP + lane) * VEC;
            if (col >= F) continue;
            Pack<VEC, TX> xu[U], xv[U];
            Pack<VEC, float> xr[U];
#pragma unroll
            for (int t = 0; t < U; ++t)
                if (ok[t]) {
                    if (!same[t]) xu[t] = load_pack<VEC>(hu + (size_t)ur[t] * (size_t)a.upitch + col);
                    xv[t] = load_pack<VEC>(hv + (size_t)vr[t] * (size_t)a.vpitch + col);
                    if constexpr (REL) xr[t] = load_pack<VEC>(a.rel + (size_t)tr[t] * F + col);
                }
#pragma unroll
            for (int t = 1; t < U; ++t)
                if (same[t]) xu[t] = xu[t - 1];   // ascending t: a run of equal u passes its one loaded row along
#pragma unroll
            for (int t = 0; t < U; ++t)
                if (ok[t]) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        if constexpr (REL) acc[t] = __builtin_fmaf(xu[t].at(k) * xr[t].v[k], xv[t].at(k), acc[t]);
                        else acc[t] = __builtin_fmaf(xu[t].at(k), xv[t].at(k), acc[t]);
                    }
                }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const float s = group_sum<GROUP>(acc[t]);
            if (lane == j + t) my_out = s;
        }
    }
    if (p < a.P) static_cast<float *>(a.out)[p] = my_out;
}

template <int VEC, int GROUP, typename TX>
static void launch_pair_dot(const PairArgs &a, hipStream_t st)
{
    const dim3 grid((unsigned)ceil_div(a.P, kPairThreads)), block(kPairThreads);   // GPB windows of GROUP pairs: 256 pairs per workgroup
    if (a.rel) hipLaunchKernelGGL((k_pair_dot<VEC, GROUP, true, TX>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_pair_dot<VEC, GROUP, false, TX>), grid, block, 0, st, a);
}

// ------------------------------------------------------------------------------------------------------------------------- mlp
template <int VEC, int GROUP, typename TX>
__global__ __launch_bounds__(kPairThreads) void k_pair_mlp(const PairArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int GPB = kPairThreads / GROUP, PASSES = kPairRows / GPB, UB = PASSES >= 4 ? 4 : PASSES;
    static_assert(GROUP >= 16 && PASSES * GPB == kPairRows && PASSES % UB == 0 && PASSES <= GROUP, "whole batches of passes over a tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char pair_smem[];
    const int F = a.feat, H = a.hidden, N = a.n_out;
    const PairLds L = pair_lds(F, H, N, a.cat != 0, B16);
    const int K1 = L.k1, Kp1 = L.kp1, Hp = L.hp, pitch_m = L.pitch_m, pitch_z = L.pitch_z;
    TX *mtile = reinterpret_cast<TX *>(pair_smem);
    TX *ztile = reinterpret_cast<TX *>(pair_smem + L.z_off);
    const int lane = (int)threadIdx.x % GROUP, grp = (int)threadIdx.x / GROUP;

    // once per workgroup: the k padding of the m tile (no row store reaches it), the k padding of the z tile that no sub-tile of phase 2
    // covers (bf16: [roundup16(hidden), Hp)) ...
    const int npad = Kp1 - K1;
    for (int i = threadIdx.x; i < kPairRows * npad; i += kPairThreads) mtile[(i / npad) * pitch_m + K1 + i % npad] = (TX)0.0f;
    const int zcov = (H + 15) & ~15, zpad = Hp > zcov ? Hp - zcov : 0;
    for (int i = threadIdx.x; i < kPairRows * zpad; i += kPairThreads) ztile[(i / zpad) * pitch_z + zcov + i % zpad] = (TX)0.0f;
    // ... and, bf16, the images of both weights
    const __bf16 *wimg1 = nullptr, *wimg2 = nullptr;
    if constexpr (B16) {
        __bf16 *i1 = reinterpret_cast<__bf16 *>(pair_smem + L.w1_off), *i2 = reinterpret_cast<__bf16 *>(pair_smem + L.w2_off);
        pair_stage_weight(i1, pitch_m, Kp1, static_cast<const __bf16 *>(a.w1), K1, H);
        pair_stage_weight(i2, pitch_z, Hp, static_cast<const __bf16 *>(a.w2), H, N);
        wimg1 = i1;
        wimg2 = i2;
    }
    const TX *__restrict__ hu = static_cast<const TX *>(a.hu);
    const TX *__restrict__ hv = static_cast<const TX *>(a.hv);

#pragma unroll 1
    for (int tile = (int)blockIdx.x; tile < a.tiles; tile += (int)gridDim.x) {
        const int p0 = tile * kPairRows;
        // ---- phase 1: m rows into the m tile.  Lane j of a group fetches the ids of the group's slot of pass j (-1: past P).
        int my_u = -1, my_v = 0;
        if (lane < PASSES && p0 + lane * GPB + grp < a.P) pair_rows(a, p0 + lane * GPB + grp, my_u, my_v);
#pragma unroll 1
        for (int pass0 = 0; pass0 < PASSES; pass0 += UB) {
            int ur[UB], vr[UB];
#pragma unroll
            for (int b = 0; b < UB; ++b) {
                ur[b] = __shfl(my_u, pass0 + b, GROUP);
                vr[b] = __shfl(my_v, pass0 + b, GROUP);
            }
#pragma unroll 1
            for (int ct = 0; ct < a.ntiles; ++ct) {
                const int col = (ct * GROUP + lane) * VEC;
                if (col >= F) continue;
                Pack<VEC, TX> xu[UB] = {}, xv[UB] = {};
#pragma unroll
                for (int b = 0; b < UB; ++b)
                    if (ur[b] >= 0) {
                        xu[b] = load_pack<VEC>(hu + (size_t)ur[b] * (size_t)a.upitch + col);
                        xv[b] = load_pack<VEC>(hv + (size_t)vr[b] * (size_t)a.vpitch + col);
                    }
#pragma unroll
                for (int b = 0; b < UB; ++b) {
                    TX *mrow = mtile + ((pass0 + b) * GPB + grp) * pitch_m;
                    if (a.cat) {
                        store_raw_pack<VEC, TX>(mrow + col, xu[b]);
                        store_raw_pack<VEC, TX>(mrow + F + col, xv[b]);
                    } else {
                        float pr[VEC];
#pragma unroll
                        for (int k = 0; k < VEC; ++k) pr[k] = xu[b].at(k) * xv[b].at(k);
                        if constexpr (B16) store_pack_bf16<VEC>(mrow + col, pr, VEC);
                        else store_pack<VEC>(mrow + col, pr);
                    }
                }
            }
        }
        __syncthreads();   // the m tile (and, the first time, the padding and the images) is complete; every wavefront has left phase 3

        // ---- phase 2: z = relu(m . W1 + b1) into the z tile
        if (((H + 15) >> 4) >= 4) pair_mlp_phase<kPairRB, kPairToZ, TX>(mtile, pitch_m, Kp1, a.w1, wimg1, K1, H, a.b1, ztile, pitch_z, Hp, a, p0);
        else pair_mlp_phase<1, kPairToZ, TX>(mtile, pitch_m, Kp1, a.w1, wimg1, K1, H, a.b1, ztile, pitch_z, Hp, a, p0);
        __syncthreads();   // the z tile is complete; every wavefront has left the m tile

        // ---- phase 3: out = act(z . W2 + b2)
        if (((N + 15) >> 4) >= 4) pair_mlp_phase<kPairRB, kPairToOut, TX>(ztile, pitch_z, Hp, a.w2, wimg2, H, N, a.b2, nullptr, 0, 0, a, p0);
        else pair_mlp_phase<1, kPairToOut, TX>(ztile, pitch_z, Hp, a.w2, wimg2, H, N, a.b2, nullptr, 0, 0, a, p0);
        // no third barrier: the next tile's phase 1 writes the m tile only
    }
}

template <int VEC, int GROUP, typename TX>
static int launch_pair_mlp(const PairArgs &a, int grid, size_t lds, hipStream_t st)
{
    if constexpr (GROUP < 16) {
        return fail(GNNAGG_ERR_STATE, "internal: gnnagg_pair_score_run runs the mlp on groups of 16 lanes and more");
    } else {
        static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
        if (lds > 64 * 1024 && big_lds_ok.first()) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pair_mlp<VEC, GROUP, TX>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        kPairLdsBytes));
            big_lds_ok.done();
        }
        hipLaunchKernelGGL((k_pair_mlp<VEC, GROUP, TX>), dim3((unsigned)grid), dim3(kPairThreads), lds, st, a);
        return GNNAGG_OK;
    }
}

static int pair_score_run(int kind, int combine, const int *u, const int *v, const int *ptr, const int *idx, int num_rows, int num_pairs,
                          const int *src, const void *hu, long long hu_pitch, const void *hv, long long hv_pitch, int x_dtype, int feat,
                          const float *rel, const int *etype, int num_rel, const void *w1, const float *b1, int hidden, const void *w2,
                          const float *b2, int n_out, void *out, int out_dtype, int flags, void *stream)
{
    static const char *who = "gnnagg_pair_score_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    const bool dot = kind == GNNAGG_PAIR_DOT;
    if (kind != GNNAGG_PAIR_DOT && kind != GNNAGG_PAIR_MLP) return bad("unknown kind " + std::to_string(kind));
    if (combine != GNNAGG_PAIR_MUL && combine != GNNAGG_PAIR_CAT) return bad("unknown combine " + std::to_string(combine));
    if (num_pairs < 0) return bad("num_pairs = " + std::to_string(num_pairs) + " is negative");
    if (feat < 1) return bad("feat = " + std::to_string(feat) + " must be >= 1");
    if (hu_pitch < feat) return bad("hu_pitch = " + std::to_string(hu_pitch) + " is below feat = " + std::to_string(feat));
    if (hv_pitch < feat) return bad("hv_pitch = " + std::to_string(hv_pitch) + " is below feat = " + std::to_string(feat));
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (out_dtype != GNNAGG_DTYPE_F32 && out_dtype != GNNAGG_DTYPE_BF16) return bad("unknown out_dtype " + std::to_string(out_dtype));
    if (x_dtype == GNNAGG_DTYPE_F32 && out_dtype == GNNAGG_DTYPE_BF16) return bad("out_dtype: fp32 operands give a fp32 out, not a bf16 one");
    if (flags & ~GNNAGG_FLAG_RELU) return bad("flags = " + std::to_string(flags) + ": GNNAGG_FLAG_RELU is the only flag");
    const bool coo = u || v, csr = ptr || idx;
    if (coo && csr) return bad("d_u / d_v and d_ptr / d_idx are both given: a call takes ONE pair form");
    if (coo && !(u && v)) return bad(u ? "d_v is null (d_u is given)" : "d_u is null (d_v is given)");
    if (csr && !(ptr && idx)) return bad(ptr ? "d_idx is null (d_ptr is given)" : "d_ptr is null (d_idx is given)");
    if (csr && num_rows < 1) return bad("num_rows = " + std::to_string(num_rows) + " must be >= 1 with d_ptr");
    if (etype && !rel) return bad("d_etype needs d_rel");
    if (rel && !etype) return bad("d_rel needs d_etype");
    if (dot) {
        if (w1 || w2 || b1 || b2) return bad(std::string(w1 ? "d_w1" : w2 ? "d_w2" : b1 ? "d_b1" : "d_b2") + " is given, kind dot takes no weights");
        if (out_dtype != GNNAGG_DTYPE_F32) return bad("out_dtype: kind dot gives a fp32 out");
        if (flags) return bad("flags = " + std::to_string(flags) + ": kind dot takes no flag");
        if (combine != GNNAGG_PAIR_MUL) return bad("combine: kind dot takes GNNAGG_PAIR_MUL (0)");
        if (rel && num_rel < 1) return bad("num_rel = " + std::to_string(num_rel) + " must be >= 1 with d_rel");
    } else {
        if (rel) return bad("d_rel / d_etype are given, kind mlp takes no relations");
        if (hidden < 1) return bad("hidden = " + std::to_string(hidden) + " must be >= 1");
        if (n_out < 1) return bad("n_out = " + std::to_string(n_out) + " must be >= 1");
        if (!pair_supported(kind, combine, feat, hidden, n_out, x_dtype))
            return bad("feat = " + std::to_string(feat) + ", hidden = " + std::to_string(hidden) + ", n_out = " + std::to_string(n_out) +
                       " lie outside the range of gnnagg_pair_score_supported");
    }
    if (num_pairs > 0) {
        if (!coo && !csr) return bad("neither d_u / d_v nor d_ptr / d_idx is given");
        if (!hu) return bad("d_hu is null");
        if (!hv) return bad("d_hv is null");
        if (!dot && !w1) return bad("d_w1 is null");
        if (!dot && !w2) return bad("d_w2 is null");
        if (!out) return bad("d_out is null");
    }
    if (num_pairs == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: a divisor of feat and of both pitches, no wider than the alignment of hu and hv (their addresses OR-ed have the
    // alignment of the worse one) -- the rule of gnnagg_block_gcn_run; rel rows are feat floats apart and want the lane's width in floats
    const int fp = (int)gcd_ll(gcd_ll(feat, hu_pitch), hv_pitch);
    const void *xa = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(hu) | reinterpret_cast<uintptr_t>(hv));
    Geometry g = x16 ? typed_geometry(feat, xa, 2, fp) : pick_geometry(feat, xa, rel, nullptr, fp);
    if (x16 && rel) {
        int vec = g.vec;
        while (vec > 1 && (reinterpret_cast<uintptr_t>(rel) % (size_t)std::min(16, vec * 4)) != 0) vec >>= 1;
        if (vec != g.vec) {
            const int lanes = ceil_div(feat, vec);
            int group = 8;
            while (group < 64 && group < lanes) group <<= 1;
            g = {vec, group, ceil_div(lanes, group)};
        }
    }
    PairArgs a = {};
    a.u = u; a.v = v; a.ptr = ptr; a.idx = idx; a.src = src; a.etype = etype; a.rel = rel;
    a.hu = hu; a.hv = hv; a.w1 = w1; a.w2 = w2; a.b1 = b1; a.b2 = b2; a.out = out; a.upitch = hu_pitch; a.vpitch = hv_pitch;
    a.P = num_pairs; a.nrows = num_rows; a.feat = feat; a.num_rel = num_rel; a.hidden = hidden; a.n_out = n_out; a.ntiles = g.ntiles;
    a.cat = combine == GNNAGG_PAIR_CAT; a.relu = (flags & GNNAGG_FLAG_RELU) != 0; a.out_bf16 = out_dtype == GNNAGG_DTYPE_BF16;
    hipStream_t st = (hipStream_t)stream;
    int rc = GNNAGG_OK;
    if (dot) {
        if (x16) {
            DISPATCH_GEOM_16BIT(g, (launch_pair_dot<VEC, GROUP, __bf16>(a, st)))
        } else {
            DISPATCH_GEOM(g, (launch_pair_dot<VEC, GROUP, float>(a, st)))
        }
    } else {
        if (g.group < 16) g.group = 16;   // 16 groups are a row block of a tile
        a.tiles = ceil_div(num_pairs, kPairRows);
        const int grid = std::min(a.tiles, pair_grid_cap(combine, feat, hidden, n_out, x_dtype));
        const size_t lds = (size_t)pair_lds(feat, hidden, n_out, a.cat != 0, x16).bytes;
        if (x16) {
            DISPATCH_GEOM_16BIT(g, (rc = launch_pair_mlp<VEC, GROUP, __bf16>(a, grid, lds, st)))
        } else {
            DISPATCH_GEOM(g, (rc = launch_pair_mlp<VEC, GROUP, float>(a, grid, lds, st)))
        }
        if (rc != GNNAGG_OK) return rc;
    }
    HIP_TRY(hipGetLastError());
    return GNNAGG_OK;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_pair_score_run(int kind, int combine, const int *d_u, const int *d_v, const int *d_ptr, const int *d_idx, int num_rows,
                          int num_pairs, const int *d_src_nodes, const void *d_hu, long long hu_pitch, const void *d_hv, long long hv_pitch,
                          int x_dtype, int feat, const float *d_rel, const int *d_etype, int num_rel, const void *d_w1, const float *d_b1,
                          int hidden, const void *d_w2, const float *d_b2, int n_out, void *d_out, int out_dtype, int flags, void *hip_stream)
{
    return pair_score_run(kind, combine, d_u, d_v, d_ptr, d_idx, num_rows, num_pairs, d_src_nodes, d_hu, hu_pitch, d_hv, hv_pitch, x_dtype, feat,
                          d_rel, d_etype, num_rel, d_w1, d_b1, hidden, d_w2, d_b2, n_out, d_out, out_dtype, flags, hip_stream);
}

int gnnagg_pair_score_supported(int kind, int combine, int feat, int hidden, int n_out, int x_dtype)
{
    return pair_supported(kind, combine, feat, hidden, n_out, x_dtype) ? 1 : 0;
}

int gnnagg_pair_score_grid_cap(int kind, int combine, int feat, int hidden, int n_out, int x_dtype)
{
    if (!pair_supported(kind, combine, feat, hidden, n_out, x_dtype)) return 0;
    return kind == GNNAGG_PAIR_MLP ? pair_grid_cap(combine, feat, hidden, n_out, x_dtype) : 0x7fffffff;   // (dot: one window per lane group, no cap)
}

}  // extern "C"
#pragma GCC visibility pop
