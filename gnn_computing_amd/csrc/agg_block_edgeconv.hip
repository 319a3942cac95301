// agg_block_edgeconv.hip -- an edge-MLP layer on ONE sampled block in one launch: gnnagg_block_edgeconv_run (include/gnnagg.h section H,
// "Block EdgeConv layer").  The message of an edge is a two-layer MLP of BOTH endpoints, the row is a reduction of its messages:
//
//   m_p   = [x_i , x_s - x_i]  (diff: EdgeConv / DGCNN)   or   [x_i , x_s]  (cat: the MPNN / interaction-network message)
//   msg_p = relu(m_p . W1 + b1) . W2 + b2                                   [n_out], the contract of k_pair_mlp (pair_mlp.cuh)
//   out_i = act(reduce_{p in row i} msg_p)                                  reduce: sum | mean | max;  a row without edges: +0
//
// Ownership.  256 threads own kEcRB = 16 consecutive destination rows, the row blocks blockIdx.x, blockIdx.x + gridDim.x, ... per
// workgroup.  A row has ONE owner: no atomics, no scratch, and no bit of out depends on the grid.  The row block's kEcRB + 1 ptr entries
// lie in LDS (two copies by the parity of the row block: the epilogue of one block reads its copy while a fast wavefront loads the next).
// Edge tiles.  The positions ptr[r0] .. ptr[r0 + 16] are walked in tiles of kPairRows = 32 consecutive positions, whatever rows they
// belong to: a tile ends inside a row, a long row spans many tiles, an empty row owns no slot.
//   phase 1  one lane group per slot, the gathers of up to 4 slots in flight.  The lane that loads a slot's idx finds its row with a
//            binary search over the 17 ptr entries in LDS (the largest r with ptr[r] <= p: never an empty row), applies src_nodes to both
//            ids once, and notes the row in slot_row (-1 past the block's last position).  Both rows are loaded, m is formed in
//            registers -- diff: one fp32 subtraction, for bf16 rounded once -- and stored to the m tile; dead slots store zeros.
//   phase 2  z = relu(m . W1 + b1) into the z tile, phase 3  msg = z . W2 + b2 as fp32 into the message tile: pair_mlp_phase, the chains,
//            the B-operand sharing and the NRB = 1 split of k_pair_mlp; bf16: the weight images staged once per workgroup.
//   fold     thread c takes column c of the message tile: it walks the 32 slots in ascending order with the running value of the current
//            row in a register (sum / mean: a plain add; max: v > run ? v : run, with a NaN kept), loads it from the accumulator tile
//            [16, n_out] when the row changes and stores it back when the row ends or the tile does.  A row's messages are folded in
//            ascending CSR order from +0 (max: from -inf) in one chain, however the tiles cut it.
//   epilogue once per row block, thread c again: empty rows +0, mean divides by (float) deg as k_block_gcn does, the optional ReLU,
//            store_y_typed.  Column c of the accumulator tile is touched by thread c alone: it needs no barrier at all.
// LDS: [ptr copies, slot_row: 384 bytes][accumulator tile: 16 x pitch_n fp32][m tile: 32 rows of pitch_m  U  message tile: 32 x pitch_n
// fp32][z tile: 32 rows of pitch_z][bf16: wimg1][bf16: wimg2].  The message tile ALIASES the m tile (the region has the size of the
// larger): m is dead once every wavefront has left phase 2, which is what barrier 2 says.  The alias costs the k padding of the m tile,
// which is zeroed per tile instead of once.
// Four barriers per tile: (1) m tile and slot_row complete before phase 2 reads them; (2) z complete before phase 3 reads it, and every
// wavefront off the m tile before phase 3 writes messages over it; (3) messages complete before the fold reads them across wavefronts;
// (4) the fold done before the next tile's phase 1 writes m over the messages and slot_row.  One more per row block: its ptr copy is
// complete before phase 1 searches it.  Neither m, z nor a message reaches HBM.
#include "pair_mlp.cuh"

namespace gnnagg {
namespace {

constexpr int kEcRB = 16;                  // destination rows of a workgroup's row block: the block layers' tile
constexpr int kEcLdsBytes = 160 * 1024;    // LDS of a CU: the budget of every tile + both weight images
constexpr int kEcMaxDim = 256;             // feat, hidden and n_out (n_out <= kPairThreads: one thread per column in the fold)
constexpr int kEcPerCu = 8;                // workgroups per CU the grid is capped at (fewer where the LDS of a workgroup allows fewer)
constexpr int kEcHeadBytes = (2 * 32 + kPairRows) * (int)sizeof(int);   // two ptr copies of 32 ints, slot_row

struct EcArgs {
    const int *ptr, *idx, *src;
    const void *x, *w1, *w2;
    const float *b1, *b2;
    void *out;
    long long xpitch;   // elements between rows of x
    int num_dst, feat, hidden, n_out, ntiles, diff, is_max, mean, relu, out_bf16, row_blocks;
};

// kernel and launcher agree through ec_lds; P: the m and z tiles of pair_lds with k1 = 2 feat (pair_mlp.cuh)
struct EcLds {
    PairLds P;
    int pitch_n, acc_off, m_off, z_off, w1_off, w2_off, bytes;
};
__host__ __device__ constexpr EcLds ec_lds(int feat, int hidden, int n_out, bool b16)
{
    EcLds l = {};
    const int es = b16 ? 2 : 4;
    l.P = pair_lds(feat, hidden, n_out, true, b16);
    l.pitch_n = ((n_out + 15) & ~15) + 4;   // the 4 rows a D register group stores start 16 banks apart
    l.acc_off = kEcHeadBytes;
    l.m_off = l.acc_off + kEcRB * l.pitch_n * 4;
    const int mbytes = kPairRows * l.P.pitch_m * es, gbytes = kPairRows * l.pitch_n * 4;
    l.z_off = l.m_off + (mbytes > gbytes ? mbytes : gbytes);
    l.w1_off = l.z_off + kPairRows * l.P.pitch_z * es;
    l.w2_off = l.w1_off + (b16 ? ((hidden + 15) & ~15) * l.P.pitch_m * 2 : 0);
    l.bytes = l.w2_off + (b16 ? ((n_out + 15) & ~15) * l.P.pitch_z * 2 : 0);
    return l;
}

static bool ec_supported(int combine, int feat, int hidden, int n_out, int dtype)
{
    if (dtype != GNNAGG_DTYPE_F32 && dtype != GNNAGG_DTYPE_BF16) return false;
    if (combine != GNNAGG_EDGECONV_DIFF && combine != GNNAGG_EDGECONV_CAT) return false;
    if (feat < 1 || feat > kEcMaxDim || hidden < 1 || hidden > kEcMaxDim || n_out < 1 || n_out > kEcMaxDim) return false;
    return ec_lds(feat, hidden, n_out, dtype == GNNAGG_DTYPE_BF16).bytes <= kEcLdsBytes;
}

// workgroups a launch of this shape is capped at: as many per CU as their LDS allows, kEcPerCu at the most
static int ec_grid_cap(int feat, int hidden, int n_out, int dtype)
{
    const int per_cu = kEcLdsBytes / ec_lds(feat, hidden, n_out, dtype == GNNAGG_DTYPE_BF16).bytes;
    return std::min(std::max(per_cu, 1), kEcPerCu) * device_cu_count();
}

// A lane's VEC elements of an m row -- bf16: their bits in words, fp32: the values -- in pieces of at most 8 bytes.  A 16-byte LDS store
// that ends a basic block with a VALU write of its data registers behind the label is the place `make lint` looks for
// (scripts/check_store_hazard.py); phase 1 stores at the end of loop bodies, so it never issues one.
template <int VEC>
__device__ __forceinline__ void store_m_words(__bf16 *p, const unsigned (&w)[(VEC + 1) / 2])
{
    if constexpr (VEC == 1) {
        *reinterpret_cast<unsigned short *>(p) = (unsigned short)w[0];
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<unsigned *>(p) = w[0];
    } else {
#pragma unroll
        for (int k = 0; k < VEC / 4; ++k) reinterpret_cast<uint2 *>(p)[k] = make_uint2(w[2 * k], w[2 * k + 1]);
    }
}
template <int VEC>
__device__ __forceinline__ void store_m_floats(float *p, const float (&v)[VEC])
{
    if constexpr (VEC == 1) {
        *p = v[0];
    } else {
#pragma unroll
        for (int k = 0; k < VEC / 2; ++k) reinterpret_cast<float2 *>(p)[k] = make_float2(v[2 * k], v[2 * k + 1]);
    }
}
template <int VEC, typename TX>
__device__ __forceinline__ void store_m_raw(TX *p, const Pack<VEC, TX> &x)
{
    if constexpr (std::is_same<TX, __bf16>::value) store_m_words<VEC>(p, x.w);
    else store_m_floats<VEC>(p, x.v);
}
template <int VEC, typename TX>
__device__ __forceinline__ void store_m_rounded(TX *p, const float (&v)[VEC])
{
    if constexpr (std::is_same<TX, __bf16>::value) {
        unsigned w[(VEC + 1) / 2];
        if constexpr (VEC == 1) {
            w[0] = bf16x2_bits(v[0], 0.0f);
        } else {
#pragma unroll
            for (int k = 0; k < VEC / 2; ++k) w[k] = bf16x2_bits(v[2 * k], v[2 * k + 1]);
        }
        store_m_words<VEC>(p, w);
    } else {
        store_m_floats<VEC>(p, v);
    }
}

template <int VEC, int GROUP, typename TX>
__global__ __launch_bounds__(kPairThreads) void k_block_edgeconv(const EcArgs a)
{
    constexpr bool B16 = std::is_same<TX, __bf16>::value;
    constexpr int GPB = kPairThreads / GROUP, PASSES = kPairRows / GPB, UB = PASSES >= 4 ? 4 : PASSES;
    static_assert(GROUP >= 16 && PASSES * GPB == kPairRows && PASSES % UB == 0 && PASSES <= GROUP, "whole batches of passes over a tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char ec_smem[];
    const int F = a.feat, H = a.hidden, N = a.n_out;
    const EcLds L = ec_lds(F, H, N, B16);
    const int K1 = L.P.k1, Kp1 = L.P.kp1, Hp = L.P.hp, pitch_m = L.P.pitch_m, pitch_z = L.P.pitch_z, pitch_n = L.pitch_n;
    int *ptr_s = reinterpret_cast<int *>(ec_smem);
    int *slot_row = ptr_s + 64;
    float *acct = reinterpret_cast<float *>(ec_smem + L.acc_off);
    TX *mtile = reinterpret_cast<TX *>(ec_smem + L.m_off);
    float *msg = reinterpret_cast<float *>(ec_smem + L.m_off);   // the alias: see the header
    TX *ztile = reinterpret_cast<TX *>(ec_smem + L.z_off);
    const int tid = (int)threadIdx.x, lane = tid % GROUP, grp = tid / GROUP;

    // once per workgroup: the k padding of the z tile that no sub-tile of phase 2 covers (bf16: [roundup16(hidden), Hp)) and, bf16, the
    // images of both weights
    const int npad = Kp1 - K1;
    const int zcov = (H + 15) & ~15, zpad = Hp > zcov ? Hp - zcov : 0;
    for (int i = tid; i < kPairRows * zpad; i += kPairThreads) ztile[(i / zpad) * pitch_z + zcov + i % zpad] = (TX)0.0f;
    const __bf16 *wimg1 = nullptr, *wimg2 = nullptr;
    if constexpr (B16) {
        __bf16 *i1 = reinterpret_cast<__bf16 *>(ec_smem + L.w1_off), *i2 = reinterpret_cast<__bf16 *>(ec_smem + L.w2_off);
        pair_stage_weight(i1, pitch_m, Kp1, static_cast<const __bf16 *>(a.w1), K1, H);
        pair_stage_weight(i2, pitch_z, Hp, static_cast<const __bf16 *>(a.w2), H, N);
        wimg1 = i1;
        wimg2 = i2;
    }
    const TX *__restrict__ x = static_cast<const TX *>(a.x);
    const float acc0 = a.is_max ? -INFINITY : 0.0f;

    int par = 0;   // the copy of the ptr entries this row block uses
#pragma unroll 1
    for (int rb = (int)blockIdx.x; rb < a.row_blocks; rb += (int)gridDim.x, par ^= 32) {
        const int r0 = rb * kEcRB;
        const int nr = a.num_dst - r0 < kEcRB ? a.num_dst - r0 : kEcRB;
        int *ps = ptr_s + par;
        if (tid <= kEcRB) ps[tid] = a.ptr[tid <= nr ? r0 + tid : a.num_dst];   // rows past num_dst: empty
        if (tid < N)
            for (int r = 0; r < kEcRB; ++r) acct[r * pitch_n + tid] = acc0;
        __syncthreads();   // this row block's ptr copy is complete (the other copy may still be read by a slower wavefront's epilogue)
        const int e0 = ps[0], e1 = ps[kEcRB];
#pragma unroll 1
        for (int p0 = e0; p0 < e1; p0 += kPairRows) {
            // ---- phase 1: m rows into the m tile.  Lane j of a group fetches the ids of the group's slot of pass j (-1: a dead slot).
            for (int i = tid; i < kPairRows * npad; i += kPairThreads) mtile[(i / npad) * pitch_m + K1 + i % npad] = (TX)0.0f;
            int my_u = -1, my_v = 0;
            if (lane < PASSES) {
                const int slot = lane * GPB + grp, p = p0 + slot;
                int r = -1;
                if (p < e1) {
                    int lo = 0, hi = kEcRB;   // ps[0] <= p < ps[kEcRB]
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (ps[mid] <= p) lo = mid;
                        else hi = mid;
                    }
                    r = lo;
                    my_u = r0 + r;
                    my_v = a.idx[p];
                    if (a.src) {
                        my_u = a.src[my_u];
                        my_v = a.src[my_v];
                    }
                }
                slot_row[slot] = r;
            }
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
                            xu[b] = load_pack<VEC>(x + (size_t)ur[b] * (size_t)a.xpitch + col);
                            xv[b] = load_pack<VEC>(x + (size_t)vr[b] * (size_t)a.xpitch + col);
                        }
#pragma unroll
                    for (int b = 0; b < UB; ++b) {
                        TX *mrow = mtile + ((pass0 + b) * GPB + grp) * pitch_m;
                        store_m_raw<VEC, TX>(mrow + col, xu[b]);
                        if (a.diff) {
                            float d[VEC];
#pragma unroll
                            for (int k = 0; k < VEC; ++k) d[k] = xv[b].at(k) - xu[b].at(k);
                            store_m_rounded<VEC, TX>(mrow + F + col, d);
                        } else {
                            store_m_raw<VEC, TX>(mrow + F + col, xv[b]);
                        }
                    }
                }
            }
            __syncthreads();   // (1) the m tile and slot_row are complete

            // ---- phase 2: z = relu(m . W1 + b1) into the z tile
            if (((H + 15) >> 4) >= 4) pair_mlp_phase<kPairRB, kPairToZ, TX>(mtile, pitch_m, Kp1, a.w1, wimg1, K1, H, a.b1, ztile, pitch_z, Hp, a, 0);
            else pair_mlp_phase<1, kPairToZ, TX>(mtile, pitch_m, Kp1, a.w1, wimg1, K1, H, a.b1, ztile, pitch_z, Hp, a, 0);
            __syncthreads();   // (2) the z tile is complete; every wavefront has left the m tile, which the messages now overwrite

            // ---- phase 3: msg = z . W2 + b2, fp32, into the message tile
            if (((N + 15) >> 4) >= 4) pair_mlp_phase<kPairRB, kPairToMsg, TX>(ztile, pitch_z, Hp, a.w2, wimg2, H, N, a.b2, nullptr, pitch_n, 0, a, 0, msg);
            else pair_mlp_phase<1, kPairToMsg, TX>(ztile, pitch_z, Hp, a.w2, wimg2, H, N, a.b2, nullptr, pitch_n, 0, a, 0, msg);
            __syncthreads();   // (3) the message tile is complete

            // ---- fold: column tid of the 32 messages into the rows' accumulators, ascending slots
            if (tid < N) {
                int cur = -1;
                float run = 0.0f;
#pragma unroll 1
                for (int j = 0; j < kPairRows; ++j) {
                    const int r = slot_row[j];
                    if (r < 0) break;   // dead slots are the tile's last
                    if (r != cur) {
                        if (cur >= 0) acct[cur * pitch_n + tid] = run;
                        cur = r;
                        run = acct[r * pitch_n + tid];
                    }
                    const float v = msg[j * pitch_n + tid];
                    if (a.is_max) run = (v > run || v != v) ? v : run;   // the compare of chain_block_edges, and a NaN is kept
                    else run = run + v;
                }
                if (cur >= 0) acct[cur * pitch_n + tid] = run;
            }
            __syncthreads();   // (4) the fold is done with the message tile and slot_row, which the next phase 1 writes
        }
        // ---- epilogue: the row block's accumulators to out
        if (tid < N) {
            for (int r = 0; r < nr; ++r) {
                const int deg = ps[r + 1] - ps[r];
                float v[1] = {acct[r * pitch_n + tid]};
                if (deg == 0) v[0] = 0.0f;
                else if (a.mean) v[0] = v[0] / (float)deg;
                if (a.relu) v[0] = v[0] < 0.0f ? 0.0f : v[0];   // (a NaN stays a NaN: relu_pack)
                store_y_typed<1>(a.out, a.out_bf16, 1, 0, 0u, (size_t)(r0 + r) * N + tid, v);
            }
        }
    }
}

template <int VEC, int GROUP, typename TX>
static int launch_edgeconv(const EcArgs &a, int grid, size_t lds, hipStream_t st)
{
    if constexpr (GROUP < 16) {
        return fail(GNNAGG_ERR_STATE, "internal: gnnagg_block_edgeconv_run runs groups of 16 lanes and more");
    } else {
        static OncePerDevice big_lds_ok;   // > 64 KB of dynamic LDS needs the attribute: once per instantiation and device
        if (lds > 64 * 1024 && big_lds_ok.first()) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_block_edgeconv<VEC, GROUP, TX>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, kEcLdsBytes));
            big_lds_ok.done();
        }
        hipLaunchKernelGGL((k_block_edgeconv<VEC, GROUP, TX>), dim3((unsigned)grid), dim3(kPairThreads), lds, st, a);
        HIP_TRY(hipGetLastError());
        return GNNAGG_OK;
    }
}

static int block_edgeconv_run(const int *blk_ptr, const int *blk_idx, int num_dst, const int *src, const void *x, int x_dtype, long long x_pitch,
                              int feat, int combine, const void *w1, const float *b1, int hidden, const void *w2, const float *b2, int n_out,
                              void *out, int out_dtype, int reduce, int flags, void *stream)
{
    static const char *who = "gnnagg_block_edgeconv_run: ";
    auto bad = [&](const std::string &m) { return fail(GNNAGG_ERR_ARG, who + m); };
    if (num_dst < 0) return bad("num_dst = " + std::to_string(num_dst) + " is negative");
    if (combine != GNNAGG_EDGECONV_DIFF && combine != GNNAGG_EDGECONV_CAT) return bad("unknown combine " + std::to_string(combine));
    if (feat < 1) return bad("feat = " + std::to_string(feat) + " must be >= 1");
    if (hidden < 1) return bad("hidden = " + std::to_string(hidden) + " must be >= 1");
    if (n_out < 1) return bad("n_out = " + std::to_string(n_out) + " must be >= 1");
    if (x_pitch < feat) return bad("x_pitch = " + std::to_string(x_pitch) + " is below feat = " + std::to_string(feat));
    if (x_dtype != GNNAGG_DTYPE_F32 && x_dtype != GNNAGG_DTYPE_BF16) return bad("unknown x_dtype " + std::to_string(x_dtype));
    if (out_dtype != GNNAGG_DTYPE_F32 && out_dtype != GNNAGG_DTYPE_BF16) return bad("unknown out_dtype " + std::to_string(out_dtype));
    if (x_dtype == GNNAGG_DTYPE_F32 && out_dtype == GNNAGG_DTYPE_BF16) return bad("out_dtype: fp32 operands give a fp32 out, not a bf16 one");
    if (reduce != GNNAGG_REDUCE_SUM && reduce != GNNAGG_REDUCE_MEAN && reduce != GNNAGG_REDUCE_MAX)
        return bad("unknown reduce " + std::to_string(reduce));
    if (flags & ~GNNAGG_FLAG_RELU) return bad("flags = " + std::to_string(flags) + ": GNNAGG_FLAG_RELU is the only flag");
    if (!ec_supported(combine, feat, hidden, n_out, x_dtype))
        return bad("feat = " + std::to_string(feat) + ", hidden = " + std::to_string(hidden) + ", n_out = " + std::to_string(n_out) +
                   " lie outside the range of gnnagg_block_edgeconv_supported");
    if (num_dst > 0) {
        if (!blk_ptr) return bad("d_blk_ptr is null");
        if (!x) return bad("d_x is null");
        if (!w1) return bad("d_w1 is null");
        if (!w2) return bad("d_w2 is null");
        if (!out) return bad("d_out is null");
    }
    if (num_dst == 0) return GNNAGG_OK;

    const bool x16 = x_dtype == GNNAGG_DTYPE_BF16;
    // a lane's columns: the rule of gnnagg_block_gcn_run for x (a divisor of feat and of the pitch, no wider than x's alignment); the
    // second half of an m row starts at column feat, a multiple of the lane's width.  Groups of 8 lanes run as groups of 16.
    const int fp = (int)gcd_ll(feat, x_pitch);
    Geometry g = x16 ? typed_geometry(feat, x, 2, fp) : pick_geometry(feat, x, nullptr, nullptr, fp);
    if (g.group < 16) g.group = 16;
    EcArgs a;
    a.ptr = blk_ptr; a.idx = blk_idx; a.src = src; a.x = x; a.w1 = w1; a.w2 = w2; a.b1 = b1; a.b2 = b2; a.out = out; a.xpitch = x_pitch;
    a.num_dst = num_dst; a.feat = feat; a.hidden = hidden; a.n_out = n_out; a.ntiles = g.ntiles;
    a.diff = combine == GNNAGG_EDGECONV_DIFF; a.is_max = reduce == GNNAGG_REDUCE_MAX; a.mean = reduce == GNNAGG_REDUCE_MEAN;
    a.relu = (flags & GNNAGG_FLAG_RELU) != 0; a.out_bf16 = out_dtype == GNNAGG_DTYPE_BF16;
    a.row_blocks = ceil_div(num_dst, kEcRB);
    const int grid = std::min(a.row_blocks, ec_grid_cap(feat, hidden, n_out, x_dtype));
    const size_t lds = (size_t)ec_lds(feat, hidden, n_out, x16).bytes;
    hipStream_t st = (hipStream_t)stream;
    int rc = GNNAGG_OK;
    if (x16) {
        DISPATCH_GEOM_16BIT(g, (rc = launch_edgeconv<VEC, GROUP, __bf16>(a, grid, lds, st)))
    } else {
        DISPATCH_GEOM(g, (rc = launch_edgeconv<VEC, GROUP, float>(a, grid, lds, st)))
    }
    return rc;
}

}  // namespace
}  // namespace gnnagg

using namespace gnnagg;

#pragma GCC visibility push(default)
extern "C" {

int gnnagg_block_edgeconv_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const void *d_x, int x_dtype,
                              long long x_pitch, int feat, int combine, const void *d_w1, const float *d_b1, int hidden, const void *d_w2,
                              const float *d_b2, int n_out, void *d_out, int out_dtype, int reduce, int flags, void *hip_stream)
{
    return block_edgeconv_run(d_blk_ptr, d_blk_idx, num_dst, d_src_nodes, d_x, x_dtype, x_pitch, feat, combine, d_w1, d_b1, hidden, d_w2, d_b2,
                              n_out, d_out, out_dtype, reduce, flags, hip_stream);
}

int gnnagg_block_edgeconv_supported(int combine, int feat, int hidden, int n_out, int x_dtype)
{
    return ec_supported(combine, feat, hidden, n_out, x_dtype) ? 1 : 0;
}

int gnnagg_block_edgeconv_grid_cap(int combine, int feat, int hidden, int n_out, int x_dtype)
{
    return ec_supported(combine, feat, hidden, n_out, x_dtype) ? ec_grid_cap(feat, hidden, n_out, x_dtype) : 0;
}

}  // extern "C"
#pragma GCC visibility pop
