/*
 * gnnagg.h -- C-ABI of libgnnagg.so, the MI355X-native neighbor-aggregation library.
 *
 * This is the drop-in boundary for the hot path of xxcclong/GNN-Computing
 * (include/aggregator.h, aggr_gcn.h, aggr_gat.h, spmm.h, graph_schedule.h, src/data.cu).
 * Plain pointers and sizes only; every `d_*` / "device" pointer is HIP device memory owned by
 * the caller, every `h_*` / "host" pointer is host memory.  No torch / C++ types cross it.
 *
 * Section A mirrors, name for name, the flat API the reference's own PyTorch binding is written
 * against (reference Figure7/kernel.cpp:15-35, defined in Figure7/kernel_generated.cu:15-74);
 * a reference-side binding only has to link this library instead of compiling the CUDA headers.
 * Section B is the same functionality with status codes, streams, reductions and heads.
 * Section C is the host graph preparation (reference src/data.cu, include/graph_schedule.h).
 * Section D is the 1-D row-partition / halo-exchange support (no reference counterpart:
 * the reference asserts GPUNUM == 1, Figure9/main.cu:19).
 *
 * Error model: Section A keeps the reference's abort-on-error behaviour (include/util.h:82-104:
 * message with the failing call, then exit(1)) unless gnnagg_set_abort_on_error(0) was called, in
 * which case the error is recorded and the call returns (0 for the *_init functions).
 * Sections B-D return GNNAGG_OK or an error code; gnnagg_last_error() gives the text.
 * All `run` entry points are asynchronous on the handle's stream (reference: run() never
 * synchronises, aggr_gcn.h:396,407); schedule / create are synchronous.
 */
#ifndef GNNAGG_H
#define GNNAGG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNAGG_OK 0
#define GNNAGG_ERR_ARG 1    /* bad argument / contract violation (reference: assert) */
#define GNNAGG_ERR_HIP 2    /* HIP runtime failure (reference: checkCudaErrors) */
#define GNNAGG_ERR_STATE 3  /* e.g. scheduled run without a schedule (reference: assert aggr_gcn.h:392) */
#define GNNAGG_ERR_IO 4     /* graph files missing / malformed (reference: assert(fexist), data.cu:40) */

/* enum Schedule, reference include/graph_schedule.h:8-14 (same values) */
#define GNNAGG_SCHED_LOCALITY 0
#define GNNAGG_SCHED_NEIGHBOR_GROUPING 1
#define GNNAGG_SCHED_LOCALITY_NEIGHBOR_GROUPING 2
#define GNNAGG_SCHED_NOP 3

/* reduction over a row's neighbors */
#define GNNAGG_REDUCE_SUM 0  /* reference aggr_gcn.h:13-35; val == NULL means weight 1 */
#define GNNAGG_REDUCE_MEAN 1 /* sum then / deg   (reference: caller passes val = 1/deg) */
#define GNNAGG_REDUCE_MAX 2  /* max_e val*x, 0 for an empty row (no reference kernel) */

/* run modes */
#define GNNAGG_MODE_ROWS 0      /* `scheduled = 0`: one work item per CSR row, sequential FMA chain in CSR order */
#define GNNAGG_MODE_SCHEDULED 1 /* `scheduled = 1`: work items = groups of the last schedule() call */
#define GNNAGG_MODE_BALANCED 2  /* library-chosen chunking of long rows (gnnagg_schedule_balanced) */

typedef int64_t gnnagg_handle; /* opaque; same width as the reference's `int64_t at` (kernel.cpp:15) */

const char *gnnagg_last_error(void);
int gnnagg_version(void);
void gnnagg_set_abort_on_error(int on);

/* ---------------------------------------------------------------------------------------------
 * A. Flat API -- one-to-one with reference Figure7/kernel.cpp:15-35
 * ------------------------------------------------------------------------------------------- */
/* kernel.cpp:15 / kernel_generated.cu:15-19.  ptr[num_v+1], idx[num_e], val[num_e] on device,
 * borrowed for the life of the handle (the reference's torch path never frees them either). */
int64_t GCN_init_impl(int *ptr, int *idx, float *val, int num_v, int num_e);
/* kernel.cpp:17 / kernel_generated.cu:21-24 (Aggregator_GCN::updateval, aggr_gcn.h:540-544) */
void GCN_update_val_impl(int64_t at, float *val);
/* kernel.cpp:19 / kernel_generated.cu:26-32 (run_with_feat, aggr_gcn.h:411-444).  `blocksize` is a
 * CUDA block-geometry hint in the reference; accepted and ignored. */
void GCN_run_impl(int64_t at, float *feat, float *out_feat, int blocksize, int scheduled, int featlen);
/* kernel.cpp:21 / kernel_generated.cu:34-39: schedule(neighbor_grouping, arr), arr[0] = NG */
void GCN_schedule_impl(int64_t at, int *arr);
/* kernel.cpp:23 / kernel_generated.cu:41-45 */
int64_t GAT_init_impl(int *ptr, int *idx, int num_v, int num_e);
/* kernel.cpp:25 / kernel_generated.cu:47-50 (Aggregator_GAT::run_with_feat, aggr_gat.h:355-394);
 * att is [V,2]; leaky slope 0.2 (aggr_gat.h:347) */
void GAT_run_impl(int64_t at, float *feat, float *att, float *out_feat, int blocksize, int scheduled, int featlen);
/* kernel.cpp:27-31 / kernel_generated.cu:52-65 (aggr_gat.h:402-425) */
void GAT_run_u_add_v_impl(int64_t at, float *att, float *outval, int blocksize);
void GAT_run_add_to_center_impl(int64_t at, float *inval, float *outatt, int blocksize);
void GAT_run_div_each_impl(int64_t at, float *inatt, float *inoutval, int blocksize);
/* kernel.cpp:35 / kernel_generated.cu:69-74 */
void GAT_schedule_impl(int64_t at, int *arr);

/* ---------------------------------------------------------------------------------------------
 * B. Status-returning API (streams, reductions, heads, lifetime)
 * ------------------------------------------------------------------------------------------- */
/* Aggregator_GCN ctor, aggr_gcn.h:365-374.  d_val may be NULL (implicit weight 1). */
int gnnagg_gcn_create(const int *d_ptr, const int *d_idx, const float *d_val, int num_v, int num_e,
                      gnnagg_handle *out);
/* Aggregator_GAT ctor, aggr_gat.h:302-313 */
int gnnagg_gat_create(const int *d_ptr, const int *d_idx, int num_v, int num_e, gnnagg_handle *out);
/* Frees what the handle allocated (schedules, scratch).  Never frees caller pointers.  Waits for the handle's stream first.  May be called
 * while a call on ANOTHER handle is being captured into a HIP graph (a garbage collector frees handles where it finds them): the frees
 * and waits are made in the relaxed capture mode and leave that capture valid -- provided that the capturing stream is a NON-BLOCKING one (hipStreamNonBlocking,
 * as torch's are) or the dying handle's stream is not the null stream: the wait for the legacy null stream is a wait for every blocking
 * stream, and a blocking stream that is capturing is still invalidated by it.  A handle whose own call is being captured, or is held by
 * a capture that will still be replayed, must outlive it. */
int gnnagg_destroy(gnnagg_handle h);
/* hipStream_t as void*; NULL = default stream.  Work of later calls is enqueued there, and whatever the library reads of the caller's
 * arrays on the HOST (the CSR, when a schedule or plan is built) is copied on that stream and waited for -- i.e. ordered behind the
 * caller's work on it.  Set it before schedule() / the first run when the arrays were produced on a non-null stream. */
int gnnagg_set_stream(gnnagg_handle h, void *hip_stream);
/* Per-handle knobs.  Every knob is an option; the four a C++ driver linked against the class shim cannot reach through code also
 * read an environment variable (in brackets) when the handle is made.  INTEGRATION.md section 5 is the table of all of them.
 *   "partitions" [GNNAGG_PARTITIONS]      -1 the library decides (average degree >= 96), 0 never, N > 0: N source ranges for the balanced mode
 *   "tile_width"                          floats per column tile of the 2-D blocked balanced mode: 32 / 64 / 128 / 256 (64)
 *   "slice_kb"                            target size of the X slice an XCD's L2 holds (4096)
 *   "scratch_limit_mb"                    > 0: cap on the scratch (partial rows + tiled image of X) the blocked order may take;
 *                                         a handle that would need more -- or more than half of the free device memory, or
 *                                         whose allocation fails -- moves to the chunked plan for good
 *   "fast_rows" [GNNAGG_FAST_ROWS]        1: GNNAGG_MODE_ROWS (`scheduled = 0`) runs the balanced order -- results within the
 *                                         1e-5 bound instead of bit-exact CSR-order chains; 0: canonical order.  Default 0 for
 *                                         handles made through this section, 1 for the reference-facing surfaces (see
 *                                         "reference_defaults"); the environment variable overrides both
 *   "reference_defaults"                  1: what GCN_init_impl / GAT_init_impl, the C++ class shim (include/compat) and the pybind-
 *                                         named Python functions apply to the handles they make: fast_rows = 1 unless
 *                                         GNNAGG_FAST_ROWS says otherwise.  A reference driver's run(vin, vout, B, 0) is then as
 *                                         fast as its scheduled run; aggr_gcn's own result differs from it by association only
 *   "fast_scheduled" [GNNAGG_FAST_SCHEDULED]  1 (default): GNNAGG_MODE_SCHEDULED (`scheduled = 1`) runs the balanced order.  The
 *                                         reference's scheduled kernels add group partials with atomicAdd (aggr_gcn.h:112,
 *                                         aggr_gat.h:196-203): every association is one of its legal results.  A schedule must
 *                                         still have been made; num_target / get_schedule / mode_params of GNNAGG_MODE_SCHEDULED
 *                                         keep describing the user's groups, the order that RUNS is the one GNNAGG_MODE_BALANCED's
 *                                         queries describe; GAT calls that ask for newval keep the scheduled order -- and so does a
 *                                         locality schedule that DROPPED edges (total_num_v below the largest column id + 1,
 *                                         graph_schedule.h:23-44): the balanced order covers every edge.  0: the user's groups,
 *                                         folded in the restated order (bit-exact against the oracle)
 *   "aux_stream" [GNNAGG_AUX_STREAM]      0: GNNAGG_MODE_ROWS runs its hub rows on the handle's stream, before the short rows, instead of
 *                                         beside them on an auxiliary stream (slower by the hub rows' duration, but the process keeps
 *                                         a single queue); 1 (default)
 *   "rows_blocked"                        1 (default): GNNAGG_MODE_ROWS runs its canonical chains on the 2-D blocked order where the
 *                                         graph allows it (gnnagg_rows_blocked_ranges); 0: always the row kernels.  Same bits either way
 *                                         (GAT included: non-finite weights and zero denominators, "Attention logits" below)
 *   "rows_medium_edges"                   GNNAGG_MODE_ROWS on the row kernels: rows above this many edges, up to the hub threshold
 *                                         max(1024, 16 x mean degree), run on 128-thread workgroups (one gather wavefront + the chain)
 *                                         instead of one lane group each.  0 (default): max(128, E / 4500), an empty class from 4.6 M
 *                                         edges on; -1: no such class.  Same bits whatever the value
 *   "rows_hub_tile"                       GNNAGG_MODE_ROWS, hub rows (GCN flavours): 32- or 64-column tiles per workgroup of the long-row
 *                                         kernel; 0 (default): 64 where the launch has more (row, tile) items than twice the CUs.  Same bits
 *   "rows_hub_edges"                      chained rows mode: rows with a (row, range) sub-row above this many edges leave the chained
 *                                         launches for the long-row kernel (0: the library's rule)
 * Twelve options.  [GNNAGG_XCD_REMAP] 0 / 1 / 2 (workgroup -> XCD mapping: identity / equal-count / work-balanced ranges, default 2) is an
 * environment-only measurement switch.  libgnnagg_extras.so (-DGNNAGG_EXTRAS, Section E) additionally knows "partition_min_degree",
 * the older forms "retile", "tiled", "spans", "inkernel_combine", "host_plan" and [GNNAGG_PLAN]: second-tier A / B material, constants in
 * the shipped library.
 * Options that change the library-chosen order drop it; it is rebuilt on the next use.
 * History is not visible: a handle that has run, been re-scheduled and had options moved and moved back computes bit for bit, and reports
 * through every query, what a new handle with the same configuration calls does (tests/test_gpu_handle_lifetime.py) -- with the one
 * exception stated above, the move to the chunked plan "for good" under "scratch_limit_mb", which lasts until "partitions" is set again.
 * A call that is refused for its arguments (GNNAGG_ERR_ARG, GNNAGG_ERR_STATE) leaves the handle as it was: the schedule in force, the plans
 * and gnnagg_last_nn_path are unchanged.  (A call that fails on an allocation or another HIP error may have dropped what it was rebuilding.)
 * Captured HIP graphs: a captured call holds the handle's scratch and plan pointers, so any later call on the handle that grows scratch (a
 * wider feat, more heads, another dtype) or drops a plan (one of the options that change the order, gnnagg_schedule,
 * gnnagg_schedule_balanced) invalidates the capture, which must be captured again before it is replayed. */
int gnnagg_set_option(gnnagg_handle h, const char *name, int value);
/* What the library-chosen blocked order cost to build and holds (the reference prints its schedule time, graph_schedule.h:125-127):
 * wall seconds of the last construction of the balanced mode's 2-D blocked order (0: the handle runs the chunked plan, built in O(V))
 * and of the rows mode's chain plan; device bytes of the plans' arrays; device bytes of the scratch the runs so far have reserved
 * (partial rows, tiled images of X / Y, compact attention terms).  Any output pointer may be NULL. */
int gnnagg_plan_info(gnnagg_handle h, double *plan_seconds, double *rows_plan_seconds, long long *plan_bytes, long long *scratch_bytes);
/* Aggregator_GCN::updateval, aggr_gcn.h:540-544: re-aliases the edge values (borrowed; read at run time). */
int gnnagg_update_val(gnnagg_handle h, const float *d_val);

/* Per-row degrees for aggregations that are computed in TWO passes over disjoint edge sets of the same rows (the row-partitioned
 * step of section D: local-source edges while the halo exchange is in flight, halo-source edges after it).  d_row_aux[num_v]
 * (int32, borrowed, read at run time; NULL switches it off) changes GNNAGG_MODE_BALANCED runs of this handle as follows:
 *   GNNAGG_REDUCE_MEAN  divides by d_row_aux[row] -- the row's degree in the WHOLE graph -- instead of the edges this handle holds
 *                       (the reference's mean is val = 1/deg per edge, Figure7/our.py: every term is x/deg, so the two passes add);
 *                       GNNAGG_FLAG_ACCUMULATE then adds the pass's quotient to what the row holds
 *   GNNAGG_REDUCE_MAX   with GNNAGG_FLAG_ACCUMULATE: y = max(y, result) where d_row_aux[row] > 0 edges were already folded into y
 *                       by the earlier pass, y = result where none were (y then holds the empty row's 0, not a maximum)
 * GNNAGG_REDUCE_SUM is not affected.  Rows this handle has no edges for are left untouched by an accumulating run. */
int gnnagg_set_row_aux(gnnagg_handle h, const int *d_row_aux);

/* Aggregator::schedule, aggregator.h:67-99 / Aggregator_GCN::schedule aggr_gcn.h:501-538.
 * kind = GNNAGG_SCHED_*; param[0] = NG or par_num, param[1] = NG for the combined schedule.
 * total_num_v: the reference reads the global `n` (aggregator.h:79); pass num_v for a full graph. */
int gnnagg_schedule(gnnagg_handle h, int kind, const int *param, int total_num_v);
/* Library-chosen chunking of long rows into work items of <= chunk edges (0 = choose from the
 * degree distribution).  Used by GNNAGG_MODE_BALANCED. */
int gnnagg_schedule_balanced(gnnagg_handle h, int chunk);
/* Summation order of GNNAGG_MODE_BALANCED: rows are cut into chunks of *chunk edges (partial FMA chains
 * from 0, like the reference's neighbor groups); seg_chunks > 0 means the chunk partials of a row are folded
 * in ascending order inside segments of seg_chunks chunks and the segment sums are then added in ascending
 * order; 0 means one flat ascending fold.  (Rows of at most seg_chunks chunks are identical either way.) */
int gnnagg_balanced_params(gnnagg_handle h, int *chunk, int *seg_chunks);
/* The same for any mode.  GNNAGG_MODE_SCHEDULED with a neighbor-grouping schedule: *chunk = NG and *seg_chunks = 16
 * when the plan kernel runs it (the reference adds the group partials with fp32 atomics in arbitrary order,
 * aggr_gcn.h:112, so every fixed order is one of its outcomes up to association), 0 (flat ascending fold) when NG is
 * so small that the one-item-per-lane-group kernel is used, and always 0 for the locality schedules.
 * GNNAGG_MODE_ROWS: one chain per row (*chunk = INT_MAX, *seg_chunks = 0). */
int gnnagg_mode_params(gnnagg_handle h, int mode, int *chunk, int *seg_chunks);
/* Source partitions of the balanced mode: 0 for the chunked order reported by gnnagg_balanced_params; P > 0 when the library
 * chose the source-partitioned (2-D blocked) order for a high-degree graph (avg degree >= 96): the groups are those of
 * gnnagg_locality_schedule(par_num = P, neighbor_num = chunk, total = *total_cols) -- partition-major, row-minor, CSR order
 * inside a sub-row -- folded flat in ascending group order per row; gnnagg_get_schedule(h, GNNAGG_MODE_BALANCED, ...) returns
 * them.  *total_cols (may be NULL) = largest neighbor id + 1: the column count the ranges are cut from (the CSR need not be
 * square). */
int gnnagg_balanced_partitions(gnnagg_handle h, int *partitions, int *total_cols);
/* GNNAGG_MODE_ROWS of a GCN handle: *ranges = the number of source ranges when the canonical chains run on the 2-D blocked order
 * (option "rows_blocked", default 1: graphs of average degree >= "partition_min_degree" whose rows list their neighbors in ascending
 * order -- range after range is then the CSR order, and every (row, column) stays the reference's one sequential chain,
 * aggr_gcn.h:13-35, with the gathers served by the L2; sum / mean, feature widths above 32), 0 when the row kernels run.  The count is the
 * chain plan's, which is cut on first use for the width of the run (or, by this query, for 256 columns): it may differ between two handles with
 * the same options, the results of their runs do not. */
int gnnagg_rows_blocked_ranges(gnnagg_handle h, int *ranges);
/* Aggregator::num_target (aggregator.h:126), and the scheduled arrays copied to host buffers
 * (any may be NULL): ptr_s[num_target+1], idx_s[ptr_s[num_target]], target[num_target], val_s. */
int gnnagg_num_target(gnnagg_handle h, int mode, int *out);
int gnnagg_get_schedule(gnnagg_handle h, int mode, int *h_ptr_s, int *h_idx_s, int *h_target, float *h_val_s);

/* Aggregator_GCN::run / run_with_feat, aggr_gcn.h:379-444.  x,y are [V,feat] row-major fp32 on
 * device.  mode = GNNAGG_MODE_*, reduce = GNNAGG_REDUCE_*.  y is fully overwritten. */
int gnnagg_gcn_run(gnnagg_handle h, const float *d_x, float *d_y, int feat, int mode, int reduce);
/* Same with flags.  GNNAGG_FLAG_ACCUMULATE (balanced mode, sum): y += A.x -- the row's result is computed as
 * usual and added to the value already in y with one fp32 add; rows without edges are left untouched.  Used by the
 * row-partitioned path to add the halo-column part after the local-column part. */
#define GNNAGG_FLAG_ACCUMULATE 1
/* GNNAGG_FLAG_RELU (any mode / reduce): y = max(result, 0) -- the activation that follows the aggregation in the
 * reference's 3-layer model (Figure7/our.py:176, F.relu on the output of gcn_run), applied to the finished row by the
 * producing kernel instead of one more pass over y.  With GNNAGG_FLAG_ACCUMULATE: y = max(y + A.x, 0), rows without
 * edges included.
 * Non-finite features (GCN and GAT, every mode): plain IEEE propagation -- an Inf or NaN in x[s] reaches exactly the rows that have s
 * as a neighbor (the padding of the kernels never multiplies a real source by zero); GNNAGG_FLAG_RELU keeps a NaN (-Inf becomes 0);
 * GNNAGG_REDUCE_MAX over a NaN operand is unspecified. */
#define GNNAGG_FLAG_RELU 2
int gnnagg_gcn_run_ex(gnnagg_handle h, const float *d_x, float *d_y, int feat, int mode, int reduce, int flags);
/* y = A.x with x / y in the given element types (no reference counterpart: the reference's surface is float *).  Accumulation,
 * partial rows and the hub fold stay fp32; a bf16 y is ONE round-to-nearest-even of the fp32 result, at the store.  bf16 -> fp32 is
 * exact and the chains keep their order, so a bf16 x gives bit for bit what gnnagg_gcn_run_ex gives on x widened to fp32.
 * (F32, F32) is gnnagg_gcn_run_ex exactly.  The other three combinations:
 *   mode    GNNAGG_MODE_BALANCED (a handle on the 2-D blocked order -- high-degree graphs -- runs the chunked plan, built beside it
 *           on first use); GNNAGG_MODE_SCHEDULED where the plan kernel runs it ("fast_scheduled" = 1, the default, or a
 *           neighbor-grouping schedule); GNNAGG_MODE_ROWS where "fast_rows" maps it to the balanced order
 *   reduce  sum, mean, max;   flags  GNNAGG_FLAG_RELU; GNNAGG_FLAG_ACCUMULATE with a fp32 y (the accumulation target stays fp32)
 *   feat    any F >= 1; x / y at any 2-byte offset (narrower lanes)
 * Everything else returns GNNAGG_ERR_ARG with a gnnagg_last_error() text naming the combination -- an unknown dtype code, ACCUMULATE
 * into a bf16 y, the canonical rows mode (fast_rows = 0), an order the item kernels run -- and nothing falls back to fp32.
 * gnnagg_gcn_run_with_nn is fp32 only (its typed form: gnnagg_gcn_run_with_nn_typed); the fused GAT aggregation has its own typed
 * call, gnnagg_gat_run_typed. */
#define GNNAGG_DTYPE_F32 0
#define GNNAGG_DTYPE_BF16 1
int gnnagg_gcn_run_typed(gnnagg_handle h, const void *d_x, int x_dtype, void *d_y, int y_dtype, int feat, int mode, int reduce,
                         int flags);
/* Measurement aid (no reference counterpart): the gather ceiling of gnnagg_gcn_run(h, d_x, ., feat, mode, SUM).  Launches
 * the same kernel over the same work items with the same descriptor / neighbor-id / edge-value loads and the same
 * feature-row gathers (same addresses, same batching), but consumes the data with integer XORs instead of the
 * dependent FMA chains and stores nothing.  Its duration is what the memory system needs to deliver this launch's
 * gathers; bench.py reports roofline.frac = probe time / kernel time.  GNNAGG_MODE_BALANCED (or a neighbor-grouping
 * schedule that runs on the plan kernel); asynchronous on the handle's stream. */
int gnnagg_gcn_probe_gather(gnnagg_handle h, const float *d_x, int feat, int mode);
/* The same for gnnagg_gat_run on the 2-D blocked balanced order (k_gat_span): neighbor ids, compact attention terms and
 * tile-row gathers as in the real run, no exp, no chain, no store.  GNNAGG_ERR_ARG on the other GAT paths. */
int gnnagg_gat_probe_gather(gnnagg_handle h, const float *d_x, const float *d_att, int feat, int heads, int mode);
/* Measurement aid (no reference counterpart): the rate the memory system offers to ROW GATHERS in these kernels' own access shape,
 * independent of any graph.  One launch; lane groups of L lanes (L = the power of two >= seg_bytes / 16, 8 .. 64; 256 / L groups per
 * workgroup) each take `ids_per_group` consecutive entries of d_ids (coalesced id loads, 8 gathers in flight) and read seg_bytes at
 * d_rows + id * pitch_bytes; the data is XOR-consumed and never stored.  Where the gathered rows live -- one XCD's L2, the Infinity
 * Cache, HBM -- is the caller's choice of ids (workgroup b runs on XCD b % 8).  seg_bytes and pitch_bytes multiples of 16,
 * ids_per_group a multiple of L, n_ids a multiple of ids_per_group x 256 / L.  Asynchronous on hip_stream.  bench.py times this
 * launch to quote each roofline fraction against a ceiling that bounds the bytes it divides (gather-model bytes are cache-served). */
int gnnagg_probe_row_gather(const void *d_rows, long long pitch_bytes, int seg_bytes, const int *d_ids, long long n_ids, int ids_per_group,
                            void *hip_stream);
/* Aggregator_GCN::run_clock, aggr_gcn.h:462-489 (Figure 8 load-balance study).  Runs the one-item-per-lane-group
 * kernel of mode rows (the reference's aggr_gcn_clock) or scheduled (aggr_gcn_target_clock) with per-workgroup
 * stamps: d_timer[3b] = start, [3b+1] = end (ticks of the constant wall clock, gnnagg_wall_clock_hz), [3b+2] = CU id.
 * Call with d_timer == NULL to get *num_blocks (the timer needs 3 * num_blocks entries; pass the run's d_x / d_y to the
 * query when they may be less than 16-byte aligned -- the lane geometry, and with it the grid, follows their alignment).
 * With d_timer != NULL, *num_blocks is in/out: in = the workgroups d_timer has room for (GNNAGG_ERR_ARG when the launch
 * needs more), out = the workgroups launched. */
int gnnagg_gcn_run_clock(gnnagg_handle h, const float *d_x, float *d_y, int feat, int mode, unsigned long long *d_timer,
                         int *num_blocks, int *waves_per_cu);
long long gnnagg_wall_clock_hz(void);
/* Aggregator_GCN::runEdgeWise, aggr_gcn.h:446-460 (edge-parallel atomics; any feat). */
int gnnagg_gcn_run_edgewise(gnnagg_handle h, const float *d_x, float *d_y, int feat);
/* matmul_NN, include/dense.h:4-23: c[m,n] = a[m,k] . b[k,n], row-major fp32 (the dense combine after an
 * aggregation).  f32 MFMA, accumulation in ascending k. */
int gnnagg_matmul_nn(const float *d_a, const float *d_b, float *d_c, int m, int n, int k, void *hip_stream);
/* gnnagg_matmul_nn with a / b / c in the given element types (GNNAGG_DTYPE_F32 / GNNAGG_DTYPE_BF16; no reference counterpart).
 * (F32, F32, F32) is gnnagg_matmul_nn exactly: the same launch, the same bits.  (BF16, BF16, F32) and (BF16, BF16, BF16) run the bf16
 * MFMA (v_mfma_f32_32x32x16_bf16) with fp32 accumulators:
 *   sizes   any m, n, k >= 0 (k == 0: c = +0; m == 0 or n == 0: nothing is done); a / b / c at any element-aligned address (a 2-byte
 *           offset for bf16, a 4-byte one for a fp32 c: narrower loads, the same kernel)
 *   sums    a bf16 x bf16 product is exact in fp32; the order and rounding of the additions inside a bf16 MFMA are not documented, so
 *           the result is NOT bit-comparable to the ascending-k chain of gnnagg_matmul_nn.  What holds: where every partial sum in any
 *           order is an integer below 2^24 the result is that integer exactly; otherwise |c - c64| <= 1e-5 . sum_k |a_k b_k| against
 *           the float64 product of the same bf16 operands (16-bit accumulation would sit at 4-5e-4)
 *   tails   k, row and column tails contribute exact zeros built in registers; nothing behind an operand is read, and a NaN / inf in
 *           row r of a reaches row r of c only
 *   bf16 c  the same accumulation, then ONE round-to-nearest-even of what the fp32-c call stores (NaN kept, overflow to inf)
 *   the same inputs give the same bits on every call; no allocation, synchronisation or memset: capturable in a HIP graph
 * Everything else returns GNNAGG_ERR_ARG with a gnnagg_last_error() text naming the combination -- an unknown dtype code, a and b of
 * different types, fp32 operands with a bf16 c -- nothing is converted and nothing falls back.  Arguments are checked before any
 * device call.  gnnagg_gcn_run_with_nn stays fp32 only; gnnagg_gcn_run_with_nn_typed is the aggregation with this product behind it. */
int gnnagg_matmul_nn_typed(const void *d_a, int a_dtype, const void *d_b, int b_dtype, void *d_c, int c_dtype,
                           int m, int n, int k, void *hip_stream);
/* The front half of a GAT layer in one call (no reference counterpart; Figure7/our.py:179-188 takes two dense launches for it):
 *   feat[m, n] = x[m, k] . w[k, n], n = heads . D, and att[m, heads, 2] fp32, the array gnnagg_gat_run reads:
 *   att[r, h, 0] = sum_c feat[r, h D + c] . a_dst[h, c] (the centre term),  att[r, h, 1] = the same sum with a_src (the source term).
 *   feat    bit for bit what gnnagg_matmul_nn / gnnagg_matmul_nn_typed writes for the same operands and feat_dtype (the same kernels)
 *   att     taken from feat AS STORED (a bf16 feat is widened); products and sums in fp32, in an order that is fixed but unspecified:
 *           |att - att64| <= 1e-5 . sum_c |feat . a| against float64 on the stored feat, exact where every partial sum is an integer below 2^24
 *   types   (x, w and a_dst / a_src, feat): (F32, F32, F32), (BF16, BF16, F32), (BF16, BF16, BF16); att is always fp32
 *   sizes   m == 0: nothing is done; k == 0 (or n == 0): +0 in feat and att.  Every operand at any element-aligned address.  Nothing behind an
 *           operand is read, nothing outside feat[m . n] and att[m . heads . 2] is written; a NaN / inf in row r of x reaches row r only
 *   *path   (may be NULL; written on the host) 1: the attention terms came out of the GEMM kernel's epilogue -- bf16 operands, n <= 128 with
 *           all of k in one LDS image (k <= 602 at n = 128), one head or D = 8, 16, 32, 64; 2: a row-dot kernel behind the GEMM read feat back
 *           (every fp32 call, every other bf16 shape, and the zero fill of k == 0); 0: m == 0.  Measured: profiles/gat_project/
 *           (the environment variable GNNAGG_GAT_PROJECT_FUSE=0, read at every call, sends every call down path 2: the measurement's switch)
 *   Asynchronous on hip_stream; no allocation, no synchronisation: a warm call can be captured in a HIP graph (it has no handle and no
 *           scratch: nothing a later call could invalidate -- unlike the captures of handle calls, see gnnagg_set_option).
 * Everything else -- an unknown dtype code, another type combination, heads < 1, n % heads != 0, a negative size, a NULL operand with
 * m, n > 0 -- returns GNNAGG_ERR_ARG with a text naming the function and the combination, before any device call. */
int gnnagg_gat_project(const void *d_x, int x_dtype, const void *d_w, int w_dtype,
                       const void *d_a_dst, const void *d_a_src,      /* [heads, D], w_dtype */
                       void *d_feat, int feat_dtype, float *d_att,    /* [M, N], [M, heads, 2] fp32 */
                       int m, int n, int k, int heads, int *path, void *hip_stream);
/* Aggregator_GCN::run_with_nn, aggr_gcn.h:491-499 (kernel aggr_gcn_nn :304-359): y = A.x, then
 * transformed[V,feat_out] = y . weight[feat_in,feat_out].  Both outputs are fully overwritten (the
 * reference accumulates into whatever they held). */
int gnnagg_gcn_run_with_nn(gnnagg_handle h, const float *d_x, float *d_y, const float *d_weight, float *d_transformed,
                           int feat_in, int feat_out, int mode);
/* gnnagg_gcn_run_with_nn with typed operands, every reduce and the fused ReLU (no reference counterpart): the aggregate -> ReLU -> next
 * layer's combine of a GCN forward in one call.  One rule: THE PRODUCT IS TAKEN FROM THE ROW AS IT IS STORED IN y.
 *   y            bit for bit what gnnagg_gcn_run_typed(h, d_x, x_dtype, d_y, y_dtype, feat, mode, reduce, flags) writes: fp32 chains, the
 *                ReLU applied to the finished fp32 row, a bf16 y produced by one round-to-nearest-even
 *   transformed  [V, feat_out] = y . weight[feat, feat_out], row-major
 *   x            y      weight  transformed   product
 *   f32 | bf16   f32    f32     f32           the ascending-k fp32 fmaf chain: bit-equal to gnnagg_matmul_nn(y, weight)
 *   f32 | bf16   bf16   bf16    f32           bf16 MFMA, fp32 accumulation: the contract of gnnagg_matmul_nn_typed (exact where every partial
 *                                             sum is an integer below 2^24, else within 1e-5 . sum|y w| of the float64 product of the stored y)
 *   f32 | bf16   bf16   bf16    bf16          one round-to-nearest-even of what the row above computes on the same inputs
 *   flags   GNNAGG_FLAG_RELU (NaN stays NaN); GNNAGG_FLAG_ACCUMULATE is refused;   reduce  sum, mean, max
 *   weight / transformed at any element-aligned address; x / y as in gnnagg_gcn_run_typed
 * Every other dtype combination, a NULL operand, feat / feat_out < 1 and ACCUMULATE return GNNAGG_ERR_ARG with a text naming the function
 * and the four dtypes, before the handle is looked at.  An all-fp32 request without ReLU is gnnagg_gcn_run_with_nn's path (with `reduce`)
 * on every order that covers; every other request runs where gnnagg_gcn_run_typed runs (the plan kernel) and is refused with that
 * function's text elsewhere.  Where the launcher takes the product as the epilogue of the aggregation kernel (one lane group spans the
 * row, groups of >= 16 lanes, hubs folded in the kernel; bf16 product: also a bf16 row of 64, and a weight of at most 128 x 32) the
 * finished rows meet in LDS and never come back from memory: the bf16 product then runs on v_mfma_f32_16x16x32_bf16 from a bf16 tile that
 * is the stored y bit for bit.  Elsewhere the typed aggregation is followed by the dense GEMM on the stored y; the contract is the same on
 * both paths.  Which shapes take the epilogue is decided by measurement against the back-to-back pair (arxiv-shaped, profiles/nn_typed/:
 * fp32 128 -> 32 with ReLU 97.0 against 108.0 us, 256 -> 64 209 against 271; bf16 128 -> 32 65.3 against 68.6, 64 -> 32 44.5 against 45.6; the
 * bf16 epilogue with a wider weight lost -- 128 -> 64 88 against 72 us -- and is not taken). */
int gnnagg_gcn_run_with_nn_typed(gnnagg_handle h, const void *d_x, int x_dtype, void *d_y, int y_dtype, const void *d_weight, int w_dtype,
                                 void *d_transformed, int t_dtype, int feat, int feat_out, int mode, int reduce, int flags);
/* Which way the last gnnagg_gcn_run_with_nn / gnnagg_gcn_run_with_nn_typed call on this handle took its product: 0 no such call yet,
 * 1 epilogue of the aggregation kernel, 2 aggregation then separate GEMM.  (What the launcher decided, not a prediction.) */
int gnnagg_last_nn_path(gnnagg_handle h, int *path);
/* Input check the reference does not have (an out-of-range neighbor id is a silent out-of-bounds gather there):
 * *bad_rows = rows with ptr[r] > ptr[r+1], *bad_indices = neighbor ids outside [0, num_cols) (num_cols <= 0: num_v).
 * Synchronises the handle's stream. */
int gnnagg_check_csr(gnnagg_handle h, int num_cols, int *bad_rows, int *bad_indices);
/* Aggregator::csr2edgelist, aggregator.h:115-122: d_edgelist[2E] = (src, dst) pairs */
int gnnagg_csr2edgelist(gnnagg_handle h, int *d_edgelist);

/* Aggregator_GAT::run / run_with_feat, aggr_gat.h:317-394.  att is [V,heads,2] (heads = 1 is the
 * reference layout), x,y are [V,feat], feat % heads == 0.  d_newval (may be NULL) receives the
 * un-normalised edge weights [E,heads] the reference's scheduled kernel materialises (:187).
 * Attention logits (every GAT call, slope > 0):
 *   weights    w_e = expf(s > s * slope ? s : s * slope) with s = att[dst, h, 0] + att[src, h, 1], all in fp32 and WITHOUT subtracting a
 *              row maximum, as the reference (aggr_gat.h:138-143): w_e is +Inf above expf's overflow threshold (a leaky logit above
 *              88.7), +0 below its underflow threshold (below -104), NaN for a NaN term.  Callers that may reach those ranges use
 *              gnnagg_gat_run_shifted below, which subtracts the row maximum of the leaky logits (gnnagg_gat_row_shift) before the exp.
 *              (Shifting att[., h, 0] instead is NOT the same softmax unless slope = 1: leaky-ReLU does not commute with a shift.)
 *   locality   att[s, h, 1] reaches exactly head h of the rows that have s as a neighbor, att[r, h, 0] exactly head h of row r: every
 *              other element of y and d_newval is bit-equal to the run without the change.
 *   +Inf, NaN  a +Inf or NaN weight in a (row, head) makes that head's columns of the row NaN, in every mode; d_newval holds the +Inf or
 *              NaN itself at those edges.
 *   0 / 0      a (row, head) that has edges whose weights are all +0 -- the denominator is 0 --
 *                GNNAGG_MODE_ROWS in its canonical order ("fast_rows" = 0), on the row kernels and on the 2-D blocked order alike:
 *                  NaN, aggr_gat's 0 / 0 (aggr_gat.h:163);
 *                every grouped order (the balanced chunked plan, the 2-D blocked balanced order, GNNAGG_MODE_SCHEDULED, "fast_rows" =
 *                  1): the un-divided numerator, as scaleArray divides where the scalar is non-zero (aggr_gat.h:207-213) -- +0 for
 *                  finite features;
 *              rows without edges stay +0 everywhere.  A zero weight is an exact no-op in every chain: the other (row, head)s keep their
 *              bound, and d_newval holds +0 at those edges.
 * (tests/test_gpu_gat_logits.py, tests/test_gat_logits_host.py.  Not specified: denormal weights and logits within a few ulps of the
 * two thresholds -- device expf and libm may differ there by a class --, slope <= 0.) */
int gnnagg_gat_run(gnnagg_handle h, const float *d_x, const float *d_att, float *d_y, int feat, int heads,
                   float slope, int mode, float *d_newval);
/* gnnagg_gat_run with x / y in the given element types (GNNAGG_DTYPE_F32 / GNNAGG_DTYPE_BF16; no reference counterpart).  d_att
 * [V,heads,2] and d_newval [E,heads] stay fp32.  Numerator, denominator, exp, LDS stage, partial rows, hub fold and the softmax
 * division stay fp32 and keep their order, and bf16 -> fp32 is exact, so a bf16 x gives bit for bit what gnnagg_gat_run gives on x
 * widened to fp32 (same handle, same mode), newval included; a bf16 y is ONE round-to-nearest-even of that fp32 result, at the store
 * (NaN kept, overflow to inf as in a plain conversion); rows without edges are +0.
 * (F32, F32) is gnnagg_gat_run exactly.  The other three combinations:
 *   mode    GNNAGG_MODE_BALANCED (a handle on the 2-D blocked order -- high-degree graphs -- runs the chunked plan, built beside it
 *           on first use; the handle keeps its blocked order for fp32 calls); GNNAGG_MODE_SCHEDULED where the plan kernel runs it (a
 *           neighbor-grouping schedule, or "fast_scheduled" = 1, the default, on a call without d_newval); GNNAGG_MODE_ROWS where
 *           "fast_rows" = 1 maps it to the balanced order (handles of the reference-named surface start that way)
 *   feat    any F >= 1 with feat % heads == 0; x / y at any 2-byte (bf16) or 4-byte (fp32) offset (narrower lanes)
 * Everything else returns GNNAGG_ERR_ARG with a gnnagg_last_error() text naming the combination -- an unknown dtype code, the
 * canonical rows mode (fast_rows = 0), an order the item kernels run -- and nothing falls back to fp32.
 * Still fp32 only: gnnagg_gat_run_part, gnnagg_gat_probe_gather, the distributed step (gnnagg_dist_step_*), the backward entry point
 * and the edge-softmax pieces below. */
int gnnagg_gat_run_typed(gnnagg_handle h, const void *d_x, int x_dtype, const float *d_att, void *d_y, int y_dtype,
                         int feat, int heads, float slope, int mode, float *d_newval);
/* The max-shifted, overflow-safe edge softmax (no reference counterpart; what DGL's and PyG's edge softmax do).
 *
 * shift[V,heads] (fp32): the maximum over the row's edges of the fp32 leaky logit, formed as
 * leaky(att[r,h,0] + max_s att[s,h,1]) (slope > 0); +0 for a row without edges.
 * For slope > 0 the fp32 addition, the fp32 multiplication by the slope and the select are non-decreasing, so this is bit for bit the
 * per-edge maximum of max(s, s * slope), from one gather-max over the 4-byte source terms: no feature row is touched.  Any heads >= 1;
 * column ids up to max(num_v, largest id + 1) as everywhere.  The same bits on every call.  A (row, head) whose logits are all -Inf
 * holds -Inf, one with a +Inf logit +Inf; what it holds for a (row, head) with a NaN term is not specified (NaN, or the maximum of the
 * others).  slope <= 0 returns GNNAGG_ERR_ARG.  Asynchronous on the handle's stream, no allocation, no synchronisation. */
int gnnagg_gat_row_shift(gnnagg_handle h, const float *d_att, int heads, float slope, float *d_shift);
/* gnnagg_gat_run_typed with w_e = expf(leaky(att[dst,h,0] + att[src,h,1]) - shift[dst,h]).
 * d_shift == NULL: the library computes gnnagg_gat_row_shift into scratch of the handle first (same stream).
 * With the row maximum as the shift every weight is <= 1, the maximal edge of a (row, head) has weight exactly 1, the denominator lies
 * in [1, degree], and finite attention terms can give neither +Inf nor 0 / 0.
 *   subtraction  ONE fp32 subtraction of the rounded leaky logit: d = fl32(max(s, s * slope) - shift), then expf(d); never a fused
 *                s * slope - shift.
 *   order        the chains, the LDS stage, the partial rows, the hub fold and the division keep the order of gnnagg_gat_run_typed (the
 *                shift is constant per (row, head): all partial sums of a row are in one scale).  d_shift may be ANY array: an all-zero
 *                d_shift gives bit for bit what gnnagg_gat_run_typed gives on the same handle and mode (x - 0.0f is x), Inf and NaN
 *                inputs included.
 *   types        all four combinations of GNNAGG_DTYPE_F32 / GNNAGG_DTYPE_BF16 for x and y; d_att and d_shift stay fp32.  bf16 as in
 *                gnnagg_gat_run_typed: exact widening, ONE round-to-nearest-even at the store.  Rows without edges are +0.
 *   orders       those the 16-bit combinations of gnnagg_gat_run_typed run on, for fp32 x / y too: GNNAGG_MODE_BALANCED on the chunked plan
 *                (a handle on the 2-D blocked order builds the chunked plan beside it and keeps its blocked order for the other calls),
 *                GNNAGG_MODE_SCHEDULED where the plan kernel runs it, GNNAGG_MODE_ROWS where "fast_rows" = 1.  Everything else returns
 *                GNNAGG_ERR_ARG with a text naming the combination -- the canonical rows mode, an order the item kernels run, an unknown
 *                dtype code -- and nothing falls back to the unshifted run.  There is no d_newval.  Arguments are checked before any
 *                device call.
 *   non-finite   plain IEEE: a (row, head) with a NaN or +Inf logit is NaN in that head's columns (Inf - Inf), every other (row, head)
 *                is bit-equal to the run without the change; a -Inf logit is a weight of +0; a (row, head) whose logits are all -Inf is
 *                NaN.
 *   streams      asynchronous on the handle's stream; nothing is synchronised or allocated once the handle's scratch (V * heads floats
 *                more when d_shift == NULL) exists, and a warm call can be captured in a HIP graph.  The capture holds the handle's scratch
 *                and plan pointers: a later call that grows scratch (wider feat, more heads, another dtype) or drops a plan (a replan option,
 *                gnnagg_schedule*) invalidates it, and it must be captured again (gnnagg_set_option).
 * Unshifted still: gnnagg_gat_run / _typed themselves, gnnagg_gat_run_att and the three-step adapter below, the span kernels of the 2-D
 * blocked order, the canonical rows mode, gnnagg_gat_run_part, the distributed step and the backward extras.
 * (tests/test_gpu_gat_shift.py, tests/test_gat_shift_host.py) */
int gnnagg_gat_run_shifted(gnnagg_handle h, const void *d_x, int x_dtype, const float *d_att, const float *d_shift,
                           void *d_y, int y_dtype, int feat, int heads, float slope, int mode);
/* GATv2, the "dynamic attention" form (no reference counterpart; what DGL's GATv2Conv and PyG's GATv2Conv aggregate with): score,
 * edge softmax and aggregation in one call, one gather per edge.  For row r, head h (D = feat / heads) and every edge j of the row, in
 * CSR order:
 *     z_jc = xd[r, hD + c] + xs[j, hD + c]         l_jc = z_jc > z_jc * slope ? z_jc : z_jc * slope
 *     e_j  = sum_c a[h, c] * l_jc                  alpha_j = exp(e_j - max_k e_k) / sum_k exp(e_k - max_k e_k)
 *     y[r, hD + c] = sum_j alpha_j * xs[j, hD + c]
 *   operands     d_xs [n_src, feat] and d_xd [num_v, feat] hold x_dtype elements (GNNAGG_DTYPE_F32 / GNNAGG_DTYPE_BF16, the same type for both;
 *                bf16 is widened exactly); d_a [heads, D] is fp32; d_y [num_v, feat] holds y_dtype elements.  d_xd == d_xs is the shared-weight
 *                form.  d_y aliases neither input.  Column ids may exceed num_v (d_xs has that many rows).  x / y at any element offset.
 *   arithmetic   fp32 throughout; the softmax is always max-shifted (online, one rescale per batch of 4 edges at most), so finite inputs with
 *                finite scores give finite results whatever the scores' magnitude.  A bf16 y is ONE round-to-nearest-even of the fp32 result.
 *                A row without edges is +0.  No self loops are added; a duplicate edge counts twice.
 *   order        a row's result depends on its edges in CSR order and on the lane geometry of (feat, heads, x_dtype) only -- never on a
 *                pointer's alignment or on other rows; no atomics; the same bits on every call (DESIGN.md "GATv2").
 *   non-finite   plain IEEE: the result has the class map (finite / +Inf / -Inf / NaN, element for element) of the two-pass float64 formulas
 *                above, as long as the finite scores of a (row, head) lie within 60 of each other (no fp32 weight is 0 where float64's is
 *                not).  A -Inf score is a weight of exactly +0 wherever it stands in the row; a (row, head) whose scores are all -Inf is NaN
 *                (0 / 0); a (row, head) with a +Inf or NaN score is NaN in that head's columns (Inf - Inf); every (row, head) the non-finite
 *                value does not reach is bit-equal to the run without it.  The scored row is the summed row: a -Inf in xs[j, c] that masks
 *                edge j makes column c of that (row, head) NaN (0 * -Inf) and leaves the head's other columns finite.  A row without edges
 *                is +0 whatever its xd row holds; a source row that no edge names is never read into a result; a bf16 y is one rounding of
 *                the fp32 y (NaN kept).  (tests/test_gpu_attn_nonfinite.py, tests/test_attn_nonfinite_host.py)
 *   refusals     GNNAGG_ERR_ARG with a text naming the argument, d_y untouched: a handle that is not a GAT aggregator, a null pointer, an unknown
 *                dtype code, feat < 1, feat % heads != 0, slope outside [0, 1], feat > 1024 (the kernel's limit).
 *   streams      on the handle's stream.  The first call builds the list of long rows (one read of ptr, ordered behind the stream) and a call
 *                allocates only while the handle's scratch is smaller than its (feat, heads, x_dtype) needs; any later call of such a shape
 *                allocates and synchronises nothing and can be captured in a HIP graph -- until a call of a shape that needs more scratch
 *                (wider feat, more heads, another dtype) reallocates it: the capture must then be made again (gnnagg_set_option).
 * (tests/test_gpu_gatv2.py, tests/test_gatv2_host.py) */
int gnnagg_gatv2_run(gnnagg_handle h, const void *d_xs, const void *d_xd, int x_dtype, const float *d_a, void *d_y, int y_dtype, int feat,
                     int heads, float slope);
/* Scaled dot-product attention over the graph's edges (no reference counterpart beyond the unnormalised score of its aggr_sddmm.h; what
 * PyG's TransformerConv aggregates with, DGL's u_dot_v + edge_softmax + u_mul_e_sum, the sparse attention of graph transformers): score,
 * edge softmax and aggregation in one call, two gathers per edge.  For row r, head h (D = feat / heads) and every edge j of the row, in
 * CSR order:
 *     e_j = sum_c (scale * q[r, hD + c]) * k[j, hD + c]          alpha_j = exp(e_j - max_k e_k) / sum_k exp(e_k - max_k e_k)
 *     y[r, hD + c] = sum_j alpha_j * v[j, hD + c]
 *   operands     d_q has at least num_v rows, row i at element i * q_pitch; d_k and d_v have n_src rows (any size the largest column id
 *                needs), row j at element j * kv_pitch for both.  Pitches are in elements and >= feat, so the column views of one
 *                [n, 3 * feat] projection x . [Wq | Wk | Wv] serve as the three operands without a copy.  q, k and v hold x_dtype elements
 *                (GNNAGG_DTYPE_F32 / GNNAGG_DTYPE_BF16; bf16 is widened exactly); d_y is dense [num_v, feat] of y_dtype elements.  d_q, d_k
 *                and d_v may be one pointer.  d_y aliases no input.  Any element offset, any pitch >= feat.
 *   arithmetic   fp32 throughout.  scale (finite, either sign) is multiplied into the row's q elements ONCE, and a score is the fp32 FMA
 *                chain of (scale * q) and k: a power-of-two scale gives the bits of the call with q scaled beforehand.  The softmax is
 *                always max-shifted (online, at most one rescale per batch of edges; never an exp of an unshifted score), so finite
 *                inputs with finite scores give finite results whatever the scores' magnitude.  A bf16 y is ONE round-to-nearest-even of
 *                the fp32 result.  A row without edges is +0.  No self loops are added; a duplicate edge counts twice.
 *   order        a row's result depends on its edges in CSR order and on the lane geometry of (feat, heads, x_dtype) only -- never on a
 *                pointer's alignment, a pitch or other rows; no atomics; the same bits on every call (DESIGN.md "Dot-product attention").
 *   error        against the float64 formulas, |y - ref|[r, hD + c] <= 1e-5 * (1 + L[r, h]) * S[r, hD + c] with
 *                L[r, h] = max_j |scale| * sum_c |q k| and S[r] = sum_j alpha_j |v_j| (the 1e-5 bar widened by the score's condition number).
 *   non-finite   plain IEEE: the result has the class map (finite / +Inf / -Inf / NaN, element for element) of the two-pass float64 formulas
 *                above, as long as the finite scores of a (row, head) lie within 60 of each other (no fp32 weight is 0 where float64's is
 *                not).  A -Inf score -- the mask of attention callers, a -Inf in k -- is a weight of exactly +0 wherever it stands in the
 *                row, and the finite elements keep the error bound, taken over the edges that are left; a (row, head) whose scores are all
 *                -Inf is NaN (0 / 0); a (row, head) with a +Inf or NaN score is NaN in that head's columns (Inf - Inf); every (row, head) the
 *                non-finite value does not reach is bit-equal to the run without it.  A +Inf in v[:, c] is +Inf in column c of every row that
 *                gathers it (weights are positive), never NaN.  A row without edges is +0 whatever its q row holds; a source row that no
 *                edge names is never read into a result; a bf16 y is one rounding of the fp32 y (NaN kept).
 *                (tests/test_gpu_attn_nonfinite.py, tests/test_attn_nonfinite_host.py)
 *   refusals     GNNAGG_ERR_ARG with a text naming the argument, nothing launched, d_y untouched: a handle that is not a GAT aggregator, a
 *                null pointer, an unknown dtype code, feat < 1, feat % heads != 0, a pitch below feat, a non-finite scale, feat > 1024
 *                (the kernel's limit, GATv2's).
 *   streams      on the handle's stream.  The list of long rows and the scratch are those of gnnagg_gatv2_run (built by the first call of
 *                either kind; the scratch grows to whichever call needs more), so one handle serves both calls in any order.  A call
 *                whose shape the scratch already covers allocates and synchronises nothing and can be captured in a HIP graph -- until a
 *                call of either kind reallocates the scratch: the capture must then be made again (gnnagg_set_option).
 * (tests/test_gpu_dot_attn.py, tests/test_dot_attn_host.py) */
int gnnagg_dot_attn_run(gnnagg_handle h, const void *d_q, long long q_pitch, const void *d_k, const void *d_v, long long kv_pitch,
                        int x_dtype, void *d_y, int y_dtype, int feat, int heads, float scale);
/* gnnagg_gatv2_run and gnnagg_dot_attn_run with a per-edge score bias (no reference counterpart; the spatial and edge encodings of
 * Graphormer, relative-position and edge-type bias tables, the attention masks of dropped or padded edges, the biased sparse attention of
 * SAN / GPS).  Everything said under the two calls above holds; what is added:
 *   operand      d_bias is fp32 and dense, [num_e, bias_heads] row-major with bias_heads = 1 (one value per edge serves every head) or
 *                bias_heads = heads.  It is indexed by the POSITION p of the edge in the CSR (ptr, idx) the handle was created with --
 *                edge p of row r is ptr[r] <= p < ptr[r + 1] -- and by head.  For edge p, head h:
 *                    e_p = (the score above: the fp32 chain, reduced over the head) + d_bias[p * bias_heads + (bias_heads == 1 ? 0 : h)]
 *                ONE fp32 addition after the per-head reduction and before the batch maximum; the index is taken in 64 bits.  Batches, the
 *                single guarded rescale, the segments and their ordered merge are those of the calls above.  d_bias needs 4-byte alignment
 *                only (any element offset).  d_y aliases no input, the bias included.
 *   no bias      d_bias == NULL is gnnagg_gatv2_run / gnnagg_dot_attn_run bit for bit (the same kernels are launched; bias_heads is then
 *                ignored); a bias of all +0.0 gives those bits too.
 *   error        the bound of the calls above with L[r, h] = max over the row's edges with a finite bias of (the call's L term + |bias|).
 *   masks        a bias of -Inf is a mask, and "non-finite" above applies to the sum as it stands: a masked edge has a weight of exactly +0
 *                wherever it stands in the row and the finite elements keep the error bound, taken over the edges that are left; a
 *                (row, head) whose edges are all masked is NaN (0 / 0); a +Inf or NaN bias makes that (row, head) NaN; every other
 *                (row, head) is bit-equal to the run without the non-finite value.  Rows without edges are +0 and have no bias to read.
 *                For GATv2 a bias mask poisons no column: the source row stays finite (compare "the scored row is the summed row").
 *   refusals     those of the calls above under this function's name, and GNNAGG_ERR_ARG naming bias_heads = N where d_bias != NULL and
 *                bias_heads is neither 1 nor heads; nothing launched, d_y untouched.
 *   streams      no handle state is added: the list of long rows and the scratch are those of the calls above and sized alike, so one
 *                handle serves biased and unbiased calls of both kinds in any order, and a biased call is captured in a HIP graph like an
 *                unbiased one.  The capture holds d_bias as it holds the other operands: rewrite the bias in place between replays.
 * (tests/test_gpu_attn_bias.py, tests/test_attn_bias_host.py) */
int gnnagg_gatv2_run_bias(gnnagg_handle h, const void *d_xs, const void *d_xd, int x_dtype, const float *d_a, void *d_y, int y_dtype,
                          int feat, int heads, float slope, const float *d_bias, int bias_heads);
int gnnagg_dot_attn_run_bias(gnnagg_handle h, const void *d_q, long long q_pitch, const void *d_k, const void *d_v, long long kv_pitch,
                             int x_dtype, void *d_y, int y_dtype, int feat, int heads, float scale, const float *d_bias, int bias_heads);
/* The two calls above with the attention weights and the softmax's row statistics handed back (what gnnagg_gat_run's d_newval and
 * gnnagg_gat_row_shift / div are to the 2018 form; PyG's return_attention_weights, DGL's get_attention; the tensors a backward pass
 * would save).  Everything said under gnnagg_gatv2_run, gnnagg_dot_attn_run and the two _bias calls holds, d_bias == NULL included;
 * what is added:
 *   d_alpha      fp32, dense [num_e, heads] row-major, indexed like d_bias with bias_heads == heads: by the POSITION p of the edge in the
 *                handle's CSR (ptr[r] <= p < ptr[r + 1]) and by head, the index taken in 64 bits.
 *                    alpha[p, h] = expf(e_p - ms) / den
 *                e_p is the fp32 score the walk formed for that edge and head -- the same FMA chain, head reduction and single bias add
 *                that y was summed with, stored once and read back, not a second formula; ms is the (row, head)'s FINAL shift, its
 *                maximum M, or 0 where M is -Inf (the walk's own rule); den is the denominator y was divided by.
 *   d_stat       fp32, dense [num_v, heads, 2]: stat[r, h, 0] = M, stat[r, h, 1] = den, the pair as it stands (not M + log den, which
 *                loses the weights' precision at large scores).  All num_v * heads * 2 values are written by every call: a row without
 *                edges and an all-masked (row, head) are (-Inf, +0); a (row, head) that a +Inf or NaN score reaches has a NaN den and
 *                an unspecified M.
 *   operands     both are required; a caller who wants neither has the calls above.  4-byte alignment only (any element offset).  They
 *                alias nothing the call reads or writes (with num_e == 0 d_alpha is never written: any non-null pointer serves).
 *   y            bit-equal to the call without the two outputs, on every shape and every bias form.
 *   error        |alpha - ref| <= 1e-5 * (1 + L[r, h]) * ref against the float64 two-pass formulas: the calls' y bound with v the
 *                indicator of one edge's source.  M is within 1e-5 * (1 + L) of the float64 maximum, den within that relative bound.
 *   non-finite   alpha has the class map of the float64 formulas: a -Inf score or bias gives +0 exactly (the bit pattern) and the row's
 *                other weights keep the bound; an all-masked (row, head), and one with a +Inf or NaN score, is NaN on every one of its
 *                edges; every (row, head) the non-finite value does not reach is bit-equal to the run without it.
 *   refusals     those of the _bias calls under these names, and GNNAGG_ERR_ARG naming d_alpha / d_stat when null; nothing launched,
 *                d_y, d_alpha and d_stat untouched.
 *   streams      two or three launches on the handle's stream: the walk (which leaves the raw scores in d_alpha and the pairs in d_stat),
 *                the merge of multi-segment rows, and an edge-parallel finishing pass that turns the scores into weights in place.  The
 *                finishing pass finds an edge's row by bisection over the handle's ptr and keeps no plan: no handle state is added.  One
 *                handle serves weights and no-weights calls of both kinds in any order; a call of a shape that has run allocates and
 *                synchronises nothing and is captured in a HIP graph like the calls above.  A call without weights launches the kernels
 *                it launched before these calls existed.
 * (tests/test_gpu_attn_weights.py, tests/test_attn_weights_host.py) */
int gnnagg_gatv2_run_weights(gnnagg_handle h, const void *d_xs, const void *d_xd, int x_dtype, const float *d_a, void *d_y, int y_dtype,
                             int feat, int heads, float slope, const float *d_bias, int bias_heads, float *d_alpha, float *d_stat);
int gnnagg_dot_attn_run_weights(gnnagg_handle h, const void *d_q, long long q_pitch, const void *d_k, const void *d_v, long long kv_pitch,
                                int x_dtype, void *d_y, int y_dtype, int feat, int heads, float scale, const float *d_bias, int bias_heads,
                                float *d_alpha, float *d_stat);
/* The two attentions with a feature VECTOR per edge (no reference counterpart; the edge_dim / edge_attr argument of PyG's GATv2Conv and
 * TransformerConv and of DGL's equivalents, after the layer's own projection to feat columns: bond features of molecular graphs, relation
 * embeddings of knowledge graphs, the edge channel of GPS / SAN-style graph transformers) -- without the [num_e, feat] intermediate
 * xs[idx] + ef that the calls above would need.  One entry point per attention; each carries the optional bias and the optional weights
 * and statistics.  Everything said under gnnagg_gatv2_run, gnnagg_dot_attn_run, the _bias and the _weights calls holds -- batches, the
 * single guarded rescale, segments and their ordered merge, the bias add, the masks, the weights-out form, "no atomics, the same bits on
 * every call", "depends on the lane geometry of (feat, heads, x_dtype) only, never on alignment or pitch"; what is added:
 *   operand      d_ef holds [num_e, feat] elements of x_dtype (the type of the other operands), row p at element p * ef_pitch with
 *                ef_pitch >= feat, the offset taken in 64 bits.  Rows are indexed by the POSITION p of the edge in the handle's CSR
 *                (ptr[r] <= p < ptr[r + 1]), exactly like d_bias.  Any element offset, any pitch >= feat.  d_y aliases no input.
 *   arithmetic   fp32 throughout; bf16 is widened exactly and nothing is rounded back to bf16 before use.  For edge p = (row r, source j):
 *                GATv2 (gnnagg_gatv2_run_edge; GATv2Conv(edge_dim=)):
 *                    z_jc = xd[r, c] + (xs[j, c] + ef[p, c])     the inner add first, each ONE fp32 add
 *                    e_p  = sum_c a[h, c] * leaky(z_jc)          y[r] = sum_p alpha_p * xs[j]     (the summed row is xs[j] WITHOUT ef)
 *                dot-product (gnnagg_dot_attn_run_edge; TransformerConv(edge_dim=)):
 *                    k'_p = k[j] + ef[p],  v'_p = v[j] + ef[p]   each ONE fp32 add per element
 *                    e_p  = sum_c (scale * q[r, c]) * k'_p[c]    the FMA chain of gnnagg_dot_attn_run
 *                    y[r] = sum_p alpha_p * v'_p
 *                so, for fp32 operands, gnnagg_dot_attn_run_edge on (ptr, idx) gives the bits of gnnagg_dot_attn_run on the graph
 *                (ptr, 0 .. num_e - 1) with k' and v' materialised by one fp32 add, and gnnagg_gatv2_run_edge gives that graph's alpha and
 *                stat with xs' = xs[idx] + ef (its y sums xs[j], not xs').
 *   zero         an ef of all +0.0 gives the values of the call without it (== on every element; only the sign of a zero may differ).
 *   error        the bounds of the calls above with L taken over the scores WITH ef (and the bias), S[r] = sum_p alpha_p |v'_p| for the
 *                dot-product and sum_p alpha_p |xs_j| for GATv2.
 *   non-finite   non-finite ef elements follow plain IEEE on k', v' and z: the call has the class map of the float64 formulas on those
 *                operands, and every (row, head) the value does not reach is bit-equal to the run without it.
 *   outputs      d_bias may be NULL (bias_heads is then ignored).  d_alpha and d_stat are both NULL (no weights out) or both given.
 *   refusals     those of the _weights calls under these names, and GNNAGG_ERR_ARG naming the argument for a null d_ef (where num_e > 0),
 *                for ef_pitch < feat, and for exactly one of d_alpha / d_stat; nothing launched, d_y, d_alpha and d_stat untouched.
 *   streams      no handle state is added: the segment list, the slots and the scratch are those of the calls above and sized alike.  One
 *                handle serves edge and non-edge calls of both kinds in any order; a call of a shape that has run allocates and synchronises
 *                nothing and is captured in a HIP graph, which holds d_ef as it holds the other operands (rewrite ef in place between
 *                replays).  Where the d_ef base or ef_pitch * element size is not 16-byte aligned the whole call loads element by element:
 *                the aligned run's bits.  A call without ef launches the kernels it launched before these calls existed.
 * (tests/test_gpu_attn_edge.py, tests/test_attn_edge_host.py) */
int gnnagg_gatv2_run_edge(gnnagg_handle h, const void *d_xs, const void *d_xd, int x_dtype, const float *d_a, const void *d_ef,
                          long long ef_pitch, void *d_y, int y_dtype, int feat, int heads, float slope, const float *d_bias, int bias_heads,
                          float *d_alpha, float *d_stat);
int gnnagg_dot_attn_run_edge(gnnagg_handle h, const void *d_q, long long q_pitch, const void *d_k, const void *d_v, long long kv_pitch,
                             const void *d_ef, long long ef_pitch, int x_dtype, void *d_y, int y_dtype, int feat, int heads, float scale,
                             const float *d_bias, int bias_heads, float *d_alpha, float *d_stat);
/* Multi-aggregation: several reductions of the same neighbourhood from ONE gather, times degree scalers (no reference counterpart; the
 * aggregation stage of PNA -- PyG's PNAConv and aggr=["mean", "min", "max", "std"] / MultiAggregation, DGL's PNAConv).  On a GCN handle.
 *   messages     for edge position p of row r (ptr[r] <= p < ptr[r + 1]) the message is m_p[c] = val[p] * x[idx[p], c], ONE fp32 multiply;
 *                m_p = x[idx[p]] exactly where the handle has no val.  val is read at call time (gnnagg_update_val is honoured).  d_x is
 *                dense [n_src, feat] of x_dtype (GNNAGG_DTYPE_F32 / GNNAGG_DTYPE_BF16; bf16 is widened exactly).  Column ids may exceed
 *                num_v (d_x has that many rows).  d_y aliases no input.
 *   per row      with d = ptr[r + 1] - ptr[r] (the handle's own degree; row_aux is not consulted), per column:
 *                    S1 = sum_p m_p (a plain fp32 add per edge)   S2 = sum_p m_p * m_p   mn = min_p m_p   mx = max_p m_p
 *                    sum = S1        mean = S1 / (float)d (one fp32 division)        min = mn        max = mx
 *                    var = max(S2 / d - mean * mean, 0)  (the two-moment form PyG and DGL compute, clamped: never negative)
 *                    std = sqrtf(var)
 *                A row without edges is +0 in every block.
 *   layout       d_y is dense [num_v, S * A * feat] of y_dtype, A and S the numbers of set bits of aggr_mask and scaler_mask.  Blocks in
 *                ascending bit order, scaler-major: column (s_pos * A + a_pos) * feat + c -- PyG's cat([out * scaler ...]) order.  A bf16 y
 *                is ONE round-to-nearest-even of the fp32 value.
 *   scalers      identity = 1; amplification = logf(d + 1) / delta; attenuation = delta / logf(d + 1): one fp32 scalar per row, multiplied
 *                into the finished fp32 aggregate once.  delta is the caller's training-set mean of log(d + 1).  The aggregate is computed
 *                once whatever S is.
 *   order        for a row of at most 128 edges S1 is the sequential fp32 chain s = s + m_p in CSR order from +0 (reproducible on the host
 *                with numpy float32).  Longer rows are cut at the attention calls' segment (512 edges) and chunk boundaries and folded in
 *                ascending order.  No atomics; the same bits on every call.  A block's bits never depend on which other blocks or scalers
 *                were selected, nor on a pointer's alignment.  min and max are exact for any order.
 *   error        |sum - ref| <= 1e-5 * sum_p |m_p| against float64, mean within that / d; |var - ref| <= 4e-5 * S2 / d.
 *   non-finite   three rules, for messages that are +-Inf or NaN (from x, from val, or 0 * Inf formed by the multiply):
 *                sum, mean, var, std: the class map (finite / +Inf / -Inf / NaN, element for element) of the float64 two-moment formulas
 *                over the fp32 messages.  var and std are NaN wherever a message of the (row, column) is +-Inf or NaN (the clamp above
 *                keeps a NaN).  One case stays unspecified: var / std where the fp32 chain S2 overflows although every message is finite
 *                -- inherent to the two-moment form.
 *                min, max: NaN messages are SKIPPED (np.fmin.reduce / np.fmax.reduce), +-Inf messages are exact, and a (row, column) whose
 *                messages are all NaN is NaN, never a value no message had.  This differs from torch.amin / torch.amax (and PyG's min /
 *                max aggregation), which propagate a NaN.
 *                Every (row, column) that no non-finite message reaches keeps the bits of the run without it.  A NaN is stored as the
 *                quiet NaN 0x7fc00000 (a bf16 y: its one rounding) whatever NaN operands met on the way, so what "order" says of a block's
 *                bits holds here too.
 *   refusals     GNNAGG_ERR_ARG with a text naming the argument, nothing launched, d_y untouched: a handle that is not a GCN aggregator, a
 *                null pointer, an unknown dtype code, feat < 1, feat > 1024 (the kernel's limit), a mask that is 0 or has unknown bits, a
 *                non-identity scaler with delta not finite or <= 0.
 *   streams      on the handle's stream.  The first call builds the list of long rows (one read of ptr, ordered behind the stream) and a
 *                call allocates only while the handle's scratch for the partials of multi-segment rows is smaller than its (feat, x_dtype)
 *                needs; any later call of a covered shape allocates and synchronises nothing and can be captured in a HIP graph (one or
 *                two launches in a line) -- until a call that needs more scratch reallocates it: the capture must then be made again.
 * (tests/test_gpu_multi_aggr.py, tests/test_multi_aggr_host.py; non-finite: tests/test_gpu_multi_aggr_nonfinite.py,
 * tests/test_multi_aggr_nonfinite_host.py; shapes, masks and handle history: tests/test_gpu_multi_aggr_shapes.py; DESIGN.md "Multi-aggregation") */
#define GNNAGG_AGGR_SUM 1
#define GNNAGG_AGGR_MEAN 2
#define GNNAGG_AGGR_MIN 4
#define GNNAGG_AGGR_MAX 8
#define GNNAGG_AGGR_VAR 16
#define GNNAGG_AGGR_STD 32
#define GNNAGG_SCALER_IDENTITY 1
#define GNNAGG_SCALER_AMPLIFICATION 2
#define GNNAGG_SCALER_ATTENUATION 4
int gnnagg_gcn_run_multi(gnnagg_handle h, const void *d_x, int x_dtype, void *d_y, int y_dtype, int feat, int aggr_mask, int scaler_mask,
                         float delta);
/* The fused GAT aggregation in TWO passes over disjoint edge sets of the same rows (two handles over the same rows: the
 * row-partitioned step's local-source edges, then its halo-source edges once the exchange has landed).  GNNAGG_MODE_BALANCED on
 * the chunked plan; 16-byte aligned rows of at most 256 columns, head widths that are multiples of 4 (a lane's four columns lie in one head).
 *   part = 1  d_y[row, :] receives the NUMERATOR sum_e w_e x_e and d_den_io[row, h] the denominator sum_e w_e; no division
 *   part = 2  both are added to what part 1 left (old + new, one fp32 add per element), then the row is divided
 *             (scaleArray, aggr_gat.h:207-213); rows this handle has no edges for are divided all the same
 *   part = 3  a pass in between (staged halo exchange, gnnagg_dist_step_create_staged): both are added, nothing is divided
 * Weights as under "Attention logits": a +Inf / NaN weight in either pass makes the (row, head) NaN (d_den_io holds the +Inf / NaN
 * after part 1), zero weights are no-ops.  What a (row, head) with edges receives when its denominator over BOTH passes is 0 is not
 * specified. */
int gnnagg_gat_run_part(gnnagg_handle h, const float *d_x, const float *d_att, float *d_y, int feat, int heads, float slope, int part,
                        float *d_den_io);
/* Aggregator_GAT::run_att, aggr_gat.h:395-401 (attGat :5-31): out_val[E,heads] = softmax weights w_e / sum_row(w), divided unguarded as
 * attGat does: with the weights of "Attention logits" above, NaN at an edge whose weight is +Inf or NaN and +0 at the finite edges of that
 * (row, head); NaN on every edge of a (row, head) whose weights are all +0. */
int gnnagg_gat_run_att(gnnagg_handle h, const float *d_att, float *d_out_val, int heads, float slope);
/* aggr_gat.h:402-425, single head as in the reference */
int gnnagg_gat_run_u_add_v(gnnagg_handle h, const float *d_att, float *d_out_val);
int gnnagg_gat_run_add_to_center(gnnagg_handle h, const float *d_in_val, float *d_out_att);
int gnnagg_gat_run_div_each(gnnagg_handle h, const float *d_in_att, float *d_inout_val);

/* spmm<L>, spmm.h:223-265 (naive thread-per-row baseline; empty rows are left untouched) */
int gnnagg_spmm_naive(const int *d_ptr, const int *d_idx, const float *d_val, const float *d_x, float *d_y,
                      int num_v, int feat, void *hip_stream);
/* valid(), spmm.h:35-69 (validate2 :11-21): number of elements with |(ref-ans)/ref| > 1e-2 */
int gnnagg_validate(const float *d_ref, const float *d_ans, int num, int *h_diff, void *hip_stream);
/* validReordered(), spmm.h:71-91 (validateReordered :23-33) */
int gnnagg_validate_reordered(const float *d_ref, const float *d_ans, const int *d_map, int num_v, int feat,
                              int *h_diff, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * C. Host graph preparation (pure host code; usable without a GPU)
 * ------------------------------------------------------------------------------------------- */
/* load_graph, src/data.cu:31-139.  Reads <datadir><dset>.config/.graph (or the .ptrdump/.edgedump
 * caches, which it also writes), applies <datadir><dset>.reorder<reorder_suffix> when shuffle != 0
 * and the file exists.  Unlike the reference (data.cu:34 hard-codes "../data/") datadir is honoured.
 * Outputs are malloc'ed; release with gnnagg_free_host.  rows / reverse_rows are NULL outputs when
 * no reorder was applied. */
int gnnagg_load_graph(const char *datadir, const char *dset, const char *reorder_suffix, int shuffle,
                      int *num_v, int *num_e, int **h_ptr, int **h_idx, int **h_rows, int **h_reverse_rows);
void gnnagg_free_host(void *p);
/* reorderCSR, src/data.cu:4-29 */
int gnnagg_reorder_csr(const int *h_ptr, const int *h_idx, const int *h_map, const int *h_reverse_map,
                       int num_v, int num_e, int *h_newptr, int *h_newidx);
/* neighbor_grouping_schedule, graph_schedule.h:91-126.  Outputs may be NULL to size first. */
int gnnagg_neighbor_grouping_schedule(const int *h_ptr, int neighbor_num, int num_v, int *h_ptr_out,
                                      int *h_target_out, int *num_groups);
/* locality_schedule :17-63 (neighbor_num <= 0) / localityNeighborGrouping :156-211 */
int gnnagg_locality_schedule(const int *h_ptr, const int *h_idx, const float *h_val, int par_num,
                             int neighbor_num, int num_v, int total_num_v, int *h_ptr_out, int *h_idx_out,
                             float *h_val_out, int *h_target_out, int *num_groups);

/* Locality reorder GENERATOR: the clustering of script/cluster2.py:29-171 (MinHash with num_perm
 * permutations, LSH at Jaccard `threshold`, greedy union-find merge of the most similar candidate rows
 * until clusters reach cluster_cap nodes).  0 / 0.0 select the reference's constants (64, 0.2, 64).
 * h_rows_out[i] = old node id placed at new position i: the content of a <dset>.reorder<suffix> file. */
int gnnagg_cluster_reorder(const int *h_ptr, const int *h_idx, int num_v, float threshold, int num_perm, int cluster_cap,
                           unsigned long long seed, int *h_rows_out, int *num_clusters);
/* The same clustering with a choice of the order the clusters are written in.  order_mode 0: by first member (the
 * reference script, cluster2.py:156-171; = gnnagg_cluster_reorder).  order_mode 1: cache-aware greedy -- each next cluster
 * is the one whose rows find the largest share of their source rows among the cache_rows most recently gathered rows (an
 * LRU model of one XCD's L2; 0 = 4096 rows, 2 MB of 512-byte feature rows), so clusters with overlapping neighbor sets
 * become neighbors in the new numbering.  Deterministic: the rows are a function of the arguments (graphs of 20 M edges and more
 * are walked by 64 logical walkers in bulk-synchronous rounds -- GNNAGG_REORDER_WALKERS overrides the count, never the thread count). */
int gnnagg_cluster_reorder_ex(const int *h_ptr, const int *h_idx, int num_v, float threshold, int num_perm, int cluster_cap,
                              unsigned long long seed, int order_mode, int cache_rows, int *h_rows_out, int *num_clusters);

/* ---------------------------------------------------------------------------------------------
 * D. 1-D row partition + halo exchange support
 * ------------------------------------------------------------------------------------------- */
/* nnz-balanced contiguous row blocks: bounds[nparts+1], bounds[0]=0, bounds[nparts]=num_v. */
int gnnagg_partition_rows(const int *h_ptr, int num_v, int nparts, int *h_bounds);
/* For rank `rank` owning rows [bounds[rank], bounds[rank+1]): builds the local CSR whose column ids
 * are local-X slots: owned columns -> col - bounds[rank]; remote columns -> n_local + halo slot,
 * halo slots grouped by owner rank in ascending global id.  h_local_ptr[n_local+1] and
 * h_local_idx[nnz_local] are caller-allocated; h_halo_ids (malloc'ed, gnnagg_free_host) lists the
 * global ids of the halo slots; h_halo_counts[nparts] = halo ids owned by each rank. */
int gnnagg_halo_plan(const int *h_ptr, const int *h_idx, int num_v, const int *h_bounds, int nparts, int rank,
                     int *h_local_ptr, int *h_local_idx, int **h_halo_ids, int *h_halo_counts, int *num_halo);
/* The same plan from the rank's OWN rows only: h_ptr_slice[0 .. n_local] (any base offset: the slice of a global ptr array
 * or a 0-based local one) and h_idx_slice[nnz_local] with GLOBAL column ids; num_cols = global column count.  Nothing of
 * the other ranks' rows is needed (gnnagg_halo_plan reads the same data out of a global CSR). */
int gnnagg_halo_plan_slice(const int *h_ptr_slice, const int *h_idx_slice, int num_cols, const int *h_bounds, int nparts, int rank,
                           int *h_local_ptr, int *h_local_idx, int **h_halo_ids, int *h_halo_counts, int *num_halo);
/* The stage plan of a staged halo exchange (gnnagg_dist_step_create_staged): how the rows of every (reader <- owner) list are dealt
 * to stages.  GNNAGG_STAGES_STRIPE: every stage takes slice j of k of EVERY list (each stage keeps all links of the xGMI mesh busy);
 * GNNAGG_STAGES_OWNER: stage s carries the whole lists of the pairs at ring distance s + 1 (world - 1 stages, one peer per stage).
 * Both ends of a pair cut their common list by the same rule, so no coordination is needed.
 *   receiving side (h_recv_rows[world], rows per owner in gnnagg_halo_plan's owner-major slot order; NULL to skip):
 *     h_stage_recv[n_stages][world], h_new_of_old[n_halo] (may be NULL) = the stage-major slot of every owner-major slot: renumber
 *     the halo columns of the local CSR and the halo id list with it; requests still go out owner-major, every owner's list in
 *     the order its rows will ARRIVE (stage by stage)
 *   sending side (h_send_rows[world], rows per reader as served reader-major; NULL to skip):
 *     h_stage_send[n_stages][world], h_send_order[n_send] (may be NULL) = for every stage-major position of the send buffer the index
 *     into the reader-major serve list
 * *n_stages is always written (call with both lists NULL to size the outputs). */
#define GNNAGG_STAGES_STRIPE 0
#define GNNAGG_STAGES_OWNER 1
int gnnagg_halo_stage_plan(const long long *h_recv_rows, const long long *h_send_rows, int world, int rank, int mode, int k, int *n_stages,
                           long long *h_stage_recv, int *h_new_of_old, long long *h_stage_send, int *h_send_order);
/* out[i,:] = x[ids[i],:] for i < n  (send-buffer pack before the all-to-all) */
int gnnagg_pack_rows(const float *d_x, const int *d_ids, int n, int feat, float *d_out, void *hip_stream);

/* RCCL transport (one process per GPU; SURVEY.md 8e: grouped ncclSend / ncclRecv over the xGMI mesh).  librccl is loaded
 * on first use (GNNAGG_ERR_STATE when it cannot be); the communicator binds to the calling thread's current HIP device.
 *   gnnagg_dist_unique_id            rank 0 creates the 128-byte id; the launcher hands it to the other ranks (a file, an
 *                                    environment variable, MPI, a torch.distributed broadcast ...)
 *   gnnagg_dist_comm_create          every rank, same id (collective: returns when all `world` ranks have called it)
 *   gnnagg_dist_comm_create_from_file  the same with the id passed through `path`: all a C++ driver started once per GPU needs.
 *                                    Ranks > 0 publish a fresh random token (<path>.req.<rank>); rank 0 removes whatever an earlier
 *                                    launch left at `path`, draws the id and publishes {magic, world, id, tokens} atomically; a
 *                                    rank accepts only a file that carries ITS token, so a stale file from a crashed run can never
 *                                    feed mismatched ids to ncclCommInitRank (which would hang).  Every wait is bounded by
 *                                    timeout_s (120 when <= 0).  `path` should still be unique per launch (two concurrent
 *                                    launches on one path would fight over it)
 *   gnnagg_dist_alltoallv            h_send_counts[p] / h_recv_counts[p] elements of elem_bytes bytes to / from rank p,
 *                                    packed contiguously in rank order in d_send / d_recv; asynchronous on hip_stream
 *   gnnagg_dist_halo_exchange        one aggregation's halo pull: packs x_local[send_ids] (rows the peers asked for, in
 *                                    rank order) into d_send_buf and exchanges rows of feat floats into d_x_halo */
#define GNNAGG_UNIQUE_ID_BYTES 128
typedef int64_t gnnagg_comm;
int gnnagg_dist_unique_id(char *id128);
int gnnagg_dist_comm_create(const char *id128, int rank, int world, gnnagg_comm *out);
int gnnagg_dist_comm_create_from_file(const char *path, int rank, int world, int timeout_s, gnnagg_comm *out);
int gnnagg_dist_comm_destroy(gnnagg_comm c);
int gnnagg_dist_comm_info(gnnagg_comm c, int *rank, int *world);
/* What really carries this communicator's messages, so that a measurement can say it: the file the nccl* entry points were
 * loaded from (dladdr), whether that was the GNNAGG_RCCL_LIB override (a test double: ranks as processes on one GPU) and the PCI bus id
 * of the HIP device the communicator is bound to (ranks all-gather it: fewer distinct ids than ranks = ranks sharing a GPU).  Any
 * output may be NULL; strings are NUL-terminated and truncated to their capacity. */
int gnnagg_dist_transport_info(gnnagg_comm c, char *library_path, int library_path_cap, char *pci_bus_id, int pci_bus_id_cap, int *is_override);
int gnnagg_dist_alltoallv(gnnagg_comm c, const void *d_send, const long long *h_send_counts, void *d_recv,
                          const long long *h_recv_counts, int elem_bytes, void *hip_stream);
int gnnagg_dist_halo_exchange(gnnagg_comm c, const float *d_x_local, const int *d_send_ids, const long long *h_send_rows,
                              const long long *h_recv_rows, int feat, float *d_send_buf, float *d_x_halo, void *hip_stream);

/* GAT halo rows travel with their attention terms in ONE exchange: out[i, :] = [x[ids[i], 0 .. feat) | att[ids[i], 0 .. att_width)]
 * (att_width = 2 * heads), and the receiving side's split into the halo tails of X_ext / att_ext. */
int gnnagg_pack_rows2(const float *d_x, const float *d_att, const int *d_ids, int n, int feat, int att_width, float *d_out, void *hip_stream);
int gnnagg_unpack_rows2(const float *d_in, int n, int feat, int att_width, float *d_x_out, float *d_att_out, void *hip_stream);

/* The whole row-partitioned step behind ONE host call (pack -> grouped send / recv on a communication stream ->
 * local-source pass -> event wait -> halo-source pass).  Asynchronous: stream operations only (fork / join of the caller's stream
 * and the step's own communication stream through events), nothing allocated per step, so a warm step can be captured into a HIP
 * graph (the capture holds the aggregators' scratch and plan pointers: a later call on them that grows scratch or drops a plan -- a wider
 * feat, more heads, another dtype, a replan option, gnnagg_schedule* -- invalidates it; capture again, gnnagg_set_option).  A rank without peers (comm = 0 or world 1) or without halo rows never creates the second stream.
 *   gnnagg_dist_step_create   comm (0: single rank); agg_local = aggregator over the edges whose source is an owned row, agg_remote
 *                             = aggregator over the halo-source edges (0: none); d_send_ids / h_send_rows / h_recv_rows = the plan
 *                             of gnnagg_dist_halo_exchange (the counts are copied)
 *   gnnagg_dist_step_gcn      y = A_loc . x_local, then y += A_rem . x_halo (GNNAGG_FLAG_ACCUMULATE); agg_remote's column ids are
 *                             halo slots (0-based); reduce = mean / max need gnnagg_set_row_aux on the aggregators (total degrees on
 *                             both for mean; local-source degrees on agg_remote for max)
 *   gnnagg_dist_step_gat      x_ext = [X_local ; X_halo], att_ext likewise ([., heads, 2]); ONE exchange carries [x | att] rows
 *                             (d_send_buf [n_send, feat + 2 heads], d_recv_buf [n_halo, feat + 2 heads]); both aggregators index
 *                             X_ext slots; d_den [n_local, heads] carries the denominators between the two passes
 *                             (gnnagg_gat_run_part)
 *   gnnagg_dist_step_create_staged  the exchange PIPELINED against the halo-source pass: the halo rows arrive in n_stages stages,
 *                             stage s with its own grouped send / recv (h_send_rows / h_recv_rows: [n_stages][world], rows) and its
 *                             own event, and agg_remote[s] (0: no edges) -- an aggregator over the halo-source edges whose source
 *                             arrives in stage s -- runs as soon as stage s has landed, while stage s + 1 is in flight.  Buffers are
 *                             STAGE-MAJOR: d_send_ids, d_send_buf, the halo tail and d_recv_buf list stage 0's rows in rank order,
 *                             then stage 1's ...; agg_remote[s] indexes the whole halo tail (GCN: 0-based halo slots; GAT: X_ext
 *                             slots).  How the rows are dealt to stages is the caller's plan (gnn_computing_amd/dist.py:
 *                             "stripe" -- every stage takes 1/K of EVERY peer's rows, so each stage keeps all xGMI links of the
 *                             mesh busy; "owner" -- stage s exchanges with the peers at ring distance s + 1 only).  The result
 *                             is y = local pass, then += stage 0's pass, += stage 1's ... in this fixed order: deterministic.
 *                             mean: total degrees on every aggregator; max: agg_remote[s] gets the edges folded BEFORE stage s */
typedef int64_t gnnagg_dist_step_t;
int gnnagg_dist_step_create(gnnagg_comm comm, gnnagg_handle agg_local, gnnagg_handle agg_remote, const int *d_send_ids,
                            const long long *h_send_rows, const long long *h_recv_rows, gnnagg_dist_step_t *out);
int gnnagg_dist_step_create_staged(gnnagg_comm comm, gnnagg_handle agg_local, int n_stages, const gnnagg_handle *agg_remote,
                                   const int *d_send_ids, const long long *h_send_rows, const long long *h_recv_rows,
                                   gnnagg_dist_step_t *out);
/* (n_stages, the world size of the step's communicator -- 1 without one) */
int gnnagg_dist_step_info(gnnagg_dist_step_t step, int *n_stages, int *world);
int gnnagg_dist_step_destroy(gnnagg_dist_step_t step);
int gnnagg_dist_step_gcn(gnnagg_dist_step_t step, const float *d_x_local, float *d_x_halo, float *d_send_buf, float *d_y, int feat, int reduce,
                         void *hip_stream);
int gnnagg_dist_step_gat(gnnagg_dist_step_t step, float *d_x_ext, float *d_att_ext, int n_local, float *d_send_buf, float *d_recv_buf,
                         float *d_den, float *d_y, int feat, int heads, float slope, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * F. Neighbour sampling: seeds + fanout -> a relabelled CSR block (csrc/sample.hip; the host twin in csrc/host_graph.cpp)
 * ------------------------------------------------------------------------------------------- */
/* One call takes a device CSR, a list of seed rows, a fanout and a 64-bit seed and returns a message-flow block: one row per seed, at
 * most `fanout` neighbours per row drawn uniformly without replacement, neighbours kept in CSR order; optionally relabelled to compact
 * source ids (seeds first), optionally with the position of every kept edge in the full CSR.  The block is a rectangular CSR: an
 * aggregator created over (d_blk_ptr, d_blk_idx) gathers from a feature matrix with one row per source id.
 *
 * The specification.  Row i of the CSR lists the rows that row i aggregates from.  For a seed row r with the d edges at positions
 * p in [ptr[r], ptr[r+1]):
 *   fanout = -1, or d <= fanout   every edge is kept
 *   d > fanout >= 1               the kept edges are the `fanout` edges with the smallest key(seed, p)
 *   fanout = 0 or < -1            GNNAGG_ERR_ARG
 * Kept edges appear in increasing p: a sampled row is a subsequence of the full row.  key depends on the seed and on the edge's position
 * in the full CSR only -- not on the batch, the row's place in it, the launch geometry or the device -- so row r gets the same sample in
 * every batch that holds it.  The key is built from murmur3's 32-bit finalizer, all arithmetic uint32 with wrap-around:
 *   fmix(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 *   s   = fmix(fmix(lo32(seed) + 0x9E3779B9) ^ hi32(seed))          once per call
 *   key = fmix(fmix(p ^ s) + s)
 * For a fixed seed this is a bijection of p: two edges never tie and there is no tie rule.  Known answers:
 *   s(seed = 0) = 0xaa3e5b61   s(seed = 1) = 0x70f6c6d8
 *   key(1, p = 0) = 0x34d106be   key(1, p = 1) = 0x00486268   key(1, p = 2) = 0x62a55a72   key(1, p = 3) = 0xb34bc796
 *
 * Relabelling (d_src_nodes given): src_nodes[i] = seeds[i] for i < num_seeds (x_dst = x_src[:num_seeds], as DGL's to_block); every other
 * distinct neighbour id follows in the order of its first appearance in the block's edge list; blk_idx holds positions in src_nodes.
 * Duplicate seeds are allowed: each is a row of its own, and an edge to a duplicated seed is relabelled to its first occurrence.  Without
 * d_src_nodes, blk_idx holds global ids (the reference's CSRSubGraph with vertexset = the seeds).
 *
 * gnnagg_sampler_create borrows the CSR (it must outlive the sampler) and allocates a num_v-entry map that is "unseen" between calls.
 * gnnagg_sampler_sample:
 *   d_blk_ptr [num_seeds + 1], d_blk_idx [cap_e], d_blk_eid NULL or [cap_e], d_src_nodes NULL or [num_seeds + cap_e],
 *   d_counts device int[2]: edges kept, source rows (num_v without relabelling)
 *   - everything is enqueued on the sampler's stream (gnnagg_sampler_set_stream; the null stream at first); the call makes no host
 *     synchronisation once the sampler's scratch has its size (it grows with num_seeds and cap_e, never shrinks).  Not capturable into a
 *     HIP graph: sizes are data-dependent and the caller reads d_counts back.
 *   - the sampler's map and scratch belong to the handle: calls on ONE sampler must be ordered.  Calls on one stream are; a caller that
 *     changes the stream between two calls synchronises, or orders the new stream behind the old one with an event, before the second
 *     call.  Two samplers over the same CSR are independent.
 *   - data-dependent sizes stay on the device in d_counts and d_blk_ptr[num_seeds]
 *   - with fanout >= 1, cap_e = num_seeds * fanout always suffices
 *   - if more edges are kept than cap_e, d_blk_ptr and d_counts[0] are still complete and say what was needed; nothing is written past
 *     any capacity and the other outputs are unspecified.  The kept edges of one call must stay below 2^31.
 *   - GNNAGG_ERR_ARG: a null pointer (d_seeds with num_seeds > 0, d_blk_ptr, d_blk_idx with cap_e > 0, d_counts), num_seeds < 0, a bad
 *     fanout, cap_e < 0, num_seeds + cap_e >= 2^31, a handle that is no live sampler.  A refused call leaves the sampler as it was.
 *   - num_seeds = 0 is a valid call that writes blk_ptr[0] = 0 and the counts
 *   - a seed that is no row of the graph is a row without edges (the host twin refuses it: GNNAGG_ERR_ARG)
 *   - no atomics touch the outputs: the result is a function of the arguments, bit for bit
 * gnnagg_sample_block_host is the same function of the same arguments on host arrays (OpenMP over the rows, a serial relabel): the
 * library's CPU path for data-loader workers, usable without a GPU.
 * The reference's sampleVertex* signatures are out of scope: they expand active flags over the globals n, m and no driver calls them;
 * the global-id form above is what a later shim would forward to.
 * (tests/test_sampling_host.py, tests/test_gpu_sampling.py, tests/test_gpu_sampling_forward.py; DESIGN.md "Neighbour sampling")
 *
 * Weighted sampling.  A sampler may carry one weight per edge, w[p], float32, indexed by the edge's position p in the full CSR like val,
 * bias and ef (DGL's sample_neighbors(prob=), PyG's NeighborLoader(weight_attr=)): neighbours are drawn without replacement with
 * probability proportional to w (Efraimidis-Spirakis: the smallest keys -log(u) / w), and an edge of weight zero is never drawn.
 *   Eligibility   an edge is eligible iff w[p] > 0: true for +Inf; false for 0, -0, negative values and NaN.  An ineligible edge is
 *                 never kept, at any fanout.
 *   Rows          a row with d+ eligible edges keeps min(d+, fanout) of them; fanout = -1 keeps every eligible edge.  Kept edges stay
 *                 in CSR order.  Relabelling, eid, capacities, refusals and streams are as above.
 *   Key           from the uniform key u = key(seed, p) above, in integer arithmetic and ONE IEEE division:
 *                   b    = bit length of u                        (0 for u = 0, else 32 - clz(u); 0 ... 32)
 *                   fr   = low 32 bits of ((2u + 1) << (32 - b))  (the fraction of (2u + 1) / 2^b - 1, Q32)
 *                   i    = fr >> 24;   r = (fr >> 8) & 0xFFFF
 *                   lg   = L[i] + (((L[i+1] - L[i]) * r) >> 16)   (64-bit product)
 *                   E    = ((33 - b) << 26) - lg                  uint32, Q6.26:  -log2((u + 1/2) / 2^32)
 *                   q    = float32(E) / w[p]                      conversion and division correctly rounded (to nearest), float32;
 *                                                                 +Inf and denormal quotients are kept as they are
 *                   wkey = the bit pattern of q as uint32 (q >= 0, so uint32 order is float order); 0xFFFFFFFF for an ineligible edge
 *                 L[i] = round(2^26 * log2(1 + i/256)), i = 0 ... 256: 257 integer literals in csrc/sample_key.h, the one text the
 *                 device and the host share.  Every 2^26 * log2(1 + i/256) lies at least 0.0029 from a half-integer, so the literals
 *                 do not depend on the libm that produced them.  E / 2^26 is within 2.9e-6 of the exact value.
 *   Selection     the kept edges of a row with d+ > fanout are the `fanout` eligible edges with the smallest wkey.  wkey is no bijection:
 *                 among equal keys the lower position p wins.
 *   Nothing else is floating point: no library log or exp, nothing that depends on FMA contraction, no tolerance.  Known answers:
 *     L[1] = 377457   L[128] = 39256169   L[256] = 67108864
 *     E(u = 0) = 2214592512   E(u = 0x80000000) = 67108864   E(u = 0xFFFFFFFF) = 3
 *     wkey(seed = 1, p, w = 1.5), p = 0 ... 3:  0x4cc24fa9  0x4dd18b60  0x4c6ace39  0x4baf60af   (E = 152812522, 659169777, 92329303,
 *     34480653)
 *   - constant weights give a valid uniform sample, but NOT the unweighted call's sample: E decreases in u, and quantisation ties go to
 *     the lower position
 *   - weights are not scale-invariant bit for bit (2w rounds other quotients than w)
 *   - +Inf weights all tie at key 0: such a row keeps its first `fanout` +Inf edges in CSR order
 * gnnagg_sampler_set_weights(s, d_w): d_w [num_e] is borrowed like the CSR; NULL returns the sampler to uniform sampling (it then launches
 * the kernels it launched before).  The call counts the eligible edges of every row on the sampler's stream (flags, one scan, a
 * difference at the row boundaries: num_e + 1 ints of scratch, released before it returns) and waits for the count: the per-call work
 * stays O(1) per seed before the select.  The weights are read again by every sample: whoever changes them in place calls
 * set_weights again.  GNNAGG_ERR_ARG: a handle that is no live sampler.  A refused or failed call leaves the sampler as it was.
 * gnnagg_sample_block_host_weighted is gnnagg_sample_block_host with h_w [num_e] (NULL: that function itself).
 * (tests/sampling_weighted_ref.py, tests/test_sampling_weighted_host.py, tests/test_gpu_sampling_weighted.py) */
typedef int64_t gnnagg_sampler;
int gnnagg_sampler_create(const int *d_ptr, const int *d_idx, int num_v, int num_e, gnnagg_sampler *out);
int gnnagg_sampler_destroy(gnnagg_sampler s);
int gnnagg_sampler_set_stream(gnnagg_sampler s, void *hip_stream);
int gnnagg_sampler_sample(gnnagg_sampler s, const int *d_seeds, int num_seeds, int fanout, unsigned long long seed,
                          int *d_blk_ptr, int *d_blk_idx, int *d_blk_eid, long long cap_e, int *d_src_nodes, int *d_counts);
int gnnagg_sample_block_host(const int *h_ptr, const int *h_idx, int num_v, const int *h_seeds, int num_seeds, int fanout,
                             unsigned long long seed, int *h_blk_ptr, int *h_blk_idx, int *h_blk_eid, long long cap_e,
                             int *h_src_nodes, int *h_counts);
int gnnagg_sampler_set_weights(gnnagg_sampler s, const float *d_w);
int gnnagg_sample_block_host_weighted(const int *h_ptr, const int *h_idx, const float *h_w, int num_v, const int *h_seeds, int num_seeds,
                                      int fanout, unsigned long long seed, int *h_blk_ptr, int *h_blk_idx, int *h_blk_eid,
                                      long long cap_e, int *h_src_nodes, int *h_counts);

/* Block aggregation: the GCN / SAGE aggregation of one sampled block in one launch, straight from (d_blk_ptr, d_blk_idx) -- no handle, no
 * plan, no gathered copy of the source rows (csrc/agg_block.hip).  A block is used once and its rows hold at most `fanout` edges: there is
 * nothing a plan could balance, and creating one costs more than the run.  For destination row i < num_dst and column c < feat, over the
 * edges p in [blk_ptr[i], blk_ptr[i+1]) in increasing p:
 *   s(p) = d_src_nodes ? d_src_nodes[blk_idx[p]] : blk_idx[p]          the row of x
 *   w(p) = !d_val ? 1.0f : d_eid ? d_val[d_eid[p]] : d_val[p]
 *   sum    acc = 0.0f;  acc = fmaf(widen(x[s(p)][c]), w(p), acc)       one fp32 chain per (row, column), CSR order
 *   mean   the sum, then acc / (float)deg where deg > 0                deg = the row's edges IN THE BLOCK
 *   max    acc = -inf;  t = widen(x) * w;  acc = t > acc ? t : acc;    0 for a row without edges
 *   then ReLU if flagged (a NaN stays a NaN); y[i][c] = acc            a bf16 y is ONE round-to-nearest-even at the store
 *   x_dst (optional): x_dst[i][:] = x[d_src_nodes[i]][:]               the row copied as it is, no arithmetic
 * These are the operations and the order of the handle's rows mode: for fp32 the result is, bit for bit, what a GCN aggregator created
 * over (d_blk_ptr, d_blk_idx, val) gives in GNNAGG_MODE_ROWS on x[src_nodes].
 *   operands     d_x holds rows of `feat` elements of x_dtype, x_pitch ELEMENTS apart (x_pitch >= feat, as the pitches of
 *                gnnagg_dot_attn_run): the matrix the block was sampled from, read through d_src_nodes, or -- d_src_nodes NULL -- the
 *                rows blk_idx names directly (x[src_nodes], the previous layer's output, or a block of global ids).  d_val NULL: weight 1;
 *                d_val without d_eid: one value per edge of the block; with d_eid: d_val holds one value per edge of the full CSR and
 *                d_eid [edges of the block] the position of every block edge in it (the sampler's d_blk_eid).  d_y and d_x_dst are dense
 *                [num_dst, feat] of y_dtype / x_dtype and alias no input.
 *   types        GNNAGG_DTYPE_F32 and GNNAGG_DTYPE_BF16 for x and y, all four pairs; accumulation is fp32.  A bf16 x gives the fp32 call
 *                on x widened (exact).
 *   determinism  the bits depend on the arguments only, never on alignment, pitch or lane geometry (lanes are as wide as feat, x_pitch
 *                and the alignment of x, y and x_dst allow).  No atomics.
 *   non-finite   +-Inf / NaN reach exactly the rows that hold them as neighbours (no padding lane multiplies a real source row by zero);
 *                GNNAGG_REDUCE_MAX over a NaN operand is unspecified.
 *   flags        GNNAGG_FLAG_RELU only.
 *   the call     stateless: no handle, no allocation, no host synchronisation, ONE launch on hip_stream; capturable into a HIP graph
 *                (num_dst is the caller's, the edge count is read from d_blk_ptr on the device).  num_dst = 0 is a valid call that
 *                launches nothing.  Ids are not validated, as everywhere else.
 *   rows         a row of any length is walked by its one lane group: the chain cannot be split without changing its bits, and a
 *                sampled row is short.  For blocks taken with fanout = -1 that hold hub rows a handle's rows mode remains the fast path.
 *   refusals     GNNAGG_ERR_ARG with a text naming the argument, before any HIP call: a null d_blk_ptr, d_x or d_y with num_dst > 0;
 *                num_dst < 0; feat < 1; x_pitch < feat; an unknown x_dtype, y_dtype or reduce; any flag but GNNAGG_FLAG_RELU; d_eid
 *                without d_val; d_x_dst without d_src_nodes.
 * (tests/block_run_ref.py, tests/test_block_run_host.py, tests/test_gpu_block_run.py; DESIGN.md "Block aggregation") */
int gnnagg_block_gcn_run(const int *d_blk_ptr, const int *d_blk_idx, int num_dst, const int *d_src_nodes, const float *d_val,
                         const int *d_eid, const void *d_x, int x_dtype, long long x_pitch, void *d_y, int y_dtype, void *d_x_dst,
                         int feat, int reduce, int flags, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * E. Extras: libgnnagg_extras.so only (`make -C gnn_computing_amd/csrc extras`, -DGNNAGG_EXTRAS).  NOT in the shipped library:
 *    the reference is forward-only and SURVEY 2.2 marks its one backward kernel ("Experiment", no caller) out of scope.
 * ------------------------------------------------------------------------------------------- */
#ifdef GNNAGG_EXTRAS
/* Backward of the GCN / SAGE sum aggregation y = A.x (no reference counterpart: the reference is forward-only):
 * d_dinput[V, feat] = A^T . d_doutput with the aggregator's edge values, as a deterministic gather over the
 * transposed CSR (built once per handle) on the balanced kernels.  Square graphs (neighbor ids < num_v). */
int gnnagg_gcn_run_bwd(gnnagg_handle h, const float *d_doutput, float *d_dinput, int feat);
/* Aggregator_GAT::run_bwd, aggr_gat.h:426-434 (kernel aggr_gat_fine_bwd :222-296, marked "Experiment" in the reference and
 * called by none of its drivers).  Backward of the single-head fused aggregation out_r = sum_e w_e x_s / D_r given the
 * forward pass's un-normalised edge weights newval[E] (w_e) and denominators div[V] (D_r):
 *   d_feat_grad[V,feat]  = gradient w.r.t. the input features through the aggregation (attention held constant)
 *   d_a_b_grad[V,2]      = gradient w.r.t. att: [.,0] centre term, [.,1] source term
 * Differences from the reference kernel, which stops short of its own comments: all `feat` columns (not 32), the
 * leaky-ReLU slope applied where z_e < 0 (the reference tests newval < 0, never true), the centre-term gradient is
 * produced, and both outputs are OVERWRITTEN with deterministic sums (the reference atomically accumulates into
 * caller-zeroed buffers).  heads == 1 only. */
int gnnagg_gat_run_bwd(gnnagg_handle h, const float *d_output, const float *d_doutput, const float *d_newval, const float *d_div,
                       const float *d_infeat, float *d_a_b_grad, float *d_feat_grad, float relu_slope, int feat);
#endif /* GNNAGG_EXTRAS */

#ifdef __cplusplus
}
#endif
#endif /* GNNAGG_H */
