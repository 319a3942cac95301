"""GPU: a handle with a history computes what a fresh handle in the same configuration computes.

Every other GPU test makes a fresh aggregator, configures it once, runs it and throws it away; callers keep one handle per graph for the life
of a model (examples/forward_3layer.py).  A handle is a state machine of lazily built caches (csrc/api_internal.h: plan, plan_sched, plan_part,
rb, rows_plan, t0_sorted, the grow-only scratch, the hub counters, gatv2, ...), each dropped at a different place or never.  Here one handle
lives through a list of steps; after EVERY run step the same run is made on fresh outputs on a replay twin (every configuration call of the
history, none of the runs) and on a minimal twin (only the configuration still in force), both brand-new handles, and tests/lifetime_helper.py
asserts: the queries agree, the outputs are bit-equal (GCN and GAT: no atomics, fixed fold order), the long-lived handle's output is the oracle
restated from the handle's own queries (GCN bit for bit; GAT within the bound the same call already has in the suite), the guard words around
every output are intact and rows without edges read 0 (or stay at the canary under ACCUMULATE).  A call the header refuses must raise, write
nothing and change no query.  The failure message is the whole step list.

Transition -> scripted test:
    feature width (scratch grown and oversized, hub-counter stride, t0_sorted reuse)     test_width_walk
    rb built from another ntiles_hint / after rows_blocked_ranges()                      test_rows_blocked_chain_whatever_built_it
    dtype (sorted-rows rule by row bytes, the chunked plan beside the blocked order)     test_dtype_walk
    reduce x flags, ACCUMULATE through build_balanced_plan_keep, set_row_aux             test_flags_and_reductions
    schedule() kinds, plan_sched dropped / rebuilt, schedule_balanced                    test_schedules
    each of the twelve options set and set back                                          test_option_set_and_set_back
    scratch_limit_mb demotion for good, partitions = -1 re-enables                       test_demotion_is_sticky_until_partitions_is_set
    updateval / in-place rewrite on every order                                          test_edge_values_follow_the_callers_array
    GAT: heads, stable / shift / row_shift (shift, den, partial_den sized by heads)     test_gat_lifetime_softmax_forms
    GAT: run_v2 scratch growth with (feat, heads, dtype)                                test_gat_lifetime_run_v2_scratch_growth
    GAT: newval and the same run without, edge ops, run_part 1 + 2, probe_gather        test_gat_lifetime_outputs_and_passes
    run_with_nn / run_with_nn_typed and last_nn_path                                     test_fused_product
    the stream in force                                                                  test_streams
    refused calls in mid-life                                                            test_refused_calls_in_mid_life
    a handle freed inside another handle's graph capture                                 test_a_handle_freed_while_another_handles_call_is_captured
"""
import os

import pytest
import torch

import lifetime_helper as lh
from lifetime_helper import MODES, Life

pytestmark = pytest.mark.gpu


def run_modes(life, op, p, modes=MODES):
    """the same call in rows, scheduled and balanced mode: where the header refuses the combination, Life.run asserts the refusal"""
    return {mode: life.run(op, dict(p, mode=mode)) for mode in modes}


def with_schedule(kind, gname, fast_scheduled=0, **kw):
    """a handle whose scheduled mode is an order of its own: a neighbor-grouping schedule the plan kernel runs, in the restated order"""
    life = Life(kind, gname, **kw)
    life.do(("opt", "fast_scheduled", fast_scheduled))
    life.do(("sched", "neighbor_grouping", [32]))
    return life


# ------------------------------------------------------------------------------------------------------------------ width walk
@pytest.mark.parametrize("gname", ["G_plan", "G_blocked"])
def test_width_walk(gname):
    """602 -> 32 -> 130 -> 7 -> 64 -> 602, fp32: scratch that grew and is now oversized, the hub counters read at another stride, t0_sorted built at
    the first narrow width and reused at the next"""
    life = with_schedule("gcn", gname)
    for F in (602, 32, 130, 7, 64, 602):
        run_modes(life, "run", {"F": F})


def test_rows_blocked_chain_whatever_built_it():
    """the rows-mode chain plan takes its hub threshold from the width of the first run that builds it, or from the query: three histories,
    the same bits, equal to the sequential chain (Life.run judges rows mode against orc.gcn_seq)"""
    results = []
    for first in (602, 64, "query"):
        life = Life("gcn", "G_blocked", minimal=False)
        if first == "query":
            life.do(("query_rb",))
            assert life.history[-1][-1] > 1
        order = (602, 64) if first != 64 else (64, 602)
        outs = {F: life.run("run", {"F": F, "mode": "rows"}) for F in order}
        outs["mean"] = life.run("run", {"F": 64, "mode": "rows", "reduce": "mean"})
        assert life.h.rows_blocked_ranges() > 1
        results.append(outs)
    for other in results[1:]:
        for k in results[0]:
            assert torch.equal(results[0][k]["y"][0], other[k]["y"][0]), k


# ------------------------------------------------------------------------------------------------------------------ dtype walk
@pytest.mark.parametrize("gname", ["G_plan", "G_blocked"])
def test_dtype_walk(gname):
    """fp32 -> (bf16, bf16) -> (bf16, fp32) -> fp32 -> (fp32, bf16) at widths 128 and 64.  G_plan: the short rows are degree-sorted by ROW BYTES
    (fp32 64, bf16 128 and 64 sorted, fp32 128 not), every combination bit-equal to the fresh handles and the oracle.  G_blocked: the typed runs
    take the chunked plan built beside the blocked order on first use; the blocked order stays in force for the next fp32 run."""
    life = with_schedule("gcn", gname, fast_scheduled=1)
    parts = life.h.balanced_partitions()
    assert (parts > 1) == (gname == "G_blocked")
    for xdt, ydt in (("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("f32", "bf16")):
        for F in (128, 64):
            run_modes(life, "run", {"F": F, "xdt": xdt, "ydt": ydt})
            assert life.h.balanced_partitions() == parts, life.story()
    life.do(("opt", "fast_rows", 1))       # rows mode on the balanced order takes the 16-bit types too
    run_modes(life, "run", {"F": 64, "xdt": "bf16", "ydt": "bf16"})


# ------------------------------------------------------------------------------------------------------------------ flags and reductions
@pytest.mark.parametrize("gname", ["G_plan", "G_blocked"])
def test_flags_and_reductions(gname):
    """sum, mean, max x {plain, RELU, ACCUMULATE, ACCUMULATE | RELU} interleaved on one handle.  On G_blocked an ACCUMULATE run builds the chunked
    plan beside the blocked order (build_balanced_plan_keep); the plain balanced run that follows must still be the blocked order as reported.
    Then set_row_aux -> mean / max ACCUMULATE -> set_row_aux(None) -> plain mean / max."""
    life = with_schedule("gcn", gname)
    parts = life.h.balanced_partitions()
    F = 64
    for flags in ({}, {"relu": True}, {"acc": True}, {"acc": True, "relu": True}):
        for reduce in ("sum", "mean", "max"):
            run_modes(life, "run", dict(flags, F=F, reduce=reduce))
            if flags.get("acc"):
                life.run("run", {"F": F, "mode": "balanced"})       # the plain run right behind an accumulating one
                assert life.h.balanced_partitions() == parts, life.story()
    life.do(("row_aux", "deg1"))
    for reduce in ("mean", "max", "sum"):
        for flags in ({"acc": True}, {}, {"acc": True, "relu": True}):
            run_modes(life, "run", dict(flags, F=F, reduce=reduce))
    life.do(("row_aux", None))
    for reduce in ("mean", "max"):
        run_modes(life, "run", {"F": F, "reduce": reduce})
    assert life.h.balanced_partitions() == parts


# ------------------------------------------------------------------------------------------------------------------ schedules
@pytest.mark.parametrize("fast_scheduled", [0, 1])
def test_schedules(fast_scheduled):
    """neighbor_grouping 32 -> 2 (padding ratio above 1.5: plan_sched dropped, the item kernels run) -> 16, locality 3 -> locality_neighbor_grouping
    (3, 4) -> neighbor_grouping 16, fp32 and bf16 after each (the typed run is refused where the item kernels run the schedule); then
    schedule_balanced 4 -> 64 -> 0 with runs between"""
    life = Life("gcn", "G_plan")
    life.do(("opt", "fast_scheduled", fast_scheduled))
    assert life.g.padding_ratio(2) > 1.5 and life.g.padding_ratio(32) <= 1.5 and life.g.padding_ratio(16) <= 1.5
    for kind, param in (("neighbor_grouping", [32]), ("neighbor_grouping", [2]), ("neighbor_grouping", [16]), ("locality", [3]),
                        ("locality_neighbor_grouping", [3, 4]), ("neighbor_grouping", [16])):
        life.do(("sched", kind, param))
        for F in (64, 130):
            run_modes(life, "run", {"F": F})
        run_modes(life, "run", {"F": 64, "xdt": "bf16", "ydt": "bf16"}, modes=("scheduled", "balanced"))
        life.run("run", {"F": 64, "mode": "scheduled", "reduce": "mean", "relu": True})
    for chunk in (4, 64, 0):
        life.do(("sched_bal", chunk))
        for F in (32, 130):
            run_modes(life, "run", {"F": F})


# ------------------------------------------------------------------------------------------------------------------ options
OPTION_CASES = [   # (option, graph, the mode it governs, width)
    ("partitions", "G_blocked", "balanced", 130), ("tile_width", "G_blocked", "balanced", 130), ("slice_kb", "G_blocked", "balanced", 130),
    ("scratch_limit_mb", "G_blocked", "balanced", 64), ("fast_rows", "G_plan", "rows", 64), ("reference_defaults", "G_plan", "rows", 64),
    ("fast_scheduled", "G_plan", "scheduled", 64), ("aux_stream", "G_plan", "rows", 130), ("rows_blocked", "G_blocked", "rows", 130),
    ("rows_medium_edges", "G_plan", "rows", 64), ("rows_hub_tile", "G_plan", "rows", 130), ("rows_hub_edges", "G_blocked", "rows", 130),
]


@pytest.mark.parametrize("name,gname,mode,F", OPTION_CASES)
def test_option_set_and_set_back(name, gname, mode, F):
    """a warm run in the mode the option governs, the option at a non-default legal value, the option back: the last run equals the first bit
    for bit, every run equals the twins', and the minimal twin (which never saw the option move) reports the same queries"""
    assert len({c[0] for c in OPTION_CASES}) == 12
    life = Life("gcn", gname)
    life.do(("sched", "neighbor_grouping", [32]))
    back = life.m.opts[name]
    first = run_modes(life, "run", {"F": F})
    for value in lh.OPTION_VALUES[name]:
        if value == back:
            continue
        life.do(("opt", name, value))
        run_modes(life, "run", {"F": F})
        life.run("run", {"F": 32, "mode": mode, "reduce": "mean"})
        life.do(("opt", name, back))
        last = run_modes(life, "run", {"F": F})
        for m in MODES:
            assert torch.equal(first[m]["y"][0], last[m]["y"][0]), "%s set to %d and back: mode %s\n%s" % (name, value, m, life.story())


def test_demotion_is_sticky_until_partitions_is_set():
    """scratch_limit_mb = 1 on G_blocked: the balanced run demotes the handle to the chunked plan for good -- it stays there after the limit is
    lifted (the replay twin, which replays the demoting run, is the reference; the minimal twin is on the blocked order and Life.run asserts
    that it differs) -- and partitions = -1 re-enables the blocked order"""
    life = Life("gcn", "G_blocked")
    parts = life.h.balanced_partitions()
    assert parts > 1
    run_modes(life, "run", {"F": 64}, modes=("rows", "balanced"))
    life.do(("opt", "scratch_limit_mb", 1))
    life.run("run", {"F": 130, "mode": "balanced"})
    assert life.m.demoted and life.h.balanced_partitions() == 0 and life.h.balanced_params()[1] == 16
    life.run("run", {"F": 130, "mode": "balanced", "reduce": "mean"})
    life.do(("opt", "scratch_limit_mb", 0))
    run_modes(life, "run", {"F": 64}, modes=("rows", "balanced"))
    assert life.h.balanced_partitions() == 0, "demoted for good: " + life.story()
    life.do(("opt", "partitions", -1))
    assert not life.m.demoted
    run_modes(life, "run", {"F": 64}, modes=("rows", "balanced"))
    assert life.h.balanced_partitions() == parts, life.story()


# ------------------------------------------------------------------------------------------------------------------ edge values
@pytest.mark.parametrize("gname", ["G_plan", "G_blocked"])
def test_edge_values_follow_the_callers_array(gname):
    """a handle that has run on its balanced order (chunked plan / 2-D blocked), in rows mode (row kernels / the rows-blocked chain) and on a user
    locality schedule: updateval(v2), v2 rewritten in place, updateval(v3) -- every path follows the caller's array at run time"""
    life = Life("gcn", gname)
    life.do(("opt", "fast_scheduled", 0))
    life.do(("sched", "locality", [3]))

    def everywhere():
        run_modes(life, "run", {"F": 64})
        life.run("run", {"F": 130, "mode": "balanced", "acc": True})
        life.run("run", {"F": 64, "mode": "balanced", "xdt": "bf16", "ydt": "f32"})
    everywhere()
    life.do(("updateval", "v2"))
    everywhere()
    life.do(("rewrite", "v2", 4711))
    everywhere()
    life.do(("sched", "locality_neighbor_grouping", [3, 4]))
    life.do(("rewrite", "v2", 4712))
    everywhere()
    life.do(("updateval", "v3"))
    everywhere()


# ------------------------------------------------------------------------------------------------------------------ GAT
@pytest.mark.parametrize("gname", ["G_plan", "G_blocked"])
def test_gat_lifetime_softmax_forms(gname):
    """one Aggregator_GAT through run -> stable -> shift -> row_shift at H = 1, 8, 1 (shift / den / partial_den sized by heads) -- then the first
    run again, bit-equal to its first result.  (The GAT theme is three tests, this one and the next two, each on one long-lived handle: the
    float64 judges of the shifted and the GATv2 forms take most of the time.)"""
    life = Life("gat", gname)
    life.do(("sched", "neighbor_grouping", [32]))
    first = run_modes(life, "run", {"H": 1, "D": 128})
    for H, D in ((1, 128), (8, 16), (1, 128)):
        run_modes(life, "run", {"H": H, "D": D})
        life.run("run", {"H": H, "D": D, "mode": "balanced", "stable": True})
        life.run("run", {"H": H, "D": D, "mode": "scheduled", "stable": True, "xdt": "bf16", "ydt": "bf16"})
        life.run("run", {"H": H, "D": D, "mode": "balanced", "shift": True})
        life.run("run", {"H": H, "D": D, "mode": "rows", "stable": True})      # refused: the canonical rows mode has no shifted form
        life.run("row_shift", {"H": H, "D": D})
    last = run_modes(life, "run", {"H": 1, "D": 128})
    for m in MODES:
        assert torch.equal(first[m]["y"][0], last[m]["y"][0]), "mode %s\n%s" % (m, life.story())


@pytest.mark.parametrize("gname", ["G_plan", "G_blocked"])
def test_gat_lifetime_run_v2_scratch_growth(gname):
    """run -> run_v2 at (1, 128) fp32, (8, 16) bf16, (2, 301) fp32 on G_plan (gatv2.scratch grows with feat, heads and dtype; narrower shapes on
    G_blocked, whose float64 judge costs five times as much per column) -> a stable run -> run_v2 at the first shape again -> the first run
    again, bit-equal to its first result"""
    life = Life("gat", gname)
    life.do(("sched", "neighbor_grouping", [32]))
    first = run_modes(life, "run", {"H": 8, "D": 16})
    shapes = ((1, 128, "f32"), (8, 16, "bf16"), (2, 301, "f32")) if gname == "G_plan" else ((4, 3, "f32"), (8, 16, "bf16"), (8, 16, "f32"))
    for H, D, dt in shapes + shapes[:1]:
        life.run("v2", {"H": H, "D": D, "xdt": dt, "ydt": dt})
        life.run("run", {"H": 8, "D": 16, "mode": "balanced", "stable": True, "xdt": dt, "ydt": "f32"})
    last = run_modes(life, "run", {"H": 8, "D": 16})
    for m in MODES:
        assert torch.equal(first[m]["y"][0], last[m]["y"][0]), "mode %s\n%s" % (m, life.story())


@pytest.mark.parametrize("gname", ["G_plan", "G_blocked"])
def test_gat_lifetime_outputs_and_passes(gname):
    """one Aggregator_GAT through run, a stable run and run_v2 (the scratch of the previous test's forms exists), a head width the span kernel does
    not tile, run with newval under fast_scheduled = 1 (keeps the user's groups) and the same run without, run_att / run_u_add_v /
    run_add_to_center / run_div_each, run_part 1 + 2, the probe (2-D blocked order only: refused on G_plan; writes nothing and disturbs
    nothing) -- then the first run again, bit-equal to its first result"""
    life = Life("gat", gname)
    life.do(("sched", "neighbor_grouping", [32]))
    first = run_modes(life, "run", {"H": 1, "D": 128})
    life.run("run", {"H": 8, "D": 16, "mode": "balanced", "stable": True})
    life.run("v2", {"H": 8, "D": 16, "xdt": "bf16", "ydt": "bf16"})
    run_modes(life, "run", {"H": 4, "D": 3})        # the descriptor form of the blocked order (force_host_plan)
    for newval in (True, False):
        run_modes(life, "run", {"H": 8, "D": 16, "newval": newval})
    life.run("edge_ops", {"H": 8, "D": 16})
    life.run("part", {"H": 1, "D": 128})
    life.run("part", {"H": 8, "D": 16})
    life.run("part", {"H": 4, "D": 3})              # refused: a lane's four columns must lie inside one head
    x0, att0 = life.P.x(128).clone(), life.P.att(1).clone()
    life.run("probe", {"H": 1, "D": 128, "mode": "balanced"})
    life.run("probe", {"H": 1, "D": 128, "mode": "rows"})      # refused
    assert torch.equal(x0, life.P.x(128)) and torch.equal(att0, life.P.att(1))
    last = run_modes(life, "run", {"H": 1, "D": 128})
    for m in MODES:
        assert torch.equal(first[m]["y"][0], last[m]["y"][0]), "mode %s\n%s" % (m, life.story())


# ------------------------------------------------------------------------------------------------------------------ fused product
def test_fused_product():
    """run -> run_with_nn -> run_with_nn_typed (fp32, bf16 128 -> 32, bf16 128 -> 64 which falls back to the GEMM) -> run: last_nn_path is what
    today's rules say (1 for the two fp32 products and for bf16 128 -> 32, 2 for bf16 128 -> 64), stays put over plain runs and is 0 only on the
    twins that never ran the product"""
    life = with_schedule("gcn", "G_plan")
    run_modes(life, "run", {"F": 128})
    assert life.h.last_nn_path() == 0
    run_modes(life, "nn", {"F": 128, "OUT": 32})
    assert life.h.last_nn_path() == 1
    for p, want in (({"xdt": "f32", "ydt": "f32", "tdt": "f32", "OUT": 32}, 1), ({"xdt": "bf16", "ydt": "bf16", "tdt": "f32", "OUT": 32}, 1),
                    ({"xdt": "bf16", "ydt": "bf16", "tdt": "bf16", "OUT": 32}, 1), ({"xdt": "bf16", "ydt": "bf16", "tdt": "f32", "OUT": 64}, 2),
                    ({"xdt": "f32", "ydt": "f32", "tdt": "f32", "OUT": 32, "relu": True, "reduce": "mean"}, 1)):
        life.run("nn_typed", dict(p, F=128, mode="balanced"))
        assert life.h.last_nn_path() == want, (p, life.story())
        life.run("nn_typed", dict(p, F=128, mode="scheduled"))
        life.run("nn_typed", dict(p, F=128, mode="rows"))          # refused unless all fp32 without ReLU
        life.run("run", {"F": 64, "mode": "balanced"})
    run_modes(life, "nn", {"F": 602, "OUT": 32})
    assert life.h.last_nn_path() == 2
    run_modes(life, "run", {"F": 128})


# ------------------------------------------------------------------------------------------------------------------ streams
@pytest.mark.parametrize("gname", ["G_plan", "G_blocked"])
def test_streams(gname):
    """the width walk with the current torch stream switched null -> side -> second side -> null between steps (the new stream waits for the old
    one, as test_stream_is_honoured; everything is synchronised before it is compared).  Hub rows in rows mode: the auxiliary-stream fork / join
    and the hub counters move with the stream.  Also passes under GNNAGG_TEST_STREAM=side (the base stream is then a side stream)."""
    life = with_schedule("gcn", gname)
    names = ("null", "side", "side2", "null", "side2", "side")
    used = []
    for F, name in zip((602, 32, 130, 7, 64, 602), names):
        life.do(("stream", name))
        del life.launched_on[:]
        run_modes(life, "run", {"F": F})
        life.run("run", {"F": F, "mode": "rows", "reduce": "mean", "relu": True})
        # every launch of the step went to the stream just switched to (Life._run also asserts that it is torch's current stream there)
        assert life.launched_on == [life.streams[name].cuda_stream] * 4, life.story()
        used.append(life.streams[name].cuda_stream)
    assert len(set(used)) == 3 and used[0] == used[3] and used[1] == used[5] and used[2] == used[4], used
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ refused calls
@pytest.mark.parametrize("kind,gname", [("gcn", "G_plan"), ("gcn", "G_blocked"), ("gat", "G_plan")])
def test_refused_calls_in_mid_life(kind, gname):
    """after warm runs, each call the header refuses: it raises, leaves y at its canary and every query as it was, and the next accepted runs
    match the twins and the oracle restated from the handle's queries.  Two of these left the handle half-changed before this test existed:
    a refused schedule() dropped plan_sched under a schedule that stayed in force, and a refused run_with_nn set last_nn_path."""
    life = with_schedule(kind, gname)
    p = {"F": 64} if kind == "gcn" else {"H": 1, "D": 128}
    run_modes(life, "run", p)
    names = lh.REFUSALS_GCN + ("schedule_locality0", "nn_scheduled_after_nop") if kind == "gcn" else lh.REFUSALS_GAT + ("schedule_locality0",)
    for what in names:
        if what in ("scheduled_after_nop", "nn_scheduled_after_nop"):
            continue
        life.do(("refuse", what))
        run_modes(life, "run", p)
    if kind == "gcn":
        life.run("nn", {"F": 64, "OUT": 32, "mode": "balanced"})
    for what in ("scheduled_after_nop",) + (("nn_scheduled_after_nop",) if kind == "gcn" else ()):
        life.do(("refuse", what))          # (makes schedule(nop) first: an accepted configuration call)
        run_modes(life, "run", p)          # the scheduled run is asserted to be refused, the others to match
    life.do(("sched", "neighbor_grouping", [16]))
    run_modes(life, "run", p)


# ------------------------------------------------------------------------------------------------------------------ the end of a life
def test_a_handle_freed_while_another_handles_call_is_captured():
    """A Python caller's handle is freed where the garbage collector finds it (Aggregator.__del__; a `pytest.raises(...) as e` block is
    enough to keep one in a dead cycle), and that may be in the middle of a graph capture of a call on ANOTHER handle.  gnnagg_destroy
    synchronises and frees: under the global capture mode that invalidated the capture in progress, with no error at the destroy and
    hipErrorStreamCaptureInvalidated at the end of the capture (tests/test_gpu_bf16.py::test_graph_capture_and_replay failed so, depending on
    when the collector ran).  Three handles die inside the capture: one that never ran, one with an auxiliary stream and events (rows mode with
    hub rows) whose stream is the null stream, one whose stream is a side stream.  The capture ends, replays and gives the bits of a plain
    run; nothing of the captured handle is touched, so this replays no capture whose scratch or plan has gone."""
    import gnn_computing_amd as gnc
    P = lh.pool("G_plan")
    F = 64
    x = P.x(F)
    new = lambda: gnc.Aggregator_GCN(P.dptr, P.didx, P.val_d["v1"], F, F)
    live, never_ran, ran_rows, ran_on_side = new(), new(), new(), new()
    ref, scratch = torch.empty_like(x), torch.empty_like(x)
    live.run(x, ref, 512, "balanced")                # warm: plan, scratch, counters
    ran_rows.run(x, scratch, 512, "rows")
    ran_rows.run(x, scratch, 512, "balanced")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ran_on_side.run(x, scratch, 512, "balanced")
    torch.cuda.synchronize()
    buf, y = lh.canary(P.g.V, F, torch.float32)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        live.run(x, y, 512, "balanced")
        for dying in (never_ran, ran_rows, ran_on_side):
            dying.close()
    assert lh.untouched(buf)                         # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ref) and lh.guards_intact(buf)
    live.run(x, scratch, 512, "balanced")            # and the handle goes on as before
    torch.cuda.synchronize()
    assert torch.equal(scratch, ref)


# ------------------------------------------------------------------------------------------------------------------ random walks
def _walk(kind):
    seed = int(os.environ.get("FUZZ_SEED", str(lh.FUZZ_SEED_DEFAULT)))
    for case in range(int(os.environ.get("FUZZ_CASES", str(lh.FUZZ_CASES_DEFAULT)))):
        gname, steps = lh.gen_walk(seed, case, kind)
        life = Life(kind, gname, minimal=False)
        for _, st in steps:
            life.do(st)
        torch.cuda.synchronize()


def test_lifetime_random_walk_gcn():
    """a seeded random sequence of the transitions above on one GCN handle over G_plan / G_blocked (tests/lifetime_helper.py: gen_walk; its
    conditions are asserted on the CPU by tests/test_handle_lifetime_host.py), the replay twin and the oracle after every run"""
    _walk("gcn")


def test_lifetime_random_walk_gat():
    _walk("gat")
