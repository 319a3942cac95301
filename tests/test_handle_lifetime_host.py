"""CPU: the step generator of the lifetime random walks (tests/lifetime_helper.py: gen_walk, run on the GPU by
tests/test_gpu_handle_lifetime.py::test_lifetime_random_walk_*) cannot degenerate into configuration calls and refusals.  For the default seed
and case count: every transition kind occurs, every kind is followed at least once by an accepted run in each of the three modes, every walk
holds at least as many accepted runs as configuration steps, and at most one step in five of any walk is a documented refusal.  Also: the
graphs are what the GPU tests take them for, and the model's padding ratio restates do_schedule's rule."""
import numpy as np
import pytest

import lifetime_helper as lh


@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_the_default_walks_cover_every_transition_in_every_mode(kind):
    kinds = lh.GCN_KINDS if kind == "gcn" else lh.GAT_KINDS
    seen, followed, per_walk = lh.walk_summary(kind)
    assert seen == set(kinds)
    for k in kinds:
        assert followed.get(k, set()) == set(lh.MODES), (k, followed.get(k))
    assert len(per_walk) == lh.FUZZ_CASES_DEFAULT
    for runs, config, refused, steps in per_walk:
        assert runs >= config, (runs, config)
        assert 5 * refused <= steps, (refused, steps)


@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_walks_are_a_function_of_the_seed_and_use_both_graphs(kind):
    a, b = lh.gen_walk(7, 0, kind), lh.gen_walk(7, 0, kind)
    assert a == b and a != lh.gen_walk(8, 0, kind)
    assert {lh.gen_walk(7, c, kind)[0] for c in range(2)} == {"G_plan", "G_blocked"}
    for _, st in a[1]:      # every step is one of the recorder's classes, every run says what the model expects of it
        assert st[0] in ("opt", "sched", "sched_bal", "updateval", "rewrite", "row_aux", "stream", "run", "refuse")
        if st[0] == "run":
            assert st[2]["expect"] in ("ok", "refused")


def test_g_plan_is_the_graph_the_issue_describes():
    g = lh.g_plan()
    assert g.V == 2 * 2048 + 37 and 35000 < g.E < 45000 and g.E // g.V < 96 and not g.blocked
    deg = set(g.deg.tolist())
    for chunk in (4, 64):
        assert {chunk - 1, chunk, chunk + 1, 0, 16 * chunk - 1, 16 * chunk, 16 * chunk + 1, 32 * chunk, 17 * 16 * chunk + 3} <= deg
    short = g.deg[g.deg <= 8]
    assert (np.diff(short) < 0).any() and (np.diff(short) > 0).any()          # non-monotone
    assert g.pick_chunk() == 64
    # the neighbor-grouping schedules of the Schedules theme: 32 and 16 run on the plan kernel, 2 is dropped to the item kernels
    assert g.padding_ratio(32) <= 1.5 and g.padding_ratio(16) <= 1.5 and g.padding_ratio(2) > 1.5


def test_the_model_refuses_what_the_header_refuses():
    m = lh.Model("gcn", lh.g_plan())
    assert not m.accepts("run", {"mode": "scheduled", "F": 64})                                  # no schedule yet
    assert not m.accepts("run", {"mode": "rows", "F": 64, "xdt": "bf16"})                         # canonical rows mode is fp32 only
    assert not m.accepts("run", {"mode": "balanced", "F": 64, "acc": True, "ydt": "bf16"})        # ACCUMULATE into a bf16 y
    assert not m.accepts("run", {"mode": "balanced", "F": 64, "acc": True, "reduce": "mean"})     # mean + ACCUMULATE without row_aux
    assert not m.accepts("run", {"mode": "rows", "F": 64, "acc": True})
    m.apply(("sched", "neighbor_grouping", [2]))
    m.apply(("opt", "fast_scheduled", 0))
    assert m.accepts("run", {"mode": "scheduled", "F": 64}) and not m.accepts("run", {"mode": "scheduled", "F": 64, "xdt": "bf16"})
    m.apply(("sched", "neighbor_grouping", [32]))
    assert m.accepts("run", {"mode": "scheduled", "F": 64, "xdt": "bf16"})
    m.apply(("opt", "fast_rows", 1))
    assert m.accepts("run", {"mode": "rows", "F": 64, "xdt": "bf16"})
    m.apply(("row_aux", "deg1"))
    assert m.accepts("run", {"mode": "balanced", "F": 64, "acc": True, "reduce": "mean"})
    assert not m.accepts("run", {"mode": "rows", "F": 64, "reduce": "mean"})
