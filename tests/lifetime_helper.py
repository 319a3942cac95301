"""Helper of tests/test_gpu_handle_lifetime.py and tests/test_handle_lifetime_host.py: the property that a handle with a history computes
what a fresh handle in the same configuration computes.

Three parts.
  * Pure Python, no GPU: the graphs, a MODEL of a handle's configuration (options, schedule, row_aux, stream) that says which calls the header
    refuses, and the seeded step generator of the random walks.
  * `Life`: one long-lived aggregator with a recorder.  Every call goes through `Life.do(step)` (or `Life.run` / `Life.refuse`), which makes it
    with the stream in force as torch's current stream; configuration calls and run calls are recorded in order.  From the record it makes two twins, each a brand-new handle on the same CSR:
        replay twin   every accepted configuration call of the history in order and none of the runs -- it differs from the long-lived handle
                      only by what runs leave behind (lazy plans, sorted descriptors, scratch, counters, rb, gatv2, force_host_plan).  One
                      exception: a run that DEMOTED the handle for good ("scratch_limit_mb", gnnagg.h) is replayed, because the header makes
                      that run's effect part of the configuration;
        minimal twin  only the configuration still in force: the last value of each option that differs from its default, the last schedule /
                      schedule_balanced, the current val / row_aux pointers.
    Calls the library refused are never replayed: a refused call must leave nothing behind, so the twins without it are the reference.
  * The judges: twins bit for bit (`torch.equal` over the whole buffer, guard words included), queries equal, and the long-lived handle's
    output against the oracle restated from the handle's own queries exactly as tests/test_gpu_parity.py / test_gpu_blocked.py restate it.

A step is a tuple whose first element is its class:
    ("opt", name, value)  ("sched", kind, [params])  ("sched_bal", chunk)  ("updateval", key)  ("rewrite", key, seed)  ("row_aux", key | None)
    ("stream", "null" | "side" | "side2")  ("query_rb",)  ("run", op, {params})  ("refuse", what)
"""
import functools

import numpy as np

# ------------------------------------------------------------------------------------------------------------------ graphs (numpy only)
SORT_WINDOW = 2048
GCN_WIDTHS = (602, 130, 64, 32, 7)
GAT_SHAPES = ((1, 128), (8, 16), (4, 3), (2, 301))
GUARD = 8          # guard elements before and after every output (16 bytes of bf16, 32 of fp32: the views keep 16-byte alignment)
CANARY = 7.0

OPTION_DEFAULTS = {"partitions": -1, "tile_width": 64, "slice_kb": 4096, "scratch_limit_mb": 0, "fast_rows": 0, "reference_defaults": 0,
                   "fast_scheduled": 1, "aux_stream": 1, "rows_blocked": 1, "rows_medium_edges": 0, "rows_hub_tile": 0, "rows_hub_edges": 0}
REPLAN_OPTIONS = ("partitions", "tile_width", "slice_kb", "rows_hub_edges")   # gnnagg_set_option: these drop the library-chosen order
# a legal non-default value of every shipped option (the Options theme and the walks)
OPTION_VALUES = {"partitions": (0, 4), "tile_width": (32, 128), "slice_kb": (16, 64), "scratch_limit_mb": (4096,), "fast_rows": (1,),
                 "reference_defaults": (1,), "fast_scheduled": (0,), "aux_stream": (0,), "rows_blocked": (0,), "rows_medium_edges": (-1, 40),
                 "rows_hub_tile": (32, 64), "rows_hub_edges": (150,)}


class Graph:
    def __init__(self, name, ptr, idx, base_opts):
        self.name, self.ptr, self.idx = name, ptr, idx
        self.V, self.E = len(ptr) - 1, len(idx)
        self.deg = np.diff(ptr)
        self.base_opts = base_opts     # options every handle on this graph starts with (part of the recorded history)
        self.blocked = self.E // self.V >= 96   # "partitions" = -1: the library picks the 2-D blocked order from this average degree on

    def pick_chunk(self):
        """api.hip pick_chunk: the chunk of the chunked plan the library builds on its own (restated as tests/test_gpu_bf16.py does)"""
        chunk = 64
        while chunk < 512 and chunk < 2 * (self.E // self.V):
            chunk *= 2
        return chunk

    def padding_ratio(self, ng):
        """api.hip build_plan_into: lane groups a neighbor-grouping schedule occupies on the plan kernel over the chunks it has; above 1.5
        do_schedule drops plan_sched and the item kernels run the schedule"""
        deg = self.deg.astype(np.int64)
        seg = 16 * ng
        n0 = int((deg <= ng).sum())
        padded, chunks = 0, n0
        for d in deg[deg > ng]:
            parts = [d] if d <= seg else [min(seg, d - j * seg) for j in range(-(-d // seg))]
            for p in parts:
                nch = -(-p // ng)
                padded += 8 * (-(-nch // 8))
                chunks += nch
        return (padded + n0) / chunks if chunks else 1.0


@functools.lru_cache(maxsize=None)
def g_plan():
    """V = 2 * 2048 + 37 rows from an explicit degree list: the boundary degrees of test_plan_boundaries_exact_multiples for chunk 4 and 64
    scattered between rows of 0 .. 8 edges in non-monotone order.  More than one 2048-row sort window with a ragged last one, segments, hubs and
    big rows at both chunks; about 40 k edges, average degree 9: the chunked plan."""
    V = 2 * SORT_WINDOW + 37
    deg = np.array([(r * 7 + 3) % 9 for r in range(V)], np.int64)
    special = []
    for chunk in (4, 64):
        special += [chunk - 1, chunk, chunk + 1, 0, 16 * chunk - 1, 16 * chunk, 16 * chunk + 1, 32 * chunk, 17 * 16 * chunk + 3]
    for k, d in enumerate(special):     # spread over both sort windows and the ragged tail, never next to each other
        deg[(k * 229 + 11) % V] = d
    assert len({(k * 229 + 11) % V for k in range(len(special))}) == len(special)
    ptr = np.zeros(V + 1, np.int32)
    ptr[1:] = np.cumsum(deg)
    E = int(ptr[-1])
    idx = np.random.default_rng(20260).integers(0, V, E).astype(np.int32)
    return Graph("G_plan", ptr, idx, ())


@functools.lru_cache(maxsize=None)
def g_blocked():
    """the hub_graph(700, 220000) shape of tests/test_gpu_blocked.py (every row's neighbors ascending: the rows-mode chain applies), with
    slice_kb = 16 so that several source ranges exist"""
    import gnn_computing_amd as gnc
    ptr_t, idx_t = gnc.graph.powerlaw_csr(700, 220000, seed=6, alpha=0.9)
    ptr, idx = ptr_t.numpy().astype(np.int32), idx_t.numpy().astype(np.int32)
    assert all(np.all(np.diff(idx[ptr[r]:ptr[r + 1]]) >= 0) for r in range(len(ptr) - 1))
    return Graph("G_blocked", ptr, idx, (("opt", "slice_kb", 16),))


GRAPHS = {"G_plan": g_plan, "G_blocked": g_blocked}


# ------------------------------------------------------------------------------------------------------------------ the model (no GPU)
class Model:
    """What the header lets one predict about a handle from its configuration calls alone."""

    def __init__(self, kind, graph, val_key="v1"):
        self.kind, self.g = kind, graph
        self.opts = dict(OPTION_DEFAULTS)
        self.sched = None            # (kind, params) of the last accepted schedule(), None after nop
        self.sched_bal = None        # chunk of the last schedule_balanced() still in force
        self.val_key, self.row_aux = val_key, None
        self.demoted = False         # a run moved the handle to the chunked plan for good (scratch_limit_mb)

    def apply(self, step):
        c = step[0]
        if c == "opt":
            name, value = step[1], step[2]
            if name == "reference_defaults":
                self.opts["fast_rows"] = int(value != 0)
            self.opts[name] = value
            if name in REPLAN_OPTIONS:
                self.sched_bal = None
            if name == "partitions":
                self.demoted = False
        elif c == "sched":
            self.sched = None if step[1] == "nop" else (step[1], list(step[2]))
        elif c == "sched_bal":
            self.sched_bal = step[1]
        elif c == "updateval":
            self.val_key = step[1]
        elif c == "row_aux":
            self.row_aux = step[1]

    # -- which order a mode runs
    def effective_mode(self, mode, newval=False):
        if mode == "rows" and self.opts["fast_rows"]:
            return "balanced"
        if mode == "scheduled" and self.opts["fast_scheduled"] and self.sched is not None and not newval:
            return "balanced"
        return mode

    def plan_sched_valid(self):
        return self.sched is not None and self.sched[0] == "neighbor_grouping" and self.g.padding_ratio(self.sched[1][0]) <= 1.5

    def on_plan_kernel(self, mode, newval=False):
        """where gnnagg_gcn_run_typed / gnnagg_gat_run_typed / the shifted run are accepted"""
        m = self.effective_mode(mode, newval)
        return m == "balanced" or (m == "scheduled" and self.plan_sched_valid())

    def accepts(self, op, p):
        """True when the header says the library runs this call on a handle in this configuration"""
        mode = p.get("mode", "balanced")
        if mode == "scheduled" and self.sched is None:
            return False
        if self.kind == "gcn":
            typed = p.get("xdt", "f32") != "f32" or p.get("ydt", "f32") != "f32"
            reduce, acc = p.get("reduce", "sum"), p.get("acc", False)
            aux_run = self.row_aux is not None and reduce != "sum"
            if op == "run":
                if acc and (mode != "balanced" or (reduce != "sum" and self.row_aux is None) or p.get("ydt", "f32") != "f32"):
                    return False
                if aux_run and mode != "balanced":
                    return False
                return self.on_plan_kernel(mode) if typed else True
            if op == "nn":
                return not aux_run
            if op == "nn_typed":
                if aux_run:
                    return False
                return self.on_plan_kernel(mode) if (typed or p.get("relu", False)) else True
            if op == "probe":    # balanced mode, or a neighbor-grouping schedule on the plan kernel
                return self.on_plan_kernel(mode)
            raise ValueError(op)
        if op == "run":
            typed = p.get("xdt", "f32") != "f32" or p.get("ydt", "f32") != "f32" or p.get("stable", False) or p.get("shift", False)
            newval = p.get("newval", False)
            if newval and typed and (p.get("stable", False) or p.get("shift", False)):
                return False
            if newval and self.effective_mode(mode, True) == "scheduled" and self.sched[0] != "neighbor_grouping":
                return False
            return self.on_plan_kernel(mode, newval) if typed else True
        if op == "part":     # gnnagg_gat_run_part: 16-byte lanes inside one head, rows of at most 256 columns
            return p["H"] * p["D"] <= 256 and p["D"] % 4 == 0
        if op == "probe":    # only the 2-D blocked balanced order has a probe instantiation
            return (self.effective_mode(mode) == "balanced" and self.g.blocked and self.opts["partitions"] != 0 and not self.demoted and
                    not self.sched_bal)
        return True


# ------------------------------------------------------------------------------------------------------------------ the walk generator
GCN_KINDS = ("width", "dtype", "flags", "reduce", "schedule", "schedule_balanced", "option", "updateval", "rewrite", "row_aux", "stream",
             "nn", "refusal")
GAT_KINDS = ("shape", "dtype", "softmax", "schedule", "schedule_balanced", "option", "stream", "v2", "newval", "edge_ops", "part", "refusal")
MODES = ("rows", "scheduled", "balanced")
# options a walk toggles (scratch_limit_mb's demotion and slice_kb on G_blocked have scripted tests of their own)
WALK_OPTIONS = ("partitions", "tile_width", "fast_rows", "fast_scheduled", "aux_stream", "rows_blocked", "rows_medium_edges", "rows_hub_tile",
                "rows_hub_edges")
SCHEDULES = (("neighbor_grouping", [32]), ("neighbor_grouping", [2]), ("neighbor_grouping", [16]), ("locality", [3]),
             ("locality_neighbor_grouping", [3, 4]), ("nop", [0]))


def gen_walk(seed, case, kind):
    """One walk: (graph name, [(transition kind or None, step), ...]).  Pure Python.  A transition is followed by runs in the modes the model
    allows; at most one step in five is a documented refusal, and there are at least as many accepted runs as configuration steps."""
    rng = np.random.default_rng([seed, case, 0 if kind == "gcn" else 1])
    gname = "G_plan" if case % 2 == 0 else "G_blocked"
    g = GRAPHS[gname]()
    m = Model(kind, g)
    for st in g.base_opts:
        m.apply(st)
    kinds = GCN_KINDS if kind == "gcn" else GAT_KINDS
    widths = GCN_WIDTHS if gname == "G_plan" else (130, 64, 32, 7)     # (602 on G_blocked: the scripted width walk)
    shapes = GAT_SHAPES if gname == "G_plan" else ((1, 128), (8, 16), (4, 3))
    cur = {"F": 64, "xdt": "f32", "ydt": "f32", "reduce": "sum", "acc": False, "relu": False} if kind == "gcn" else \
          {"H": 1, "D": 128, "xdt": "f32", "ydt": "f32", "stable": False, "shift": False, "newval": False}
    steps = []
    counts = {"run": 0, "config": 1, "refuse": 0}
    m.apply(("sched", "neighbor_grouping", [32]))     # every walk starts with a schedule in place, so that all three modes are open
    steps.append(("schedule", ("sched", "neighbor_grouping", [32])))

    def emit(tkind, step):
        steps.append((tkind, step))

    def run_step(mode, tkind=None, op="run", extra=None):
        p = dict(cur, mode=mode)
        if op != "run":
            p = dict(F=cur["F"], mode=mode, xdt=cur["xdt"], ydt=cur["ydt"]) if kind == "gcn" else dict(H=cur["H"], D=cur["D"])
        if extra:
            p.update(extra)
        ok = m.accepts(op, p)
        if not ok:
            if (counts["refuse"] + 1) * 5 > len(steps) + 1:     # the share of refusals stays at or below one step in five
                return False
            counts["refuse"] += 1
        else:
            counts["run"] += 1
        emit(tkind, ("run", op, dict(p, expect="ok" if ok else "refused")))
        return ok

    for t in [str(k) for k in rng.permutation(kinds)]:      # every walk makes every transition once, in a random order
        before = len(steps)
        if t == "width":
            cur["F"] = int(rng.choice(widths))
        elif t == "shape":
            cur["H"], cur["D"] = [int(v) for v in shapes[int(rng.integers(len(shapes)))]]
        elif t == "dtype":
            cur["xdt"], cur["ydt"] = [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", "bf16")][int(rng.integers(4))]
        elif t == "flags":
            cur["acc"], cur["relu"] = bool(rng.integers(2)), bool(rng.integers(2))
        elif t == "reduce":
            cur["reduce"] = str(rng.choice(["sum", "mean", "max"]))
        elif t == "softmax":
            cur["stable"], cur["shift"] = [(False, False), (True, False), (False, True)][int(rng.integers(3))]
            if cur["stable"] or cur["shift"]:
                cur["newval"] = False
        elif t == "newval":
            cur["newval"] = not cur["newval"]
            if cur["newval"]:
                cur["stable"] = cur["shift"] = False
        elif t == "schedule":
            sk, sp = SCHEDULES[int(rng.integers(len(SCHEDULES) - (0 if rng.random() < 0.3 else 1)))]    # (nop: rarely)
            st = ("sched", sk, list(sp))
            m.apply(st); counts["config"] += 1; emit(t, st)
        elif t == "schedule_balanced":
            st = ("sched_bal", int(rng.choice([4, 64, 0])))
            m.apply(st); counts["config"] += 1; emit(t, st)
        elif t == "option":
            name = str(rng.choice(WALK_OPTIONS))
            cand = [v for v in OPTION_VALUES[name] + (OPTION_DEFAULTS[name],) if v != m.opts[name]]
            st = ("opt", name, int(cand[int(rng.integers(len(cand)))]))
            m.apply(st); counts["config"] += 1; emit(t, st)
        elif t == "updateval":
            st = ("updateval", str(rng.choice([k for k in ("v1", "v2", "v3") if k != m.val_key])))
            m.apply(st); counts["config"] += 1; emit(t, st)
        elif t == "rewrite":
            emit(t, ("rewrite", m.val_key, int(rng.integers(1 << 20)))); counts["config"] += 1
        elif t == "row_aux":
            st = ("row_aux", None if m.row_aux is not None else "deg1")
            m.apply(st); counts["config"] += 1; emit(t, st)
        elif t == "stream":
            emit(t, ("stream", str(rng.choice(["null", "side", "side2"])))); counts["config"] += 1
        elif t == "refusal":
            what = str(rng.choice(REFUSALS_GCN if kind == "gcn" else REFUSALS_GAT))
            if (counts["refuse"] + 1) * 5 <= len(steps) + 1:
                counts["refuse"] += 1
                if what == "scheduled_after_nop":       # (Life.refuse makes schedule(nop) first)
                    m.apply(("sched", "nop", [0]))
                emit(t, ("refuse", what))
            else:
                t = None
        first = t if len(steps) == before else None    # parameter transitions ride on the first run that follows them
        if t == "nn":
            if run_step("balanced" if cur["xdt"] != "f32" or cur["ydt"] != "f32" else str(rng.choice(MODES)), first,
                        "nn" if (cur["xdt"], cur["ydt"]) == ("f32", "f32") and rng.random() < 0.5 else "nn_typed",
                        {"OUT": 32, "F": 128 if cur["F"] > 130 else cur["F"]}) is not False:
                first = None
        elif t in ("v2", "edge_ops", "part"):
            extra = {"xdt": cur["xdt"], "ydt": cur["ydt"]} if t == "v2" else {}
            if t == "part" and rng.random() < 0.7 and not m.accepts("part", cur):      # (sometimes left as it is: a documented refusal)
                extra = {"H": 1, "D": 128}
            if run_step("balanced", first, t, extra) is not False:
                first = None
        # the runs after the transition: every mode the call allows (and, rarely, one it does not: a documented refusal)
        for md in [str(v) for v in rng.permutation(MODES)]:
            if run_step(md, first) is not False:
                first = None
        while counts["run"] < counts["config"]:      # never more configuration than accepted runs
            run_step("balanced", None, "run", {"xdt": "f32", "ydt": "f32", "acc": False, "reduce": "sum"} if kind == "gcn"
                     else {"xdt": "f32", "ydt": "f32", "stable": False, "shift": False, "newval": False})
    return gname, steps


REFUSALS_GCN = ("acc_bf16_y", "typed_canonical_rows", "scheduled_after_nop", "unknown_option", "illegal_option_value", "schedule_ng0",
                "schedule_balanced_neg")
REFUSALS_GAT = ("scheduled_after_nop", "unknown_option", "illegal_option_value", "schedule_ng0", "schedule_balanced_neg", "v2_feat_1025",
                "v2_heads_not_dividing")
FUZZ_SEED_DEFAULT, FUZZ_CASES_DEFAULT = 196, 2


def walk_summary(kind, seed=FUZZ_SEED_DEFAULT, cases=FUZZ_CASES_DEFAULT):
    """what tests/test_handle_lifetime_host.py asserts about the generator: (kinds seen, {kind: modes of the accepted runs that follow it before
    the next transition}, per walk (accepted runs, configuration steps, refusals, steps))"""
    seen, followed, per_walk = set(), {}, []
    for case in range(cases):
        _, steps = gen_walk(seed, case, kind)
        cur, runs, config, refused = None, 0, 0, 0
        for tkind, st in steps:
            if tkind is not None:
                cur = tkind
                seen.add(tkind)
            if st[0] == "run":
                if st[2]["expect"] == "ok":
                    runs += 1
                    if cur is not None and st[1] == "run":
                        followed.setdefault(cur, set()).add(st[2]["mode"])
                else:
                    refused += 1
            elif st[0] == "refuse":
                refused += 1
            else:
                config += 1
        per_walk.append((runs, config, refused, len(steps)))
    return seen, followed, per_walk


# ------------------------------------------------------------------------------------------------------------------ the GPU side
DEV = "cuda:0"


def _torch():
    import torch
    return torch


def bf16_values(shape, seed, scale=1.0):
    """fp32 numpy array whose every value is a bf16 value: one array serves the fp32 and the bf16 run of a width (bf16 -> fp32 is exact)"""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).float().numpy()


class Pool:
    """The caller's arrays of one graph: CSR, edge values (v1 .. v3, rewritten in place by ("rewrite", key, seed)), row_aux, features per
    width.  The long-lived handle and its twins borrow the SAME device arrays, as the header's aliasing contract has it."""

    def __init__(self, g):
        torch = _torch()
        self.g = g
        self.dptr, self.didx = torch.from_numpy(g.ptr).to(DEV), torch.from_numpy(g.idx).to(DEV)
        self.val_h = {k: np.random.default_rng(100 + i).standard_normal(g.E, dtype=np.float32) for i, k in enumerate(("v1", "v2", "v3"))}
        self.val_d = {k: torch.from_numpy(v).to(DEV) for k, v in self.val_h.items()}
        self.val_version = {k: 0 for k in self.val_h}
        self.aux_h = {"deg1": (g.deg + 1).astype(np.int32)}      # a divisor that is NOT the handle's own degree: a run that ignores it shows
        self.aux_d = {k: torch.from_numpy(v).to(DEV) for k, v in self.aux_h.items()}
        self._x, self._att, self._w, self._memo = {}, {}, {}, {}

    def rewrite(self, key, seed):
        torch = _torch()
        self.val_h[key] = np.random.default_rng(seed).standard_normal(self.g.E, dtype=np.float32)
        self.val_d[key].copy_(torch.from_numpy(self.val_h[key]).to(DEV))     # in place: the handles keep reading the same pointer
        self.val_version[key] += 1

    def x(self, F, dt="f32"):
        torch = _torch()
        if F not in self._x:
            h = bf16_values((self.g.V, F), 7000 + F)
            d = torch.from_numpy(h).to(DEV)
            self._x[F] = (h, d, d.to(torch.bfloat16))
        return self._x[F][0] if dt == "host" else self._x[F][1] if dt == "f32" else self._x[F][2]

    def att(self, H, what="dev"):
        torch = _torch()
        if H not in self._att:
            h = np.random.default_rng(8000 + H).standard_normal((self.g.V, H, 2), dtype=np.float32) * np.float32(0.4)
            self._att[H] = (h, torch.from_numpy(h).to(DEV))
        return self._att[H][0 if what == "host" else 1]

    def w(self, F, OUT, dt="f32"):
        torch = _torch()
        if (F, OUT) not in self._w:
            h = bf16_values((F, OUT), 9000 + F + OUT, 0.3)
            d = torch.from_numpy(h).to(DEV)
            self._w[(F, OUT)] = (h, d, d.to(torch.bfloat16))
        return self._w[(F, OUT)][0 if dt == "host" else 1 if dt == "f32" else 2]

    def memo(self, key, fn):
        """oracle results are computed once and shared (never modified: the judges copy before they apply flags)"""
        if key not in self._memo:
            if len(self._memo) > 48:      # (rewritten edge values make new keys: the old ones are never asked for again)
                self._memo.clear()
            self._memo[key] = fn()
        return self._memo[key]


_POOLS = {}


def pool(gname):
    if gname not in _POOLS:
        _POOLS[gname] = Pool(GRAPHS[gname]())
    return _POOLS[gname]


def canary(V, F, dtype):
    """(whole buffer, [V, F] view): 7.0 everywhere, GUARD elements before and after the view"""
    torch = _torch()
    buf = torch.full((V * F + 2 * GUARD,), CANARY, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + V * F].view(V, F)


def guards_intact(buf):
    return bool((buf[:GUARD] == CANARY).all().item()) and bool((buf[-GUARD:] == CANARY).all().item())


def untouched(buf):
    return bool((buf == CANARY).all().item())


class Life:
    """One long-lived aggregator with its recorder (module docstring)."""

    def __init__(self, kind, gname, val_key="v1", minimal=True):
        import gnn_computing_amd as gnc
        torch = _torch()
        self.gnc, self.kind, self.gname = gnc, kind, gname
        self.P = pool(gname)
        self.g = self.P.g
        self.val0 = val_key
        self.m = Model(kind, self.g, val_key)
        self.history = []          # every step, in order, with what became of it
        self.config = []           # the accepted configuration calls (and demoting runs): what the replay twin replays
        self.check_minimal = minimal
        self.base_stream = torch.cuda.current_stream()
        self.streams = {"null": self.base_stream}
        self.stream = self.base_stream
        self.nn_path = 0
        self.launched_on = []      # the stream of every run step (test_streams asserts that it is the one just switched to)
        self.h = self._fresh(val_key)
        for st in self.g.base_opts:
            self.do(st)

    # -- handles
    def _fresh(self, val_key):
        gnc, P = self.gnc, self.P
        if self.kind == "gcn":
            return gnc.Aggregator_GCN(P.dptr, P.didx, P.val_d[val_key], 32, 32)
        return gnc.Aggregator_GAT(P.dptr, P.didx, 32, 32)

    def _apply_config(self, h, st):
        gnc, P = self.gnc, self.P
        c = st[0]
        if c == "opt":
            h.set_option(st[1], st[2])
        elif c == "sched":
            h.schedule(gnc.Schedule[st[1]], list(st[2]))
        elif c == "sched_bal":
            h.schedule_balanced(st[1])
        elif c == "updateval":
            h.updateval(P.val_d[st[1]])
        elif c == "row_aux":
            h.set_row_aux(None if st[1] is None else P.aux_d[st[1]])
        elif c == "run":                               # (a demoting run, replayed into an output nobody reads)
            self._launch(h, st[1], st[2], self._outputs(st[1], st[2]))
        else:
            raise ValueError(st)

    def replay_twin(self):
        h = self._fresh(self.val0)
        for st in self.config:
            self._apply_config(h, st)
        return h

    def minimal_twin(self):
        m = self.m
        h = self._fresh(m.val_key)
        for name, value in m.opts.items():
            if name != "reference_defaults" and value != OPTION_DEFAULTS[name]:
                h.set_option(name, value)
        if m.sched is not None:
            self._apply_config(h, ("sched", m.sched[0], m.sched[1]))
        if m.sched_bal is not None:
            h.schedule_balanced(m.sched_bal)
        if m.row_aux is not None:
            h.set_row_aux(self.P.aux_d[m.row_aux])
        return h

    def story(self):
        return "history of the long-lived handle on %s:\n  " % self.gname + "\n  ".join(repr(s) for s in self.history)

    # -- queries
    def queries(self, h):
        """everything the issue lists except last_nn_path (judged by the nn steps): values, or the error class where the query refuses"""
        gnc = self.gnc

        def q(fn):
            try:
                return fn()
            except gnc.GnnAggError as e:
                return ("error", e.code)
        out = {"balanced_params": q(h.balanced_params), "balanced_partitions": q(h.balanced_partitions),
               "balanced_partition_columns": q(h.balanced_partition_columns), "num_target": q(lambda: h.num_target)}
        for mode in MODES:
            out["mode_params " + mode] = q(lambda: h.mode_params(mode))
        for mode in MODES:                 # (the rows mode has no schedule: the error class is the answer that must agree)
            out["get_schedule " + mode] = q(lambda: h.get_schedule(mode))
        return out

    @staticmethod
    def same_queries(a, b):
        diff = []
        for k in a:
            va, vb = a[k], b[k]
            if isinstance(va, tuple) and len(va) == 3 and isinstance(va[0], np.ndarray):
                eq = isinstance(vb, tuple) and len(vb) == 3 and isinstance(vb[0], np.ndarray) and all(np.array_equal(x, y) for x, y in zip(va, vb))
            else:
                eq = va == vb
            if not eq:
                diff.append(k)
        return diff

    # -- streams
    def _switch_stream(self, name):
        torch = _torch()
        if name not in self.streams:
            self.streams[name] = torch.cuda.Stream()
        new = self.streams[name]
        new.wait_stream(self.stream)          # as test_stream_is_honoured: the new stream is ordered behind the work enqueued so far
        self.stream = new

    # -- one step
    def do(self, st):
        with self._on_stream():
            return self._do(st)

    def _on_stream(self):
        """every call of a step -- on the handle and on its twins -- is made with the stream in force current (Aggregator._use_current_stream
        reads torch's current stream at each call)"""
        return _torch().cuda.stream(self.stream)

    def _do(self, st):
        c = st[0]
        if c in ("opt", "sched", "sched_bal", "updateval", "row_aux"):
            self._apply_config(self.h, st)
            self.m.apply(st)
            self.config.append(st)
            self.history.append(st)
        elif c == "rewrite":
            self.P.rewrite(st[1], st[2])
            self.history.append(st)
        elif c == "stream":
            self._switch_stream(st[1])
            self.history.append(st)
        elif c == "query_rb":
            self.history.append(st + (self.h.rows_blocked_ranges(),))
        elif c == "run":
            return self._run(st[1], dict(st[2]))
        elif c == "refuse":
            return self._refuse(st[1])
        else:
            raise ValueError(st)

    def run(self, op, p):
        with self._on_stream():
            return self._run(op, p)

    def refuse(self, what):
        with self._on_stream():
            return self._refuse(what)

    def twin_run(self, op, p):
        """the outputs of one more run on a new replay twin: what a judge needs beside the step itself (the fp32 result a bf16 output is one
        rounding of) is not run on the long-lived handle, whose history stays the step list"""
        with self._on_stream():
            tw = self.replay_twin()
            outs = self._outputs(op, p)
            self._launch(tw, op, p, outs)
            _torch().cuda.synchronize()
            tw.close()
        return outs

    # -- runs
    def _dt(self, name):
        torch = _torch()
        return torch.float32 if name == "f32" else torch.bfloat16

    def _outputs(self, op, p):
        torch = _torch()
        V, E = self.g.V, self.g.E
        if self.kind == "gcn":
            F = p["F"]
            outs = {"y": canary(V, F, self._dt(p.get("ydt", "f32")))}
            if op in ("nn", "nn_typed"):
                outs["t"] = canary(V, p["OUT"], self._dt(p.get("tdt", "f32")))
            return outs
        H, D = p["H"], p["D"]
        if op == "edge_ops":
            return {"att_w": canary(E, H, torch.float32), "uv": canary(E, 1, torch.float32), "center": canary(V, 1, torch.float32),
                    "div": canary(E, 1, torch.float32)}
        if op == "row_shift":
            return {"shift": canary(V, H, torch.float32)}
        outs = {"y": canary(V, H * D, self._dt(p.get("ydt", "f32")))}
        if op == "part":
            outs["den"] = canary(V, H, torch.float32)
        if p.get("newval"):
            outs["newval"] = canary(E, H, torch.float32)
        return outs

    def _launch(self, h, op, p, outs):
        """the call itself, on handle h, into outs"""
        torch = _torch()
        P = self.P
        mode = p.get("mode", "balanced")
        if self.kind == "gcn":
            F = p["F"]
            x = P.x(F, p.get("xdt", "f32"))
            y = outs["y"][1]
            if op == "run":
                h.run(x, y, 128, mode, reduce=p.get("reduce", "sum"), accumulate=p.get("acc", False), relu=p.get("relu", False))
            elif op == "nn":
                h.run_with_nn(x, y, P.w(F, p["OUT"]), outs["t"][1], 128, mode)
            elif op == "nn_typed":
                h.run_with_nn_typed(x, y, P.w(F, p["OUT"], p.get("ydt", "f32")), outs["t"][1], mode, p.get("reduce", "sum"), p.get("relu", False))
            elif op == "probe":
                h.probe_gather(x, mode)
            else:
                raise ValueError(op)
            return
        H, D = p["H"], p["D"]
        F = H * D
        att = P.att(H)
        if op == "run":
            shift = None
            if p.get("shift"):      # the caller's shift array: the row maxima, computed by the same handle (row_shift is exact: test_gpu_gat_shift.py)
                shift = self._shift_ref(H)
            h.run(P.x(F, p.get("xdt", "f32")), att, outs["y"][1], 128, mode, heads=H, newval=outs["newval"][1] if p.get("newval") else None,
                  stable=p.get("stable", False), shift=shift)
        elif op == "row_shift":
            h.row_shift(att, H, 0.2, out=outs["shift"][1])
        elif op == "v2":
            h.run_v2(P.x(F, p.get("xdt", "f32")), P.x(F, p.get("xdt", "f32")), self._a(H, D), outs["y"][1], heads=H)
        elif op == "part":
            h.run_part(P.x(F), att, outs["y"][1], outs["den"][1], 1, heads=H)
            h.run_part(P.x(F), att, outs["y"][1], outs["den"][1], 2, heads=H)
        elif op == "edge_ops":
            a1 = P.att(1)
            h.run_att(att, outs["att_w"][1], 128, heads=H)
            h.run_u_add_v(a1, outs["uv"][1].view(-1))
            w = torch.exp(torch.nn.functional.leaky_relu(outs["uv"][1].view(-1), 0.2))
            h.run_add_to_center(w, outs["center"][1].view(-1))
            outs["div"][1].view(-1).copy_(w)
            h.run_div_each(outs["center"][1].view(-1), outs["div"][1].view(-1))
        elif op == "probe":
            h.probe_gather(P.x(F), att, mode, heads=H)
        else:
            raise ValueError(op)

    def _a(self, H, D):
        torch = _torch()
        return self.P.memo(("a", H, D), lambda: torch.from_numpy(np.random.default_rng(H * 1000 + D).standard_normal((H, D), dtype=np.float32)).to(DEV))

    def _shift_ref(self, H):
        from test_gat_shift_host import row_shift_ref
        torch = _torch()
        g = self.g
        return self.P.memo(("shift", H), lambda: torch.from_numpy(row_shift_ref(g.ptr, g.idx, self.P.att(H, "host"), H, 0.2)).to(DEV))

    def _run(self, op, p):
        """One run step: the call on the long-lived handle, the same call on fresh outputs on the twins, then judgements 1 - 4 of the issue.
        The twins are configured BEFORE the handle runs (their plan construction waits for the stream), then the handle and the twins are
        launched back to back on the stream in force and the device is synchronised once, before anything is compared: between two steps
        only wait_stream orders one stream behind the other."""
        torch = _torch()
        gnc = self.gnc
        expect = p.pop("expect", None)
        accepted = self.m.accepts(op, p)
        if expect is not None:
            assert (expect == "ok") == accepted, "the generator and the model disagree on %r\n%s" % ((op, p), self.story())
        assert torch.cuda.current_stream() == self.stream, "the step is not launched on the stream in force\n" + self.story()
        self.launched_on.append(self.stream.cuda_stream)
        step = ("run", op, dict(p))
        outs = self._outputs(op, p)
        limited = self.m.opts["scratch_limit_mb"] > 0        # this run may demote the handle for good: what the replay twin replays is known after it
        parts_before = self.h.balanced_partitions() if limited else None
        before = None if accepted else (self.queries(self.h), self.h.last_nn_path() if self.kind == "gcn" else 0)
        twins = []
        if accepted and not limited:
            twins.append(("replay twin", self.replay_twin()))
            if self.check_minimal:
                twins.append(("minimal twin", self.minimal_twin()))
        try:
            self._launch(self.h, op, p, outs)
            raised = None
        except (gnc.GnnAggError, TypeError, ValueError) as e:
            raised = e
        self.history.append(step + (("refused: %s" % raised) if raised else "ok",))
        what = "step %d %r\n%s" % (len(self.history), step, self.story())
        if not accepted:     # a combination the library refuses is asserted to be refused, with nothing written and nothing changed
            torch.cuda.synchronize()
            assert raised is not None, "the header refuses this call, the library ran it: " + what
            assert all(untouched(b) for b, _ in outs.values()), "a refused call wrote to its output: " + what
            diff = self.same_queries(before[0], self.queries(self.h))
            assert not diff, "a refused run changed what the handle reports: %s\n%s" % (diff, what)
            if self.kind == "gcn":
                assert self.h.last_nn_path() == before[1], "a refused run changed last_nn_path: " + what
            return None
        assert raised is None, "refused: %s\n%s" % (raised, what)
        if limited:
            if parts_before > 0 and self.h.balanced_partitions() == 0:
                self.m.demoted = True            # moved to the chunked plan for good: the header makes this run part of the configuration
                self.config.append(("run", op, dict(p)))
                replay = self._fresh(self.val0)
                for st in self.config[:-1]:
                    self._apply_config(replay, st)
            else:
                replay = self.replay_twin()
            twins.append(("replay twin", replay))
            if self.check_minimal:
                twins.append(("minimal twin", self.minimal_twin()))
        all_touts = []
        for name, tw in twins:
            touts = self._outputs(op, p)
            self._launch(tw, op, p, touts)
            all_touts.append(touts)
        torch.cuda.synchronize()             # once, before anything is compared
        hq = self.queries(self.h)
        for (name, tw), touts in zip(twins, all_touts):
            tq = self.queries(tw)
            if name == "minimal twin" and self.m.demoted:
                # the documented sticky history: once the limit is lifted the minimal twin is on the blocked order, the handle on the chunked
                # plan.  (While the limit is in force the minimal twin demotes itself as soon as it runs the balanced mode: nothing to assert.)
                if self.m.opts["scratch_limit_mb"] == 0:
                    assert "balanced_partitions" in self.same_queries(hq, tq), "a demotion for good that the minimal twin shares: " + what
                tw.close()
                continue
            diff = self.same_queries(hq, tq)
            assert not diff, "queries differ from the %s: %s\n%s" % (name, diff, what)
            if op != "probe":
                for k in outs:
                    assert torch.equal(outs[k][0], touts[k][0]), "%s: output %r differs from the %s\n%s" % (op, k, name, what)
            if op in ("nn", "nn_typed"):
                assert self.h.last_nn_path() == tw.last_nn_path(), "last_nn_path differs from the %s: %s" % (name, what)
            elif self.kind == "gcn":
                assert tw.last_nn_path() == 0, what
            tw.close()
        if self.kind == "gcn":
            if op in ("nn", "nn_typed"):
                self.nn_path = self.h.last_nn_path()
            assert self.h.last_nn_path() == self.nn_path, "last_nn_path changed without a run_with_nn call: " + what
        for b, _ in outs.values():
            assert guards_intact(b), "guard words overwritten: " + what
        if op == "probe":
            assert all(untouched(b) for b, _ in outs.values()), "the probe wrote: " + what
            return outs
        (judge_gcn if self.kind == "gcn" else judge_gat)(self, op, p, outs, what)
        return outs

    # -- refused calls in mid-life
    def _refuse(self, what):
        """a call the header says is refused: it must raise, leave y at its canary and the handle's queries as they were"""
        torch = _torch()
        gnc, P, g = self.gnc, self.P, self.g
        if what in ("scheduled_after_nop", "nn_scheduled_after_nop"):
            self._do(("sched", "nop", [0]))        # (an accepted configuration call of its own)
        before = self.queries(self.h)
        nn_before = self.h.last_nn_path() if self.kind == "gcn" else 0
        bufs = []
        F = 64

        def y(dt=None, f=F):
            b = canary(g.V, f, dt or torch.float32)
            bufs.append(b[0])
            return b[1]
        h = self.h
        calls = {
            "acc_bf16_y": lambda: h.run(P.x(F), y(torch.bfloat16), 128, "balanced", accumulate=True),
            "typed_canonical_rows": lambda: h.run(P.x(F, "bf16"), y(), 128, "rows"),
            "scheduled_after_nop": lambda: (h.run(P.x(F), y(), 128, "scheduled") if self.kind == "gcn"
                                            else h.run(P.x(128), P.att(1), y(f=128), 128, "scheduled")),
            "nn_scheduled_after_nop": lambda: h.run_with_nn(P.x(F), y(), P.w(F, 32), y(f=32), 128, "scheduled"),
            "unknown_option": lambda: h.set_option("no_such_option", 1),
            "illegal_option_value": lambda: h.set_option("tile_width", 48),
            "schedule_ng0": lambda: h.schedule(gnc.Schedule.neighbor_grouping, [0]),
            "schedule_locality0": lambda: h.schedule(gnc.Schedule.locality, [0]),
            "schedule_balanced_neg": lambda: h.schedule_balanced(-1),
            "v2_feat_1025": lambda: h.run_v2(torch.zeros((g.V, 1025), device=DEV), torch.zeros((g.V, 1025), device=DEV),
                                             torch.zeros(1025, device=DEV), y(f=1025), heads=1),
            "v2_heads_not_dividing": lambda: h.run_v2(P.x(128), P.x(128), torch.zeros(128, device=DEV), y(f=128), heads=3),
        }
        if what == "typed_canonical_rows" and self.m.opts["fast_rows"]:
            what = "acc_bf16_y"          # (with fast_rows = 1 the rows mode is the balanced order and takes bf16: not a refusal then)
        try:
            calls[what]()
            raised = None
        except (gnc.GnnAggError, ValueError) as e:
            raised = e
        torch.cuda.synchronize()
        self.history.append(("refuse", what, str(raised)))
        msg = "step %d %r\n%s" % (len(self.history), ("refuse", what), self.story())
        assert raised is not None, "the header refuses this call, the library accepted it: " + msg
        assert all(untouched(b) for b in bufs), "a refused call wrote to its output: " + msg
        diff = self.same_queries(before, self.queries(self.h))
        assert not diff, "a refused call changed what the handle reports: %s\n%s" % (diff, msg)
        if self.kind == "gcn":
            assert self.h.last_nn_path() == nn_before, "a refused call changed last_nn_path: " + msg


# ------------------------------------------------------------------------------------------------------------------ the judges
def _gcn_order(life, op, p):
    """the order this call ran in, from the handle's own queries"""
    h, g, m = life.h, life.g, life.m
    mode = m.effective_mode(p.get("mode", "balanced"))
    reduce = p.get("reduce", "sum")
    if reduce == "max":
        return ("max",)
    if mode == "rows":
        return ("seq",) if reduce == "sum" else ("mean_rows",)
    if mode == "scheduled":
        kind, params = m.sched
        if kind == "neighbor_grouping":
            return ("ng", params[0], h.mode_params("scheduled")[1])
        return ("loc", params[0], g.V, params[1] if kind == "locality_neighbor_grouping" else 0)
    parts = h.balanced_partitions()
    typed = p.get("xdt", "f32") != "f32" or p.get("ydt", "f32") != "f32" or (op == "nn_typed" and p.get("relu", False))
    aux_run = m.row_aux is not None and reduce != "sum"
    if parts > 0 and (p.get("acc", False) or aux_run or typed):
        return ("ng", g.pick_chunk(), 16)     # the chunked plan built beside the blocked order (restated as tests/test_gpu_bf16.py does)
    chunk, seg = h.balanced_params()
    if parts > 0:
        assert seg == 0
        return ("loc", parts, h.balanced_partition_columns(), chunk)
    return ("ng", chunk, seg)


def _gcn_sum(life, F, order):
    from oracle import oracle as orc
    P, g = life.P, life.g
    key = life.m.val_key
    val, x = P.val_h[key], P.x(F, "host")

    def compute():
        if order[0] == "max":
            return orc.gcn_max(g.ptr, g.idx, val, x)
        if order[0] == "seq":
            return orc.gcn_seq(g.ptr, g.idx, val, x)
        if order[0] == "mean_rows":
            return orc.gcn_mean(g.ptr, g.idx, val, x)
        if order[0] == "ng":
            ps, tg = orc.neighbor_grouping(g.ptr, order[1])
            return orc.gcn_grouped(ps, tg, g.idx, val, x, g.V, seg=order[2])
        ps, ix, tg, vs = orc.locality_schedule(g.ptr, g.idx, order[1], order[2], ng=order[3], val=val)
        return orc.gcn_grouped(ps, tg, ix, vs, x, g.V, seg=0)
    return P.memo(("gcn", key, P.val_version[key], F, order), compute)


def judge_gcn(life, op, p, outs, what):
    """bit-equal to the oracle restated from the handle's own queries (tests/test_gpu_parity.py / test_gpu_blocked.py), canaries included"""
    torch = _torch()
    from oracle import oracle as orc
    g, m = life.g, life.m
    F, reduce = p["F"], p.get("reduce", "sum")
    order = _gcn_order(life, op, p)
    ref = _gcn_sum(life, F, order)
    has = (g.deg > 0)[:, None]
    aux_run = m.row_aux is not None and reduce != "sum"
    if reduce == "mean" and order[0] != "mean_rows":
        d = (life.P.aux_h[m.row_aux] if aux_run else np.maximum(g.deg, 1))[:, None].astype(np.float32)
        ref = np.where(has, ref / d, np.float32(0)).astype(np.float32)
    base = np.float32(CANARY)
    if p.get("acc", False):
        if reduce == "max":
            new = np.maximum(base, ref)        # row_aux > 0 everywhere: an earlier pass has folded edges into y
        else:
            new = (base + ref).astype(np.float32)
        if p.get("relu", False):
            ref = np.maximum(np.where(has, new, base), 0)        # y = max(y + A.x, 0), rows without edges included
        else:
            ref = np.where(has, new, base)                        # rows without edges stay untouched
    elif p.get("relu", False):
        ref = np.maximum(ref, 0)
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    want = torch.from_numpy(ref).to(life._dt(p.get("ydt", "f32")))
    got = outs["y"][1].cpu()
    assert torch.equal(got, want), "the long-lived handle's y is not the oracle's %r (%d elements differ): %s" % (
        order, int((got != want).sum()), what)
    if not p.get("acc", False):
        assert bool((got[torch.from_numpy(g.deg == 0)] == 0).all()), "rows without edges must read 0: " + what
    if op in ("nn", "nn_typed"):
        t = outs["t"][1]
        y = outs["y"][1]
        if y.dtype == torch.float32:       # the ascending-k chain of the stored y (tests/test_gpu_parity.py, test_gpu_nn_typed.py)
            assert np.array_equal(t.cpu().numpy(), orc.matmul_nn(y.cpu().numpy(), life.P.w(F, p["OUT"], "host"))), "transformed: " + what
        elif t.dtype == torch.bfloat16:    # one rounding of what the fp32-transformed call computes on the same inputs (test_gpu_nn_typed.py)
            b32 = life.twin_run(op, dict(p, tdt="f32"))      # (on a twin: bit-equal to the handle by the comparison above)
            assert torch.equal(t, b32["t"][1].to(torch.bfloat16)), "transformed (bf16): " + what
        else:                              # bf16 product: the bound of gnnagg_matmul_nn_typed against float64 of the stored operands
            y64, w64 = y.double(), life.P.w(F, p["OUT"], "bf16").double()
            err = (t.double() - y64 @ w64).abs()
            bound = 1e-5 * (y64.abs() @ w64.abs()) + 1e-30
            assert bool((err <= bound).all().item()), "transformed (bf16 product): " + what


def _gat_order(life, p):
    h, g, m = life.h, life.g, life.m
    mode = m.effective_mode(p.get("mode", "balanced"), p.get("newval", False))
    if mode == "rows":
        return ("rows",)
    if mode == "scheduled":
        kind, params = m.sched
        if kind == "neighbor_grouping":
            return ("ng", params[0], h.mode_params("scheduled")[1])
        return ("loc", params[0], g.V, params[1] if kind == "locality_neighbor_grouping" else 0)
    parts = h.balanced_partitions()
    typed = p.get("xdt", "f32") != "f32" or p.get("ydt", "f32") != "f32" or p.get("stable", False) or p.get("shift", False)
    if parts > 0 and typed:
        return ("ng", g.pick_chunk(), 16)
    chunk, seg = h.balanced_params()
    if parts > 0:
        return ("loc", parts, h.balanced_partition_columns(), chunk)
    return ("ng", chunk, seg)


def gat_scale(g, w, x, H):
    """sum_e w_e |x_e| / sum_e w_e, the error scale of tests/test_gpu_parity.py::gat_scale (the same float64 sums, taken row by row)"""
    F = x.shape[1]
    s = np.zeros((g.V, F))
    if g.E:
        contrib = np.repeat(w, F // H, axis=1).astype(np.float64) * np.abs(x[g.idx])
        nz = g.deg > 0
        s[nz] = np.add.reduceat(contrib, g.ptr[:-1][nz].astype(np.int64), axis=0)
    return s.astype(np.float32)


def judge_gat(life, op, p, outs, what):
    """within the bound the same call already has in the suite: assert_within with RTOL = 1e-5 on gat_scale + |ref| (tests/test_gpu_parity.py),
    the GATv2 bound of tests/test_gpu_gatv2.py, the shifted bound of tests/test_gpu_gat_shift.py"""
    torch = _torch()
    from oracle import oracle as orc
    from test_gpu_parity import RTOL, assert_within
    P, g = life.P, life.g
    H, D = p["H"], p["D"]
    F = H * D
    empty = torch.from_numpy(g.deg == 0)
    if op == "edge_ops":
        att, a1 = P.att(H, "host"), P.att(1, "host")
        np.testing.assert_allclose(outs["att_w"][1].cpu().numpy(), P.memo(("gat_att", H), lambda: orc.gat_att(g.ptr, g.idx, att, H)), rtol=RTOL,
                                   err_msg=what)
        uv = outs["uv"][1].view(-1)
        assert np.array_equal(uv.cpu().numpy(), orc.gat_u_add_v(g.ptr, g.idx, a1)), "u_add_v: " + what
        w = torch.exp(torch.nn.functional.leaky_relu(uv, 0.2)).cpu().numpy()
        center = outs["center"][1].view(-1).cpu().numpy()
        np.testing.assert_allclose(center, orc.gat_add_to_center(g.ptr, w), rtol=RTOL, err_msg=what)
        assert np.array_equal(outs["div"][1].view(-1).cpu().numpy(), orc.gat_div_each(g.ptr, center, w)), "div_each: " + what
        return
    att, x = P.att(H, "host"), P.x(F, "host")
    if op == "row_shift":
        from test_gat_shift_host import row_shift_ref
        assert np.array_equal(outs["shift"][1].cpu().numpy(), row_shift_ref(g.ptr, g.idx, att, H, 0.2)), "row_shift: " + what
        return
    y = outs["y"][1]
    if op == "v2":
        from test_gatv2_host import gatv2_bound, gatv2_ref, worst_ratio
        a = life._a(H, D).cpu().numpy()
        ref, L, S = P.memo(("v2", H, D), lambda: gatv2_ref(g.ptr, g.idx, x, x, a, H, 0.2, block_edges=max(256, (1 << 22) // F)))
        if y.dtype == torch.float32:
            ratio = worst_ratio(y.cpu().numpy(), ref, gatv2_bound(L, S, H))
            assert ratio <= 1.0, "GATv2: worst ratio %.3g against the bound: %s" % (ratio, what)
        else:      # one rounding of the fp32-y run on the same inputs (tests/test_gpu_gatv2.py)
            b32 = life.twin_run("v2", dict(p, ydt="f32"))
            assert torch.equal(y, b32["y"][1].to(torch.bfloat16)), "GATv2: the bf16 y is not one rounding of the fp32 y: " + what
        assert bool((y.cpu()[empty] == 0).all()), what
        return
    if op == "part":
        ref = P.memo(("gat_fused", H, D), lambda: orc.gat_fused(g.ptr, g.idx, att, x, H))
    elif p.get("stable") or p.get("shift"):
        from test_gat_shift_host import gat_ref_shifted, gat_scale_shifted, row_shift_ref
        from test_gat_logits_host import worst_ratio

        def shifted():
            shift = row_shift_ref(g.ptr, g.idx, att, H, 0.2)
            return (gat_ref_shifted(g.ptr, g.idx, att, x, shift, H, 0.2), gat_scale_shifted(g.ptr, g.idx, att, x, shift, H, 0.2))
        ref, scale = P.memo(("gat_shifted", H, D), shifted)
        got = y.float().cpu().numpy()
        if y.dtype == torch.float32:
            ratio = worst_ratio(got, ref, scale + np.abs(ref))
            assert ratio <= 1.0, "shifted GAT: worst ratio %.3g of the bound: %s" % (ratio, what)
        else:
            b32 = life.twin_run("run", dict(p, ydt="f32"))
            assert torch.equal(y, b32["y"][1].to(torch.bfloat16)), "shifted GAT: the bf16 y is not one rounding of the fp32 y: " + what
        assert bool((y.cpu()[empty] == 0).all()), what
        return
    else:
        order = _gat_order(life, p)

        def grouped():
            if order[0] == "rows":
                return orc.gat_fused(g.ptr, g.idx, att, x, H)
            if order[0] == "ng":
                return orc.gat_grouped(*orc.neighbor_grouping(g.ptr, order[1]), g.idx, att, x, g.V, H, seg=order[2])[0]
            ps, ix, tg, _ = orc.locality_schedule(g.ptr, g.idx, order[1], order[2], ng=order[3])
            return orc.gat_grouped(ps, tg, ix, att, x, g.V, H, seg=0)[0]
        ref = P.memo(("gat", H, D, order), grouped)
    scale = P.memo(("gat_scale", H, D), lambda: gat_scale(g, P.memo(("gat_att", H), lambda: orc.gat_att(g.ptr, g.idx, att, H)), x, H))
    if y.dtype == torch.float32:
        assert_within(y.cpu().numpy(), ref, scale + np.abs(ref), what)
    else:      # a bf16 y is ONE rounding of the fp32 result of the same configuration and mode (run on a twin) (tests/test_gpu_bf16_gat.py)
        b32 = life.twin_run(op, dict(p, ydt="f32"))
        assert torch.equal(y, b32["y"][1].to(torch.bfloat16)), "GAT: the bf16 y is not one rounding of the fp32 y: " + what
        assert_within(b32["y"][1].cpu().numpy(), ref, scale + np.abs(ref), what)
    assert bool((y.cpu()[empty] == 0).all()), "rows without edges must read 0: " + what
    if p.get("newval"):      # CSR edge order, the weights of the canonical rows mode (tests/test_gpu_blocked.py)
        ref_nv = P.memo(("newval", H, D), lambda: orc.gat_grouped(*orc.neighbor_grouping(g.ptr, 1 << 30), g.idx, att, x, g.V, H, seg=0)[1])
        np.testing.assert_allclose(outs["newval"][1].cpu().numpy(), ref_nv, rtol=1e-6, err_msg=what)
