"""The lane-geometry census: the three host pickers of the aggregation kernels restated in Python, and one table of shapes per picker.

Every aggregation kernel is a template over a lane geometry and the host picks the instantiation from (F, heads, element size, pointer
alignment):
    pick_geometry   (csrc/kernel_util.cuh)    fp32 calls:           (VEC, GROUP, ntiles), 12 (VEC, GROUP) cases (DISPATCH_GEOM_CASES)
    typed_geometry  (csrc/kernel_util.cuh)    typed calls:          (VEC, GROUP, ntiles), 16 cases (DISPATCH_GEOM_16BIT)
    gatv2_geometry  (csrc/gatv2_shared.cuh)   run_v2 and run_dot:   6 segmented (GROUP, NF) cases and 5 general fragment counts
Each restatement below returns exactly the tuple its picker switches on.  Each table maps (F or (heads, D), element size) to the tuple
the entry is INTENDED to reach, written out by hand: tests/test_geometry_census_host.py checks the restatements against the tables and
the tables against the `case` labels read out of the sources, tests/test_gpu_geometry_census.py runs every entry against float64.

The rule: a `case` label added to one of the switches needs an entry here (the host test fails until it has one).

All entries assume operands aligned to 16 bytes (torch allocations; the GPU test asserts it), so shape and dtype alone select the
geometry.  Every shape is one the API documents as supported."""

GATV2_MAX_FEAT = 1024   # common.h: kGatv2MaxFeat (tests/test_gatv2_host.py checks the Python constant against the header)


# ------------------------------------------------------------------------------------------------------------ the three pickers
def _group_and_tiles(lanes):
    group = 8
    while group < 64 and group < lanes:
        group <<= 1
    return group, (lanes + group - 1) // group


def pick_geometry(F, dhead=None, align=16):
    """kernel_util.cuh pick_geometry for fp32 rows of F elements whose pointers are all `align`-byte aligned; dhead: the head width of a
    GAT call (a lane's columns lie inside one head), F for GCN.  Returns (vec, group, ntiles)."""
    dhead = F if dhead is None else dhead
    vec = 1
    if F % 4 == 0 and dhead % 4 == 0 and align % 16 == 0:
        vec = 4
    elif F % 2 == 0 and dhead % 2 == 0 and align % 8 == 0:
        vec = 2
    group, ntiles = _group_and_tiles((F + vec - 1) // vec)
    return vec, group, ntiles


def typed_geometry(F, esize, dhead=None, align=16):
    """kernel_util.cuh typed_geometry (align_class of dhead at X, lanes of at most 16 bytes): esize 2 = bf16 x, 4 = fp32 x.
    Returns (vec, group, ntiles)."""
    dhead = F if dhead is None else dhead
    vec = 16 // esize
    while vec > 1 and (dhead % vec != 0 or align % (vec * esize) != 0):
        vec >>= 1
    group, ntiles = _group_and_tiles((F + vec - 1) // vec)
    return vec, group, ntiles


def gatv2_geometry(F, heads, esize):
    """gatv2_shared.cuh gatv2_geometry: (segred, vec, group, nf_raw, nf, lph), or None where the picker refuses the shape.  nf_raw is the
    fragment count the row needs, nf the instantiated one it is rounded up to (attn_launch_typed switches on group * 10 + nf, or on nf)."""
    if F < 1 or heads < 1 or F % heads != 0 or F > GATV2_MAX_FEAT:
        return None
    D, vec = F // heads, 16 // esize
    if D % vec == 0:
        lph = D // vec
        if lph & (lph - 1) == 0 and lph <= 64:
            group, nf_raw = _group_and_tiles(F // vec)
            return True, vec, group, nf_raw, (1 if nf_raw <= 1 else 2 if nf_raw <= 2 else 4), lph
    nf_raw = (F + 63) // 64
    nf = 1 if nf_raw <= 1 else 2 if nf_raw <= 2 else 4 if nf_raw <= 4 else 10 if nf_raw <= 10 else 16
    return False, 1, 64, nf_raw, nf, 0


# ------------------------------------------------------------------------------------------------------------ the tables
# GCN, fp32 x (pick_geometry; the typed fp32-x call's typed_geometry gives the same tuples): F -> (vec, group, ntiles).  Per VEC the
# smallest F of each GROUP, then the smallest F of two and of three column tiles.
GCN_F32 = {
    4: (4, 8, 1), 36: (4, 16, 1), 68: (4, 32, 1), 132: (4, 64, 1), 260: (4, 64, 2), 516: (4, 64, 3),
    2: (2, 8, 1), 18: (2, 16, 1), 34: (2, 32, 1), 66: (2, 64, 1), 130: (2, 64, 2), 258: (2, 64, 3),
    1: (1, 8, 1), 9: (1, 16, 1), 17: (1, 32, 1), 33: (1, 64, 1), 65: (1, 64, 2), 129: (1, 64, 3),
}
# GCN, bf16 x (typed_geometry, 2-byte elements): the 16-byte lanes of 8 elements come on top; below them the same F as above
GCN_BF16 = {
    8: (8, 8, 1), 72: (8, 16, 1), 136: (8, 32, 1), 264: (8, 64, 1), 520: (8, 64, 2), 1032: (8, 64, 3),
    4: (4, 8, 1), 36: (4, 16, 1), 68: (4, 32, 1), 132: (4, 64, 1), 260: (4, 64, 2), 516: (4, 64, 3),
    2: (2, 8, 1), 18: (2, 16, 1), 34: (2, 32, 1), 66: (2, 64, 1), 130: (2, 64, 2), 258: (2, 64, 3),
    1: (1, 8, 1), 9: (1, 16, 1), 17: (1, 32, 1), 33: (1, 64, 1), 65: (1, 64, 2), 129: (1, 64, 3),
}
# Modes: every entry runs in balanced mode with the four dtype pairs; GNNAGG_MODE_ROWS (the canonical CSR-order chains) and the item
# kernels of a restated schedule are fp32 x / fp32 y only -- the typed calls refuse them (api.hip: "fast_rows", "item kernels").
# The nn epilogue of run_with_nn_typed depends on more than the geometry (agg_gcn.hip launch_gcn_plan: one column tile, groups of 16
# lanes or more -- or the 8 x 8 groups of a bf16 row of 64 into a bf16 y --, the hubs folded in the kernel, the W image within LDS); every
# other entry takes the aggregation kernel and a GEMM behind it.  The GPU test prints last_nn_path per entry.

# GAT: (heads, D) -> (vec, group, ntiles); VEC must divide the head width D.  Per VEC the smallest F of each GROUP on a head count
# that is no power of two where F allows one, two and three column tiles, and entries where D forces a narrower lane than F would.
# Route notes (api.hip gat_run, agg_gat.hip launch_gat_plan): with several column tiles the hubs are folded by k_combine, not in the
# plan kernel; in rows mode the long-row kernel takes hub rows only where D % 32 == 0 (tile_in_head), elsewhere the item kernels run.
GAT_F32 = {
    (1, 4): (4, 8, 1), (3, 12): (4, 16, 1), (1, 68): (4, 32, 1), (11, 12): (4, 64, 1), (5, 52): (4, 64, 2), (3, 172): (4, 64, 3),
    (1, 2): (2, 8, 1), (3, 6): (2, 16, 1), (1, 34): (2, 32, 1), (11, 6): (2, 64, 1), (5, 26): (2, 64, 2), (3, 86): (2, 64, 3),
    (1, 1): (1, 8, 1), (3, 3): (1, 16, 1), (1, 17): (1, 32, 1), (11, 3): (1, 64, 1), (5, 13): (1, 64, 2), (3, 43): (1, 64, 3),
    (2, 6): (2, 8, 1),      # F = 12 alone would take 16-byte lanes
    (2, 3): (1, 8, 1),      # F = 6 alone would take 8-byte lanes
    (4, 32): (4, 32, 1),    # D % 32 == 0: the rows mode's long-row kernel (tile_in_head)
}
GAT_BF16 = {
    (1, 8): (8, 8, 1), (3, 24): (8, 16, 1), (1, 136): (8, 32, 1), (11, 24): (8, 64, 1), (5, 104): (8, 64, 2), (3, 344): (8, 64, 3),
    (1, 4): (4, 8, 1), (3, 12): (4, 16, 1), (1, 68): (4, 32, 1), (11, 12): (4, 64, 1), (5, 52): (4, 64, 2), (3, 172): (4, 64, 3),
    (1, 2): (2, 8, 1), (3, 6): (2, 16, 1), (1, 34): (2, 32, 1), (11, 6): (2, 64, 1), (5, 26): (2, 64, 2), (3, 86): (2, 64, 3),
    (1, 1): (1, 8, 1), (3, 3): (1, 16, 1), (1, 17): (1, 32, 1), (11, 3): (1, 64, 1), (5, 13): (1, 64, 2), (3, 43): (1, 64, 3),
    (2, 12): (4, 8, 1),     # F = 24 is a multiple of 8, D = 12 is not: 8-byte lanes
    (2, 6): (2, 8, 1),      # F = 12 alone would take 8-byte lanes
    (2, 3): (1, 8, 1),      # F = 6 alone would take 4-byte lanes
    (8, 4): (4, 8, 1),      # README's general-path case of the attention calls; here 8-byte lanes
    (4, 32): (8, 16, 1),    # D % 32 == 0 (see GAT_F32)
}

# run_v2 / run_dot: (heads, D) -> {element size: (segred, vec, group, nf_raw, nf, lph)}.  Every switch label of the shared launcher for both
# element sizes; every rounded fragment count (nf_raw < nf: whole fragments past F); head counts 3, 5, 6, 7 in the segmented geometry
# (idle lanes inside a group, a partly filled last fragment); lph = 64; one shape segmented in bf16 and general in fp32.
GATV2 = {
    (3, 4):   {4: (True, 4, 8, 1, 1, 1),     2: (False, 1, 64, 1, 1, 0)},
    (8, 4):   {4: (True, 4, 8, 1, 1, 1),     2: (False, 1, 64, 1, 1, 0)},     # README's general-path case (bf16)
    (3, 16):  {4: (True, 4, 16, 1, 1, 4),    2: (True, 8, 8, 1, 1, 2)},
    (5, 16):  {4: (True, 4, 32, 1, 1, 4),    2: (True, 8, 16, 1, 1, 2)},
    (3, 64):  {4: (True, 4, 64, 1, 1, 16),   2: (True, 8, 32, 1, 1, 8)},
    (3, 128): {4: (True, 4, 64, 2, 2, 32),   2: (True, 8, 64, 1, 1, 16)},
    (5, 64):  {4: (True, 4, 64, 2, 2, 16),   2: (True, 8, 64, 1, 1, 8)},
    (7, 128): {4: (True, 4, 64, 4, 4, 32),   2: (True, 8, 64, 2, 2, 16)},
    (3, 256): {4: (True, 4, 64, 3, 4, 64),   2: (True, 8, 64, 2, 2, 32)},     # fp32: 3 -> 4 fragments, lph = 64
    (5, 128): {4: (True, 4, 64, 3, 4, 32),   2: (True, 8, 64, 2, 2, 16)},     # fp32: 3 -> 4, the third fragment half filled
    (6, 128): {4: (True, 4, 64, 3, 4, 32),   2: (True, 8, 64, 2, 2, 16)},
    (1, 512): {4: (False, 1, 64, 8, 10, 0),  2: (True, 8, 64, 1, 1, 64)},     # general in fp32 (lph = 128), segmented in bf16 (lph = 64)
    (3, 7):   {4: (False, 1, 64, 1, 1, 0),   2: (False, 1, 64, 1, 1, 0)},
    (1, 100): {4: (False, 1, 64, 2, 2, 0),   2: (False, 1, 64, 2, 2, 0)},
    (1, 150): {4: (False, 1, 64, 3, 4, 0),   2: (False, 1, 64, 3, 4, 0)},
    (3, 50):  {4: (False, 1, 64, 3, 4, 0),   2: (False, 1, 64, 3, 4, 0)},
    (1, 300): {4: (False, 1, 64, 5, 10, 0),  2: (False, 1, 64, 5, 10, 0)},
    (1, 550): {4: (False, 1, 64, 9, 10, 0),  2: (False, 1, 64, 9, 10, 0)},
    (1, 700): {4: (False, 1, 64, 11, 16, 0), 2: (False, 1, 64, 11, 16, 0)},
    (2, 475): {4: (False, 1, 64, 15, 16, 0), 2: (False, 1, 64, 15, 16, 0)},
}


# ------------------------------------------------------------------------------------------------------------ what the tables reach
def geom_labels(table):
    """the `case` labels (vec * 100 + group) a (vec, group, ntiles) table reaches"""
    return {v * 100 + g for v, g, _ in table.values()}


def gatv2_labels(esize):
    """(segmented labels group * 10 + nf, general labels nf) that GATV2 reaches at one element size"""
    seg, gen = set(), set()
    for per_size in GATV2.values():
        segred, _, group, _, nf, _ = per_size[esize]
        if segred:
            seg.add(group * 10 + nf)
        else:
            gen.add(nf)
    return seg, gen
