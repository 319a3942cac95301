"""CPU: the lane-geometry census (tests/geometry_census.py) against itself and against the sources.

1. every table entry: the Python restatement of its picker gives the tuple the entry was written for;
2. the `case` labels of DISPATCH_GEOM_CASES / DISPATCH_GEOM_16BIT (csrc/kernel_util.cuh) and of the two switches of attn_launch_typed
   (csrc/gatv2_shared.cuh), through which both attention kernels (csrc/agg_gatv2.hip, csrc/agg_dot.hip) are launched, read out of the
   sources, are exactly the labels the tables reach: a case added to (or taken out of) a switch fails here until the census has (or
   drops) a shape for it;
3. the restatements at the edges of their domain."""
import os
import re

import pytest

import geometry_census as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn_computing_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def case_labels(text):
    return [int(n) for n in re.findall(r"\bcase\s+(\d+)\s*:", text)]


def macro_body(text, name):
    """the text of `#define name(...)` up to the end of its last continued line"""
    m = re.search(r"^#define %s\b.*?[^\\\n][ \t]*\n" % re.escape(name), text, re.S | re.M)
    assert m, "no #define %s" % name
    return m.group(0)


def function_switches(text, name):
    """the texts of the `switch` statements inside the definition of the static function `name`"""
    m = re.search(r"^static int %s\(.*?^}" % re.escape(name), text, re.S | re.M)
    assert m, "no definition of %s" % name
    return re.split(r"\bswitch\s*\(", m.group(0))[1:]


# ------------------------------------------------------------------------------------------------------------ 1. restatement
@pytest.mark.parametrize("F,want", sorted(gc.GCN_F32.items()))
def test_gcn_fp32_entries(F, want):
    assert gc.pick_geometry(F) == want
    assert gc.typed_geometry(F, 4) == want     # a typed call with an fp32 x (bf16 y) picks the same lanes


@pytest.mark.parametrize("F,want", sorted(gc.GCN_BF16.items()))
def test_gcn_bf16_entries(F, want):
    assert gc.typed_geometry(F, 2) == want


@pytest.mark.parametrize("hd,want", sorted(gc.GAT_F32.items()))
def test_gat_fp32_entries(hd, want):
    H, D = hd
    assert gc.pick_geometry(H * D, D) == want
    assert gc.typed_geometry(H * D, 4, D) == want


@pytest.mark.parametrize("hd,want", sorted(gc.GAT_BF16.items()))
def test_gat_bf16_entries(hd, want):
    H, D = hd
    assert gc.typed_geometry(H * D, 2, D) == want


@pytest.mark.parametrize("hd,want", sorted(gc.GATV2.items()))
def test_gatv2_entries(hd, want):
    H, D = hd
    assert sorted(want) == [2, 4]
    for esize, tup in want.items():
        assert gc.gatv2_geometry(H * D, H, esize) == tup, esize


def test_the_tables_hold_what_they_promise():
    # every (VEC, GROUP) with one, two and three (or more) column tiles per VEC
    for table, vecs in ((gc.GCN_F32, (1, 2, 4)), (gc.GCN_BF16, (1, 2, 4, 8)), (gc.GAT_F32, (1, 2, 4)), (gc.GAT_BF16, (1, 2, 4, 8))):
        got = set(table.values())
        for v in vecs:
            assert {(v, g, 1) for g in (8, 16, 32, 64)} <= got, v
            assert (v, 64, 2) in got and any(t[0] == v and t[2] >= 3 for t in got), v
    # the smallest F of every GCN tuple
    for table, pick in ((gc.GCN_F32, gc.pick_geometry), (gc.GCN_BF16, lambda F: gc.typed_geometry(F, 2))):
        for F, want in table.items():
            assert all(pick(f) != want for f in range(1, F)), F
    # GAT: per narrower VEC an entry where D, not F, forces it
    for table, esize in ((gc.GAT_F32, 4), (gc.GAT_BF16, 2)):
        forced = {gc.typed_geometry(H * D, esize, D)[0] for (H, D) in table if gc.typed_geometry(H * D, esize)[0] > gc.typed_geometry(H * D, esize, D)[0]}
        assert forced == {v for v in (1, 2, 4) if v < 16 // esize}, forced
    assert gc.GAT_BF16[(8, 4)] == (4, 8, 1)
    # attention: every rounded fragment count, odd head counts in the segmented geometry, lph = 64, segmented in one type only
    rounded = {(t[0], t[3], t[4]) for per in gc.GATV2.values() for t in per.values() if t[3] < t[4]}
    assert rounded == {(True, 3, 4), (False, 3, 4), (False, 5, 10), (False, 8, 10), (False, 9, 10), (False, 11, 16), (False, 15, 16)}
    seg_heads = {H for (H, D), per in gc.GATV2.items() if per[4][0] or per[2][0]}
    assert {3, 5, 6, 7} <= seg_heads
    assert any(t[5] == 64 for per in gc.GATV2.values() for t in per.values())
    assert gc.GATV2[(1, 512)][2][0] and not gc.GATV2[(1, 512)][4][0]
    for (H, D) in gc.GATV2:
        assert H * D <= gc.GATV2_MAX_FEAT


# ------------------------------------------------------------------------------------------------------------ 2. the sources
def test_dispatch_geom_labels_are_the_ones_the_tables_reach():
    text = source("kernel_util.cuh")
    fp32 = case_labels(macro_body(text, "DISPATCH_GEOM_CASES"))
    assert len(fp32) == len(set(fp32)) == 12
    body16 = macro_body(text, "DISPATCH_GEOM_16BIT")
    assert "DISPATCH_GEOM_CASES(KERNEL_CALL)" in body16
    extra = case_labels(body16)
    assert len(extra) == len(set(extra)) == 4
    assert case_labels(macro_body(text, "DISPATCH_GEOM")) == []   # DISPATCH_GEOM adds no label of its own
    assert set(fp32) == gc.geom_labels(gc.GCN_F32) == gc.geom_labels(gc.GAT_F32)
    assert set(fp32) | set(extra) == gc.geom_labels(gc.GCN_BF16) == gc.geom_labels(gc.GAT_BF16)
    # and the label is vec * 100 + group with the constants the case sets
    for lab, vec, group in re.findall(r"case (\d+): \{ constexpr int VEC = (\d+), GROUP = (\d+);", text):
        assert int(lab) == int(vec) * 100 + int(group)


@pytest.mark.parametrize("file,functor,kernel", [("agg_gatv2.hip", "Gatv2Kernel", "k_gatv2"), ("agg_dot.hip", "DotKernel", "k_dot_attn")])
def test_attention_switch_labels_are_the_ones_the_table_reaches(file, functor, kernel):
    switches = function_switches(source("gatv2_shared.cuh"), "attn_launch_typed")
    assert len(switches) == 2
    seg, gen = (case_labels(s) for s in switches)
    assert switches[0].startswith("g.group * 10 + g.nf") and switches[1].startswith("g.nf")
    assert len(seg) == len(set(seg)) and len(gen) == len(set(gen))
    seg32, gen32 = gc.gatv2_labels(4)
    seg16, gen16 = gc.gatv2_labels(2)
    assert set(seg) == seg32 and set(gen) == gen32 == gen16
    # 16-bit rows have at most 128 16-byte lanes: the four-fragment case is compiled for fp32 only
    assert re.search(r"case 644:\s*if constexpr \(VEC == 4\)", switches[0])
    assert seg16 == set(seg) - {644}
    # group * 10 + nf, as instantiated
    for lab, group, nf in re.findall(r"case (\d+):\s*(?:if constexpr \(VEC == 4\) )?return attn_launch_inst<K, VEC, (\d+), (\d+), TX, true>", switches[0]):
        assert int(lab) == int(group) * 10 + int(nf)
    for lab, nf in re.findall(r"case (\d+):\s*return attn_launch_inst<K, 1, 64, (\d+), TX, false>", switches[1]):
        assert int(lab) == int(nf)
    # that switch is the only one: the kernel's file has no switch and no label of its own, names its kernel for the shared launcher and
    # goes through attn_launch_typed once per element type
    text = source(file)
    assert not re.search(r"\bswitch\s*\(", text) and case_labels(text) == []
    assert re.search(r"struct %s \{[^}]*return &%s<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>;" % (functor, kernel), text)
    assert re.findall(r"return attn_launch_typed<%s, (\d), (\w+)>\(a, g, stream, no_inst\);" % functor, text) == [("8", "__bf16"), ("4", "float")]


def test_the_label_readers_see_an_added_and_a_removed_case():
    """the readers themselves: a label more or less in the text is a label more or less in what they return"""
    text = source("kernel_util.cuh")
    body = macro_body(text, "DISPATCH_GEOM_CASES")
    more = body.replace("case 464:", "case 864: { } break; \\\n        case 464:")
    assert set(case_labels(more)) - set(case_labels(body)) == {864}
    less = re.sub(r"case 208:.*\n", "", body)
    assert set(case_labels(body)) - set(case_labels(less)) == {208}


# ------------------------------------------------------------------------------------------------------------ 3. the edges
def test_restatement_edges():
    assert gc.gatv2_geometry(1024, 1, 4) == (False, 1, 64, 16, 16, 0)   # lph = 256 > 64: the general geometry
    assert gc.gatv2_geometry(1024, 1, 2) == (False, 1, 64, 16, 16, 0)   # lph = 128
    assert gc.gatv2_geometry(1024, 4, 4) == (True, 4, 64, 4, 4, 64)
    assert gc.gatv2_geometry(1024, 2, 2) == (True, 8, 64, 2, 2, 64)
    assert gc.gatv2_geometry(1, 1, 4) == gc.gatv2_geometry(1, 1, 2) == (False, 1, 64, 1, 1, 0)
    assert gc.gatv2_geometry(1025, 1, 4) is None and gc.gatv2_geometry(0, 1, 4) is None and gc.gatv2_geometry(8, 0, 4) is None
    assert gc.gatv2_geometry(10, 3, 4) is None and gc.gatv2_geometry(16, 3, 2) is None   # F % heads != 0
    assert gc.pick_geometry(1) == gc.typed_geometry(1, 2) == gc.typed_geometry(1, 4) == (1, 8, 1)
    assert gc.pick_geometry(1024) == (4, 64, 4) and gc.typed_geometry(1024, 2) == (8, 64, 2)
    # narrower pointers narrow the lane (the census itself runs 16-byte aligned operands only)
    assert gc.pick_geometry(128, align=8) == (2, 64, 1) and gc.pick_geometry(128, align=4) == (1, 64, 2)
    assert gc.typed_geometry(128, 2, align=2) == (1, 64, 2) and gc.typed_geometry(128, 2, align=8) == (4, 32, 1)
