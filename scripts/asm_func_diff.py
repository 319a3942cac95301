#!/usr/bin/env python3
"""Function-by-function comparison of two device assembly files (hipcc $(HIPFLAGS) --cuda-device-only -S) of the same kernel file, as
profiles/gemm_refactor/asm_diff.txt did for the GEMM move: are the functions the parent has instruction-identical in this change?

    scripts/asm_func_diff.py PARENT.s HEAD.s [--rename REGEX=REPL ...] [--label TEXT]

Compared per function: its instruction text (comments, blank lines and assembler directives other than labels dropped) and its
.amdhsa_kernel descriptor block.  Normalised: the function's own symbol and the .LBB<n>_ function index.  --rename rewrites PARENT symbol
names before they are looked up in HEAD (a template that gained a defaulted parameter has new mangled names for the same instantiations).
Descriptor lines that differ are printed; exit status 1 when a parent function is missing or different."""
import argparse
import re
import sys


def functions(path):
    """{symbol: [instruction lines]}, {symbol: [descriptor lines]}"""
    funcs, desc = {}, {}
    cur = None
    kd = None
    for raw in open(path):
        line = raw.split(";")[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kd = m.group(1)
            desc[kd] = []
            continue
        if kd is not None:
            if line.strip() == ".end_amdhsa_kernel":
                kd = None
            else:
                desc[kd].append(line.strip())
            continue
        m = re.match(r"^([A-Za-z_][\w.$]*):", line)
        if m and (m.group(1).startswith("__hip_cuid_") or m.group(1).startswith("amdhsa.")):   # per-compilation id; the metadata note
            cur = None
            continue
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            funcs[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        s = line.strip()
        if s.startswith(".") and not s.startswith(".LBB"):
            continue
        funcs[cur].append(s)
    return funcs, desc


def normal(lines, name):
    out = []
    for s in lines:
        s = s.replace(name, "<self>")
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        out.append(s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("head")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    pf, pd = functions(a.parent)
    hf, hd = functions(a.head)

    def head_name(n):
        for rx, repl in renames:
            n = re.sub(rx, repl, n)
        return n

    same = diff = missing = renamed = 0
    dsame = ddiff = dmissing = 0
    notes = []
    dnotes = {}
    seen = set()
    for n, body in pf.items():
        hn = head_name(n)
        renamed += hn != n
        seen.add(hn)
        if hn not in hf:
            missing += 1
            notes.append("    missing here: %s" % n)
            continue
        if normal(body, n) == normal(hf[hn], hn):
            same += 1
        else:
            diff += 1
            notes.append("    different: %s (%d instructions in the parent, %d here)" % (n, len(body), len(hf[hn])))
    for n, d in pd.items():
        hn = head_name(n)
        if hn not in hd:
            dmissing += 1
            continue
        a_, b_ = normal(d, n), normal(hd[hn], hn)
        if a_ == b_:
            dsame += 1
        else:
            ddiff += 1
            changed = "; ".join(x for x in a_ if x not in b_) + "  ->  " + "; ".join(x for x in b_ if x not in a_)
            dnotes.setdefault(changed, []).append(n)
    new = [n for n in hf if n not in seen]
    print("%s: parent functions: %d, identical: %d, different: %d, missing: %d, looked up under a new name: %d, new here: %d; "
          "kernel descriptors: parent %d, identical: %d, different: %d, missing: %d"
          % (a.label or a.head, len(pf), same, diff, missing, renamed, len(new), len(pd), dsame, ddiff, dmissing))
    for s in notes:
        print(s)
    for changed, names in dnotes.items():
        print("    descriptor lines that differ, in %d kernels (%s ...): %s" % (len(names), names[0], changed))
    return 1 if (diff or missing or dmissing) else 0


if __name__ == "__main__":
    sys.exit(main())
