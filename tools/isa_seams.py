#!/usr/bin/env python3
"""Seams of one kernel in a -save-temps ISA file: the runs of MFMAs and what sits in the gaps between them.

A "run" is a stretch of the instruction stream in which consecutive MFMAs are at most --fill non-MFMA instructions
apart (the interleaved epilogue, waits and fragment reads of a k-step); a "gap" is a longer stretch without any MFMA,
i.e. code during which the matrix pipe has nothing queued.  For every gap the instruction-class mix is printed
(v_mov, v_accvgpr_*, v_cvt, other VALU, ds_read, global/buffer, s_waitcnt, scalar, branch), with the label of the basic
block it starts in, so a gap on a loop back-edge shows up once although it is paid on every iteration.

Usage: python tools/isa_seams.py build/csrc/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s <kernel name substring> [--fill N] [--min N]
  --fill N   largest non-MFMA stretch that still counts as inside a run (default 24)
  --min N    smallest gap that is listed with its mix (default: fill + 1)
The file holds no encodings, so code size is given as an instruction count; the byte size of a kernel is the size of its
symbol in the code object (llvm-readelf -s)."""
import argparse
import collections
import re


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_accvgpr"):
        return "accvgpr"
    if op.startswith("v_mov"):
        return "v_mov"
    if op.startswith("v_cvt"):
        return "v_cvt"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch", "s_barrier", "s_setpc", "s_swappc")):
        return "branch"
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith("s_"):
        return "salu"
    return "other"


ORDER = ["v_mov", "accvgpr", "v_cvt", "valu", "lds", "vmem", "wait", "salu", "branch", "nop", "other"]


def kernel_body(text, sub):
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\s*s_endpgm", text, re.S | re.M):
        if sub in m.group(1):
            return m.group(1), m.group(2)
    raise SystemExit(f"no kernel whose name contains {sub!r}")


def instructions(body):
    """(opcode, label of the enclosing basic block) for every instruction of the kernel, in program order."""
    label, out = "entry", []
    for line in body.split("\n"):
        lm = re.match(r"^(\.LBB\w+):", line)
        if lm:
            label = lm.group(1)
            continue
        if not line.startswith("\t"):
            continue
        s = line.strip()
        if not s or s.startswith((".", ";")):
            continue
        out.append((s.split()[0], label))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("isa")
    ap.add_argument("kernel")
    ap.add_argument("--fill", type=int, default=24)
    ap.add_argument("--min", type=int, default=None)
    a = ap.parse_args()
    fill = a.fill
    gmin = a.min if a.min is not None else fill + 1
    name, body = kernel_body(open(a.isa).read(), a.kernel)
    ins = instructions(body)
    n_mfma = sum(1 for op, _ in ins if op.startswith("v_mfma"))
    print(f"{name}\n  {len(ins)} instructions, {n_mfma} MFMAs; run = MFMAs at most {fill} instructions apart, gaps >= {gmin} listed")
    # split into alternating gaps and runs
    segs, cur, run_mfma, run_other = [], [], 0, 0    # cur = pending non-MFMA instructions since the last MFMA
    for op, lab in ins:
        if op.startswith("v_mfma"):
            if len(cur) > fill or (not segs and run_mfma == 0):
                if run_mfma:
                    segs.append(("run", run_mfma, run_other))
                if cur:
                    segs.append(("gap", cur))
                run_mfma, run_other = 0, 0
            else:
                run_other += len(cur)
            cur = []
            run_mfma += 1
        else:
            cur.append((op, lab))
    if run_mfma:
        segs.append(("run", run_mfma, run_other))
    if cur:
        segs.append(("gap", cur))
    tot_gap = 0
    for s in segs:
        if s[0] == "run":
            print(f"  run  {s[1]:5d} MFMAs, {s[2]:5d} other ({s[2] / s[1]:.2f} per MFMA)")
            continue
        g = s[1]
        if len(g) < gmin:
            print(f"  gap  {len(g):5d} (short)")
            continue
        tot_gap += len(g)
        c = collections.Counter(classify(op) for op, _ in g)
        labs = []
        for _, lab in g:
            if not labs or labs[-1] != lab:
                labs.append(lab)
        mix = "  ".join(f"{k} {c[k]}" for k in ORDER if c[k])
        top = collections.Counter(op for op, _ in g).most_common(4)
        print(f"  gap  {len(g):5d}  [{labs[0]}{'..' + labs[-1] if len(labs) > 1 else ''}]  {mix}")
        print("             top: " + ", ".join(f"{k} {v}" for k, v in top))
    print(f"  instructions in listed gaps: {tot_gap} of {len(ins)}")


if __name__ == "__main__":
    main()
