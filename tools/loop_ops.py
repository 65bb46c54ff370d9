#!/usr/bin/env python3
"""Opcode counts per basic block of a one-wave kernel's granule loop.

The block walk of tools/loop_boundary.sh (the loop is the innermost one that
holds `s_setprio 0`) plus a histogram: for every block of the loop, in layout
order, its label, its instruction count and how often each opcode occurs.
A block is found again in another build by what it holds, not by its label:
the window is the block with the 144 v_pk_fma_f32, the long-block requantize
the one with the 27 ds_read_b32 and the nine v_pk_mad_u16.

  tools/loop_ops.py [file.s] [mangled-name prefix] [-m MIN] [-b LABEL] [-g REGEX]

  -m MIN    only blocks of at least MIN instructions (default 1)
  -b LABEL  only this block (.LBB1_123, or bb.7 for an unlabelled one)
  -g REGEX  after the histogram, the block's instructions whose text matches
            (e.g. -g 'v_add_u32.*0x' for adds of a literal)
The last line sums the loop: instructions and the opcode classes.
"""
import argparse
import collections
import re

FAST = "go-mp3_amd/csrc/build/kernels_fast.s"
PROD = "_ZN4mp3g2v319granule_fast_kernelILb0ELb0ELi0E"  # <false, false, MP3G_OUT_S16>

is_instr = lambda l: bool(re.match(r"\s*(s_|v_|ds_|buffer_|global_|scratch_|flat_)", l))
opcode = lambda l: l.split(";")[0].split()[0]


def klass(op):
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_", "scratch_", "flat_")):
        return "VMEM"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    return "VALU"


def loop_blocks(path, kernel):
    lines = open(path).read().split("\n")
    i0 = next(i for i, l in enumerate(lines) if l.startswith(kernel) and l.split(";")[0].rstrip().endswith(":"))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[i0:i1]
    sp = next(i for i, l in enumerate(body) if "s_setprio 0" in l)
    h = max(i for i in range(sp) if "Loop Header" in body[i])
    lab = next(re.match(r"^(\.LBB\w+):", body[j]).group(1) for j in (h, h - 1) if re.match(r"^\.LBB\w+:", body[j]))
    bb = lab[2:]
    starts = [i for i, l in enumerate(body) if re.match(r"^(\.LBB\w+:|; %bb\.\d+:)", l)]
    out = []
    for n, s in enumerate(starts):
        e = starts[n + 1] if n + 1 < len(starts) else len(body)
        m = re.match(r"^(\.LBB\w+):", body[s])
        head = body[s] + (body[s + 1] if s + 1 < len(body) and not is_instr(body[s + 1]) else "")
        if (m and m.group(1) == lab) or re.search(r"(Header=|Parent Loop )%s\b" % re.escape(bb), head):
            name = m.group(1) if m else re.match(r"^; %(bb\.\d+):", body[s]).group(1)
            out.append((name, [l for l in body[s:e] if is_instr(l)]))
    return body[0].split(":")[0], lab, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file", nargs="?", default=FAST)
    ap.add_argument("kernel", nargs="?", default=PROD)
    ap.add_argument("-m", "--min", type=int, default=1)
    ap.add_argument("-b", "--block")
    ap.add_argument("-g", "--grep")
    a = ap.parse_args()
    name, lab, blocks = loop_blocks(a.file, a.kernel)
    total = collections.Counter()
    n_all = 0
    print(f"{name[:60]}: loop {lab}, {len(blocks)} blocks")
    for label, ins in blocks:
        hist = collections.Counter(map(opcode, ins))
        n_all += len(ins)
        for op, c in hist.items():
            total[klass(op)] += c
        if len(ins) < a.min or (a.block and label != a.block):
            continue
        print(f"{label}: {len(ins)} instructions")
        print("    " + ", ".join(f"{op} {c}" for op, c in sorted(hist.items(), key=lambda t: (-t[1], t[0]))))
        if a.grep:
            for l in ins:
                if re.search(a.grep, l):
                    print("      " + l.split(";")[0].strip())
    print(f"loop: {n_all} instructions; " + ", ".join(f"{k} {total[k]}" for k in ("VALU", "SALU", "LDS", "VMEM", "branch", "wait")))


if __name__ == "__main__":
    main()
