# The boundary of a one-wave kernel's granule loop (the loop holding
# s_setprio 0) in build/kernels_fast.s: what the loop header waits for, and
# what the loop boundary copies.  Prints
#   * the s_waitcnt vmcnt lines of the header block (from the loop's label to
#     the first branch past the priority switch): in the steady state the only
#     vector-memory operations in flight there are the previous granule's PCM
#     stores and, until the back edge's wait, the prefetch issued before them,
#     so a vmcnt(N) with N below the number of stores parks the wave on store
#     acknowledgements;
#   * every vmcnt value the loop waits for, with the number of waits (the waits
#     of the rare paths that issue their own loads included);
#   * the v_mov_b32 of the back-edge blocks (the loop's blocks that branch to
#     the header or fall through into it) and of the header block: loop-carried
#     values the register allocator did not coalesce;
#   * the loop's instruction count.
#   tools/loop_boundary.sh [file.s] [mangled-name prefix]
set -eu
F=${1:-go-mp3_amd/csrc/build/kernels_fast.s}
K=${2:-_ZN4mp3g2v319granule_fast_kernelILb0ELb0ELi0E}  # (a mangled-name prefix)
python3 - "$F" "$K" <<'PY'
import collections, re, sys
f, k = sys.argv[1], sys.argv[2]
lines = open(f).read().split("\n")
i0 = next(i for i, l in enumerate(lines) if l.startswith(k) and l.split(";")[0].rstrip().endswith(":"))
i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[i0:i1]
sp = next(i for i, l in enumerate(body) if "s_setprio 0" in l)
# the innermost loop header before it, and its label (on that line or the one above)
h = max(i for i in range(sp) if "Loop Header" in body[i])
lab = next(re.match(r"^(\.LBB\w+):", body[j]).group(1) for j in (h, h - 1) if re.match(r"^\.LBB\w+:", body[j]))
bb = lab[2:]  # the name the block comments use
is_instr = lambda l: bool(re.match(r"\s*(s_|v_|ds_|buffer_|global_|scratch_|flat_)", l))
is_branch = lambda l: bool(re.match(r"\s*s_c?branch", l))
is_mov = lambda l: bool(re.match(r"\s*v_mov_b32", l))
vm = lambda l: re.search(r"s_waitcnt\b.*\bvmcnt\((\d+)\)", l)
# the function's blocks in layout order: (first line, label or None, in the loop?)
starts = [i for i, l in enumerate(body) if re.match(r"^(\.LBB\w+:|; %bb\.\d+:)", l)]
blocks = []
for n, s in enumerate(starts):
    e = starts[n + 1] if n + 1 < len(starts) else len(body)
    m = re.match(r"^(\.LBB\w+):", body[s])
    head = body[s] + (body[s + 1] if s + 1 < len(body) and not is_instr(body[s + 1]) else "")
    inloop = (m and m.group(1) == lab) or bool(re.search(r"(Header=|Parent Loop )%s\b" % re.escape(bb), head))
    blocks.append((s, e, m.group(1) if m else None, inloop))
loop = [b for b in blocks if b[3]]
seg = [l for s, e, _, _ in loop for l in body[s:e]]
print(f"{body[0].split(':')[0][:60]}: loop {lab}, {len(loop)} blocks, {sum(map(is_instr, seg))} instructions")
# header block: the instructions from the label to the first branch past the
# priority switch (s_setprio 0 sits in a conditional block of its own)
hb = []
for n in range(h, len(body)):
    if is_instr(body[n]):
        hb.append(body[n])
        if is_branch(body[n]) and n > sp:
            break
waits = [(n, l.strip()) for n, l in enumerate(hb) if vm(l)]
print(f"  header block ({len(hb)} instructions): {len(waits)} vmcnt waits, {sum(map(is_mov, hb))} v_mov_b32")
for n, l in waits:
    print(f"    +{n}: {l.split(';')[0].strip()}")
hist = collections.Counter(int(vm(l).group(1)) for l in seg if vm(l))
print("  vmcnt waits in the loop: " + (", ".join(f"vmcnt({v}) x{c}" for v, c in sorted(hist.items())) or "none"))
# back-edge blocks: a branch to the header's label, or laid out right before
# the header without an unconditional branch at the end (falls through)
hi = next(n for n, b in enumerate(blocks) if b[2] == lab)
back = []
for n, (s, e, _, inloop) in enumerate(blocks):
    if not inloop:
        continue
    ins = [l for l in body[s:e] if is_instr(l)]
    to_header = any(is_branch(l) and l.split(";")[0].split()[-1] == lab for l in ins)
    falls = n == hi - 1 and not (ins and re.match(r"\s*s_branch", ins[-1]))
    if to_header or falls:
        back.append(ins)
print(f"  back-edge blocks ({len(back)}, {sum(map(len, back))} instructions): "
      f"{sum(is_mov(l) for b in back for l in b)} v_mov_b32")
PY
