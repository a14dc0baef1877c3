"""Instruction mix of one kernel in a hipcc -S (gfx950) listing, per basic block and in total.
usage: python tools/isa_mix.py file.s <mangled-name-substring> [--blocks] [--loop] [--md]
--loop: only the kernel's main loop (the widest span between a label and a backward branch to it: the tile loop of
the edge kernels), split by category -- what one trip of the loop holds when every conditional block in it runs;
--md prints that view as a table row set."""
import collections
import re
import sys

txt = open(sys.argv[1]).read()
key = sys.argv[2]
m = re.search(r"^(\S*" + re.escape(key) + r"\S*):", txt, re.M)
start = m.end()
end = txt.index(".Lfunc_end", start)
lines = txt[start:end].splitlines()


def cls(l):
    op = l.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_accvgpr"):
        return "accvgpr"
    if op.startswith("v_"):
        return "valu_dpp" if ("row_" in l or "quad_perm" in l or "dpp" in l) else "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_") or "scratch" in l:
        return "scratch"
    if op.startswith(("buffer_", "global_", "flat_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    return "salu"


blocks = []
cur = [None, collections.Counter()]
for l in lines:
    s = l.strip()
    if re.match(r"^\.LBB\S*:", s) or (s.endswith(":") and not s.startswith(";")):
        blocks.append(cur)
        cur = [s, collections.Counter()]
        continue
    if not s or s.startswith((";", ".")):
        continue
    cur[1][cls(s)] += 1
blocks.append(cur)
tot = collections.Counter()
for name, c in blocks:
    tot.update(c)
    if "--blocks" in sys.argv and sum(c.values()) > 20:
        print(name, dict(c))
print("total", dict(tot), sum(tot.values()))


# ---- the main loop only, per category ----
def cat(l):
    op = l.split()[0]
    dpp = "row_" in l or "quad_perm" in l or "_dpp" in op
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith("v_accvgpr"):
        return "accvgpr moves"
    if op.startswith(("v_permlane", "v_readlane", "v_readfirstlane", "v_writelane")):
        return "cross-lane"
    if op.startswith("v_"):
        if dpp:
            return "DPP"
        if op.startswith("v_fma_mix"):
            return "v_fma_mix*"
        if op.startswith("v_pk_"):
            return "packed"
        if op.startswith(("v_max", "v_min", "v_med3")):
            return "max / min"
        if op.startswith(("v_mov", "v_swap")):
            return "moves"
        if op.startswith(("v_cmp", "v_cndmask")):
            return "compare / select"
        return "other VALU"
    if op.startswith("ds_"):
        return "(LDS)"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "(VMEM)"
    if op.startswith("s_waitcnt"):
        return "(s_waitcnt)"
    if op.startswith("s_nop"):
        return "(s_nop)"
    return "(scalar)"


def main_loop(lines):
    """Line numbers of the kernel's main loop: the strongly connected component of its control-flow graph (basic
    blocks; fall-through and branch-target edges) that holds the most instructions. Blocks of the loop that the
    compiler laid out behind the backward branch are part of it."""
    starts, label_block = [0], {}
    for i, l in enumerate(lines):
        s = l.strip()
        m = re.match(r"^(\.LBB\S*):", s)
        if m:
            if starts[-1] != i:
                starts.append(i)
            label_block[m.group(1)] = len(starts) - 1
        elif re.match(r"^(s_c?branch|s_endpgm)", s) and i + 1 < len(lines):
            starts.append(i + 1)
    starts = sorted(set(starts))
    label_block = {}
    for b, st in enumerate(starts):
        m = re.match(r"^(\.LBB\S*):", lines[st].strip())
        if m:
            label_block[m.group(1)] = b
    ends = starts[1:] + [len(lines)]
    succ = []
    for b, (st, en) in enumerate(zip(starts, ends)):
        out, fall = [], True
        for l in lines[st:en]:
            s = l.strip()
            m = re.match(r"^(s_c?branch\S*)\s+(\.LBB\S+)", s)
            if m:
                out.append(label_block[m.group(2)])
                fall = m.group(1).startswith("s_cbranch")
            elif s.startswith("s_endpgm"):
                fall = False
        if fall and b + 1 < len(starts):
            out.append(b + 1)
        succ.append(out)
    # Tarjan, iterative
    index, low, on, stack, comps, n = {}, {}, set(), [], [], 0
    for root in range(len(starts)):
        if root in index:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = low[v] = n
                n += 1
                stack.append(v)
                on.add(v)
            if k < len(succ[v]):
                work.append((v, k + 1))
                w = succ[v][k]
                if w not in index:
                    work.append((w, 0))
                elif w in on:
                    low[v] = min(low[v], index[w])
                continue
            for w in succ[v]:
                if w in on:
                    low[v] = min(low[v], low[w])
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    comps.append(comp)
    def size(comp):
        return sum(1 for b in comp for l in lines[starts[b]:ends[b]]
                   if l.strip() and not l.strip().startswith((";", ".")) and not l.strip().endswith(":"))
    best = max(comps, key=size)
    return [i for b in sorted(best) for i in range(starts[b], ends[b])]


if "--loop" in sys.argv:
    body = main_loop(lines)
    c = collections.Counter()
    for l in (lines[i] for i in body):
        s = l.strip()
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        c[cat(s)] += 1
    valu = sum(v for k, v in c.items() if not k.startswith("(") and k != "MFMA")
    md = "--md" in sys.argv
    print(f"main loop: {sum(c.values())} instructions, {valu} vector-ALU (without MFMA)")
    if md:
        print("| category | per trip |\n|---|---|")
    for k, v in sorted(c.items(), key=lambda kv: (kv[0].startswith("("), -kv[1])):
        print(f"| {k} | {v} |" if md else f"{v:6d}  {k}")
