"""Where do a kernel's global loads stand relative to its waits?  (no GPU needed)
  python tools/kernel_loads.py <csrc dir | file.hip | file.s> [kernel pattern]
A csrc directory or a .hip file is compiled to gfx950 device assembly with the flags of build.py, as tools/kernel_identity.py
does; a .s file is read as it is.  Per kernel whose demangled name matches the pattern (a regular expression) it prints the
registers and scratch of the descriptor, then one line for the code outside every loop and one per loop (a cycle of the
control-flow graph; nested loops are indented, a loop's counts exclude the loops inside it):
  loads   global_load instructions in that code
  first   how many of them are issued before the first `s_waitcnt vmcnt`
  most    the most that are issued between two `s_waitcnt vmcnt` (or the region's ends)
A `vmcnt(N)` with N no smaller than the loads issued since the last wait that counted (or with none issued yet) is not
counted: it leaves all of them in flight and waits for older work (the stores of the previous trip share the counter).
A streaming loop that issues a whole trip before it waits shows loads == first == most; one that waits for every load
shows most == 1.  The counts follow the text order of the instructions, which is the issue order inside a basic block."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_kernel_identity", os.path.join(HERE, "kernel_identity.py"))
ident = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ident)


def descriptors(text):
    """{symbol: (vgprs, scratch bytes)} from the .amdhsa_kernel blocks"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        g = lambda key: int(re.search(key + r"\s+(\d+)", m.group(2)).group(1)) if re.search(key + r"\s+(\d+)", m.group(2)) else -1
        out[m.group(1)] = (g(r"\.amdhsa_next_free_vgpr"), g(r"\.amdhsa_private_segment_fixed_size"))
    return out


def blocks_of(lines):
    """basic blocks [(first line, last line)] and their successors, from labels and s_branch / s_cbranch instructions"""
    starts = {0}
    for i, ln in enumerate(lines):
        if re.match(r"\.LBB_\d+:", ln):
            starts.add(i)
        elif re.match(r"\s*(s_c?branch\S*|s_endpgm)\b", ln) and i + 1 < len(lines):
            starts.add(i + 1)
    first = sorted(starts)
    blocks = [(a, (first[n + 1] if n + 1 < len(first) else len(lines)) - 1) for n, a in enumerate(first)]
    at = {}
    for n, (a, _) in enumerate(blocks):
        m = re.match(r"(\.LBB_\d+):", lines[a])
        if m:
            at[m.group(1)] = n
    succ = []
    for n, (_, b) in enumerate(blocks):
        m = re.match(r"\s*(s_c?branch\S*)\s+(\.LBB_\d+)", lines[b])
        out = []
        if m and m.group(2) in at:
            out.append(at[m.group(2)])
        if not re.match(r"\s*(s_branch|s_endpgm)\b", lines[b]) and n + 1 < len(blocks):
            out.append(n + 1)
        succ.append(out)
    return blocks, succ


def sccs(nodes, succ):
    """strongly connected components of the sub-graph `nodes` that hold a cycle (Tarjan, iterative)"""
    nodes = set(nodes)
    index, low, on, stack, out, k = {}, {}, set(), [], [], [0]
    for root in sorted(nodes):
        if root in index:
            continue
        work = [(root, iter([s for s in succ[root] if s in nodes]))]
        index[root] = low[root] = k[0]; k[0] += 1; stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = k[0]; k[0] += 1; stack.append(w); on.add(w)
                    work.append((w, iter([s for s in succ[w] if s in nodes])))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = stack.pop(); on.discard(w); comp.append(w)
                        if w == v:
                            break
                    if len(comp) > 1 or v in succ[v]:
                        out.append(sorted(comp))
    return sorted(out)


def loops_of(lines):
    """[(depth, header block, its own blocks without those of inner loops)]: the cycles of the control-flow graph, an inner
    loop being a cycle that remains once the header (the first block in text order) of the enclosing one is taken away"""
    blocks, succ = blocks_of(lines)
    found = []

    def walk(nodes, depth):
        for comp in sccs(nodes, succ):
            mine = len(found)
            found.append(None)
            inner_before = len(found)
            walk(comp[1:], depth + 1)
            inner = set(b for f in found[inner_before:] for b in f[3])
            found[mine] = (depth, comp[0], [b for b in comp if b not in inner], comp)
    walk(range(len(blocks)), 1)
    return blocks, [(d, h, own) for d, h, own, _ in found]


def count(lines, idx):
    """(loads, before the first vmcnt wait, most between two vmcnt waits) over the lines idx, in order"""
    loads = run = most = 0
    first = None
    for i in idx:
        ln = lines[i]
        if re.match(r"\s*global_load_", ln):
            loads += 1
            run += 1
            most = max(most, run)
        elif re.match(r"\s*s_waitcnt\b.*vmcnt", ln):
            m = re.search(r"vmcnt\((\d+)\)", ln)
            if run == 0 or (m and int(m.group(1)) >= run):   # leaves all loads of this run in flight: it waits for older work
                continue
            if first is None:
                first = run
            run = 0
    return loads, loads if first is None else first, most


def outline(body):
    lines = body.splitlines()
    blocks, loops = loops_of(lines)
    span = lambda bs: [i for n in bs for i in range(blocks[n][0], blocks[n][1] + 1)]
    in_loop = set(n for _, _, own in loops for n in own)
    rows = [("outside loops", 0, count(lines, span([n for n in range(len(blocks)) if n not in in_loop])))]
    for depth, head, own in loops:
        label = re.match(r"(\.LBB_\d+):", lines[blocks[head][0]])
        idx = span(own)
        rows.append(("loop %s (%d instructions)" % (label.group(1) if label else "@%d" % blocks[head][0], len(idx)), depth, count(lines, idx)))
    return rows


def demangle(names):
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::", "", n).split("(")[0].replace("void ", "") for n in out]


def report(text, pattern):
    funcs, _, meta = ident.split_asm(text)
    desc = descriptors(text)
    syms = [s for s in funcs if s in meta]
    for name, sym in sorted(zip(demangle(syms), syms)):
        if pattern and not re.search(pattern, name):
            continue
        v, scratch = desc.get(sym, (-1, -1))
        print("%s   vgpr %d scratch %d" % (name, v, scratch))
        for what, ind, (loads, first, most) in outline(funcs[sym]):
            if loads or ind == 0:
                print("  %s%-40s loads %3d  first %3d  most %3d" % ("  " * ind, what, loads, first, most))


def main(argv):
    if not argv:
        sys.exit(__doc__)
    src, pattern = argv[0], argv[1] if len(argv) > 1 else ""
    if src.endswith(".s"):
        with open(src) as f:
            texts = [(os.path.basename(src), f.read())]
    else:
        files = [src] if src.endswith(".hip") else sorted(os.path.join(src, f) for f in os.listdir(src) if f.endswith(".hip"))
        with tempfile.TemporaryDirectory() as tmp:
            with ThreadPoolExecutor(max_workers=6) as ex:
                asm = list(ex.map(lambda f: ident.assemble(f, os.path.join(tmp, os.path.basename(f)[:-4] + ".s")), files))
        texts = [(os.path.basename(f), a) for f, a in zip(files, asm)]
    for name, text in texts:
        print("== %s" % name)
        report(text, pattern)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
