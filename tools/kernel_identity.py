"""Is the gfx950 device code of two csrc directories the same, kernel by kernel?  (no GPU needed)
  python tools/kernel_identity.py CSRC_A CSRC_B [--rename OLD=NEW ...] [file.hip ...]
Every .hip of both directories is compiled to device assembly with the flags of build.py.  The compiler emits template
instantiations in the order the host code first names them, so the files are not compared as a whole: per file, the set
of symbols, each function's instructions, each kernel's descriptor block and each kernel's metadata entry (registers,
LDS, scratch, kernarg layout) must match.  Each directory keeps its place in a tree (it finds ../../include/sdhip.h).
A kernel that B calls by another name is compared all the same with --rename OLD=NEW (repeatable): OLD, a substring of
A's mangled symbols, is written as NEW in A's assembly before the comparison.
Prints `<file>: kernels N, identical N` per file; exits 1 and names the symbols on any difference."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location(
    "_sdhip_build", os.path.join(ROOT, "pmt_learning_for_semantic_segmentation_and_disparity_amd", "build.py"))
build = importlib.util.module_from_spec(_spec)   # by path: the package itself needs a built libsdhip.so
_spec.loader.exec_module(build)


def assemble(src, out):
    cmd = [build.HIPCC] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("hipcc failed on %s\n%s" % (src, r.stderr))
    with open(out) as f:
        return f.read()


def rename(text, pairs):
    """The assembly with every OLD of `pairs` [(OLD, NEW), ...] written as NEW.  A mangled symbol counts the letters of each
    identifier in front of it (`16slot_fold_kernel`): where OLD is a whole identifier that count follows the name."""
    for old, new in pairs:
        text = text.replace("%d%s" % (len(old), old), "%d%s" % (len(new), new)).replace(old, new)
    return text


def _code(line):
    """The line without its comment and trailing blanks."""
    return line.split(";", 1)[0].rstrip()


def split_asm(text):
    """-> (functions {symbol: text}, descriptors {symbol: text}, metadata {symbol: text})"""
    funcs, desc, meta = {}, {}, {}
    lines = text.splitlines()
    sym = body = None
    for ln in lines:
        m = re.match(r"(\S+):\s*; @(\S+)\s*$", ln)
        if sym is None:
            if m and m.group(1) == m.group(2) and not ln.startswith("__hip_cuid"):
                sym, body = m.group(1), []
            continue
        if re.match(r"\.Lfunc_end\d+:", ln):
            # .LBB<n>_<m>: <n> is the function's position in the file
            txt = "\n".join(c for c in map(_code, body) if c)
            funcs[sym] = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", txt)
            k = re.search(r"^\s*\.amdhsa_kernel .*?^\s*\.end_amdhsa_kernel", funcs[sym], re.M | re.S)
            if k:
                desc[sym] = k.group(0)
            sym = None
        else:
            body.append(ln)
    md = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", text, re.M | re.S)
    for entry in re.split(r"^  - ", md.group(1) if md else "", flags=re.M)[1:]:
        meta[re.search(r"\.name:\s+(\S+)", entry).group(1)] = entry
    return funcs, desc, meta


def compare_asm(a, b):
    """-> (number of kernels in a, number identical, [complaints])"""
    (fa, da, ma), (fb, db, mb) = split_asm(a), split_asm(b)
    bad = {}
    for s in sorted(set(fa) ^ set(fb)):
        bad[s] = "only in %s" % ("A" if s in fa else "B")
    for s in sorted(set(ma) ^ set(mb)):
        bad.setdefault(s, "kernel metadata only in %s" % ("A" if s in ma else "B"))
    for s in sorted(set(fa) & set(fb)):
        what = [n for n, x, y in (("code", fa, fb), ("descriptor", da, db), ("metadata", ma, mb)) if x.get(s) != y.get(s)]
        if what:
            bad[s] = ", ".join(what) + " differ"
    return len(ma), sum(1 for s in ma if s not in bad), ["%s: %s" % (s, w) for s, w in sorted(bad.items())]


def compare_dirs(dir_a, dir_b, only=(), renames=()):
    """-> {file: (kernels, identical, [complaints])} over the .hip files of both directories"""
    names = [set(f for f in os.listdir(d) if f.endswith(".hip")) for d in (dir_a, dir_b)]
    res = {f: (0, 0, ["file only in %s" % ("A" if f in names[0] else "B")]) for f in names[0] ^ names[1] if not only or f in only}
    both = sorted(f for f in names[0] & names[1] if not only or f in only)
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(os.path.join(d, f), os.path.join(tmp, "%s_%s.s" % (f[:-4], tag))) for f in both for d, tag in ((dir_a, "a"), (dir_b, "b"))]
        with ThreadPoolExecutor(max_workers=6) as ex:
            asm = list(ex.map(lambda j: assemble(*j), jobs))
    for i, f in enumerate(both):
        res[f] = compare_asm(rename(asm[2 * i], renames), asm[2 * i + 1])
    return res


def main(argv):
    argv, renames = list(argv), []
    while "--rename" in argv:
        i = argv.index("--rename")
        if i + 1 >= len(argv) or not all(argv[i + 1].partition("=")[::2]):
            sys.exit("--rename takes OLD=NEW")
        renames.append(tuple(argv[i + 1].split("=", 1)))
        del argv[i:i + 2]
    if len(argv) < 2:
        sys.exit(__doc__)
    res = compare_dirs(argv[0], argv[1], argv[2:], renames)
    ok = True
    for f in sorted(res):
        n, same, bad = res[f]
        print("%-16s kernels %3d, identical %3d" % (f, n, same))
        for b in bad:
            print("    " + b)
        ok = ok and not bad
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
