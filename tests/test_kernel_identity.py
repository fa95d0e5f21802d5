"""tools/kernel_identity.py: the device code of two csrc trees is compared kernel by kernel, whatever order the compiler
emits the kernels in.  Compiles hanet.hip (the smallest file) for gfx950; no GPU needed."""
import importlib.util
import os
import re
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pmt_learning_for_semantic_segmentation_and_disparity_amd", "csrc")

_spec = importlib.util.spec_from_file_location("kernel_identity", os.path.join(ROOT, "tools", "kernel_identity.py"))
ki = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ki)

SEED_MUL = "0x9E3779B97F4A7C15ULL"     # in dropout_channels_kernel only


def _block(text, first, nxt):
    a, b = text.index(first), text.index(nxt)
    assert a < b
    return a, b


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """hanet.hip as it is, with one constant of one kernel changed, with two kernels' launches trading places, and with one
    kernel under another name; each in a tree of its own (<tree>/pkg/csrc next to <tree>/include), compiled once."""
    src = open(os.path.join(CSRC, "hanet.hip")).read()
    assert src.count(SEED_MUL) == 1
    # the compiler emits template kernels in the order the host code first names them: trade the two entry points
    a, b = _block(src, 'extern "C" int sdhip_mul_rows_fwd(', 'extern "C" int sdhip_mul_rows_bwd(')
    c = src.index('extern "C" int sdhip_dropout_channels(')
    texts = {"same": src, "const": src.replace(SEED_MUL, "0x9E3779B97F4A7C17ULL"), "swap": src[:a] + src[b:c] + src[a:b] + src[c:],
             "rename": src.replace("zero_rows_kernel", "clear_rows_kernel")}
    assert src.count("zero_rows_kernel") == 2                         # the kernel and its one launch
    base = tmp_path_factory.mktemp("kernel_identity")
    dirs = {}
    for name, text in texts.items():
        d = base / name / "pkg" / "csrc"
        d.mkdir(parents=True)
        (base / name / "include").mkdir()
        shutil.copy(os.path.join(ROOT, "include", "sdhip.h"), base / name / "include" / "sdhip.h")
        shutil.copy(os.path.join(CSRC, "sdhip_common.h"), d / "sdhip_common.h")
        (d / "hanet.hip").write_text(text)
        dirs[name] = str(d)
    with ThreadPoolExecutor(max_workers=4) as ex:
        asm = dict(zip(dirs, ex.map(lambda d: ki.assemble(os.path.join(d, "hanet.hip"), os.path.join(d, "hanet.s")), dirs.values())))
    return dirs, asm


def test_a_file_is_identical_to_itself(variants, capsys):
    dirs, _ = variants
    assert ki.main([CSRC, dirs["same"], "hanet.hip"]) == 0
    out = capsys.readouterr().out
    m = re.search(r"hanet\.hip\s+kernels\s+(\d+), identical\s+(\d+)", out)
    assert m and int(m.group(1)) == int(m.group(2)) >= 10, out


def test_a_changed_constant_is_reported_with_its_kernels(variants, capsys):
    dirs, asm = variants
    n, same, bad = ki.compare_asm(asm["same"], asm["const"])
    assert n - same == 2 and len(bad) == 2, bad                      # the f32 and the bf16 instantiation
    assert all("dropout_channels_kernel" in b and "code" in b for b in bad), bad
    assert ki.main([dirs["same"], dirs["const"]]) == 1
    assert "dropout_channels_kernel" in capsys.readouterr().out


def test_kernels_that_trade_places_are_still_identical(variants):
    _, asm = variants
    order = lambda t: re.findall(r"^(\S+):\s*; @", t, re.M)
    assert order(asm["same"]) != order(asm["swap"]) and sorted(order(asm["same"])) == sorted(order(asm["swap"]))
    assert asm["same"] != asm["swap"]
    n, same, bad = ki.compare_asm(asm["same"], asm["swap"])
    assert n == same >= 10 and not bad, bad


def test_a_renamed_kernel_is_missing_without_rename_and_identical_with_it(variants, capsys):
    dirs, asm = variants
    n, same, bad = ki.compare_asm(asm["same"], asm["rename"])
    assert n - same == 2 and len(bad) == 4, bad                       # f32 and bf16, each only in A and only in B
    assert sum("zero_rows_kernel" in b and "only in A" in b for b in bad) == 2, bad
    assert sum("clear_rows_kernel" in b and "only in B" in b for b in bad) == 2, bad
    assert ki.main([dirs["same"], dirs["rename"]]) == 1
    assert "only in A" in capsys.readouterr().out
    # the new name is one letter longer: the count in front of it in the mangled symbol follows
    n, same, bad = ki.compare_asm(ki.rename(asm["same"], [("zero_rows_kernel", "clear_rows_kernel")]), asm["rename"])
    assert n == same >= 10 and not bad, bad
    assert ki.main([dirs["same"], dirs["rename"], "--rename", "zero_rows_kernel=clear_rows_kernel"]) == 0
    m = re.search(r"hanet\.hip\s+kernels\s+(\d+), identical\s+(\d+)", capsys.readouterr().out)
    assert m and int(m.group(1)) == int(m.group(2)) >= 10
