"""The C-ABI library loads and exports every symbol include/sdhip.h declares (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sdhip_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "pmt_learning_for_semantic_segmentation_and_disparity_amd", "libsdhip.so"))
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "libsdhip.so does not export %s" % n


def test_ctypes_signatures_cover_the_header():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    bound = set(_lib.SIGNATURES) | {"sdhip_abi_version", "sdhip_last_error", "sdhip_conv_packed_elems", "sdhip_lovasz_workspace_bytes", "sdhip_diag_reload", "sdhip_abort_capture", "sdhip_flip_sample_workspace_bytes", "sdhip_graph_node_counts", "sdhip_softargmin_bwd_workspace_floats"}
    assert set(_declared()) == bound, set(_declared()) ^ bound


def test_abi_version_and_error_channel():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    assert _lib.abi_version() >= 1
    # argument validation happens before any GPU work: a bad call returns an error code and a message, never aborts
    rc = _lib._lib.sdhip_corr_fwd(None, None, None, 1, 1, 1, 1, 1, 1, 17, 1, 17, 0, None)
    assert rc < 0 and b"null" in _lib._lib.sdhip_last_error()


def _fwd(_lib, x=ctypes.c_void_p(1 << 20), w=ctypes.c_void_p(2 << 20), y=ctypes.c_void_p(3 << 20), Cin=16, stream=None):
    """sdhip_conv2d_fwd, bf16 3x3 16 -> 16 on 2 x 9 x 19; by default with made-up 256-byte-aligned operand addresses."""
    return _lib._lib.sdhip_conv2d_fwd(x, w, y, None, None, None, None, 0, 1, 2, 9, 19, Cin, 16, 9, 19, 16, 16,
                                      3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 0, _lib.BF16, stream)


def test_dry_dispatch_names_a_kernel_without_a_gpu():
    """In dry mode an entry point validates and dispatches and launches nothing: on a machine without a GPU a launch attempt
    returns SDHIP_ERR_LAUNCH, so the 0 here shows there was none, and no made-up address was dereferenced."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    with _lib.dispatch_dry():
        assert _fwd(_lib) == 0 and _lib.last_path().startswith("fast(4x16"), _lib.last_path()
        assert _fwd(_lib, x=ctypes.c_void_p((1 << 20) + 2)) == 0 and _lib.last_path().startswith("generic("), _lib.last_path()     # x misaligned
        assert _fwd(_lib, Cin=0) == _lib.ERR_ARG and _lib.last_path() == ""                                                                                   # validation as usual
        P = [ctypes.c_void_p(i << 20) for i in range(1, 5)]
        assert _lib._lib.sdhip_conv2d_fwd_add(*P, 16, 2, 9, 19, 16, 16, 9, 19, 16, 16, 3, 3, 1, 1, _lib.BF16, None) == _lib.ERR_UNSUPPORTED
    assert _lib.last_path() == "unsupported"      # the name outlives the mode


def test_dry_mode_ends_with_its_block():
    """dispatch_dry() switches the flag off on the way out, by an exception too: the next call launches again — without a
    GPU that is an SDHIP_ERR_LAUNCH; with one it is run on real tensors and writes y."""
    import pytest
    import torch
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    with pytest.raises(KeyError):
        with _lib.dispatch_dry():
            assert _fwd(_lib) == 0
            raise KeyError("out")
    if not torch.cuda.is_available():
        assert _fwd(_lib) == _lib.ERR_LAUNCH
        return
    x, y = torch.zeros(2, 9, 19, 16, dtype=torch.bfloat16, device="cuda"), torch.full((2, 9, 19, 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(_lib.packed_elems(16, 16, 9, _lib.BF16), dtype=torch.bfloat16, device="cuda")
    assert _fwd(_lib, _lib.ptr(x), _lib.ptr(w), _lib.ptr(y), stream=_lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((y == 0).all()) and _lib.last_path().startswith("fast(4x16")


def test_product_has_no_cpu_path():
    import pytest
    import torch
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, SdhipError
    with pytest.raises(SdhipError):
        N.SpatialCorrelationSampler(1, (1, 17))(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4))


def test_phase_pack_rows_tile_the_eight_sub_kernels():
    """Host logic of the sub-pixel phases of a 3x3x3 stride-2 (transposed) convolution (ops._phase_rows: the descriptor rows the
    step's batched pack launch replays): the 27 single-tap rows read every tap of the parameter exactly once, in the order of
    ops._PHASE_INDEX, and their destinations tile the eight packed sub-kernels [depth tap][tap][Mpad][64] without gaps."""
    import torch
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, _lib
    w = torch.zeros(64, 32, 3, 3, 3)                       # ConvTranspose3d(64, 32) / the adjoint view of Conv3d(32 -> 64, stride 2)
    rows, spans = ops._phase_rows(w, _lib.BF16)
    assert [r[0] for r in rows] == ops._PHASE_INDEX and sorted(r[0] for r in rows) == list(range(27))
    blk = _lib.packed_elems(32, 64, 1, _lib.BF16)          # one tap: [Mpad = 32][64]
    assert blk == 32 * 64
    assert sorted(r[1] for r in rows) == [i * blk for i in range(27)]
    assert all(r[2:] == (32, 64, 1, 27, 32 * 27, 0) for r in rows)
    assert [n for _, n in spans] == [blk * (1 + pd) * (1 + ph) * (1 + pw) for (pd, ph, pw) in ops._PHASES]
    assert spans[0][0] == 0 and all(spans[i][0] + spans[i][1] == spans[i + 1][0] for i in range(7))


# ---- the binding is derived from include/sdhip.h (signatures, return types, constants) ----

def _header_text():
    return open(os.path.join(ROOT, "include", "sdhip.h")).read()


def _types(codes):
    table = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "d": ctypes.c_double}
    return [table[c] for c in codes.split()]


def test_derived_signatures_are_exactly_the_declared_functions():
    """The strict declaration grammar of _lib.parse_header finds every function the permissive name scan finds: a declaration
    it skipped (a new return type, say) fails here instead of becoming an unprototyped call."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    sigs, _ = _lib.parse_header(_header_text())
    assert set(sigs) == set(_declared()), set(sigs) ^ set(_declared())
    assert set(_lib.SIGNATURES) == set(sigs)
    for name, (ret, args) in sigs.items():
        fn = getattr(_lib._lib, name)
        assert list(fn.argtypes) == args == _lib.SIGNATURES[name] and fn.restype is ret, name


def test_pinned_derivations():
    """A few rows written out, so that every type code and every kind of return value is checked against the parser."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    S, L = _lib.SIGNATURES, _lib._lib
    assert S["sdhip_adam_step"] == _types("p p p p p l f f f f f f p")
    assert S["sdhip_bn_finalize"] == _types("p i i p p p p p p p p i i d f f p")
    assert S["sdhip_mt_seg_fwd"] == _types("p i p p p p p p l i i f i p")                 # const int64_t* labels is a pointer
    assert S["sdhip_mt_l1_bwd"] == _types("p i p p p l p f p i p l i p")                  # long g_stride, long n
    assert S["sdhip_conv2d_wgrad_group"] == _types("p i i i p")                           # const SdhipWgradItem* items
    assert S["sdhip_dropout"] == _types("p p p l l f i p")                                # const long* seed is a pointer
    assert S["sdhip_maxpool3s2_fwd"] == _types("p i p i p i i i i i p")                   # unsigned char* idx
    assert S["sdhip_graph_node_counts"] == _types("p p") and S["sdhip_abort_capture"] == _types("p")
    for name, codes in (("sdhip_conv_packed_elems", "i i i i"), ("sdhip_lovasz_workspace_bytes", "l i"),
                        ("sdhip_softargmin_bwd_workspace_floats", "i i i i i i i"), ("sdhip_flip_sample_workspace_bytes", "i i i")):
        assert S[name] == _types(codes) and getattr(L, name).restype is ctypes.c_long, name
    assert L.sdhip_adam_step.restype is ctypes.c_int and L.sdhip_seg_terms_workspace_bytes.restype is ctypes.c_int
    assert L.sdhip_last_error.restype is ctypes.c_char_p and S["sdhip_last_error"] == []
    assert L.sdhip_diag_reload.restype is None and S["sdhip_diag_reload"] == []
    assert L.sdhip_abi_version.restype is ctypes.c_int and S["sdhip_abi_version"] == []
    assert L.sdhip_dispatch_dry.restype is None and S["sdhip_dispatch_dry"] == _types("i")
    assert L.sdhip_last_path.restype is ctypes.c_char_p and S["sdhip_last_path"] == []


def test_unknown_types_raise():
    import pytest
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    ok = "/* c */\nint sdhip_fine(const void* x, long n,\n               void* stream);\n"
    assert _lib.parse_header(ok)[0] == {"sdhip_fine": (ctypes.c_int, _types("p l p"))}
    with pytest.raises(_lib.SdhipError, match=r"sdhip_bad_param.*size_t n"):
        _lib.parse_header(ok + "int sdhip_bad_param(const void* x, size_t n,\n                    void* stream);\n")
    with pytest.raises(_lib.SdhipError, match=r"sdhip_bad_ret.*size_t"):
        _lib.parse_header(ok + "size_t sdhip_bad_ret(const void* x, int n,\n                     void* stream);\n")
    with pytest.raises(_lib.SdhipError, match=r"sdhip_bad_ret"):
        _lib.parse_header(ok + "float sdhip_bad_ret(int n);\n")
    with pytest.raises(_lib.SdhipError, match=r"sdhip_unsigned.*unsigned n"):
        _lib.parse_header("int sdhip_unsigned(unsigned n);\n")                            # a type without a parameter name is no default int


def test_call_refuses_an_undeclared_name(monkeypatch):
    import pytest
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the library was asked for %s" % name)

    monkeypatch.setattr(_lib, "_lib", Untouchable())
    for f in (_lib.call, _lib.try_call):
        with pytest.raises(_lib.SdhipError, match="sdhip_no_such_entry"):
            f("sdhip_no_such_entry")


def test_constants_come_from_the_header():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, data, metrics
    want = {"SDHIP_F32": 0, "SDHIP_BF16": 1, "SDHIP_OK": 0, "SDHIP_ERR_ARG": -1, "SDHIP_ERR_LAUNCH": -2, "SDHIP_ERR_UNSUPPORTED": -3,
            "SDHIP_ACT_HSWISH": 5, "SDHIP_ACT_HSIGMOID": 6, "SDHIP_SEG_TVERSKY": 1, "SDHIP_SEG_DICE": 2, "SDHIP_SEG_DICE_ENTROPY": 4,
            "SDHIP_METRIC_COUNTS": 10, "SDHIP_METRIC_SUMS": 4, "SDHIP_METRIC_SUM_STRIDE": 32,
            "SDHIP_SEG_THRESHOLD": 0, "SDHIP_SEG_ID_PLUS_ONE": 1, "SDHIP_SEG_LUT": 2, "SDHIP_DEPTH_PFM": 0, "SDHIP_DEPTH_U16": 1,
            "SDHIP_ACT_LINEAR": 0, "SDHIP_ACT_SIGMOID": 1, "SDHIP_ACT_TANH": 2}
    C = _lib.CONSTANTS
    assert {k: C[k] for k in want} == want
    assert set(C) == set(re.findall(r"#define\s+(SDHIP_[A-Z0-9_]*[A-Z0-9])\s+\S", _header_text())), "a #define the binding did not read"
    assert (_lib.F32, _lib.BF16) == (0, 1) and (_lib.ERR_ARG, _lib.ERR_LAUNCH, _lib.ERR_UNSUPPORTED) == (-1, -2, -3)
    assert (_lib.ACT_HSWISH, _lib.ACT_HSIGMOID) == (5, 6) and (_lib.SEG_TVERSKY, _lib.SEG_DICE, _lib.SEG_DICE_ENTROPY) == (1, 2, 4)
    assert (metrics.N_COUNTS, metrics.N_SUMS, metrics.SUM_STRIDE) == (C["SDHIP_METRIC_COUNTS"], C["SDHIP_METRIC_SUMS"], C["SDHIP_METRIC_SUM_STRIDE"])
    assert (data.SEG_THRESHOLD, data.SEG_ID_PLUS_ONE, data.SEG_LUT, data.DEPTH_PFM, data.DEPTH_U16) == (0, 1, 2, 0, 1)
    assert data.ACTIVATIONS == {"linear": 0, "sigmoid": 1, "tanh": 2}


def test_wgrad_item_matches_the_typedef():
    """_lib.WgradItem is written by hand; its member names, order and kinds are those of the typedef's body: the pointer
    members first, then the `int` list."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    body = re.search(r"typedef\s+struct\s+SdhipWgradItem\s*\{(.*?)\}\s*SdhipWgradItem\s*;", _header_text(), flags=re.S).group(1)
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        if "*" in stmt:
            fields.append((stmt.split("*")[-1].strip(), ctypes.c_void_p))
        else:
            kind, names = stmt.split(None, 1)
            assert kind == "int", stmt
            fields += [(n.strip(), ctypes.c_int) for n in names.split(",")]
    assert len(fields) == 28 and [k for _, k in fields] == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 22
    assert list(_lib.WgradItem._fields_) == fields
    assert ctypes.sizeof(_lib.WgradItem) == 6 * 8 + 22 * 4
