"""ctypes binding of libsdhip.so — the only way the package reaches the GPU.

There is no CPU or eager-PyTorch fallback: if the shared library is missing or
fails to load, importing this module raises.  `import torch` happens first on
purpose: libsdhip.so needs `libamdhip64.so.7` by soname and must bind to the HIP
runtime PyTorch-ROCm has already mapped, so that stream handles and device
pointers are shared between the two.

include/sdhip.h is the only copy of the ABI: the argument and return types of every
entry point (`SIGNATURES`) and the numeric constants (`CONSTANTS`) are read from it at
import.  A new entry point is declared there, defined in csrc/ and called; nothing is
added here.
"""
import contextlib
import ctypes
import os
import re

import torch  # noqa: F401  (must precede the dlopen below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsdhip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "sdhip.h")

NREP = int(os.environ.get("SDHIP_TUNE_NREP", "32"))   # statistics replicas the kernels spread their atomics over (env: tuning only)


class SdhipError(RuntimeError):
    pass


_ARG_TYPES = {"*": ctypes.c_void_p, "int": ctypes.c_int, "long": ctypes.c_long, "int64_t": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
_RET_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "void": None, "const char*": ctypes.c_char_p}


def parse_header(text):
    """(signatures, constants) of the text of include/sdhip.h: {name: (restype, [argtypes])} of every
    `<ret> sdhip_<name>(<params>);` and {name: value} of every `#define SDHIP_<NAME> <integer>`.  A parameter is mapped by
    its type alone (any pointer is a c_void_p); a type this does not know raises — ctypes' silent `int` is never assumed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {n: int(v) for n, v in re.findall(r"^[ \t]*#define[ \t]+(SDHIP_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    sigs = {}
    for ret, name, params in re.findall(r"^([\w \t*]+?)\s*\b(sdhip_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        ret = re.sub(r"\s*\*\s*", "*", " ".join(ret.split()))
        if ret not in _RET_TYPES:
            raise SdhipError("sdhip.h: %s has return type '%s', which the binding cannot classify" % (name, ret))
        args = []
        for par in ([] if params.strip() == "void" else params.split(",")):
            ctype = "*" if "*" in par else " ".join(w for w in par.split()[:-1] if w != "const")
            if ctype not in _ARG_TYPES:
                raise SdhipError("sdhip.h: %s has parameter '%s', which the binding cannot classify" % (name, " ".join(par.split())))
            args.append(_ARG_TYPES[ctype])
        sigs[name] = (_RET_TYPES[ret], args)
    return sigs, consts


if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libsdhip.so not found at %s — run `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc, gfx950). This package has no fallback path." % LIB_PATH)
if not os.path.exists(HEADER_PATH):
    raise ImportError(
        "sdhip.h not found at %s — the binding reads every signature and constant of libsdhip.so from it. "
        "This package has no fallback path." % HEADER_PATH)

_lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)

with open(HEADER_PATH) as _f:
    _SIGS, CONSTANTS = parse_header(_f.read())
SIGNATURES = {_name: _args for _name, (_ret, _args) in _SIGS.items()}    # name -> argtypes of every declared entry point
for _name, (_ret, _args) in _SIGS.items():
    _fn = getattr(_lib, _name)
    _fn.argtypes = _args
    _fn.restype = _ret

F32, BF16 = CONSTANTS["SDHIP_F32"], CONSTANTS["SDHIP_BF16"]
ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = CONSTANTS["SDHIP_ERR_ARG"], CONSTANTS["SDHIP_ERR_LAUNCH"], CONSTANTS["SDHIP_ERR_UNSUPPORTED"]
ACT_HSWISH, ACT_HSIGMOID = CONSTANTS["SDHIP_ACT_HSWISH"], CONSTANTS["SDHIP_ACT_HSIGMOID"]    # MobileNetV3's hard activations
SEG_TVERSKY, SEG_DICE, SEG_DICE_ENTROPY = CONSTANTS["SDHIP_SEG_TVERSKY"], CONSTANTS["SDHIP_SEG_DICE"], CONSTANTS["SDHIP_SEG_DICE_ENTROPY"]


class WgradItem(ctypes.Structure):
    """SdhipWgradItem of include/sdhip.h: written out here (tests/test_abi.py holds the field order against the typedef)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("x", "dy", "dw_packed", "dbias", "in_scale", "in_shift")] + \
               [(n, ctypes.c_int) for n in ("B", "H", "W", "Cin", "ldx", "Ho", "Wo", "Cout", "lddy", "kh", "kw", "stride", "dil", "pad_t",
                                            "pad_l", "D", "Do", "kd", "sd", "pad_d", "in_relu", "groups")]


class PyrMap(ctypes.Structure):
    """SdhipPyrMap of include/sdhip.h: one branch map of a pyramid (tests/test_pyramid.py holds it against the typedef)."""
    _fields_ = [("p", ctypes.c_void_p)] + [(n, ctypes.c_int) for n in ("h", "w", "ld", "reserved")]


def pyr_maps(entries):
    """HOST table of the sdhip_pyramid_* entry points: entries = [(tensor, h, w, ld), ...].
    -> (the argument, the array that must outlive the call)."""
    t = (PyrMap * len(entries))()
    for e, (m, h, w, ld) in zip(t, entries):
        e.p, e.h, e.w, e.ld = m.data_ptr(), h, w, ld
    return ctypes.cast(t, ctypes.c_void_p), t


def lovasz_workspace_bytes(npix, C):
    return _lib.sdhip_lovasz_workspace_bytes(npix, C)


def seg_terms_workspace_bytes(B, hw, C):
    """Workspace of sdhip_seg_sums / sdhip_seg_finish / sdhip_seg_terms_bwd for this shape (include/sdhip.h)."""
    n = _lib.sdhip_seg_terms_workspace_bytes(B, hw, C)
    if n <= 0:
        raise SdhipError("sdhip_seg_terms_workspace_bytes: unsupported shape (B %d, %d pixels, C %d; C <= 32)" % (B, hw, C))
    return n


def disp_smooth_workspace_bytes(B, H, W):
    """Workspace of sdhip_disp_smooth for this shape (include/sdhip.h)."""
    n = _lib.sdhip_disp_smooth_workspace_bytes(B, H, W)
    if n <= 0:
        raise SdhipError("sdhip_disp_smooth_workspace_bytes: unsupported shape (B %d, H %d, W %d)" % (B, H, W))
    return n


def edge_bce_workspace_bytes(n):
    """Workspace of sdhip_edge_bce for n elements (include/sdhip.h)."""
    nbytes = _lib.sdhip_edge_bce_workspace_bytes(n)
    if nbytes <= 0:
        raise SdhipError("sdhip_edge_bce_workspace_bytes: unsupported element count %d" % n)
    return nbytes


def photo_mse_workspace_bytes(npix):
    """Workspace of sdhip_photo_mse for npix pixels (include/sdhip.h)."""
    nbytes = _lib.sdhip_photo_mse_workspace_bytes(npix)
    if nbytes <= 0:
        raise SdhipError("sdhip_photo_mse_workspace_bytes: unsupported pixel count %d" % npix)
    return nbytes


def dw_pool_parts(H, W, C, k, stride, dt):
    """Pool slots of sdhip_dw_conv_fwd for this input (include/sdhip.h)."""
    n = _lib.sdhip_dw_pool_parts(H, W, C, k, stride, dt)
    if n <= 0:
        raise SdhipError("sdhip_dw_pool_parts: unsupported depthwise shape")
    return n


def dw_wgrad_parts(B, H, W, C, k, stride):
    """Partial slots of sdhip_dw_conv_wgrad for this shape (include/sdhip.h)."""
    n = _lib.sdhip_dw_wgrad_parts(B, H, W, C, k, stride)
    if n <= 0:
        raise SdhipError("sdhip_dw_wgrad_parts: unsupported depthwise shape")
    return n


def packed_elems(M, K, T, dt):
    return _lib.sdhip_conv_packed_elems(M, K, T, dt)


def graph_node_counts(graph):
    """{kernel, memset, memcpy, other, total} of a torch.cuda.CUDAGraph created with keep_graph=True."""
    c = (ctypes.c_int * 4)()
    n = _lib.sdhip_graph_node_counts(ctypes.c_void_p(graph.raw_cuda_graph()), c)
    if n < 0:
        raise SdhipError("sdhip_graph_node_counts failed: %s" % _lib.sdhip_last_error().decode())
    return {"kernel": c[0], "memset": c[1], "memcpy": c[2], "other": c[3], "total": n}


def abort_capture(stream):
    """End a broken hipGraph capture on `stream` (a torch.cuda.Stream); returns 1 if one was open (see include/sdhip.h)."""
    rc = _lib.sdhip_abort_capture(ctypes.c_void_p(stream.cuda_stream))
    if rc < 0:
        raise SdhipError("sdhip_abort_capture failed: %s" % _lib.sdhip_last_error().decode())
    return rc


def reload_diag():
    """Re-read the SDHIP_* diagnostic environment switches (they are otherwise fixed at library load)."""
    _lib.sdhip_diag_reload()


@contextlib.contextmanager
def dispatch_dry():
    """While active on this thread the convolution entry points validate and dispatch as usual and launch nothing
    (sdhip_dispatch_dry of include/sdhip.h): `with dispatch_dry(): call(...)`, then `last_path()`."""
    _lib.sdhip_dispatch_dry(1)
    try:
        yield
    finally:
        _lib.sdhip_dispatch_dry(0)


def last_path():
    """Name of the kernel the last convolution entry point on this thread chose, dry or real (sdhip_last_path)."""
    return _lib.sdhip_last_path().decode()


def _diag_switch(name):
    """Python-side diagnostic switches are read once, at import, and announced."""
    v = os.environ.get(name)
    if v:
        import sys
        sys.stderr.write("[sdhip] diagnostic switch %s=%s is set: this is not the production path\n" % (name, v))
    return v


DIAG_NO_FUSED_BN = bool(_diag_switch("SDHIP_DIAG_NO_FUSED_BN"))
DIAG_NO_SIDE = bool(_diag_switch("SDHIP_DIAG_NO_SIDE"))
DIAG_NO_GRAD_SLOTS = bool(_diag_switch("SDHIP_DIAG_NO_GRAD_SLOTS"))
DIAG_NO_WGRAD_GROUP = bool(_diag_switch("SDHIP_DIAG_NO_WGRAD_GROUP"))
DIAG_NO_PHASE_DGRAD = bool(_diag_switch("SDHIP_DIAG_NO_PHASE_DGRAD"))     # data gradient of stride-2 3-D convolutions over the zero-stuffed dY (A/B)
TUNE_WGRAD_OVERLAP = bool(_diag_switch("SDHIP_TUNE_WGRAD_OVERLAP"))     # measured and not kept as a default: see train.TrainStep
TUNE_OVERLAP_WG = int(_diag_switch("SDHIP_TUNE_OVERLAP_WG") or 128)
DIAG_NO_BN_SLOTS = bool(_diag_switch("SDHIP_DIAG_NO_BN_SLOTS"))
TUNE_FUSE1_MAX_PIX = int(_diag_switch("SDHIP_TUNE_FUSE1_MAX_PIX") or 32768)
TUNE_PRO_MAX_PIX = int(_diag_switch("SDHIP_TUNE_PRO_MAX_PIX") or 32768)
TUNE_BN_SLOT_MAX_MB = int(_diag_switch("SDHIP_TUNE_BN_SLOT_MAX_MB") or 40)
_forms = _diag_switch("SDHIP_TUNE_BAND_BX_FORMS")                          # "5x5,3x3" / "5x5" / "3x3" / "none" (A/B: the forms of the persistent kernel ops._conv_backward keeps)
TUNE_BAND_BX_FORMS = "5x5,3x3" if _forms is None else ("" if _forms == "none" else _forms)
del _forms
DIAG_NO_BNPRO = bool(_diag_switch("SDHIP_DIAG_NO_BNPRO"))
DIAG_NO_BNBWD_EPILOGUE = bool(_diag_switch("SDHIP_DIAG_NO_BNBWD_EPILOGUE"))
DIAG_STEM_S2D = _diag_switch("SDHIP_STEM_S2D")
DIAG_NO_PYRAMID_FUSE = bool(_diag_switch("SDHIP_DIAG_NO_PYRAMID_FUSE"))   # pyramids composed from single-tensor nodes, the unread b0 slab written (A/B)


def abi_version():
    return _lib.sdhip_abi_version()


def call(name, *args, unsupported_ok=False):
    """Invoke a C entry point; raise SdhipError with the library's message on failure."""
    if name not in SIGNATURES:
        raise SdhipError("%s is not declared in include/sdhip.h" % name)
    rc = getattr(_lib, name)(*args)
    if rc != 0 and not (unsupported_ok and rc == ERR_UNSUPPORTED):
        raise SdhipError("%s failed (%d): %s" % (name, rc, _lib.sdhip_last_error().decode()))
    return rc == 0


def try_call(name, *args):
    """`call` for an entry point that may decline its arguments: True = it ran, False = it answered ERR_UNSUPPORTED
    (nothing was launched; the caller takes its other route).  Any other failure raises as in `call`."""
    return call(name, *args, unsupported_ok=True)


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise SdhipError("unsupported dtype %s (f32 and bf16 only)" % t.dtype)


def code_of(dtype):      # of a step's activation dtype (a torch.dtype; anything but bf16 is the f32 path)
    return BF16 if dtype == torch.bfloat16 else F32


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
