"""1x1 weight-gradient shapes of the DenseNet towers (GEMM-like: few pixels, many channels).

  python tools/gpu_wgrad1x1.py            per-shape timing through ops._wgrad_impl (all launches of a call)
  python tools/gpu_wgrad1x1.py blocks     the DenseNet-121 tower of the headline step (both towers as one batch of 16 images,
                                          512x256 input): every block's bottlenecks and the three transitions as grouped calls
                                          (sdhip_conv2d_wgrad_group), the GEMM kernel of csrc/conv_wgrad_gemm1x1.h against the
                                          kernels it replaces (SDHIP_WGRAD_NO_GEMM=1), and a sweep of its cost-model constant
                                          (SDHIP_TUNE_WG1_TILE scales t_tile_us of plan_wg1)
"""
import ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, _lib
dtype = torch.bfloat16


def per_shape():
    shapes = [(16, 16, 32, 1024, 128, 1), (16, 16, 32, 1024, 512, 1), (16, 32, 64, 512, 128, 1), (16, 32, 64, 512, 256, 1),
              (16, 64, 128, 256, 128, 1), (16, 64, 128, 192, 128, 1), (16, 64, 128, 128, 128, 0), (8, 64, 128, 512, 128, 0),
              (16, 8, 16, 1024, 128, 1), (16, 128, 256, 64, 128, 0)]
    for (B, H, W, Cin, Cout, pro) in shapes:
        x = torch.randn(B, H, W, Cin, device="cuda").to(dtype).permute(0, 3, 1, 2)
        g = (torch.randn(B, H, W, Cout, device="cuda") * 0.1).to(dtype).permute(0, 3, 1, 2)
        w = torch.zeros(Cout, Cin, 1, 1, device="cuda")
        sc = (torch.rand(1, Cin, device="cuda") + 0.5) if pro else None
        sh = (torch.rand(1, Cin, device="cuda") - 0.5) if pro else None
        spec = ops.ConvSpec('conv', 1, 1, 1, 1, 0, 0, H, W)
        for _ in range(3):
            ops._wgrad_impl(x, Cin, g, Cout, w, None, spec, sc, sh, bool(pro), 1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops._wgrad_impl(x, Cin, g, Cout, w, None, spec, sc, sh, bool(pro), 1)
        e1.record()
        torch.cuda.synchronize()
        npix = B * H * W
        ideal = max(2.0 * npix * Cin * Cout / 2.5e15, (npix * (Cin + Cout) * 2.0) / 8e12) * 1e6
        print("B%d %dx%d %4d->%3d pro%d: %.1f us per call (all launches), ideal %.1f us" % (B, H, W, Cin, Cout, pro, e0.elapsed_time(e1) * 50, ideal), flush=True)


def switches(**env):
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    _lib.reload_diag()


class Group:
    """Layers (Cin -> Cout on the prefix of ONE [B][H][W][ldx] slab, two statistics groups) as one grouped call."""

    def __init__(self, B, H, W, ldx, layers):
        self.keep = []
        slab = torch.randn(B, H, W, ldx, device="cuda").to(dtype)
        self.items = (_lib.WgradItem * len(layers))()
        names = [f[0] for f in _lib.WgradItem._fields_]
        for it, (Cin, Cout) in zip(self.items, layers):
            dy = (torch.randn(B, H, W, Cout, device="cuda") * 0.1).to(dtype)
            sc, sh = torch.rand(2, Cin, device="cuda") + 0.5, torch.rand(2, Cin, device="cuda") - 0.5
            acc = torch.zeros(_lib.packed_elems(Cout, Cin, 1, _lib.BF16), dtype=torch.float32, device="cuda")
            self.keep += [dy, sc, sh, acc]
            vals = (slab.data_ptr(), dy.data_ptr(), acc.data_ptr(), None, sc.data_ptr(), sh.data_ptr(),
                    B, H, W, Cin, ldx, H, W, Cout, Cout, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0, 1, 2)
            for n, v in zip(names, vals):
                setattr(it, n, v)
        self.keep.append(slab)
        self.n = len(layers)

    def time_us(self, reps=20):
        run = lambda: _lib.call("sdhip_conv2d_wgrad_group", ctypes.cast(self.items, ctypes.c_void_p), self.n, 0, _lib.BF16, _lib.stream_ptr())
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / reps


def blocks():
    B = 16
    towers = [("block1 (64x128)", 64, 128, 256, [(64 + 32 * i, 128) for i in range(6)]),
              ("block2 (32x64)", 32, 64, 512, [(128 + 32 * i, 128) for i in range(12)]),
              ("block3 (16x32)", 16, 32, 1024, [(256 + 32 * i, 128) for i in range(24)]),
              ("block4 (8x16)", 8, 16, 1024, [(512 + 32 * i, 128) for i in range(16)]),
              ("transition1", 64, 128, 256, [(256, 128)]), ("transition2", 32, 64, 512, [(512, 256)]), ("transition3", 16, 32, 1024, [(1024, 512)])]
    tot = {}
    for name, H, W, ldx, layers in towers:
        g = Group(B, H, W, ldx, layers)
        line = "%-18s" % name
        switches(SDHIP_WGRAD_NO_GEMM="1", SDHIP_TUNE_WG1_TILE=None)
        t = g.time_us()
        tot["old"] = tot.get("old", 0) + t
        line += " old %7.1f us |" % t
        switches(SDHIP_WGRAD_NO_GEMM=None)
        for mult in ("0.25", "0.5", "1", "2", "4"):
            switches(SDHIP_TUNE_WG1_TILE=mult)
            t = g.time_us()
            tot[mult] = tot.get(mult, 0) + t
            line += " x%s %7.1f" % (mult, t)
        switches(SDHIP_TUNE_WG1_TILE=None)
        print(line, flush=True)
        del g
    print("%-18s" % "sum" + " old %7.1f us |" % tot["old"] + "".join(" x%s %7.1f" % (m, tot[m]) for m in ("0.25", "0.5", "1", "2", "4")))


if __name__ == "__main__":
    blocks() if "blocks" in sys.argv[1:] else per_shape()
