#!/usr/bin/env python3
"""In-kernel s_memtime stamps (csrc/vcg_stamps.hpp): where the cycles of a tile / an input row go in five bf16 kernels.

    python scripts/micro/stamps.py build [-DX ...]             (no GPU needed: hipcc cross-compiles)
    python scripts/micro/stamps.py run FAMILY [args] [--variant X[,Y]]

`build` compiles the WHOLE library (build.py's sources and flags) with -DVCG_STAMPS and the extra -D flags, e.g. -DCT_NO_DEFER (the
transposed convolution's stores issued behind their phase's MFMAs), into build/stamps[_X...]/libvcg_stamps.so, objects next to it; the
shipped libvcg_hip.so and its objects are not touched.  `run` loads that library, launches the family's workload and prints the
share of each segment:
    v2  conv3x3_c64_bf16_v2_kernel, the trunk at C5's shape                                   [batch] [plain|prelu|add] [launches]
    i9  conv_c3to64_bf16_kernel<9,3,1> as final/conv's data gradient (3 -> 256, LeakyReLU mask)    [batch] [h] [w] [mask 0/1]
    ct  convt3x3_c64_bf16_kernel, the up-sampling block's transposed convolution (64 -> 256)       [batch] [h] [w]
    f9  conv9x9_c256to3_bf16_kernel, final/conv                                                    [batch] [h] [w] [launches] [full|f32|u8]
        (full: vcg_conv9x9_to3_bf16_fwd; f32 / u8: the whole image as one window of vcg_conv9x9_to3_bf16_fwd_window, fp32 NCHW / uint8 NHWC out)
    wg  wgrad3x3_c64_bf16_kernel, the trunk's weight gradient                                      [batch] [h] [w]
`run` takes one variant: an A/B table (e.g. ct with and without --variant CT_NO_DEFER) is two invocations side by side.
The stamps are those of the LAST launch: many launches = the sustained state.  Read the shares, not the run time, of such a build.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "video-cycle_gan-upscaling_amd")
sys.path.insert(0, PKG)


def lib_path(defines):
    return os.path.join(PKG, "build", "_".join(["stamps"] + list(defines)), "libvcg_stamps.so")


def build(defines):
    import build as B
    out = lib_path(defines)
    B.build(extra_flags=["-DVCG_STAMPS"] + ["-D" + d for d in defines], objdir=os.path.dirname(out), out=out,
            jobs=min(16, os.cpu_count() or 1))
    print(out)


def arg(args, i, default, conv=int):
    return conv(args[i]) if len(args) > i else default


def timed(go, iters):
    """One launch to warm up, then `iters` back to back: microseconds per launch (events)."""
    import torch
    assert go() == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        assert go() == 0
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def sums(export, *shape):
    import numpy as np
    out = np.zeros(int(np.prod(shape)), dtype=np.uint64)
    assert export(out.ctypes.data) == 0
    return out.reshape(shape).astype(np.float64)


def run_v2(lib, L, torch, args):
    B, variant, iters = arg(args, 0, 32), arg(args, 1, "plain", str), arg(args, 2, 3)
    dev = torch.device("cuda:0")
    h = w = 256
    x = torch.randn(B, h, w, 64, device=dev).to(torch.bfloat16)
    res = torch.randn(B, h, w, 64, device=dev).to(torch.bfloat16)
    y = torch.empty_like(x)
    wk = (torch.randn(9, 64, 64, device=dev) * 0.05).to(torch.bfloat16)
    sc = torch.rand(64, device=dev) + 0.5
    sh = torch.rand(64, device=dev)
    al = torch.rand(64, device=dev)
    d = L.ConvDesc(B, 64, h, w, 64, h, w, 3, 3, 1, 1, 1)
    ep = {"plain": L.EpilogueBf16(None, None, L.ACT_NONE, 0.0, None, None),
          "prelu": L.EpilogueBf16(sc.data_ptr(), sh.data_ptr(), L.ACT_PRELU, 0.0, al.data_ptr(), None),
          "add": L.EpilogueBf16(sc.data_ptr(), sh.data_ptr(), L.ACT_NONE, 0.0, None, res.data_ptr())}[variant]
    stream = torch.cuda.current_stream().cuda_stream
    us = timed(lambda: lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), x.data_ptr(), wk.data_ptr(), y.data_ptr(), ctypes.byref(ep), stream), iters)
    print("%d launches back to back: %.1f us per launch (events)" % (iters, us))
    full = sums(lib.vcg_debug_v2_stamps, 256, 4, 6)
    s = full[:, :, :4]
    tiles = B * (h // 16) * (w // 32) / 256.0
    per = s / tiles                                       # s_memtime ticks (100 MHz constant clock) per tile
    names = ["phase A", "phase B", "vmcnt wait", "barrier"]   # A: half 0 + DMA of the next tile + drain of the previous half 1; B: half 1 + drain of half 0
    tot = per.sum(axis=2)
    print("variant %s, batch %d: %.1f tiles per workgroup; s_memtime ticks per tile (mean over 256 workgroups x 4 waves)" % (variant, B, tiles))
    for i, nm in enumerate(names):
        print("  %-11s mean %8.1f  min %8.1f  max %8.1f   share %5.1f %%" % (nm, per[:, :, i].mean(), per[:, :, i].min(), per[:, :, i].max(),
                                                                            100 * per[:, :, i].sum() / tot.sum()))
    print("  total       mean %8.1f  (per wave: %s)" % (tot.mean(), " ".join("%.1f" % v for v in tot.mean(axis=0))))
    print("  whole kernel: %.0f core clocks in %.1f us per wave (mean) -> the chip held %.3f GHz" % (
        full[:, :, 4].mean(), full[:, :, 5].mean() / 100.0, full[:, :, 4].sum() / full[:, :, 5].sum() * 0.1))


def run_i9(lib, L, torch, args):
    B, h, w, mask = arg(args, 0, 8), arg(args, 1, 512), arg(args, 2, 512), arg(args, 3, 1)
    dev = torch.device("cuda:0")
    dy = torch.randn(B, 3, h, w, device=dev)
    wk = torch.randn(9, 9, 256, 3, device=dev) * 0.01
    wd = torch.empty(4 * L.FIRST9X9_WFRAG_BYTES, dtype=torch.uint8, device=dev)
    yprev = torch.randn(B, h, w, 256, device=dev).to(torch.bfloat16)
    dx = torch.empty(B, h, w, 256, dtype=torch.bfloat16, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vcg_pack_conv9x9_3ch_bf16(wk.data_ptr(), 256, 1, wd.data_ptr(), st) == 0
    d = L.ConvDesc(B, 256, h, w, 3, h, w, 9, 9, 1, 4, 4)
    us = timed(lambda: lib.vcg_conv9x9_to3_bf16_dgrad(ctypes.byref(d), dy.data_ptr(), wd.data_ptr(), yprev.data_ptr() if mask else None, 0.2,
                                                      dx.data_ptr(), st), 10)
    print("batch %d %dx%d mask=%d: %.1f us per launch" % (B, h, w, mask, us))
    full = sums(lib.vcg_debug_i9_stamps, 512, 8, 6)
    for nm, sl, names in (("compute waves", slice(0, 6), ["MFMA loop", "barrier 1", "epilogue", "barrier 2"]),
                          ("loader waves", slice(6, 8), ["fetch issue", "barrier 1", "stash", "barrier 2"])):
        f = full[:, sl, :]
        f = f[f[:, :, 4] > 0]
        tiles = f[:, 4]
        print("%s: %.1f tiles per wave; s_memtime ticks (100 MHz) per tile, mean / min / max over waves" % (nm, tiles.mean()))
        for i, n2 in enumerate(names):
            per = f[:, i] / tiles
            print("  %-12s %8.1f %8.1f %8.1f" % (n2, per.mean(), per.min(), per.max()))
        print("  whole kernel %.0f ticks per wave = %.1f per tile" % (f[:, 5].mean(), (f[:, 5] / tiles).mean()))


def run_ct(lib, L, torch, args):
    B, h, w = arg(args, 0, 8), arg(args, 1, 256), arg(args, 2, 256)
    dev = torch.device("cuda:0")
    x = torch.randn(B, h, w, 64, device=dev).to(torch.bfloat16)
    wk = torch.randn(3, 3, 256, 64, device=dev) * 0.05
    wp = torch.empty(9, 256, 64, dtype=torch.bfloat16, device=dev)
    bias = torch.zeros(256, device=dev)
    y = torch.empty(B, 2 * h, 2 * w, 256, dtype=torch.bfloat16, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vcg_pack_conv_kernel_bf16(wk.data_ptr(), 9, 256, 64, 0, 0, wp.data_ptr(), st) == 0
    d = L.ConvDesc(B, 64, h, w, 256, 2 * h, 2 * w, 3, 3, 2, 0, 0)
    ep = L.EpilogueBf16(None, bias.data_ptr(), L.ACT_LRELU, 0.2, None, None)
    us = timed(lambda: lib.vcg_conv_transpose2d_bf16_fwd(ctypes.byref(d), x.data_ptr(), wp.data_ptr(), y.data_ptr(), ctypes.byref(ep), st), 10)
    f = sums(lib.vcg_debug_ct_stamps, 256, 8, 5)[:, :6, :]
    f = f[f[:, :, 3] > 0]
    t = f[:, 3]
    print("%-40s batch %d %dx%d: %.1f us per launch (%.2f TB/s written); %.1f tiles per wave; ticks per tile: body %.0f  barrier A %.0f  barrier B %.0f  (kernel %.0f)"
          % (os.path.relpath(lib._name, PKG), B, h, w, us, B * 4 * h * w * 512 / us / 1e6, t.mean(), (f[:, 0] / t).mean(), (f[:, 1] / t).mean(),
             (f[:, 2] / t).mean(), (f[:, 4] / t).mean()))


def run_f9(lib, L, torch, args):
    B, h, w, iters, out = arg(args, 0, 8), arg(args, 1, 512), arg(args, 2, 512), arg(args, 3, 20), arg(args, 4, "full", str)
    dev = torch.device("cuda:0")
    x = torch.randn(B, h, w, 256, device=dev).to(torch.bfloat16)
    wk = torch.randn(9, 9, 256, 3, device=dev) * 0.01
    wf = torch.empty(L.FINAL9X9_WFRAG_BYTES, dtype=torch.uint8, device=dev)
    y = torch.empty(B, 3, h, w, device=dev)
    bias = torch.zeros(3, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vcg_pack_final9x9_bf16(wk.data_ptr(), wf.data_ptr(), st) == 0
    d = L.ConvDesc(B, 256, h, w, 3, h, w, 9, 9, 1, 4, 4)
    if out == "full":
        go = lambda: lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), bias.data_ptr(), 1, y.data_ptr(), st)
    else:
        kind = {"f32": L.OUT_F32_NCHW, "u8": L.OUT_U8_NHWC}[out]
        y8 = torch.empty(B, h, w, 3, dtype=torch.uint8, device=dev)
        go = lambda: lib.vcg_conv9x9_to3_bf16_fwd_window(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), bias.data_ptr(), 1, kind,
                                                         (y8 if out == "u8" else y).data_ptr(), 0, h, 0, h, st)
    us = timed(go, iters)
    print("batch %d %dx%d, output %s: %.1f us per launch (events, %d launches)" % (B, h, w, out, us, iters))
    full = sums(lib.vcg_debug_f9_stamps, 512, 4, 8)
    full = full[full[:, 0, 5] > 0]
    rows = full[:, :, 5]
    names = ["vmcnt wait", "DMA issue", "MFMA loop", "partial+barrier", "combine+store", None, None, "acc shift"]
    tot = full[:, :, :5].sum() + full[:, :, 7].sum()
    print("%d workgroups, %.1f input rows per wave; s_memtime ticks per row (mean / min / max over waves)" % (full.shape[0], rows.mean()))
    for i, nm in enumerate(names):
        if nm is None:
            continue
        per = full[:, :, i] / rows
        print("  %-16s %8.1f %8.1f %8.1f   share %5.1f %%" % (nm, per.mean(), per.min(), per.max(), 100 * full[:, :, i].sum() / tot))
    print("  total per row    %8.1f" % (tot / rows.sum()))
    print("  whole kernel: %.0f core clocks per wave (mean)" % full[:, :, 6].mean())


def run_wg(lib, L, torch, args):
    B, h, w = arg(args, 0, 8), arg(args, 1, 256), arg(args, 2, 256)
    dev = torch.device("cuda:0")
    x = torch.randn(B, h, w, 64, device=dev).to(torch.bfloat16)
    dy = torch.randn(B, h, w, 64, device=dev).to(torch.bfloat16)
    dw = torch.empty(3, 3, 64, 64, device=dev)
    db = torch.empty(64, device=dev)
    d = L.ConvDesc(B, 64, h, w, 64, h, w, 3, 3, 1, 1, 1)
    nws = lib.vcg_conv2d_bf16_wgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    us = timed(lambda: lib.vcg_conv2d_bf16_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nws, st), 10)
    f = sums(lib.vcg_debug_wg_stamps, 256, 8, 6)
    print("%-36s batch %d %dx%d: %.1f us per launch incl. the reduction (%.2f TB/s read)" % (os.path.relpath(lib._name, PKG), B, h, w, us,
                                                                                         B * h * w * 256 / us / 1e6))
    for name, sel in (("tap-row 0 waves", f[:, 0:2]), ("tap-row 1 waves", f[:, 2:4]), ("tap-row 2 waves", f[:, 4:6])):
        g = sel.reshape(-1, 6)
        g = g[g[:, 4] > 0]
        t = g[:, 4]
        print("  %s: %.1f tiles per wave; ticks per tile: DMA wait %.0f  barrier %.0f  DMA issue %.0f  k-steps %.0f  (kernel %.0f per tile)"
              % (name, t.mean(), (g[:, 0] / t).mean(), (g[:, 1] / t).mean(), (g[:, 2] / t).mean(), (g[:, 3] / t).mean(), (g[:, 5] / t).mean()))
    g = f[:, 6:8].reshape(-1, 6)
    g = g[g[:, 4] > 0]
    if len(g):
        t = g[:, 4]
        print("  loader waves: ticks per tile: wait for the stage %.0f  barrier %.0f  issue of the next stage %.0f  (kernel %.0f per tile)"
              % ((g[:, 0] / t).mean(), (g[:, 1] / t).mean(), (g[:, 2] / t).mean(), (g[:, 5] / t).mean()))


FAMILIES = {"v2": run_v2, "i9": run_i9, "ct": run_ct, "f9": run_f9, "wg": run_wg}


def run(family, args):
    defines = []
    if "--variant" in args:
        i = args.index("--variant")
        defines = args[i + 1].split(",")
        args = args[:i] + args[i + 2:]
    import torch
    from upscaler import _lib as L
    lib = L.bind(ctypes.CDLL(lib_path(defines)))
    for fam in FAMILIES:
        export = getattr(lib, "vcg_debug_%s_stamps" % fam)
        export.restype, export.argtypes = ctypes.c_int, [ctypes.c_void_p]
    FAMILIES[family](lib, L, torch, args)


def main(argv):
    if len(argv) >= 2 and argv[1] == "build" and all(a.startswith("-D") and len(a) > 2 for a in argv[2:]):
        build([a[2:] for a in argv[2:]])
    elif len(argv) >= 3 and argv[1] == "run" and argv[2] in FAMILIES:
        run(argv[2], argv[3:])
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main(sys.argv)
