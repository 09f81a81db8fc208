"""Micro-benchmark of the 5x5 bf16 weight gradient (bf16_gwgrad.hip, two tap groups per block pair) against the fp32 weight-gradient
kernel on the same shapes: the trunk layer (64 -> 64, batch 8, 256x256) and the two up-sampling stages of the k5 generators
(Conv2DTranspose 64 -> 256 at 256x256 -> 512x512, and 256 -> 256 at 128x128 -> 256x256 as the first x4 stage's successor at batch 8
of 64x64 frames).  python scripts/kbench_gw5.py"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-cycle_gan-upscaling_amd"))

import torch

from upscaler import _engine as E
from upscaler import _lib as L

PEAK = 2500.0


def timeit(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    rt = E.Runtime.get()
    lib = rt.lib
    print("%-40s %22s %22s %8s   (ms / TFLOP/s; bf16 %% of %.0f)" % ("case", "bf16 gwgrad", "fp32 wgrad_kernel", "ratio", PEAK))
    # (name, transposed, n, cin, h, w, cout): a Conv2D 'same' stride 1, or a Conv2DTranspose(strides 2)
    cases = [("trunk 5x5 s1 64->64 b8 @256", False, 8, 64, 256, 256, 64),
             ("convT 5x5 s2 64->256 b8 256->512", True, 8, 64, 256, 256, 256),
             ("convT 5x5 s2 64->256 b8 64->128 (x4 #0)", True, 8, 64, 64, 64, 256),
             ("convT 5x5 s2 256->256 b8 128->256 (x4 #1)", True, 8, 256, 128, 128, 256)]
    for name, tr, n, cin, h, w, cout in cases:
        if tr:
            d = L.ConvDesc(n, cin, h, w, cout, 2 * h, 2 * w, 5, 5, 2, 1, 1)
            xb = torch.randn(n, h, w, cin, device=rt.device).to(torch.bfloat16)
            gb = torch.randn(n, 2 * h, 2 * w, cout, device=rt.device).to(torch.bfloat16)
            xf, gf = torch.randn(n, cin, h, w, device=rt.device), torch.randn(n, cout, 2 * h, 2 * w, device=rt.device)
            dw = torch.empty(5, 5, cout, cin, device=rt.device)
            db = torch.empty(cout, device=rt.device)
            need = lib.vcg_conv_transpose2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d))
            need32 = lib.vcg_conv_transpose2d_wgrad_workspace_bytes(ctypes.byref(d))
            ws = torch.empty(max(need, need32, 16), dtype=torch.uint8, device=rt.device)
            fb = lambda: L.check(lib.vcg_conv_transpose2d_nhwc_bf16_wgrad(ctypes.byref(d), xb.data_ptr(), gb.data_ptr(), dw.data_ptr(), ws.data_ptr(), need,
                                                                          rt.stream), "bf16")
            ff = lambda: L.check(lib.vcg_conv_transpose2d_wgrad(ctypes.byref(d), xf.data_ptr(), gf.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                                                need32, rt.stream), "fp32")
            flop = 2.0 * n * h * w * cin * cout * 25
        else:
            d = L.ConvDesc(n, cin, h, w, cout, h, w, 5, 5, 1, 2, 2)
            xb = torch.randn(n, h, w, cin, device=rt.device).to(torch.bfloat16)
            gb = torch.randn(n, h, w, cout, device=rt.device).to(torch.bfloat16)
            xf, gf = torch.randn(n, cin, h, w, device=rt.device), torch.randn(n, cout, h, w, device=rt.device)
            dw = torch.empty(5, 5, cin, cout, device=rt.device)
            db = torch.empty(cout, device=rt.device)
            need = lib.vcg_conv2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d))
            need32 = lib.vcg_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
            ws = torch.empty(max(need, need32, 16), dtype=torch.uint8, device=rt.device)
            fb = lambda: L.check(lib.vcg_conv2d_nhwc_bf16_wgrad(ctypes.byref(d), xb.data_ptr(), gb.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                                                need, rt.stream), "bf16")
            ff = lambda: L.check(lib.vcg_conv2d_wgrad(ctypes.byref(d), xf.data_ptr(), gf.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need32,
                                                      rt.stream), "fp32")
            flop = 2.0 * n * h * w * cin * cout * 25
        tb, tf = timeit(fb), timeit(ff)
        f = lambda t: "%8.3f/%7.1f" % (t, flop / t / 1e9)
        print("%-40s %22s %22s %7.1fx   %4.1f%%" % (name, f(tb), f(tf), tf / tb, 100 * flop / tb / 1e9 / PEAK), flush=True)


if __name__ == "__main__":
    main()
