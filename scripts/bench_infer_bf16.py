"""bf16 inference of make_upscaler_orig models through UpscalerOrig.to_inference_bf16(): by default the reference's own generator
(kernel_size 5, upscale_factor 4, 16 residual blocks; upscaling/upscaler/model.py:267) at 128 -> 512, batch 32, one hipGraph replay per
batch.  Prints one JSON line per run, shaped like ``bench.py --config c5``'s.

  --generator attention   the same for make_upscaler_attention (model.py:299-328, train_gan3.py's default -gm resnet-att) through its
           to_inference_bf16(); --full then times one launch of each kind the pass makes and, for the memory-bound ones (the gates,
           to_add_input), the bytes they must move per second next to vcg_norm_act_fwd_bf16 on the same tensor

  --generator cyclegan    make_generator_cyclegan (_graph.py; stem 9x9 -> --n-downsample stride-2 convolutions -> residual blocks at the
           widest width -> stride-2 transposed convolutions -> head 9x9 + tanh, --norm instance | batch) through its to_inference_bf16();
           --lr-size is the input frame, --upscale may be 1.  --fp32 then also alternates the bf16 replay and the fp32 product path as two
           arms timed by HIP events (--ab-reps repetitions each, median and min-max); --full times one launch of each kind the pass makes on
           the engine's own buffers, with FLOP/s and the bytes each must move per second

  --generator inc-resnet  make_upscaler_incep_resnet (model.py:443-497, train_gan3.py's -gm inc-resnet) at its defaults (5 3-path k3, 10 2-path
           k7, 5 2-path k3 blocks, x4; --incep-blocks A B C changes the counts) through its to_inference_bf16(); --kernel-size and
           --res-blocks do not apply.  --fp32 also alternates the bf16 replay and fp32 G.forward as two arms timed by HIP events; --full times
           one block of each kind (its 5 / 4 launches) and the launches around them on the engine's own buffers

  --fp32   also times the fp32 product path (G.forward, i.e. what G.predict runs per batch) on the same weights and frames; it may run a
           smaller batch per call (--fp32-batch), stated in its line
  --full   per-layer HIP-event times of the bf16 pass (the calls the engine makes, on its buffers), with algorithmic FLOP, TFLOP/s and the
           share of the 2.5 PFLOP/s dense bf16 peak; for the 5x5 trunk convolution also an A/B, alternated in this process, of
           vcg_conv2d_bf16_fwd (folded BN + PReLU epilogue) against vcg_conv2d_nhwc_bf16_fwd (bias only) -- the same generic kernels, so the
           pair prices the epilogue

  --u8     host-to-host frames/s of ``predict`` (fp32 numpy in and out) against the uint8 path with synchronous copies (a loop of this
           script's) and against ``upscale_frames`` (the copies overlapped), --u8-batches batches per call, --ab-reps alternated
           repetitions, median and min-max; then (orig generator) one launch of final/conv on the engine's last up-sampling tensor, fp32
           NCHW against uint8 NHWC output, by HIP events
  --band-rows R   run the tail in bands of R low-res rows (default: the automatic plan); the result line says how many bands
  --band-sweep R [R ...]   device time of one replayed batch by HIP events, unbanded and in bands of each R low-res rows, each banded
           output compared with the unbanded one

Usage: python scripts/bench_infer_bf16.py [--lr-size 128] [--lr-width W] [--batch 32] [--kernel-size 5] [--upscale 4] [--res-blocks 16]
                                          [--steps 10] [--warmup 3] [--fp32] [--full] [--u8] [--band-rows R] [--band-sweep R [R ...]]
                                          [--generator orig|attention|cyclegan|inc-resnet] [--n-downsample 2] [--norm instance]
                                          [--incep-blocks 5 10 5]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-cycle_gan-upscaling_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_BF16 = 2.5e15          # MI355X dense bf16 MFMA, FLOP/s


# algorithmic FLOP per layer (2 per multiply-add; ISSUE table: 128 -> 512 with the defaults = 372 GFLOP per frame)
def flop_conv(n, h, w, cin, cout, k):
    """Conv2D 'same', stride 1: every output pixel sums k*k*cin products per output channel"""
    return 2.0 * n * h * w * cin * cout * k * k


def flop_convt(n, h, w, cin, cout, k):
    """Conv2DTranspose stride 2 'same' on an h x w input: every input pixel scatters k*k*cout products per input channel"""
    return 2.0 * n * h * w * cin * cout * k * k


def flop_frame(h, w, k, f, res):
    t = flop_conv(1, h, w, 3, 64, 9) + (2 * res + 1) * flop_conv(1, h, w, 64, 64, k)
    hh, ww, cin = h, w, 64
    while f > 1:
        t += flop_convt(1, hh, ww, cin, 256, k)
        hh, ww, cin, f = 2 * hh, 2 * ww, 256, f // 2
    return t + flop_conv(1, hh, ww, 256, 3, 9)


def flop_frame_attention(h, w, k, f, res):
    """make_upscaler_attention: the trunk, one 3 -> 64 attention convolution per block, per stage a 6 -> cin attention convolution, the
    ConvT to 128 channels and the (s+1)^2 x 3 -> 128 to_add_input transpose (at most 2 x 2 taps reach an output), final/conv on 128"""
    t = flop_conv(1, h, w, 3, 64, 9) + (2 * res + 1) * flop_conv(1, h, w, 64, 64, k) + res * flop_conv(1, h, w, 3, 64, k)
    hh, ww, cin, s = h, w, 64, 2
    while s <= f:
        t += flop_conv(1, hh, ww, 6, cin, k) + flop_convt(1, hh, ww, cin, 128, k) + 2.0 * h * w * 3 * 128 * (s + 1) ** 2
        hh, ww, cin, s = 2 * hh, 2 * ww, 128, 2 * s
    return t + flop_conv(1, hh, ww, 128, 3, 9)


def flop_frame_cyclegan(h, w, k, f, res, nd):
    """make_generator_cyclegan with 64 filters: stem, nd stride-2 convolutions doubling the channels, 2 res convolutions per block at the widest
    width, nd + log2 f transposed convolutions halving them (not below 64), head on 64"""
    t = flop_conv(1, h, w, 3, 64, 9)
    hh, ww, c = h, w, 64
    for _ in range(nd):
        hh, ww = hh // 2, ww // 2
        t += flop_conv(1, hh, ww, c, 2 * c, k)
        c *= 2
    t += 2 * res * flop_conv(1, hh, ww, c, c, k)
    ups, ff = nd, f
    while ff > 1:
        ups, ff = ups + 1, ff // 2
    for _ in range(ups):
        t += flop_convt(1, hh, ww, c, max(c // 2, 64), k)
        hh, ww, c = 2 * hh, 2 * ww, max(c // 2, 64)
    return t + flop_conv(1, hh, ww, 64, 3, 9)


def flop_frame_incep(h, w, f, groups, kc):
    """make_upscaler_incep_resnet with 64 filters: groups = [(block type, count, kernel)]; prefinal and the tail on kernel kc"""
    px = lambda cin, cout, taps: 2.0 * h * w * cin * cout * taps
    t = flop_conv(1, h, w, 3, 64, 9)
    for btype, num, k in groups:
        if btype == "3path":
            blk = 3 * px(64, 32, 1) + px(32, 32, k * k) + px(32, 48, k * k) + px(48, 64, k * k) + px(128, 64, 1)
        else:
            blk = px(64, 32, 1) + px(64, 19, 1) + px(19, 25, k) + px(25, 32, k) + px(64, 64, 1)
        t += num * blk
    t += flop_conv(1, h, w, 64, 64, kc)
    hh, ww, cin = h, w, 64
    while f > 1:
        t += flop_convt(1, hh, ww, cin, 256, kc)
        hh, ww, cin, f = 2 * hh, 2 * ww, 256, f // 2
    return t + flop_conv(1, hh, ww, 256, 3, 9)


def time_events(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps          # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--lr-width", type=int, default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--kernel-size", type=int, default=5)
    ap.add_argument("--upscale", type=int, default=4)
    ap.add_argument("--res-blocks", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--fp32-batch", type=int, default=4)
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--ab-reps", type=int, default=5)
    ap.add_argument("--generator", choices=("orig", "attention", "cyclegan", "inc-resnet"), default="orig")
    ap.add_argument("--incep-blocks", type=int, nargs=3, default=(5, 10, 5), metavar=("A", "B", "C"))
    ap.add_argument("--n-downsample", type=int, default=2)
    ap.add_argument("--norm", choices=("instance", "batch"), default=None)
    ap.add_argument("--u8", action="store_true")
    ap.add_argument("--u8-batches", type=int, default=4)
    ap.add_argument("--band-rows", type=int, default=None)
    ap.add_argument("--band-sweep", type=int, nargs="+", default=None, metavar="R")
    args = ap.parse_args()

    import torch
    from upscaler import _lib as L
    from upscaler import data as PD
    from upscaler import model as PM

    h, B, k, f, res = args.lr_size, args.batch, args.kernel_size, args.upscale, args.res_blocks
    w = args.lr_width or h
    frame = "%dx%d->%dx%d" % (h, w, f * h, f * w)
    att, cyc, inc = args.generator == "attention", args.generator == "cyclegan", args.generator == "inc-resnet"
    make = PM.make_upscaler_attention if att else PM.make_generator_cyclegan if cyc else PM.make_upscaler_orig
    kw = {} if args.norm is None and not cyc else {"norm": args.norm or "instance"}
    if cyc:
        kw["n_downsample"] = args.n_downsample
    if inc:
        make, (na, nb_, nc) = PM.make_upscaler_incep_resnet, args.incep_blocks
        G = make((f * h, f * w, 3), upscale_factor=f, a_block_num=na, b_block_num=nb_, c_block_num=nc, seed=7)
        groups = [("3path", na, 3), ("2path", nb_, 7), ("2path", nc, 3)]
        k = 3                                  # c_block_kernel: prefinal/conv2d and the tail
    else:
        G = make((f * h, f * w, 3), kernel_size=k, upscale_factor=f, res_block_num=res, seed=7, **kw)
    inf = G.to_inference_bf16()
    rt = inf.rt
    g1 = torch.Generator().manual_seed(1234)
    x = PD.frames_u8_to_device(torch.randint(0, 256, (B, h, w, 3), generator=g1, dtype=torch.uint8))
    br = args.band_rows
    inf.capture(B, h, w, L.OUT_F32_NCHW, br)
    for _ in range(args.warmup):
        inf.replay(x, br)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        inf.replay(x, br)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    fl = flop_frame_incep(h, w, f, groups, k) if inc else flop_frame_attention(h, w, k, f, res) if att else flop_frame_cyclegan(h, w, k, f, res, args.n_downsample) if cyc else flop_frame(h, w, k, f, res)
    wl = "%s((%d,%d,3),k=%d,x%d,res=%d%s)" % (make.__name__, f * h, f * w, k, f, res, "".join(",%s=%s" % kv for kv in sorted(kw.items())))
    if inc:
        wl = "%s((%d,%d,3),x%d,blocks=%d/%d/%d)" % ((make.__name__, f * h, f * w, f) + tuple(args.incep_blocks))
    bf = {"metric": "upscaled frames/s (inference, generator only, bf16) at %s" % frame, "value": round(B * args.steps / dt, 2),
          "unit": "frames/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
          "higher_is_better": True, "dtype": "bf16", "data": "synthetic",
          "gflop_per_frame": round(fl / 1e9, 1), "tflops": round(fl * B * args.steps / dt / 1e12, 1),
          "peak_share": round(fl * B * args.steps / dt / PEAK_BF16, 3),
          "config": {"workload": "%s.to_inference_bf16(), %s, bf16 NHWC activations, "
                                 "fp32 accumulate, batch %d, one hipGraph replay per batch" % (wl, "norm behind z" if cyc else "BN folded", B),
                     "global_batch": B, "frame": frame, "launch": "hipGraph replay", "band_rows": br,
                     "tail_bands": len(inf._plan(B, h, w, br)[1]), "tail_frames_per_launch": inf._plan(B, h, w, br)[0]}}
    print(json.dumps(bf), flush=True)

    if args.u8:
        u8_host_to_host(args, inf, h, w, f, B, frame)

    if args.band_sweep:
        band_sweep(args, inf, x, h, w, k, f, B)

    if args.fp32:
        b32 = min(args.fp32_batch, B)
        xs = x[:b32].contiguous()
        with torch.no_grad():
            for _ in range(max(1, args.warmup)):
                G.forward(xs, training=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                G.forward(xs, training=False)
            torch.cuda.synchronize()
        d32 = time.perf_counter() - t0
        fps32 = b32 * args.steps / d32
        print(json.dumps({"metric": "upscaled frames/s (inference, generator only, fp32 product path) at %s" % frame, "value": round(fps32, 2),
                          "unit": "frames/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(d32 / args.steps * 1e3, 3), "higher_is_better": True, "dtype": "fp32", "data": "synthetic",
                          "bf16_speedup": round(bf["value"] / fps32, 2),
                          "config": {"workload": "G.forward(x, training=False) -- what G.predict runs per batch -- same weights and frames, "
                                                 "batch %d per call (eager launches)" % b32, "global_batch": b32, "frame": frame}}), flush=True)

    if args.fp32 and (cyc or inc):
        ab_fp32(args, G, inf, x, B, frame)

    if args.full:
        (full_incep if inc else full_attention if att else full_cyclegan if cyc else full)(args, inf, x, h, w, k, f, res, B)


def band_sweep(args, inf, x, h, w, k, f, B):
    """device time of one replayed batch by HIP events, unbanded and in bands of each height given, and whether the banded fp32 output
    equals the unbanded one bit for bit (where it does not -- a band below the generic transposed convolution's kernel threshold, DESIGN.md
    section 9.5 -- the largest difference)"""
    import statistics

    import torch
    ref = inf.replay(x, None).clone()
    for br in [None] + list(args.band_sweep):
        y = inf.replay(x, br)
        torch.cuda.synchronize()
        diff = float((y - ref).abs().max())
        ms = [time_events(lambda: inf.replay(x, br), 5) for _ in range(max(5, args.ab_reps))]
        ch, bands = inf._plan(B, h, w, br)
        print(json.dumps({"kind": "band_sweep", "k": k, "f": f, "lr": "%dx%d" % (h, w), "batch": B, "band_rows": br, "bands": len(bands),
                          "frames_per_launch": ch, "identical_to_unbanded": bool(torch.equal(y, ref)), "max_abs_diff": diff,
                          "ms_per_batch_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}),
              flush=True)


def u8_host_to_host(args, inf, h, w, f, B, frame):
    """frames/s from host memory to host memory: predict (fp32 NHWC numpy in and out) against upscale_frames (uint8 in and out), the arms
    alternated; then final/conv alone with its two output forms"""
    import statistics

    import numpy as np
    import torch
    from upscaler import _lib as L
    rt, lib, br = inf.rt, inf.rt.lib, args.band_rows
    N = B * args.u8_batches
    u8 = np.random.RandomState(5).randint(0, 256, (N, h, w, 3)).astype(np.uint8)
    xf = (u8 / 127.5 - 1).astype(np.float32)
    def synchronous():
        """the uint8 path with its copies on the compute stream, one after the other: the form upscale_frames' overlapped copies are
        measured against (the same graphs, the same conversion kernel)"""
        t = torch.from_numpy(u8)
        out = np.empty((N, f * h, f * w, 3), dtype=np.uint8)
        for i in range(0, N, B):
            xb = t[i:i + B].to(rt.device)
            nb = xb.shape[0]
            g, xin, y = inf.capture(nb, h, w, L.OUT_U8_NHWC, br)
            L.check(lib.vcg_frames_u8_to_nchw(xb.data_ptr(), xin.data_ptr(), nb, h, w, 3, rt.stream), "vcg_frames_u8_to_nchw")
            g.replay()
            torch.from_numpy(out[i:i + nb]).copy_(y)
        return out

    arms = {"predict (fp32 in/out)": lambda: inf.predict(xf, batch_size=B, band_rows=br),
            "uint8 in/out, synchronous copies (this script's loop)": synchronous,
            "upscale_frames (uint8 in/out, overlapped copies)": lambda: inf.upscale_frames(u8, batch_size=B, band_rows=br)}
    ref = None
    for name, fn in arms.items():                    # warm-up: graphs recorded, staging buffers pinned; the uint8 arms agree
        got = fn()
        if got.dtype == np.uint8:
            assert ref is None or np.array_equal(ref, got), name
            ref = got
    fps = {name: [] for name in arms}
    for _ in range(max(5, args.ab_reps)):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            fps[name].append(N / (time.perf_counter() - t0))
    for name, v in fps.items():
        print(json.dumps({"kind": "host_to_host", "arm": name, "frame": frame, "batch": B, "frames_per_call": N, "reps": len(v),
                          "frames_per_s_median": round(statistics.median(v), 1), "frames_per_s_min": round(min(v), 1),
                          "frames_per_s_max": round(max(v), 1)}), flush=True)
    if args.generator != "orig":          # the launch comparison below reads Bf16Generator's buffers (256 channels)
        return
    # one launch of final/conv on the last up-sampling stage's tensor (whatever the last pass left in it)
    Bf = inf._buffers(B, h, w)
    src = Bf["us"][-1]
    ch, hh, ww = src.shape[0], src.shape[1], src.shape[2]
    wf, bf_ = inf.final
    df = L.ConvDesc(ch, 256, hh, ww, 3, hh, ww, 9, 9, 1, 4, 4)
    y32 = torch.empty(ch, 3, hh, ww, device=rt.device)
    y8 = torch.empty(ch, hh, ww, 3, dtype=torch.uint8, device=rt.device)
    st = rt.stream
    forms = {"vcg_conv9x9_to3_bf16_fwd (fp32 NCHW)": lambda: L.check(lib.vcg_conv9x9_to3_bf16_fwd(
                 ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1, y32.data_ptr(), st), "final"),
             "window, fp32 NCHW": lambda: L.check(lib.vcg_conv9x9_to3_bf16_fwd_window(
                 ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1, L.OUT_F32_NCHW, y32.data_ptr(), 0, hh, 0, hh, st), "final"),
             "window, uint8 NHWC": lambda: L.check(lib.vcg_conv9x9_to3_bf16_fwd_window(
                 ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1, L.OUT_U8_NHWC, y8.data_ptr(), 0, hh, 0, hh, st), "final")}
    ms = {name: [] for name in forms}
    for _ in range(max(5, args.ab_reps)):
        for name, fn in forms.items():
            ms[name].append(time_events(fn, 5))
    for name, v in ms.items():
        print(json.dumps({"kind": "final_conv_launch", "form": name, "shape": "%d x %dx%d x 256" % (ch, hh, ww), "reps": len(v),
                          "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}), flush=True)


def full(args, inf, x, h, w, k, f, res, B):
    """per-layer HIP-event times of the calls the bf16 pass makes; the trunk convolution A/B against the bias-only generic entry point"""
    import torch
    from upscaler import _lib as L
    rt, lib, st = inf.rt, inf.rt.lib, inf.rt.stream
    Bf = inf._buffers(B, h, w)
    rows = []

    def row(name, ms, flop, extra=None):
        d = {"layer": name, "ms": round(ms, 4), "gflop": round(flop / 1e9, 2), "tflops": round(flop / ms / 1e9, 1),
             "peak_share": round(flop / (ms * 1e-3) / PEAK_BF16, 3)}
        d.update(extra or {})
        rows.append(d)

    # initial/conv 9x9 3 -> 64 (+PReLU)
    w0, b0, a0 = inf.first
    d0 = L.ConvDesc(B, 3, h, w, 64, h, w, 9, 9, 1, 4, 4)
    ms = time_events(lambda: L.check(lib.vcg_conv9x9_from3_bf16_fwd(ctypes.byref(d0), x.data_ptr(), w0.data_ptr(), b0.data_ptr(), a0.data_ptr(),
                                                                    Bf["skip"].data_ptr(), st), "first"), args.ab_reps)
    row("initial/conv 9x9 3->64", ms, flop_conv(B, h, w, 3, 64, 9))
    # a trunk convolution (k x k 64 -> 64, BN folded + PReLU) and its A/B against the generic kernel
    w1, s1, h1, al = inf.trunk[0][:4] if inf.trunk else (inf.prefinal[0], inf.prefinal[1], inf.prefinal[2], None)
    dk = L.ConvDesc(B, 64, h, w, 64, h, w, k, k, 1, k // 2, k // 2)
    ep = L.EpilogueBf16(s1.data_ptr(), h1.data_ptr(), L.ACT_PRELU if al is not None else L.ACT_NONE, 0.0, al.data_ptr() if al is not None else None, None)
    new = lambda: L.check(lib.vcg_conv2d_bf16_fwd(ctypes.byref(dk), Bf["skip"].data_ptr(), w1.data_ptr(), Bf["b"].data_ptr(), ctypes.byref(ep), st), "trunk")
    c1 = inf.model.blocks[0][0] if inf.model.blocks else inf.model.c_pre
    wg = torch.empty(k * k * 64 * 64, dtype=torch.bfloat16, device=rt.device)
    L.check(lib.vcg_pack_conv_frag_bf16(c1.ps[c1.name + "/kernel"].data_ptr(), k * k, 64, 64, 0, wg.data_ptr(), st), "pack frag")
    gen = lambda: L.check(lib.vcg_conv2d_nhwc_bf16_fwd(ctypes.byref(dk), Bf["skip"].data_ptr(), wg.data_ptr(), h1.data_ptr(), L.ACT_NONE, 0.0,
                                                       Bf["c"].data_ptr(), st), "trunk generic")
    ab(rows, "res_block conv %dx%d 64->64 (x%d per pass); A/B arm: bias only, no PReLU" % (k, k, 2 * res + 1), new, gen,
       flop_conv(B, h, w, 64, 64, k), args.ab_reps)
    # the up-sampling stages on the engine's chunk of frames, A/B against the generic transposed convolution
    us = Bf["us"]
    ch = us[0].shape[0]
    src, hh, ww = Bf["a"], h, w
    crop = max(k - 2, 0) // 2
    for i, ((wt, bt, slope, cin), up, u) in enumerate(zip(inf.ups, inf.model.ups, us)):
        dt = L.ConvDesc(ch, cin, hh, ww, 256, 2 * hh, 2 * ww, k, k, 2, crop, crop)
        if inf._generic(up, 0):
            kern = "generic gconv (vcg_conv_transpose2d_nhwc_bf16_fwd)"
            call = (lambda dt=dt, s=src, wt=wt, u=u, bt=bt, slope=slope:
                    L.check(lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(dt), s.data_ptr(), wt.data_ptr(), bt.data_ptr(), L.ACT_LRELU, slope,
                                                                   u.data_ptr(), st), "convT generic"))
        else:
            kern = "convt3x3_c64_bf16_kernel (vcg_conv_transpose2d_bf16_fwd)"
            ept = L.EpilogueBf16(None, bt.data_ptr(), L.ACT_LRELU, slope, None, None)
            call = (lambda dt=dt, s=src, wt=wt, u=u, ept=ept:
                    L.check(lib.vcg_conv_transpose2d_bf16_fwd(ctypes.byref(dt), s.data_ptr(), wt.data_ptr(), u.data_ptr(), ctypes.byref(ept), st), "convT"))
        name = "upscaling/%d ConvT %dx%d s2 %d->256 at %dx%d, %d frames per launch" % (i, k, k, cin, 2 * hh, 2 * ww, ch)
        row(name, time_events(call, args.ab_reps), flop_convt(ch, hh, ww, cin, 256, k), {"kernel": kern})
        src, hh, ww = u, 2 * hh, 2 * ww
    wf, bf_ = inf.final
    df = L.ConvDesc(ch, 256, hh, ww, 3, hh, ww, 9, 9, 1, 4, 4)
    ms = time_events(lambda: L.check(lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1,
                                                                  Bf["y"].data_ptr(), st), "final"), args.ab_reps)
    row("final/conv 9x9 256->3 at %dx%d, %d frames per launch" % (hh, ww, ch), ms, flop_conv(ch, hh, ww, 256, 3, 9))
    for r in rows:
        print(json.dumps(dict(r, kind="layer")), flush=True)


def full_attention(args, inf, x, h, w, k, f, res, B):
    """one launch of each kind the attention pass makes, on the engine's own buffers: HIP-event times, algorithmic FLOP, and for the
    memory-bound kernels the bytes they must move (gate: m read + y written; to_add_input: y read + written) per second, next to
    vcg_norm_act_fwd_bf16 (x read + y written) on the same tensor"""
    import torch
    from upscaler import _lib as L
    rt, lib, st = inf.rt, inf.rt.lib, inf.rt.stream
    Bf = inf._buffers(B, h, w)
    inf.forward(x)                                    # the gates' inputs and every buffer hold a pass's data
    torch.cuda.synchronize()
    rows = []

    def row(name, ms, flop=0.0, nbytes=0, extra=None):
        d = {"layer": name, "ms": round(ms, 4)}
        if flop:
            d.update({"gflop": round(flop / 1e9, 2), "tflops": round(flop / ms / 1e9, 1), "peak_share": round(flop / (ms * 1e-3) / PEAK_BF16, 3)})
        if nbytes:
            d.update({"must_move_gb": round(nbytes / 1e9, 3), "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3)})
        d.update(extra or {})
        rows.append(d)

    def norm_act(t):
        """vcg_norm_act_fwd_bf16 on tensor t (scale 1, shift 0, no activation) into a buffer of its own: the streaming yardstick"""
        n_, hh_, ww_, c_ = t.shape
        one, zero = torch.ones(c_, device=rt.device), torch.zeros(c_, device=rt.device)
        out = torch.empty_like(t)
        ms = time_events(lambda: L.check(lib.vcg_norm_act_fwd_bf16(t.data_ptr(), n_, c_, hh_ * ww_, one.data_ptr(), zero.data_ptr(), 1, L.ACT_NONE, 0.0,
                                                                    None, None, out.data_ptr(), st), "norm_act"), args.ab_reps)
        return ms, 2 * t.numel() * 2

    w0, b0, a0 = inf.first
    d0 = L.ConvDesc(B, 3, h, w, 64, h, w, 9, 9, 1, 4, 4)
    row("initial/conv 9x9 3->64", time_events(lambda: L.check(lib.vcg_conv9x9_from3_bf16_fwd(
        ctypes.byref(d0), x.data_ptr(), w0.data_ptr(), b0.data_ptr(), a0.data_ptr(), Bf["skip"].data_ptr(), st), "first"), args.ab_reps),
        flop_conv(B, h, w, 3, 64, 9))
    if inf.trunk:
        gate, w1, s1, h1, al = inf.trunk[0][:5]
        ms = time_events(lambda: inf._gate(gate, x, 3, Bf["skip"], Bf["g"], B, h, w), args.ab_reps)
        row("res_block gate %dx%d 3->64 (x%d per pass)" % (k, k, res), ms, flop_conv(B, h, w, 3, 64, k), 2 * Bf["g"].numel() * 2)
        msn, nb = norm_act(Bf["skip"])
        row("  vcg_norm_act_fwd_bf16 on the same tensor", msn, 0.0, nb, {"gate_rate_vs_norm_act": round(msn / ms, 2)})
        row("res_block conv %dx%d 64->64 + BN + PReLU (x%d per pass)" % (k, k, 2 * res + 1),
            time_events(lambda: inf._conv(Bf["g"], w1, Bf["b"], s1, h1, L.ACT_PRELU, al, None, B, h, w), args.ab_reps), flop_conv(B, h, w, 64, 64, k))
    ch, crop = Bf["chunk"], max(k - 2, 0) // 2
    src, hh, ww = Bf["a"][:ch], h, w
    for i, ((gate, wt, bt, slope, cin, cout, wa, ba), stg) in enumerate(zip(inf.ups, Bf["stages"])):
        scale = 2 ** (i + 1)
        u = stg["u"][:ch]
        ms = time_events(lambda: inf._gate(gate, u, 6, src, stg["g"], ch, hh, ww), args.ab_reps)
        row("upscaling/%d gate %dx%d 6->%d at %dx%d, %d frames per launch" % (i, k, k, cin, hh, ww, ch), ms, flop_conv(ch, hh, ww, 6, cin, k),
            2 * stg["g"].numel() * 2)
        msn, nb = norm_act(stg["g"])
        row("  vcg_norm_act_fwd_bf16 on the same tensor", msn, 0.0, nb, {"gate_rate_vs_norm_act": round(msn / ms, 2)})
        dt = L.ConvDesc(ch, cin, hh, ww, cout, 2 * hh, 2 * ww, k, k, 2, crop, crop)
        row("upscaling/%d ConvT %dx%d s2 %d->%d at %dx%d" % (i, k, k, cin, cout, 2 * hh, 2 * ww),
            time_events(lambda: L.check(lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(dt), stg["g"].data_ptr(), wt.data_ptr(), bt.data_ptr(),
                                                                               L.ACT_LRELU, slope, stg["y"].data_ptr(), st), "convT"), args.ab_reps),
            flop_convt(ch, hh, ww, cin, cout, k))
        da = L.ConvDesc(ch, 3, h, w, cout, scale * h, scale * w, scale + 1, scale + 1, scale, 0, 0)
        ms = time_events(lambda: L.check(lib.vcg_input_convt_add_bf16(ctypes.byref(da), x.data_ptr(), wa.data_ptr(), ba.data_ptr(), stg["y"].data_ptr(), st),
                                         "to_add"), args.ab_reps)
        row("upscaling/%d to_add_input (ConvT %dx%d s%d of atanh) at %dx%d" % (i, scale + 1, scale + 1, scale, 2 * hh, 2 * ww), ms, 0.0,
            2 * stg["y"].numel() * 2)
        msn, nb = norm_act(stg["y"])
        row("  vcg_norm_act_fwd_bf16 on the same tensor", msn, 0.0, nb, {"to_add_rate_vs_norm_act": round(msn / ms, 2)})
        src, hh, ww = stg["y"], 2 * hh, 2 * ww
    wf, bf_, cfin = inf.final
    df = L.ConvDesc(ch, cfin, hh, ww, 3, hh, ww, 9, 9, 1, 4, 4)
    row("final/conv 9x9 %d->3 at %dx%d, %d frames per launch" % (cfin, hh, ww, ch),
        time_events(lambda: L.check(lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1, Bf["y"].data_ptr(), st),
                                    "final"), args.ab_reps), flop_conv(ch, hh, ww, cfin, 3, 9))
    for r in rows:
        print(json.dumps(dict(r, kind="layer")), flush=True)


def ab_fp32(args, G, inf, x, B, frame):
    """the bf16 engine's replayed batch against the fp32 product path (G.forward(x, training=False), what G.predict runs per batch) on the same
    weights and frames: two arms alternated after a warm-up, each repetition timed by HIP events; ms per frame, median and min-max"""
    import statistics

    import torch
    b32 = min(args.fp32_batch, B)
    xs = x[:b32].contiguous()
    arms = {"bf16 engine, hipGraph replay, batch %d" % B: (lambda: inf.replay(x), B),
            "fp32 product path, eager launches, batch %d" % b32: (lambda: G.forward(xs, training=False), b32)}
    ms = {name: [] for name in arms}
    with torch.no_grad():
        for _ in range(max(5, args.ab_reps)):
            for name, (fn, nb) in arms.items():
                ms[name].append(time_events(fn, 3) / nb)
    med = {name: statistics.median(v) for name, v in ms.items()}
    names = list(arms)
    for name, v in ms.items():
        print(json.dumps({"kind": "bf16_vs_fp32", "arm": name, "frame": frame, "reps": len(v), "ms_per_frame_median": round(med[name], 5),
                          "ms_per_frame_min": round(min(v), 5), "ms_per_frame_max": round(max(v), 5),
                          "fp32_over_bf16": round(med[names[1]] / med[names[0]], 2)}), flush=True)


def full_cyclegan(args, inf, x, h, w, k, f, res, B):
    """one launch of each kind the cyclegan pass makes, on the engine's own buffers for its chunk of frames: HIP-event times, algorithmic FLOP
    and TFLOP/s, and the bytes the launch must move (input read + output written, bf16; the weights are negligible) per second"""
    import torch
    from upscaler import _lib as L
    rt, lib, st = inf.rt, inf.rt.lib, inf.rt.stream
    ch = inf._chunk(B, h, w)
    xc = x[:ch].contiguous()
    inf.forward(x)                                    # every buffer holds a pass's data
    torch.cuda.synchronize()
    P = inf._launches(ch, h, w)
    seen, rows = {}, []

    def row(name, ms, flop, nbytes, count, extra=None):
        d = {"layer": name, "launches_per_pass": count, "ms": round(ms, 4), "must_move_gb": round(nbytes / 1e9, 4),
             "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3)}
        if flop:
            d.update({"gflop": round(flop / 1e9, 2), "tflops": round(flop / ms / 1e9, 1), "peak_share": round(flop / (ms * 1e-3) / PEAK_BF16, 4)})
        d.update(extra or {})
        rows.append(d)

    for s in P["steps"]:
        d, op = s["d"], s["op"]
        key = (op["kind"], d.cin, d.h, d.w, d.cout, op["residual"], op["alpha"] is None)
        seen.setdefault(key, []).append(s)
    for key, steps in seen.items():
        s = steps[0]
        d, op = s["d"], s["op"]
        io = (s["z"].numel() + (s["x"].numel() if s["x"] is not None else 0)) * 2 + (xc.numel() * 4 if s["x"] is None else 0)
        fl = flop_convt(ch, d.h, d.w, d.cin, d.cout, d.kh) if op["kind"] == "convt" else flop_conv(ch, d.oh, d.ow, d.cin, d.cout, d.kh)
        kern = {"stem": "vcg_conv9x9_from3_bf16_fwd", "convt": "vcg_conv_transpose2d_nhwc_bf16_fwd"}.get(
            op["kind"], "vcg_conv2d_nhwc_bf16_fwd_stats (%d records per image)" % s["nrec"] if s["nrec"] > 0 else "vcg_conv2d_nhwc_bf16_fwd")
        name = "%s %dx%d s%d %d->%d, out %dx%d, %d frames per launch" % (op["conv"], d.kh, d.kw, d.stride, d.cin, d.cout, d.oh, d.ow, ch)
        row(name, time_events(lambda: inf._conv_step(P, s, xc), args.ab_reps), fl, io, len(steps), {"entry": kern})
        nb = (2 + (1 if s["res"] is not None else 0)) * s["z"].numel() * 2
        how = "norm on the moving statistics" if not inf.instance else "statistics from the epilogue records" if s["nrec"] > 0 else "statistics pass over z"
        row("  norm%s behind it (%s): %s" % (" + PReLU" if op["alpha"] is not None else "", how, "+ Add" if s["res"] is not None else "no Add"),
            time_events(lambda: inf._norm(P, s), args.ab_reps), 0.0, nb + (s["z"].numel() * 2 if inf.instance and s["nrec"] <= 0 else 0), len(steps))
    wf, bf_ = inf.final
    src = P["last"]
    hh, ww = src.shape[1], src.shape[2]
    df = L.ConvDesc(ch, 64, hh, ww, 3, hh, ww, 9, 9, 1, 4, 4)
    y32 = torch.empty(ch, 3, hh, ww, device=rt.device)
    y8 = torch.empty(ch, hh, ww, 3, dtype=torch.uint8, device=rt.device)
    row("head/conv 9x9 64->3 + tanh at %dx%d, fp32 NCHW out, %d frames per launch (NW = 1)" % (hh, ww, ch),
        time_events(lambda: L.check(lib.vcg_conv9x9_c64to3_bf16_fwd(ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1, y32.data_ptr(), st),
                                    "head"), args.ab_reps), flop_conv(ch, hh, ww, 64, 3, 9), src.numel() * 2 + y32.numel() * 4, 1)
    row("head/conv, window form over the whole frame, uint8 NHWC out",
        time_events(lambda: L.check(lib.vcg_conv9x9_c64to3_bf16_fwd_window(ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1, L.OUT_U8_NHWC,
                                                                           y8.data_ptr(), 0, hh, 0, hh, st), "head"), args.ab_reps),
        flop_conv(ch, hh, ww, 64, 3, 9), src.numel() * 2 + y8.numel(), 1)
    for r in rows:
        print(json.dumps(dict(r, kind="layer")), flush=True)


def full_incep(args, inf, x, h, w, k, f, res, B):
    """the inc-resnet pass on the engine's own buffers, by HIP events: the stem, one block of each kind (all its launches: head, the layers
    between, join), prefinal/conv2d, the up-sampling stages and final/conv on the engine's chunk of frames; algorithmic FLOP and TFLOP/s, and for
    the blocks the bytes their launches must move (every tensor read + written once, bf16) per second"""
    import torch
    from upscaler import _lib as L
    rt, lib, st = inf.rt, inf.rt.lib, inf.rt.stream
    Bf = inf._buffers(B, h, w)
    inf.forward(x)                                    # every buffer holds a pass's data
    torch.cuda.synchronize()
    rows = []

    def row(name, ms, flop, nbytes=0, extra=None):
        d = {"layer": name, "ms": round(ms, 4), "gflop": round(flop / 1e9, 2), "tflops": round(flop / ms / 1e9, 1),
             "peak_share": round(flop / (ms * 1e-3) / PEAK_BF16, 4)}
        if nbytes:
            d.update({"must_move_gb": round(nbytes / 1e9, 3), "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3)})
        d.update(extra or {})
        rows.append(d)

    w0, b0, _ = inf.first
    row("initial/conv/9x9 3->64", time_events(lambda: inf._stem(x, w0, b0, None, Bf["skip"]), args.ab_reps), flop_conv(B, h, w, 3, 64, 9))
    kinds = {}
    for blk in inf.blocks:
        key = (len(blk["heads"]), blk["mids"][0]["kh"], blk["mids"][0]["kw"])
        kinds.setdefault(key, []).append(blk)
    px = B * h * w
    for (nh, kh, kw), blks in kinds.items():
        blk = blks[0]
        fl = sum(2.0 * px * 64 * hp["cout"] for hp in blk["heads"]) + sum(2.0 * px * m["cin"] * m["cout"] * m["kh"] * m["kw"] for m in blk["mids"]) \
            + 2.0 * px * sum(c for _, c, _ in blk["srcs"]) * 64
        # stored channels moved: head reads 64, writes 32 per path; each middle layer reads and writes its padded tensors; join reads its
        # sources and m, writes 64
        pad = lambda c: (c + 31) // 32 * 32
        ch_moved = 64 + 32 * nh + sum(pad(m["cin"]) + pad(m["cout"]) for m in blk["mids"]) + sum(pad(c) for _, c, _ in blk["srcs"]) + 64 + 64
        name = "%s block, kernel %dx%d (x%d per pass): %d launches" % ("3-path" if nh == 3 else "2-path", kh, kw, len(blks), 2 + len(blk["mids"]))
        row(name, time_events(lambda: inf._run_block(blk, Bf["skip"], Bf["a"], Bf, B, h, w), args.ab_reps), fl, px * ch_moved * 2)
    wp, sp, hp_ = inf.prefinal
    row("prefinal/conv2d %dx%d 64->64 + BN + Add" % (k, k),
        time_events(lambda: inf._conv(Bf["a"], wp, Bf["c"], sp, hp_, L.ACT_NONE, None, Bf["skip"], B, h, w), args.ab_reps), flop_conv(B, h, w, 64, 64, k))
    us = Bf["us"]
    ch = us[0].shape[0]
    hh, ww, cin = h, w, 64
    for i in range(len(inf.ups)):
        src = Bf["c"][:ch] if i == 0 else us[i - 1]
        row("upscaling/%d ConvT %dx%d s2 %d->256 at %dx%d, %d frames per launch" % (i, k, k, cin, 2 * hh, 2 * ww, ch),
            time_events(lambda: upsample_one(inf, i, src, us[i], ch, hh, ww), args.ab_reps), flop_convt(ch, hh, ww, cin, 256, k))
        hh, ww, cin = 2 * hh, 2 * ww, 256
    row("final/conv 9x9 256->3 at %dx%d, %d frames per launch" % (hh, ww, ch),
        time_events(lambda: inf._to3(us[-1], Bf["y"][:ch]), args.ab_reps), flop_conv(ch, hh, ww, 256, 3, 9))
    for r in rows:
        print(json.dumps(dict(r, kind="layer")), flush=True)
    print(json.dumps({"kind": "launches", "entry_point_calls_per_pass_one_chunk": inf.launches(), "tail_frames_per_launch": ch,
                      "blocks": len(inf.blocks)}), flush=True)


def upsample_one(inf, i, src, dst, c, hh, ww):
    """stage i of the engine's up-sampling alone (Bf16Generator._upsample on a one-stage view)"""
    ups, layers = inf.ups, inf.up_layers
    inf.ups, inf.up_layers = ups[i:i + 1], layers[i:i + 1]
    try:
        inf._upsample(src, [dst], c, hh, ww)
    finally:
        inf.ups, inf.up_layers = ups, layers


def ab(rows, name, new, gen, flop, reps):
    """two arms alternated (A B A B ...), each timed by HIP events; medians"""
    import statistics
    tn, tg = [], []
    for _ in range(3):
        tn.append(time_events(new, reps))
        tg.append(time_events(gen, reps))
    mn, mg = statistics.median(tn), statistics.median(tg)
    rows.append({"layer": name, "ms": round(mn, 4), "gflop": round(flop / 1e9, 2), "tflops": round(flop / mn / 1e9, 1),
                 "peak_share": round(flop / (mn * 1e-3) / PEAK_BF16, 3), "generic_ms": round(mg, 4),
                 "generic_tflops": round(flop / mg / 1e9, 1), "ratio_vs_bias_only": round(mg / mn, 2),
                 "kernel": "generic gconv with the vcg_epilogue_bf16 terms (vcg_conv2d_bf16_fwd)"})


if __name__ == "__main__":
    main()
