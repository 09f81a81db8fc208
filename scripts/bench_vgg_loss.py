#!/usr/bin/env python
"""The perceptual content loss (VGG_MSE_LOSS, upscaling/upscaler/model.py:119-137) with the fp32 and with the bf16 VGG19 extractor, at the
flagship frame size (batch 8, 512x512 frames):

  1. _content_loss_and_grad alone -- features of hr and fake, the loss, its gradient back to the fake frames -- for 'vgg_mse';
  2. the full train step: bench.py --dtype bf16's pair (make_upscaler_orig k3 x2 'bf16+tail' + bf16 PatchGAN) inside make_and_compile_gan2,
     one captured hipGraph per step, with the fp32 and with the bf16 extractor behind VGG_MSE_LOSS.

    python scripts/bench_vgg_loss.py [--rounds 3] [--iters 5] [--warmup 2] [--batch 8] [--size 512] [--extractor both|fp32|bf16] [--skip-step]
                                     [--out FILE]

The two extractors are built in one process and timed in alternating rounds (fp32, bf16, fp32, bf16, ...), so both see the same machine
state; times are device events around `iters` launches after `warmup` launches.  One JSON line per round, medians, ranges and the ratios
at the end (appended to --out).  The weights are the seeded random ones: throughput does not depend on their values."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-cycle_gan-upscaling_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512, help="the (output) frames are size x size")
    ap.add_argument("--res-blocks", type=int, default=9)
    ap.add_argument("--extractor", choices=("both", "fp32", "bf16"), default="both", help="one extractor only: what a kernel trace of one pass wants")
    ap.add_argument("--skip-step", action="store_true", help="only part 1")
    ap.add_argument("--out", default=None, help="append the printed lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from upscaler import model as PM, _engine as E
    rt = E.Runtime.get()
    s, bs = args.size, args.batch
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    rng = np.random.RandomState(5)
    frames = lambda h: E.to_device_nchw(rt, (rng.randint(0, 256, (bs, h, h, 3)) / 127.5 - 1).astype(np.float32))
    hr, fake, lr = frames(s), frames(s), frames(s // 2)
    dtypes = ("fp32", "bf16") if args.extractor == "both" else (args.extractor,)
    loss = {dt: PM.VGG_MSE_LOSS((s, s, 3), 0.1, vgg19="random", dtype=dt) for dt in dtypes}
    kinds = {dt: PM._content_kind(loss[dt].loss) for dt in dtypes}

    # ---- 1. loss + gradient alone
    vals = {}

    def one(dt):
        val, dfake = PM._content_loss_and_grad(rt, kinds[dt], 1.0, fake, hr)
        vals[dt] = val
    ms = {dt: [] for dt in dtypes}
    for r in range(args.rounds):
        for dt in dtypes:
            t = timed(lambda: one(dt), args.iters, args.warmup)
            ms[dt].append(t)
            emit(json.dumps({"bench": "vgg_mse_loss_and_grad", "extractor": dt, "round": r, "batch": bs, "size": s, "iters": args.iters,
                             "ms": round(t, 3), "loss": "%.6g" % float(vals[dt].item())}))
    med = {dt: statistics.median(ms[dt]) for dt in dtypes}
    for dt in dtypes:
        emit("loss + gradient, %s extractor: median %.2f ms (range %.2f .. %.2f over %d rounds)" % (dt, med[dt], min(ms[dt]), max(ms[dt]), len(ms[dt])))
    if len(dtypes) == 2:
        emit("loss + gradient: fp32 / bf16 time ratio (medians): %.2fx" % (med["fp32"] / med["bf16"]))
    if args.skip_step:
        return finish(args, lines)

    # ---- 2. the train step around it
    def make_step(dt):
        G = PM.make_upscaler_orig((s, s, 3), kernel_size=3, upscale_factor=2, res_block_num=args.res_blocks, seed=7, trunk_dtype="bf16+tail")
        D = PM.make_discriminator_patchgan_70((s, s, 3), seed=11, dtype="bf16")
        _, _, gan = PM.make_and_compile_gan2(G, D, (s // 2, s // 2, 3), (s, s, 3), loss[dt].loss, 1.0, lambda: PM.WassersteinLosses(), 1e-2,
                                             optimizer=PM.Adam())
        gan.trainer.capture_train_step(lr, hr)
        return gan.trainer
    steps = {dt: make_step(dt) for dt in dtypes}
    ms = {dt: [] for dt in dtypes}
    for r in range(args.rounds):
        for dt in dtypes:
            tr = steps[dt]
            t = timed(lambda: tr.train_step_graph(lr, hr, read_losses=False), args.iters, args.warmup)
            losses = tr.train_step_graph(lr, hr)
            if not all(np.isfinite(v) for v in losses):
                raise RuntimeError("%s: non-finite losses %r" % (dt, losses))
            ms[dt].append(t)
            emit(json.dumps({"bench": "train_step_vgg_mse", "generator": "bf16+tail", "critic": "patchgan bf16", "extractor": dt, "round": r, "batch": bs,
                             "size": s, "res_blocks": args.res_blocks, "iters": args.iters, "ms_per_step": round(t, 3),
                             "frames_per_s": round(bs * 1000.0 / t, 2), "losses": ["%.6g" % v for v in losses]}))
    med = {dt: statistics.median(ms[dt]) for dt in dtypes}
    for dt in dtypes:
        emit("train step, %s extractor: median %.2f ms/step (range %.2f .. %.2f over %d rounds) = %.1f frames/s"
             % (dt, med[dt], min(ms[dt]), max(ms[dt]), len(ms[dt]), bs * 1000.0 / med[dt]))
    if len(dtypes) == 2:
        emit("train step: fp32 / bf16 time ratio (medians): %.2fx" % (med["fp32"] / med["bf16"]))
    finish(args, lines)


def finish(args, lines):
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
