#!/usr/bin/env python
"""The training step of the reference driver's default generator (train_gan3.py:55 -gm resnet-att): make_upscaler_attention with
make_discriminator_patchgan_70 inside make_and_compile_gan2, the faithful three-call step (predict, disc_train, gan_train) as one captured
(hipGraph) train step, with the fp32 trunk and with trunk_dtype='bf16'.

    python scripts/bench_train_attention.py [--config default|k3x2|both] [--rounds 3] [--steps 10] [--warmup 3] [--tail] [--out FILE]

Configurations: 'default' is the reference's (kernel_size 5, 16 residual blocks, x4, 128 -> 512, batch 8), 'k3x2' is kernel_size 3, x2,
256 -> 512.  Per configuration the fp32-trunk and the bf16-trunk pair are built in one process and timed in alternating rounds (fp32,
bf16, fp32, bf16, ...), so both see the same machine state; the critic is the same bf16 PatchGAN in both, so the two steps differ by the
generator's trunk alone.  One JSON line per round, then the medians, the ranges (the spread of the repeated rounds) and whether the bf16
step is faster by more than that spread (appended to --out).  Times are device events around `steps` replays of the captured step, after
`warmup` replays; frames/s = batch * steps / time.

--tail adds a third leg to the alternation, trunk_dtype='bf16' with tail_dtype='bf16' (fp32, bf16, bf16+tail, fp32, ...), and compares it
with the bf16-trunk / fp32-tail leg of the same process: the two differ by the up-sampling blocks and final/conv alone."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-cycle_gan-upscaling_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = {"default": dict(kernel_size=5, res_block_num=16, upscale_factor=4, size=128),
           "k3x2": dict(kernel_size=3, res_block_num=16, upscale_factor=2, size=256)}


LEGS = {"fp32": dict(trunk_dtype="fp32"), "bf16": dict(trunk_dtype="bf16"), "bf16+tail": dict(trunk_dtype="bf16", tail_dtype="bf16")}


def make_step(leg, cfg, batch):
    import numpy as np
    from upscaler import model as PM, _engine as E
    h, f = cfg["size"], cfg["upscale_factor"]
    G = PM.make_upscaler_attention((f * h, f * h, 3), kernel_size=cfg["kernel_size"], upscale_factor=f, res_block_num=cfg["res_block_num"],
                                   **LEGS[leg])
    D = PM.make_discriminator_patchgan_70((f * h, f * h, 3), seed=11, dtype="bf16")
    _, _, gan = PM.make_and_compile_gan2(G, D, (h, h, 3), (f * h, f * h, 3), "mse", 1.0, lambda: PM.WassersteinLosses(), 1e-2, optimizer=PM.Adam())
    tr = gan.trainer
    rng = np.random.RandomState(5)
    lr = E.to_device_nchw(tr.rt, (rng.randint(0, 256, (batch, h, h, 3)) / 127.5 - 1).astype(np.float32))
    hr = E.to_device_nchw(tr.rt, (rng.randint(0, 256, (batch, f * h, f * h, 3)) / 127.5 - 1).astype(np.float32))
    tr.capture_train_step(lr, hr)
    return tr, lr, hr


def time_round(step, steps, warmup):
    import torch
    tr, lr, hr = step
    for _ in range(warmup):
        tr.train_step_graph(lr, hr, read_losses=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        tr.train_step_graph(lr, hr, read_losses=False)
    e1.record()
    torch.cuda.synchronize()
    losses = tr.train_step_graph(lr, hr)
    return e0.elapsed_time(e1) / steps, losses


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("default", "k3x2", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tail", action="store_true", help="add the trunk_dtype='bf16', tail_dtype='bf16' leg to the alternation")
    ap.add_argument("--out", default=None, help="append the printed lines to this file")
    args = ap.parse_args()
    import numpy as np
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for name in (("default", "k3x2") if args.config == "both" else (args.config,)):
        cfg = CONFIGS[name]
        dtypes = ("fp32", "bf16", "bf16+tail") if args.tail else ("fp32", "bf16")
        steps = {dt: make_step(dt, cfg, args.batch) for dt in dtypes}
        ms = {dt: [] for dt in dtypes}
        for r in range(args.rounds):
            for dt in dtypes:
                t, losses = time_round(steps[dt], args.steps, args.warmup)
                if not all(np.isfinite(v) for v in losses):
                    raise RuntimeError("%s %s: non-finite losses %r" % (name, dt, losses))
                ms[dt].append(t)
                emit(json.dumps({"bench": "train_attention", "config": name, "trunk_dtype": LEGS[dt]["trunk_dtype"], "tail_dtype": LEGS[dt].get("tail_dtype", "fp32"), "round": r, "batch": args.batch, "in": cfg["size"],
                                 "out": cfg["upscale_factor"] * cfg["size"], "kernel_size": cfg["kernel_size"], "res_blocks": cfg["res_block_num"],
                                 "steps": args.steps, "ms_per_step": round(t, 3), "frames_per_s": round(args.batch * 1000.0 / t, 2),
                                 "losses": ["%.6g" % v for v in losses]}))
        for dt in dtypes:
            m = statistics.median(ms[dt])
            emit("%s, %s" % (name, "bf16 trunk and tail" if dt == "bf16+tail" else dt + " trunk") + ": median %.2f ms/step (range %.2f .. %.2f over %d rounds) = %.1f frames/s"
                 % (m, min(ms[dt]), max(ms[dt]), len(ms[dt]), args.batch * 1000.0 / m))
        spread = max(max(ms[dt]) - min(ms[dt]) for dt in ("fp32", "bf16"))
        gain = statistics.median(ms["fp32"]) - statistics.median(ms["bf16"])
        emit("%s: fp32 / bf16-trunk step time (medians) %.2fx; the bf16-trunk step is %.2f ms %s, the spread of the rounds is %.2f ms: %s"
             % (name, statistics.median(ms["fp32"]) / statistics.median(ms["bf16"]), abs(gain), "faster" if gain > 0 else "slower", spread,
                "faster by more than the spread" if gain > spread else "NOT faster by more than the spread"))
        if args.tail:
            spread = max(max(ms[dt]) - min(ms[dt]) for dt in ("bf16", "bf16+tail"))
            gain = statistics.median(ms["bf16"]) - statistics.median(ms["bf16+tail"])
            emit("%s: bf16-trunk / bf16-trunk-and-tail step time (medians) %.2fx; the bf16-tail step is %.2f ms %s, the spread of the rounds is %.2f ms: %s"
                 % (name, statistics.median(ms["bf16"]) / statistics.median(ms["bf16+tail"]), abs(gain), "faster" if gain > 0 else "slower", spread,
                    "faster by more than the spread" if gain > spread else "NOT faster by more than the spread"))
        del steps
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
