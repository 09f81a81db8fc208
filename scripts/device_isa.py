#!/usr/bin/env python3
"""Dump the gfx950 device assembly of every library source, for comparing two commits.

    python scripts/device_isa.py OUTDIR [SOURCE.hip ...]

Writes OUTDIR/<source>.s (hipcc -S --cuda-device-only with build.py's flags, minus the lines that carry
the per-translation-unit `__hip_cuid_` hash of the source text) and, for a full run, OUTDIR/SHA256SUMS.  A refactor that
must not change device code produces the same SHA256SUMS at its parent and at its head.
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-cycle_gan-upscaling_amd"))
import build as B  # noqa: E402


def dump(outdir, src):
    out = os.path.join(outdir, src.replace(".hip", ".s"))
    raw = out + ".raw"
    subprocess.run([B._hipcc(), "-S", "--cuda-device-only", os.path.join(B.CSRC, src), "-o", raw] + B.FLAGS,
                   check=True)
    with open(raw) as f:
        text = "".join(line for line in f if "__hip_cuid_" not in line)
    os.remove(raw)
    with open(out, "w") as f:
        f.write(text)
    return src, hashlib.sha256(text.encode()).hexdigest()


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    outdir = os.path.abspath(argv[1])
    os.makedirs(outdir, exist_ok=True)
    sources = argv[2:] or B.SOURCES
    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "4"))) as ex:
        sums = list(ex.map(lambda s: dump(outdir, s), sources))
    lines = "".join(f"{h}  {src}\n" for src, h in sums)
    sys.stdout.write(lines)
    if not argv[2:]:
        with open(os.path.join(outdir, "SHA256SUMS"), "w") as f:
            f.write(lines)


if __name__ == "__main__":
    main(sys.argv)
