#!/usr/bin/env python3
"""Dump the gfx950 device assembly of every library source, for comparing two commits.

    python scripts/device_isa.py OUTDIR [--per-kernel] [SOURCE.hip ...]

Writes OUTDIR/<source>.s (hipcc -S --cuda-device-only with build.py's flags, minus the lines that carry
the per-translation-unit `__hip_cuid_` hash of the source text) and, for a full run, OUTDIR/SHA256SUMS.  A refactor that
must not change device code produces the same SHA256SUMS at its parent and at its head.

With --per-kernel it prints one `sha256  symbol` line per kernel instead, sorted by symbol, and writes them to
OUTDIR/KERNELS.sha256 (SHA256SUMS is still written).  A kernel's text runs from its `.type SYM,@function` line through its
`.end_amdhsa_kernel` (code, register counts, LDS size) with the numbering that is local to a translation unit (block labels,
func_begin / func_end, tmp) stripped, together with the padding that aligns the comment behind such a label (its width follows the
number's), so a refactor that moves kernels between files leaves this list identical.
"""
import hashlib
import os
import re
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


_TU_LOCAL = re.compile(r"((?:\.L)?(?:BB|func_begin|func_end|tmp))\d+")


def kernels(text):
    """{symbol: sha256} of every kernel in one source's assembly"""
    lines = text.splitlines(keepends=True)
    found = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        sym = m.group(1)
        start = next(i for i, line in enumerate(lines) if re.match(r"\s*\.type\s+%s,@function" % re.escape(sym), line))
        end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        body = re.sub(r"[ \t]+;", " ;", _TU_LOCAL.sub(r"\1", "".join(lines[start:end + 1])))
        assert sym not in found, sym
        found[sym] = hashlib.sha256(body.encode()).hexdigest()
    return found


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    per_kernel = "--per-kernel" in argv
    argv = [a for a in argv if a != "--per-kernel"]
    outdir = os.path.abspath(argv[1])
    os.makedirs(outdir, exist_ok=True)
    sources = argv[2:] or B.SOURCES
    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "4"))) as ex:
        sums = list(ex.map(lambda s: dump(outdir, s), sources))
    lines = "".join(f"{h}  {src}\n" for src, h in sums)
    if not argv[2:]:
        with open(os.path.join(outdir, "SHA256SUMS"), "w") as f:
            f.write(lines)
    if per_kernel:
        found = {}
        for src in sources:
            with open(os.path.join(outdir, src.replace(".hip", ".s"))) as f:
                for sym, h in kernels(f.read()).items():
                    assert sym not in found, "kernel %s is in two sources" % sym
                    found[sym] = h
        lines = "".join(f"{h}  {sym}\n" for sym, h in sorted(found.items()))
        with open(os.path.join(outdir, "KERNELS.sha256"), "w") as f:
            f.write(lines)
    sys.stdout.write(lines)


if __name__ == "__main__":
    main(sys.argv)
