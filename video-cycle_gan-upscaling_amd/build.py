"""Build libvcg_hip.so (gfx950) in-tree with hipcc.  Usage: python build.py [--force]"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libvcg_hip.so")
SOURCES = ["conv_fwd.hip", "conv_rowchain.hip", "conv_transpose.hip", "conv_wgrad.hip", "norm.hip", "elementwise.hip", "dense.hip", "bf16_layout.hip", "bf16_conv3x3_3ch.hip", "bf16_convt3x3.hip", "bf16_conv9x9_to3.hip", "bf16_norm.hip", "bf16_wgrad.hip", "bf16_wgrad9.hip", "bf16_gconv.hip", "bf16_gwgrad.hip", "bf16_head.hip", "bf16_wgrad3.hip", "bf16_attn.hip", "bf16_incep.hip", "bf16_vgg.hip", "api.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
         "-Wno-unused-value", "-Wno-c++20-extensions"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True, extra_flags=(), objdir=None, out=OUT, jobs=4):
    """Compile SOURCES and link them into `out`.  The defaults build libvcg_hip.so; a diagnostic build (scripts/micro/stamps.py) passes
    extra -D flags and an object directory and output of its own, so that it never touches the shipped library or its objects."""
    hipcc = _hipcc()
    objdir = objdir or os.path.join(HERE, "build")
    flags = FLAGS + list(extra_flags)
    hdrs = sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(ROOT, "include", "vcg.h")]
    objs, cmds = [], []
    os.makedirs(objdir, exist_ok=True)
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            cmds.append([hipcc, "-c", src, "-o", obj] + flags)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(run, cmds))
    if force or cmds or _stale(out, objs):
        run([hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", out] + objs)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
