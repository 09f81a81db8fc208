"""The diagnostic stamp build (-DVCG_STAMPS, csrc/vcg_stamps.hpp, scripts/micro/stamps.py) keeps compiling: the code under its #ifdef is in
no shipped library, so nothing else sees it rot.  Syntax only (hipcc -fsyntax-only, host and device pass): no library is built or loaded."""
import glob
import os
import subprocess

import pytest

import build as B

STAMPED = sorted(os.path.basename(p) for p in glob.glob(os.path.join(B.CSRC, "*.hip")) if '#include "vcg_stamps.hpp"' in open(p).read())


def test_the_stamped_sources_are_library_sources():
    assert set(STAMPED) <= set(B.SOURCES), STAMPED
    families = sum(open(os.path.join(B.CSRC, s)).read().count("\nVCG_STAMP_SUMS(") for s in STAMPED)
    assert families == 5, (families, STAMPED)           # v2, i9, ct, f9, wg


@pytest.mark.parametrize("src", STAMPED)
def test_source_compiles_with_stamps(src):
    r = subprocess.run([B._hipcc(), "-fsyntax-only", os.path.join(B.CSRC, src)] + B.FLAGS + ["-DVCG_STAMPS"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
