"""Every header of e2sar_amd/csrc compiles on its own: each includes what it uses.

The device code of sar_kernels.hip sits in one header per subsystem; a header that leans on
what another happened to include before it would break the next reordering of the unit.
"""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADERS = sorted(os.path.relpath(p, ROOT) for p in glob.glob(os.path.join(ROOT, "e2sar_amd", "csrc", "*.hpp")))


def test_headers_found():
    assert len(HEADERS) >= 12, HEADERS


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("hdr", HEADERS)
def test_header_compiles_alone(hdr):
    r = subprocess.run([HIPCC, "-x", "hip", "-std=c++17", "--offload-arch=gfx950", "-Iinclude", "-Ie2sar_amd/csrc",
                        "-Wno-pragma-once-outside-header", "-fsyntax-only", hdr],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
