"""Every gfx950 kernel compiles without scratch (private-memory) traffic or register spills.

A struct left in scratch halved seg_kernel's rate once (a reference into a by-value
struct kept the whole struct in private memory: 48 B/lane of scratch loads per round);
the compiler's resource remarks catch that on the CPU, before any GPU run.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SOURCES = ["e2sar_amd/csrc/sar_kernels.hip"]
# The kernels of the one translation unit (its device code sits in e2sar_amd/csrc/*.hpp) and
# how many instantiations of each the launchers use: a header dropped from the unit, or a
# launcher that lost a variant, fails here.
KERNELS = {
    "seg_kernel": 2, "reas_kernel": 3, "reas_classify_kernel": 1, "reas_scatter_kernel": 6,
    "reas_scatter_classify_kernel": 6, "ro_key_kernel": 1, "ro_place_kernel": 1, "ro_walk_kernel": 1,
    "zero_words_kernel": 1, "fill_bytes_kernel": 1, "copy_spans_kernel": 1, "reas_gc_kernel": 1,
    "reas_recycle_kernel": 1, "reas_compact_kernel": 1, "reas_compact_finish": 1, "relay_plan_kernel": 1,
    "route_hist_kernel": 1, "route_scan_kernel": 1, "route_pack_kernel": 1, "route_append_kernel": 1,
    "collect_plan_kernel": 1, "collect_copy_kernel": 1, "emit_plan_kernel": 1, "seg_flat_kernel": 2,
    "build_plan_kernel": 1, "build_copy_kernel": 1,
    "reas_dev_kernel": 2, "reas_classify_dev_kernel": 1, "reas_scatter_dev_kernel": 6,
    "rows_kernel": 2, "rows_release_kernel": 1, "rows_shift_kernel": 1, "rows_clear_kernel": 1,
    "turn_decide_kernel": 1, "turn_out_kernel": 1, "turn_copy_kernel": 1, "turn_back_kernel": 1,
    "collect_next_plan_kernel": 1, "collect_next_copy_kernel": 1,
}
assert sum(KERNELS.values()) == 60


def _remarks(src, tmp_path):
    out = tmp_path / (os.path.basename(src) + ".o")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only",
                        "-Iinclude", "-Ie2sar_amd/csrc", "-c", src, "-o", str(out),
                        "-Rpass-analysis=kernel-resource-usage"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("src", SOURCES)
def test_no_scratch_no_spills(src, tmp_path):
    kernels = _remarks(src, tmp_path)
    assert kernels, "no kernel resource remarks parsed"
    bad = {k: v for k, v in kernels.items()
           if v.get("ScratchSize", 0) or v.get("VGPRs Spill", 0) or v.get("SGPRs Spill", 0)}
    assert not bad, f"kernels with scratch or spills: {bad}"
    # mangled names: e2sar_amd::NAME is ...9e2sar_amd<len(NAME)>NAME...
    found = {n: sum(f"9e2sar_amd{len(n)}{n}" in k for k in kernels) for n in KERNELS}
    missing = {n: (found[n], want) for n, want in KERNELS.items() if found[n] < want}
    assert not missing, f"kernels missing from the translation unit (found, expected): {missing}"
