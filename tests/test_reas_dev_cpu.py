"""e2sar_hip_reassemble_batch_dev without a GPU: the declaration and its binding, the argument
checks of DeviceReassembler.reassemble_dev in front of the library call, and what the
compiler made of the device-count kernels next to the kernels they wrap."""
import ctypes as C
import os
import re
import shutil

import pytest

from test_kernel_resources import HIPCC, SOURCES, _remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "e2sar_hip_reassemble_batch_dev"


def test_header_declares_it_and_the_table_binds_it():
    from e2sar_amd import _capi
    text = open(os.path.join(ROOT, "include", "e2sar_hip.h")).read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "not declared in include/e2sar_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["e2sar_hip_reas *r", "const uint8_t *d_packets", "uint32_t stride", "const uint32_t *d_lens",
                      "const uint32_t *d_count", "uint32_t maxPackets", "uint64_t now_ms", "void *stream"]
    res, args = _capi.SIGNATURES[NAME]
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    assert res is C.c_int and args == [vp, vp, u32, vp, vp, u32, u64, vp]
    assert "E2SAR_HIP_ABI_VERSION 1\n" in text


@pytest.fixture
def stubbed(monkeypatch):
    """A DeviceReassembler that owns no handle, and sar._call recording instead of calling."""
    import torch
    from e2sar_amd import sar
    calls = []
    monkeypatch.setattr(sar, "_call", lambda name, *args: calls.append((name, args)) or 0)
    monkeypatch.setattr(sar, "_s", lambda stream: 0x51)
    R = object.__new__(sar.DeviceReassembler)
    R._h = C.c_void_p()
    return R, calls, torch


def test_reassemble_dev_checks_before_the_library_call(stubbed):
    R, calls, torch = stubbed
    stride = 1472
    packets = torch.zeros(10 * stride + 256, dtype=torch.uint8)
    lens = torch.zeros(8, dtype=torch.int32)
    counts = torch.zeros(8, dtype=torch.int32)
    bad = [
        dict(count=counts[1:2].to(torch.int64)),                       # dtype
        dict(count=counts[1:2].to(torch.uint8)),
        dict(lens=lens.to(torch.int64)),
        dict(packets=packets.to(torch.int8)),
        dict(count=torch.zeros(1, dtype=torch.int32, device="meta")),  # another device than the batch
        dict(count=counts[1:1]),                                       # empty
        dict(max_packets=9),                                           # more than lens holds
        dict(max_packets=8, packets=packets[: 8 * stride - 1]),        # more than packets holds
    ]
    for kw in bad:
        args = dict(packets=packets, stride=stride, lens=lens, count=counts[1:2])
        args.update(kw)
        with pytest.raises(ValueError):
            R.reassemble_dev(**args)
    assert calls == []
    # a good call: the count view's own address, the bound from what the buffers hold
    R.reassemble_dev(packets, stride, lens, counts[1:2], now_ms=7)
    R.reassemble_dev(packets, stride, lens, counts[1:2], max_packets=3)
    assert calls == [(NAME, (R._h, packets.data_ptr(), stride, lens.data_ptr(), counts.data_ptr() + 4, 8, 7, 0x51)),
                     (NAME, (R._h, packets.data_ptr(), stride, lens.data_ptr(), counts.data_ptr() + 4, 3, 0, 0x51))]


# the device-count kernels, how many instantiations the launchers use, and the kernel each wraps
FAMILIES = {"reas_dev_kernel": (2, "reas_kernel"), "reas_classify_dev_kernel": (1, "reas_classify_kernel"),
            "reas_scatter_dev_kernel": (6, "reas_scatter_kernel")}


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc absent")
def test_device_count_kernels_cost_no_wave(tmp_path):
    kernels = _remarks(SOURCES[0], tmp_path)
    of = lambda n: {k: v for k, v in kernels.items() if f"9e2sar_amd{len(n)}{n}" in k}     # mangled e2sar_amd::NAME
    for name, (want, wraps) in FAMILIES.items():
        mine, theirs = of(name), of(wraps)
        assert len(mine) == want, (name, sorted(mine))
        assert theirs, wraps
        bad = {k: v for k, v in mine.items() if v.get("ScratchSize", 0) or v.get("VGPRs Spill", 0) or v.get("SGPRs Spill", 0)}
        assert not bad, f"scratch or spills: {bad}"
        low, low0 = min(v["Occupancy"] for v in mine.values()), min(v["Occupancy"] for v in theirs.values())
        assert low >= low0, f"{name}: occupancy {low} waves/SIMD below {wraps}'s {low0}"
