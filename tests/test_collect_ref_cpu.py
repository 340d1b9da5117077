"""The host model of the device-side collect against answers written out by hand, and the
three places that must agree on the index record: the C header, the ctypes struct and the
numpy dtype (CPU only)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import collect_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recs(sizes, ev0=100):
    return [(ev0 + k, 7, b, 1 + b // 1000) for k, b in enumerate(sizes)]


def _offsets(rows):
    return [int(x) for x in rows["outOffset"]]


def test_align_prefix_sums():
    sizes = [1, 16, 17, 255, 256, 257, 0, 5000]
    rows, counts = M.layout(_recs(sizes), 0, 64, 1 << 20, align=16)
    assert _offsets(rows) == [0, 16, 32, 64, 320, 576, 848, 848]
    assert counts == [8, 848 + 5008, 0, sum(sizes)]
    rows, counts = M.layout(_recs(sizes), 0, 64, 1 << 20, align=256)
    assert _offsets(rows) == [0, 256, 512, 768, 1024, 1280, 1792, 1792]
    assert counts == [8, 1792 + 5120, 0, sum(sizes)]
    rows, counts = M.layout(_recs(sizes), 0, 64, 1 << 20, align=4096)
    assert _offsets(rows) == [0, 4096, 8192, 12288, 16384, 20480, 24576, 24576]
    assert counts[1] == 24576 + 8192
    assert M.layout(_recs(sizes), 0, 64, 1 << 20, align=0)[1] == [8, 1792 + 5120, 0, sum(sizes)]   # 0 means 256
    assert [int(x) for x in rows["eventNum"]] == list(range(100, 108))
    assert [int(x) for x in rows["bytes"]] == sizes and not rows["flags"].any()


def test_capacity_cut_at_end_and_one_short():
    sizes = [100, 300, 50, 10]
    # align 256: offsets 0, 256, 768, 1024; event 2 ends at 818
    rows, counts = M.layout(_recs(sizes), 0, 64, 818)
    assert counts == [3, 1024, 1, 450] and _offsets(rows) == [0, 256, 768]
    rows, counts = M.layout(_recs(sizes), 0, 64, 817)
    assert counts == [2, 768, 2, 400]
    # record order is kept: event 3 (10 bytes) would fit behind event 1, but event 2 did not
    assert M.layout(_recs(sizes), 0, 64, 780)[1] == [2, 768, 2, 400]
    # the resumed call starts at offset 0 again
    rows, counts = M.layout(_recs(sizes), 2, 64, 817)
    assert counts == [2, 512, 0, 60] and _offsets(rows) == [0, 256]
    assert M.layout(_recs(sizes), 0, 64, 0)[1] == [0, 0, 4, 0]
    assert M.layout(_recs(sizes), 0, 2, 1 << 20)[1] == [2, 768, 2, 400]          # max_events cuts too


def test_row_mode_cut_and_truncated_flag():
    sizes = [1, 4096, 4097, 20000, 16, 15, 0]
    rows, counts = M.layout(_recs(sizes), 0, 64, 1 << 20, pitch=4096)
    assert _offsets(rows) == [4096 * k for k in range(7)]
    assert [int(f) for f in rows["flags"]] == [0, 0, 1, 1, 0, 0, 0]
    assert [int(b) for b in rows["bytes"]] == sizes                   # the full length, also when truncated
    assert counts == [7, 7 * 4096, 0, 1 + 4096 + 4096 + 4096 + 16 + 15]
    assert M.layout(_recs(sizes), 0, 64, 5 * 4096 + 15, pitch=4096)[1] == [5, 5 * 4096, 2, 1 + 3 * 4096 + 16]
    assert M.layout(_recs(sizes), 0, 64, 4095, pitch=4096)[1] == [0, 0, 7, 0]
    assert M.layout(_recs(sizes), 0, 3, 1 << 20, pitch=16)[1] == [3, 48, 4, 1 + 16 + 16]


def test_cursor_past_the_end_and_queue_clamp():
    recs = _recs([10] * 5)
    assert M.layout(recs, 5, 8, 4096)[1] == [0, 0, 0, 0]
    assert M.layout(recs, 9, 8, 4096)[1] == [0, 0, 0, 0]
    # 5 completed, 3 stored: the records past the queue's capacity were lost
    rows, counts = M.layout(recs, 0, 8, 4096, queue_capacity=3)
    assert counts == [3, 768, 0, 30]
    assert M.layout(recs, 1, 8, 4096, queue_capacity=3)[1] == [2, 512, 0, 20]
    assert M.layout(recs, 3, 8, 4096, queue_capacity=3)[1] == [0, 0, 0, 0]
    assert M.layout(recs, 4, 8, 4096, queue_capacity=3)[1] == [0, 0, 0, 0]


def test_offsets_pass_4_gib():
    recs = _recs([8 << 20] * 1024)
    rows, counts = M.layout(recs, 0, 1024, 1 << 40)
    assert int(rows["outOffset"][511]) == 511 * (8 << 20) < 1 << 32
    assert int(rows["outOffset"][512]) == 1 << 32
    assert int(rows["outOffset"][1023]) == 1023 * (8 << 20)
    assert counts == [1024, 1 << 33, 0, 1 << 33]
    rows, counts = M.layout(_recs([(1 << 32) - 1] * 3), 0, 8, 1 << 40, align=4096)
    assert _offsets(rows) == [0, 1 << 32, 1 << 33] and counts[1] == 3 << 32
    rows, counts = M.layout(_recs([100] * 3), 0, 8, 1 << 40, pitch=(1 << 32) - 16)
    assert _offsets(rows) == [0, (1 << 32) - 16, (1 << 33) - 32]


def test_bad_arguments_are_refused():
    for kw in ({"pitch": 8}, {"align": 8}, {"align": 48}, {"align": 8192}):
        with pytest.raises(ValueError):
            M.layout(_recs([1]), 0, 4, 4096, **kw)
    with pytest.raises(ValueError):
        M.layout(_recs([1]), 0, 0, 4096)


def test_expected_out_row_and_ragged():
    before = np.full(64, 0xEE, np.uint8)
    rows, _ = M.layout(_recs([3, 20]), 0, 4, 64, pitch=16)
    got = M.expected_out(before, rows, [np.arange(1, 4, dtype=np.uint8), np.arange(1, 21, dtype=np.uint8)], pitch=16)
    assert got[:16].tolist() == [1, 2, 3] + [0] * 13 and got[16:32].tolist() == list(range(1, 17))
    assert (got[32:] == 0xEE).all()
    rows, _ = M.layout(_recs([3, 20]), 0, 4, 64, align=16)
    got = M.expected_out(before, rows, [np.arange(1, 4, dtype=np.uint8), np.arange(1, 21, dtype=np.uint8)])
    assert got[:16].tolist() == [1, 2, 3] + [0xEE] * 13 and got[16:36].tolist() == list(range(1, 21))
    assert (got[36:] == 0xEE).all()


# ---- the index record in the header, the ctypes binding and the numpy dtype ----

def test_header_declares_the_collect_entry_point():
    src = open(os.path.join(ROOT, "include", "e2sar_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+e2sar_hip_reas_collect\s*\(", src)
    body = re.search(r"typedef struct e2sar_hip_collect_rec \{(.*?)\} e2sar_hip_collect_rec;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [
        ("uint64_t", "eventNum"), ("uint64_t", "outOffset"), ("uint32_t", "bytes"), ("uint16_t", "dataId"),
        ("uint16_t", "flags"), ("uint32_t", "numFragments"), ("uint32_t", "reserved")]
    assert re.search(r"#define\s+E2SAR_HIP_COLLECT_TRUNCATED\s+1u?\b", src)
    assert re.search(r"#define\s+E2SAR_HIP_ABI_VERSION\s+1\b", src)


def test_ctypes_collect_rec_layout():
    from e2sar_amd import _capi
    assert C.sizeof(_capi.CollectRec) == 32
    assert _capi.CollectRec.outOffset.offset == 8 and _capi.CollectRec.reserved.offset == 28
    assert _capi.COLLECT_TRUNCATED == 1 == M.TRUNCATED
    assert "e2sar_hip_reas_collect" in _capi.SIGNATURES


def test_numpy_collect_rec_layout():
    from e2sar_amd import _capi, sar
    assert sar.COLLECT_REC.itemsize == 32 == sar.COLLECT_REC_BYTES
    assert sar.COLLECT_REC == M.COLLECT_REC
    for name, _ in _capi.CollectRec._fields_:
        assert sar.COLLECT_REC.fields[name][1] == getattr(_capi.CollectRec, name).offset, name
