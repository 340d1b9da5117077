"""Host model of the device-side collect (e2sar_hip_reas_collect) -- TEST INFRASTRUCTURE.

The model restates the contract of include/e2sar_hip.h, not the kernels: which completed
records a call takes, where each taken event sits in the output buffer, and the four counts.
Plain Python integers, so no offset can wrap.

A record is ``(eventNum, dataId, bytes, numFragments)``; ``records_of`` makes them from what
``DeviceReassembler.poll`` returns.
"""
from __future__ import annotations

import numpy as np

COLLECT_REC = np.dtype([("eventNum", "<u8"), ("outOffset", "<u8"), ("bytes", "<u4"), ("dataId", "<u2"),
                        ("flags", "<u2"), ("numFragments", "<u4"), ("reserved", "<u4")])
TRUNCATED = 1


def records_of(polled):
    return [(int(r.eventNum), int(r.dataId), int(r.bytes), int(r.numFragments)) for r in polled]


def roundup(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def layout(records, first, max_events, out_bytes, pitch=0, align=256, queue_capacity=None):
    """-> (rows, counts).  rows: COLLECT_REC array of the taken events (``reserved`` left 0:
    it is the library's); counts: [n, bytes of out spanned, records left, event bytes copied].

    records: every record the reassembler completed, in completion order; only the first
    queue_capacity of them are stored.  The call sees records [first, first + avail)."""
    if align == 0:
        align = 256
    if pitch % 16 or align < 16 or align > 4096 or align & (align - 1) or max_events <= 0:
        raise ValueError("bad collect arguments")
    stored = len(records) if queue_capacity is None else min(len(records), queue_capacity)
    avail = max(0, stored - first)
    taken, off, copied, spanned = [], 0, 0, 0
    for i in range(min(avail, max_events)):
        ev, did, nbytes, frags = records[first + i]
        if pitch:
            if (i + 1) * pitch > out_bytes:
                break
            taken.append((ev, i * pitch, nbytes, did, TRUNCATED if nbytes > pitch else 0, frags, 0))
            copied += min(nbytes, pitch)
            spanned = (i + 1) * pitch
        else:
            if off + nbytes > out_bytes:          # the first event that does not fit ends the call
                break
            taken.append((ev, off, nbytes, did, 0, frags, 0))
            copied += nbytes
            off += roundup(nbytes, align)
            spanned = off
    n = len(taken)
    return np.array(taken, dtype=COLLECT_REC), [n, spanned, avail - n, copied]


def expected_out(before: np.ndarray, rows, sources, pitch=0) -> np.ndarray:
    """The output buffer after a collect over a buffer that held `before`: event i's bytes
    (sources[i]) at its offset, in row mode cut to the pitch and zero-filled up to it; every
    other byte as it was."""
    out = before.copy()
    for row, src in zip(rows, sources):
        o, b = int(row["outOffset"]), int(row["bytes"])
        assert len(src) == b
        if pitch:
            out[o:o + pitch] = 0
            b = min(b, pitch)
        out[o:o + b] = src[:b]
    return out
