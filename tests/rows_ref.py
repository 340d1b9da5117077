"""Host model of the rows family (e2sar_hip_rows_reassemble / _advance / _clear) -- TEST
INFRASTRUCTURE (tests/test_rows_ref_cpu.py, tests/test_gpu_rows.py).

Restates the contract in include/e2sar_hip.h in plain Python integers, one datagram after the
other; it knows nothing of waves, runs or groups.  On streams that send no fragment twice and
keep the opener of every cell determinate within a launch, the kernel must agree with it byte
for byte, whatever the order of the datagrams and however the stream is cut into launches.
"""
from __future__ import annotations

import numpy as np

COMPLETE, TRUNCATED = 1, 2
ACC_SHIFT = 36
M64 = (1 << 64) - 1
FILL = 0xA5                 # what `out` holds before anything is written

(C_COMPLETE, C_ACCEPTED, C_BYTES, C_LATE, C_EARLY, C_FOREIGN, C_BAD_HEADER, C_DATA_ERR, C_RELEASED,
 C_RELEASED_COMPLETE) = range(10)


def check_descriptor(ids, n_events, pitch):
    """The descriptor rules of the header: what a PARAMETER status refuses."""
    ids = list(ids)
    return (1 <= len(ids) <= 64 and len(set(ids)) == len(ids) and n_events > 0 and n_events & (n_events - 1) == 0
            and pitch > 0 and pitch % 256 == 0)


class Window:
    def __init__(self, ids, n_events, pitch, event_base=0, with_lb=True, fill=FILL):
        assert check_descriptor(ids, n_events, pitch)
        self.ids = [int(d) for d in ids]
        self.n_events, self.pitch, self.with_lb = n_events, pitch, with_lb
        self.hl = 36 if with_lb else 20
        self.out = np.full((n_events, len(self.ids), pitch), fill, np.uint8)
        self.clear(event_base)

    # ---- state ----
    def clear(self, event_base=0):
        n = self.n_events * len(self.ids)
        self.cur = [0] * n          # curBytes
        self.frags = [0] * n
        self.bytes = [0] * n        # S; 0 = empty
        self.flags = [0] * n
        self.counts = [0] * 16
        self.base = event_base & M64

    def cell_index(self, ev, data_id):
        return (ev & (self.n_events - 1)) * len(self.ids) + self.ids.index(data_id)

    def cells(self):
        """-> [(acc, bytes, flags)] per cell, as the device holds them."""
        return [((f << ACC_SHIFT) | c, b, fl) for c, f, b, fl in zip(self.cur, self.frags, self.bytes, self.flags)]

    # ---- one datagram ----
    def push(self, slot: bytes, length: int, stride: int):
        """slot: the datagram's slot (stride bytes); length: its d_lens entry."""
        cnt = self.counts
        if length < self.hl:
            cnt[C_BAD_HEADER] += 1
            return
        if length > stride:
            cnt[C_DATA_ERR] += 1
            return
        re = slot[self.hl - 20:self.hl]
        if re[0] != 0x10 or re[1] != 0:
            cnt[C_BAD_HEADER] += 1
            return
        data_id = int.from_bytes(re[2:4], "big")
        off = int.from_bytes(re[4:8], "big")
        blen = int.from_bytes(re[8:12], "big")
        ev = int.from_bytes(re[12:20], "big")
        pl = length - self.hl
        if data_id not in self.ids:
            cnt[C_FOREIGN] += 1
            return
        d = (ev - self.base) & M64
        if d >= self.n_events:
            cnt[C_LATE if d >> 63 else C_EARLY] += 1
            return
        if blen == 0 or off + pl > blen:
            cnt[C_DATA_ERR] += 1
            return
        c = self.cell_index(ev, data_id)
        if self.bytes[c] == 0:
            self.bytes[c] = blen
        S = self.bytes[c]
        if off + pl > S:
            cnt[C_DATA_ERR] += 1
            return
        take = min(pl, max(0, self.pitch - off))
        if take:
            row = self.out.reshape(-1, self.pitch)[c]
            row[off:off + take] = np.frombuffer(slot[self.hl:self.hl + take], np.uint8)
        if off + pl > self.pitch:
            self.flags[c] |= TRUNCATED
        self.cur[c] += pl
        self.frags[c] += 1
        cnt[C_ACCEPTED] += 1
        cnt[C_BYTES] += pl
        if pl > 0 and self.cur[c] == S:
            self.flags[c] |= COMPLETE
            cnt[C_COMPLETE] += 1

    def apply(self, pk: np.ndarray, ln, stride=None, count=None):
        """The batch's datagrams [0, n), n = min(count, len(ln)) (count None: all)."""
        pk = np.ascontiguousarray(pk, np.uint8)
        stride = stride or pk.shape[1]
        n = len(ln) if count is None else min(int(count), len(ln))
        for p in range(n):
            self.push(pk[p].tobytes(), int(ln[p]), stride)

    # ---- the ring ----
    def advance(self, k_max, k_dev=None):
        k = min(k_max, self.n_events)
        if k_dev is not None:
            k = min(k, int(k_dev))
        nid = len(self.ids)
        for e in range(k):
            r = (self.base + e) & (self.n_events - 1)
            for j in range(nid):
                c = r * nid + j
                if self.flags[c] & COMPLETE:
                    self.counts[C_RELEASED_COMPLETE] += 1
                elif self.bytes[c] != 0:
                    self.counts[C_RELEASED] += 1
                self.cur[c] = self.frags[c] = self.bytes[c] = self.flags[c] = 0
        self.base = (self.base + k) & M64
