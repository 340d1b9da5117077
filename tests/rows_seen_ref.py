"""Host model of the seen calls (e2sar_hip_rows_reassemble_seen / _advance_seen / _clear_seen) --
TEST INFRASTRUCTURE (tests/test_rows_seen_cpu.py, tests/test_gpu_rows_seen.py).

The contract of include/e2sar_hip.h in plain Python integers, on top of rows_ref.Window: a datagram
goes through rules 4b and 5b here and, unless one of them stops it, through rows_ref.Window.push as
it is -- so a stream that repeats nothing and lies on the grid gives what rows_ref gives.  A window
on a lattice is this model fed rows_strided_ref.renumber's stream, as for the plain calls.
"""
from __future__ import annotations

import rows_ref as RR
import rows_strided_ref as RS

C_DUPLICATE = 11


def magic(d: int) -> int:
    """The host's multiplier for n // d (rows_div_magic)."""
    return ((1 << 64) - 1) // d


def div(n: int, d: int):
    """(n // d, n % d) the way the kernel finds it (rows_div): the high half of n * magic(d) and
    one correction."""
    q = (n * magic(d)) >> 64
    r = n - q * d
    if r >= d:
        q, r = q + 1, r - d
    return q, r


class SeenWindow(RR.Window):
    def __init__(self, ids, n_events, pitch, frag_bytes, max_frags, event_base=0, with_lb=True, fill=RR.FILL):
        assert frag_bytes > 0 and max_frags > 0 and max_frags % 128 == 0
        self.frag_bytes, self.max_frags = frag_bytes, max_frags
        super().__init__(ids, n_events, pitch, event_base, with_lb, fill)

    def clear(self, event_base=0):
        super().clear(event_base)
        self.seen = [0] * (self.n_events * len(self.ids))        # per cell: bit f set <=> fragment f accepted

    def seen_words(self):
        """-> per cell, its max_frags // 32 words as the device holds them."""
        return [[(s >> (32 * k)) & 0xFFFFFFFF for k in range(self.max_frags // 32)] for s in self.seen]

    def push(self, slot: bytes, length: int, stride: int):
        # what rules 1-4 stop is rows_ref's business
        if RS.header_valid(slot, length, stride, self.with_lb):
            re = slot[self.hl - 20:self.hl]
            data_id = int.from_bytes(re[2:4], "big")
            off = int.from_bytes(re[4:8], "big")
            blen = int.from_bytes(re[8:12], "big")
            ev = int.from_bytes(re[12:20], "big")
            pl = length - self.hl
            inside = data_id in self.ids and ((ev - self.base) & RR.M64) < self.n_events
            if inside and blen != 0 and off + pl <= blen and pl > 0:
                f, r = div(off, self.frag_bytes)
                if r != 0 or pl > self.frag_bytes or f >= self.max_frags:          # rule 4b
                    self.counts[RR.C_DATA_ERR] += 1
                    return
                c = self.cell_index(ev, data_id)
                S = self.bytes[c] or blen
                if off + pl <= S:                                                  # rule 5 passes it
                    if (self.seen[c] >> f) & 1:                                    # rule 5b
                        self.counts[C_DUPLICATE] += 1
                        return
                    self.seen[c] |= 1 << f
        super().push(slot, length, stride)

    def advance(self, k_max, k_dev=None):
        k = min(k_max, self.n_events)
        if k_dev is not None:
            k = min(k, int(k_dev))
        nid = len(self.ids)
        for e in range(k):
            r = (self.base + e) & (self.n_events - 1)
            for j in range(nid):
                self.seen[r * nid + j] = 0
        super().advance(k_max, k_dev)
