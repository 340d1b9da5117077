"""Hand-cut fragments for the reassembly store forms -- TEST INFRASTRUCTURE.

The segmenter cuts every event at multiples of maxPld, so its datagrams reach few of the
branches of the reassembly copy code (reas_store.hpp: scatter_chunk, da_store, edge_span,
store_dwords, store_bytes, the edge loop of lds_stage_store).  The wire format allows any
cut, so this module cuts by hand: every event is three fragments, and the middle one sits at
a chosen phase a (= bufferOffset mod 16) with a chosen length L.

    head [0, 16+a)   middle [16+a, 16+a+L)   tail [16+a+L, 16+a+L+T)

`classes` is a host model of which branch the copy code takes for a fragment.  It describes
selection only: tests use it to prove their inputs reach every branch, never as an expected
value (expected bytes come from the oracle).
"""
from __future__ import annotations

import numpy as np

import oracle_ffi as O

EV0 = 1 << 33                 # first event number (above 32 bits)
DATA_ID = 7

SMALL = [0, 1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 15, 16, 17, 19, 20, 31, 32, 33]

ALL_PHASES = list(range(16))
# slots of 8976 bytes and more: the dword phases, three odd ones and a dword-incongruent even one
FEW_PHASES = [0, 1, 2, 4, 7, 8, 12, 15]

# (stride, with_lb) of every slot layout the store-form tests use.  The launchers change
# variant at 2048 (staged cold scatter), 4096 (workgroup size, chunks per thread) and 12288
# (the jumbo scatter's one-round limit); 65520 holds a maximal UDP datagram.
CONFIGS = [(48, False), (64, False), (64, True), (80, True), (1472, True), (2048, True), (2064, True),
           (4096, True), (4112, True), (8976, True), (12288, True), (12304, True), (65520, True)]


def hdr_len(with_lb: bool) -> int:
    return 36 if with_lb else 20


def phases_for(stride: int):
    return ALL_PHASES if stride <= 4112 else FEW_PHASES


def full(stride: int, hl: int):
    """Payload lengths that end at or near the slot's end, where da_window slides its load back."""
    return [stride - hl - x for x in (0, 1, 2, 3, 4, 12, 15, 16, 17)]


def lengths_for(stride: int, with_lb: bool, matrix: str):
    return SMALL if matrix == "small" else full(stride, hdr_len(with_lb))


def dgram(ev, data_id, off, blen, payload, stride, with_lb, fill=None):
    """One datagram slot: -> (row[stride] uint8, len).  Slot bytes past the datagram are
    `fill` (random bytes of a generator, else zero): a store that takes too much shows."""
    h = O.lbre_hdr(2, ev & 0xFFFF, ev, data_id, off, blen, ev)
    if not with_lb:
        h = h[16:]
    payload = np.frombuffer(bytes(payload), np.uint8)
    n = len(h) + payload.size
    assert n <= stride
    row = fill.integers(0, 256, stride, dtype=np.uint8) if fill is not None else np.zeros(stride, np.uint8)
    row[:len(h)] = np.frombuffer(h, np.uint8)
    row[len(h):n] = payload
    return row, n


def triples(stride, with_lb, phases, lengths, T=21, seed=0, ev0=EV0):
    """One event per (a, L), cut into head, middle (phase a, length L) and tail.
    -> ((rows, lens) of heads, of mids, of tails, {(ev, id): bytes}, [(a, L)] per event).
    Events whose L is 0 come last, so a test can leave them out with a row count."""
    hl = hdr_len(with_lb)
    rng = np.random.default_rng([stride, int(with_lb), seed])
    cuts = [(a, L) for a in phases if hl + 16 + a <= stride for L in lengths if 0 <= L and hl + L <= stride]
    cuts.sort(key=lambda c: c[1] == 0)                       # stable: L == 0 last
    groups = [([], []) for _ in range(3)]
    events = {}
    for k, (a, L) in enumerate(cuts):
        ev = ev0 + k
        blen = 16 + a + L + T
        data = rng.integers(0, 256, blen, dtype=np.uint8)
        events[(ev, DATA_ID)] = data.tobytes()
        for g, (lo, hi) in zip(groups, ((0, 16 + a), (16 + a, 16 + a + L), (16 + a + L, blen))):
            row, n = dgram(ev, DATA_ID, lo, blen, data[lo:hi], stride, with_lb, fill=rng)
            g[0].append(row)
            g[1].append(n)
    out = [(np.stack(r), np.array(n, np.uint32)) for r, n in groups]
    return out[0], out[1], out[2], events, cuts


def n_nonempty(cuts) -> int:
    """Number of leading events whose middle fragment is not empty."""
    return sum(1 for _, L in cuts if L > 0)


# ----------------------------------------------------------------------------------
# host model of the branch choice (selection only)


def _edge_blocks(first, last):
    return sorted({c for c in (first, first + 1, last - 1, last) if first <= c <= last})


def classes(a, plen, hl, stride):
    """The classes the 16-byte blocks of a payload of plen bytes at phase a take.

    Destination-aligned form (edge_span / da_window; the fused kernel's da_store and the
    staged scatter's read-back): ("da", "whole"), ("da", "edge", 1|2|3) with ("da", "first-edge",
    n) for the payload's first block, ("da", "tail"), ("da", "bytes"), ("da", "single"),
    ("da", "hi", 1..16) for the last block, ("da", "sh", 0|4|8|12).
    Source-aligned form (scatter_chunk): ("sa", "whole"), ("sa", "edge", n), ("sa", "tail"),
    ("sa", "bytes"), ("sa", "single")."""
    out = set()
    if plen == 0:
        return {("empty",)}
    # destination-aligned: block c covers event bytes [16c - a, 16c - a + 16) of the payload
    last = (a + plen - 1) // 16
    for c in _edge_blocks(0, last):
        lo = a if c == 0 else 0
        hi = min(16, a + plen - 16 * c)
        if c == last:
            out.add(("da", "hi", hi))
        if a & 3:
            out.add(("da", "bytes"))
            continue
        r = hl + 16 * c - a
        out.add(("da", "sh", max(0, r + 16 - stride)))
        if lo == 0 and hi == 16:
            out.add(("da", "whole"))
            continue
        t = hi & ~3
        if lo < t:
            out.add(("da", "edge", (t - lo) // 4))
            if c == 0 and lo > 0:
                out.add(("da", "first-edge", (t - lo) // 4))
        if t < hi and t >= lo:
            out.add(("da", "tail"))
        if last == 0 and lo > 0 and hi < 16:
            out.add(("da", "single"))
    # source-aligned: chunk c is slot bytes [16c, 16c + 16) against the payload [hl, hl + plen)
    pend = hl + plen
    first, lastc = hl // 16, (pend - 1) // 16
    congruent = ((a - hl) & 3) == 0
    for c in _edge_blocks(first, lastc):
        q0 = 16 * c
        lo = max(hl - q0, 0)
        hi = min(16, pend - q0)
        if not congruent:
            out.add(("sa", "bytes"))
        elif lo == 0 and hi == 16:
            out.add(("sa", "whole"))
        else:
            l4, t = (lo + 3) & ~3, hi & ~3
            if l4 < t:
                out.add(("sa", "edge", (t - l4) // 4))
            if t < hi and t >= lo:
                out.add(("sa", "tail"))
        if first == lastc and lo > 0 and hi < 16:
            out.add(("sa", "single"))
    return out


def matrix_classes(stride, with_lb, matrix):
    """Union of the classes of every middle fragment of a matrix, and the phases it holds."""
    hl = hdr_len(with_lb)
    got, phases = set(), set()
    for a in phases_for(stride):
        if hl + 16 + a > stride:
            continue
        for L in lengths_for(stride, with_lb, matrix):
            if 0 <= L and hl + L <= stride:
                got |= classes(a, L, hl, stride)
                phases.add(a)
    return got, phases
