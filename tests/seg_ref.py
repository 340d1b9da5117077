"""Host model of a segmented batch (e2sar_amd/csrc/seg_device.hpp) -- TEST INFRASTRUCTURE.

Plain numpy over the oracle's e2o_segment_event.  The model restates the contract of
e2sar_hip_segment_batch, not the kernel:

* datagram k of an event sits in slot pktBase + k; bytes [0, 36 + L) of the slot are the
  oracle's datagram (LB header, RE header, L payload bytes);
* the bytes from there to the end of the datagram's last 16-byte chunk are zero;
* nothing else is written: the rest of the slot, the slots of events at or past a
  device-side count, whatever lies in front of and behind the batch's slots;
* lens[pktBase + k] = 36 + L, no other entry is written.

``expected`` therefore starts from the caller's buffers as they were before the launch
(canary-filled, a guard region at both ends) and returns them as they must look after it.
``div_recip_f32`` restates dev_access.hpp's div_recip in float32, as the gfx950 code
computes it (a correctly rounded 1.0f / d, checked in the kernel's assembly).
"""
from __future__ import annotations

import numpy as np

import oracle_ffi as O

HDR = 36                    # LB + RE header bytes
CANARY = 0xA5               # never a zero fill, never a likely header byte
GUARD = 4096                # guard bytes at each end of a packet buffer (a multiple of 16)
GUARD_LENS = 64             # guard entries at each end of a lens buffer
CANARY_LEN = 0xA5A5A5A5

EVENT = np.dtype([("off", "<u8"), ("bytes", "<u4"), ("eventNum", "<u8"), ("dataId", "<u2"),
                  ("entropy", "<u2"), ("lbTick", "<u8"), ("pktBase", "<u4")])


def min_stride(max_pld: int) -> int:
    return (HDR + max_pld + 15) // 16 * 16


def num_packets(nbytes, max_pld):
    """ceil(bytes / maxPld) in 64 bits (0 for an empty event)."""
    b = np.asarray(nbytes, dtype=np.uint64)
    return (b // np.uint64(max_pld) + (b % np.uint64(max_pld) != 0)).astype(np.uint64)


def make_events(offs, lengths, max_pld, seed=0) -> np.ndarray:
    """An event table over arena offsets `offs`: pktBase is the exclusive prefix of the
    packet counts (what e2sar_hip_seg_plan fills in); the header fields vary per event and
    reach past 16 / 32 bits where the field allows it."""
    n = len(offs)
    ev = np.zeros(n, EVENT)
    k = np.arange(n, dtype=np.uint64)
    ev["off"] = offs
    ev["bytes"] = lengths
    ev["eventNum"] = np.uint64(0x0102030405060000 + 977 * seed) + k * np.uint64(0x100000001)
    ev["dataId"] = (4321 + 7 * k) & np.uint64(0xFFFF)
    ev["entropy"] = (0xBEEF + 257 * k) & np.uint64(0xFFFF)
    ev["lbTick"] = np.uint64(0x0123456789AB0000) + k
    npk = num_packets(ev["bytes"], max_pld)
    ev["pktBase"] = np.concatenate(([0], np.cumsum(npk)[:-1])) if n else []
    return ev


def total_packets(ev, max_pld) -> int:
    return int(num_packets(ev["bytes"], max_pld).sum())


def max_packets(ev, max_pld) -> int:
    return int(num_packets(ev["bytes"], max_pld).max()) if len(ev) else 0


def canary_buffers(n_slots: int, stride: int):
    """-> (pkts uint8 [GUARD + n_slots * stride + GUARD], lens uint32 [GUARD_LENS + n_slots + GUARD_LENS])."""
    return (np.full(2 * GUARD + n_slots * stride, CANARY, np.uint8),
            np.full(2 * GUARD_LENS + n_slots, CANARY_LEN, np.uint32))


def expected(arena, ev, max_pld, stride, ver, pkts, lens, count=None):
    """The buffers of canary_buffers (or any other state before the launch) after
    segmenting events ev[:count] (count None: all of them) of `arena`."""
    pkts, lens = pkts.copy(), lens.copy()
    n_slots = (pkts.size - 2 * GUARD) // stride
    slots = pkts[GUARD:GUARD + n_slots * stride].reshape(n_slots, stride)
    ln = lens[GUARD_LENS:GUARD_LENS + n_slots]
    full = (HDR + max_pld + 15) // 16 * 16            # bytes a full datagram's chunks span
    for e in ev[:len(ev) if count is None else count]:
        nb = int(e["bytes"])
        if nb == 0:
            continue
        data = arena[int(e["off"]):int(e["off"]) + nb]
        op, ol = O.segment_event(data, int(e["eventNum"]), int(e["dataId"]), int(e["entropy"]), int(e["lbTick"]),
                                 ver, max_pld, full)
        n, base = len(ol), int(e["pktBase"])
        assert base + n <= n_slots, "event table reaches past the packet buffer"
        assert (ol[:-1] == HDR + max_pld).all()
        slots[base:base + n - 1, :full] = 0
        slots[base:base + n - 1, :HDR + max_pld] = op[:-1, :HDR + max_pld]
        last = int(ol[-1])
        slots[base + n - 1, :(last + 15) // 16 * 16] = 0
        slots[base + n - 1, :last] = op[-1, :last]
        ln[base:base + n] = ol
    return pkts, lens


def first_difference(got, want, stride):
    """None, or a description of the first differing byte of two packet buffers."""
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    b = int(bad[0])
    where = "front guard" if b < GUARD else "slots"
    s = (b - GUARD) // stride
    n_slots = (got.size - 2 * GUARD) // stride
    if b >= GUARD and s >= n_slots:
        where = "back guard"
    c, r = divmod((b - GUARD) % stride, 16)
    return (f"{bad.size} bytes differ; first in the {where}: slot {s}, chunk {c}, byte {r} "
            f"(offset {(b - GUARD) % stride}): got {int(got[b]):#04x}, want {int(want[b]):#04x}")


def div_recip_f32(i, d):
    """dev_access.hpp's div_recip(i, d, 1.0f / d) on uint32 arrays: the index converted to
    float32 (round to nearest even), one float32 multiply by the correctly rounded
    reciprocal, truncation, and the +-1 correction in wrapping 32-bit arithmetic."""
    i = np.asarray(i, dtype=np.uint32)
    d = np.uint32(d)
    rd = np.float32(1.0) / np.float32(d)
    q = (i.astype(np.float32) * rd).astype(np.uint32)
    with np.errstate(over="ignore"):
        down = q * d > i
        up = ~down & ((q + np.uint32(1)) * d <= i)
        return np.where(down, q - np.uint32(1), np.where(up, q + np.uint32(1), q)).astype(np.uint32)


# ---------------------------------------------------------------------------------
# the event sets of the slot tests


def matrix_lengths(max_pld):
    """1..17 and m * maxPld + {-1, 0, 1} for m = 1, 2, 3 (positive lengths only)."""
    out = list(range(1, 18))
    for m in (1, 2, 3):
        out += [m * max_pld + t for t in (-1, 0, 1) if m * max_pld + t > 0]
    return out


def pack_events(cases, slack=64):
    """cases: (address residue mod 16, length) pairs.  Events are packed back to back: each
    starts at the first offset at or behind the previous event's end that has its residue.
    -> (offsets, lengths, arena bytes needed); the arena runs `slack` bytes past the last
    event (the dword path reads up to 3 bytes behind an event)."""
    offs, cur = [], 16                  # 16 bytes in front of the first event, too
    for r, n in cases:
        cur += (r - cur) % 16
        offs.append(cur)
        cur += n
    return np.array(offs, np.uint64), np.array([n for _, n in cases], np.uint32), cur + slack


def matrix_cases(max_pld, lengths=None):
    """(a): every address residue 0..15 with every length of matrix_lengths, plus one empty event."""
    lengths = matrix_lengths(max_pld) if lengths is None else lengths
    cases = [(r, n) for n in lengths for r in range(16)]
    cases.insert(len(cases) // 2, (5, 0))
    return cases


def random_arena(n, seed):
    """Random bytes, none of them zero: whatever lies in front of or behind an event shows if it leaks."""
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8)


def npk_near(chunks, spc):
    """Packet counts whose chunk count npk * spc is `chunks` or, where spc does not divide
    it, the nearest reachable count on either side."""
    return sorted({max(1, chunks // spc), -(-chunks // spc)})
