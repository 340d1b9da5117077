"""Host model of e2sar_hip_seg_emit's plan (e2sar_amd/csrc/seg_emit.hpp) -- TEST INFRASTRUCTURE.

Plain numpy.  The model restates the contract of include/e2sar_hip.h, not the kernel:

* available = min(*d_count, maxEvents) (maxEvents without a count), in row mode also at most
  dataBytes // pitch;
* taken = the longest prefix of the available events in which every event lies inside its
  source (rows: bytes <= pitch; ragged: offset + bytes <= dataBytes) and all datagrams of the
  prefix fit in maxPackets slots; nothing behind the first failing event is taken;
* reason 0 = all taken, 1 = packet capacity, 2 = an event outside its source -- also when
  rows the count names lie past dataBytes (the available count was cut by dataBytes // pitch);
* pktBase = the exclusive prefix of ceil(bytes / maxPld); the numbering rules of
  e2sar_hip_seg_numbering give the other descriptor fields.

``plan`` returns the counts and a seg_ref.EVENT table of the taken events, which
seg_ref.expected turns into the packet and lens buffers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

import seg_ref as M

M64 = (1 << 64) - 1


@dataclass
class Numbering:
    event_num_base: int = 0
    lb_tick_base: int = 0
    lb_tick_step: int = 0
    data_id: int = 0
    entropy_base: int = 0
    event_nums: Optional[np.ndarray] = None       # uint64, per source event
    ticks_as_event_num: bool = False


@dataclass
class Plan:
    n: int
    datagrams: int
    left: int
    reason: int
    events: np.ndarray                            # seg_ref.EVENT, the taken events

    @property
    def counts(self):
        return [self.n, self.datagrams, self.left, self.reason]


def plan(lengths, max_pld, max_packets, data_bytes, *, pitch=0, offsets=None, count=None, max_events=None,
         num: Numbering = Numbering()) -> Plan:
    """lengths / offsets: per source event (at least max_events entries); count: the value of
    *d_count, None for a NULL d_count."""
    assert (pitch > 0) != (offsets is not None)
    max_events = len(lengths) if max_events is None else max_events
    avail = max_events if count is None else min(int(count), max_events)
    short = False
    if pitch and data_bytes // pitch < avail:
        avail, short = data_bytes // pitch, True
    n, total, reason = avail, 0, 2 if short else 0
    for i in range(avail):
        nb = int(lengths[i])
        off = i * pitch if pitch else int(offsets[i])
        if (nb > pitch) if pitch else (off + nb > data_bytes):
            n, reason = i, 2
            break
        npk = -(-nb // max_pld)
        if total + npk > max_packets:
            n, reason = i, 1
            break
        total += npk
    ev = np.zeros(n, M.EVENT)
    base = 0
    for i in range(n):
        tick = (num.lb_tick_base + i * num.lb_tick_step) & M64
        evn = int(num.event_nums[i]) if num.event_nums is not None else (num.event_num_base + i) & M64
        ev[i] = (i * pitch if pitch else int(offsets[i]), int(lengths[i]), tick if num.ticks_as_event_num else evn,
                 num.data_id & 0xFFFF, (num.entropy_base + i) & 0xFFFF, tick, base)
        base += -(-int(lengths[i]) // max_pld)
    assert base == total
    return Plan(n, total, avail - n, reason, ev)


def first_units(lengths, max_pld, spc, unit_chunks):
    """The exclusive prefix of ceil(npk * spc / unit_chunks): what the plan leaves in
    `reserved` (not part of the contract; the CPU test pins the search rule over it)."""
    npk = M.num_packets(np.asarray(lengths, np.uint64), max_pld)
    nu = (npk * np.uint64(spc) + np.uint64(unit_chunks - 1)) // np.uint64(unit_chunks)
    return np.concatenate(([0], np.cumsum(nu))).astype(np.uint64)


def event_of_unit(first, p):
    """The last event whose first unit is <= p, by the kernel's binary search (first: the
    n + 1 entries of first_units; p < first[n])."""
    n = len(first) - 1
    e, hi = 0, n
    while hi - e > 1:
        mid = (e + hi) >> 1
        if first[mid] <= p:
            e = mid
        else:
            hi = mid
    return e
