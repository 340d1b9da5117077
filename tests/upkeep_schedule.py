"""Upkeep schedules -- TEST INFRASTRUCTURE (tests/test_upkeep_schedule_cpu.py, tests/test_gpu_upkeep.py).

A schedule is a datagram stream cut into batches with an operation list between the
batches: the life of a long-running reassembler (poll, GC, lost poll, compaction, stats)
instead of one launch and one drain.  Steps:

    ("batch", a, b, now_ms)   datagrams [a, b) arrive at clock now_ms
    ("poll", cap)             drain the completed events, cap records per call (0: all at once)
    ("lost_poll", cap)        drain the lost records likewise
    ("gc", now_ms, timeout)   one GC pass (e2sarDPReassembler.cpp:252-274)
    ("compact",)              move the live items to the alternate table / arena
    ("stats",)                counter snapshot

`replay_oracle` runs a schedule on the CPU oracle, where compaction is a no-op: the
reference frees nothing the caller can see.  `trace` restates the reference's arrival-order
rules (as test_gpu_reference_order._completes_with_a_hole does) with the GC points of the
schedule: what the oracle does not expose -- which items are live at a compaction and how
long, which fragments an event completed with -- comes from it, and the CPU test pins it to
the oracle's own counts.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

import oracle_ffi as O

N_BATCHES = 6
TIMEOUT_MS = 250


@dataclass
class Schedule:
    pk: np.ndarray            # [n, stride] datagram slots
    ln: np.ndarray            # [n] datagram lengths
    stride: int
    steps: list
    redraws: int = 0          # dirty family: draws rejected by the hole model before this one


@dataclass
class Trace:
    hole: bool = False                                  # an event completed with unwritten bytes
    completions: list = field(default_factory=list)     # (key, compaction epochs of its fragments)
    gcs: list = field(default_factory=list)             # ([(key, frags) lost], survivors) per GC
    live: list = field(default_factory=list)            # per compaction: bufferLength of every live item
    after_collect: set = field(default_factory=set)     # keys that got fragments after a GC took their item
    twice: bool = False                                 # a key collected twice (the reference logs it once)


def arena_need(lengths):
    """Arena bytes of items of these lengths: each rounded up to 256, at least 256."""
    return sum(max(256, (b + 255) // 256 * 256) for b in lengths)


def trace(s: Schedule) -> Trace:
    T = Trace()
    items, collected, epoch = {}, set(), 0
    for st in s.steps:
        if st[0] == "batch":
            _, a, b, now = st
            for p in range(a, b):
                L = int(s.ln[p])
                if L < 36:
                    continue
                ok, d, off, blen, ev, _ = O.re_parse(s.pk[p, 16:36].tobytes())
                pl = L - 36
                if not ok or off + pl > blen:
                    continue
                key = (ev, d)
                if key in collected:
                    T.after_collect.add(key)
                it = items.get(key)
                if off == 0 or it is None:
                    it = items[key] = {"blen": blen, "cur": 0, "mask": np.zeros(blen, bool), "created": now,
                                       "frags": 0, "epochs": set()}
                if off + pl > it["blen"]:
                    continue              # overruns the item it joins: dropped (oracle's third guard)
                it["cur"] += pl
                it["frags"] += 1
                it["mask"][off:off + pl] = True
                it["epochs"].add(epoch)
                if it["cur"] == it["blen"]:
                    if not it["mask"].all():
                        T.hole = True
                    T.completions.append((key, frozenset(it["epochs"])))
                    del items[key]
        elif st[0] == "gc":
            _, now, timeout = st
            lost = [k for k, it in items.items() if now - it["created"] > timeout]
            T.gcs.append(([(k, items[k]["frags"]) for k in lost], len(items) - len(lost)))
            for k in lost:
                T.twice = T.twice or k in collected
                collected.add(k)
                del items[k]
        elif st[0] == "compact":
            T.live.append([it["blen"] for it in items.values()])
            epoch += 1
    return T


def replay_oracle(s: Schedule, queue_capacity: int = 0):
    """One result per step: None (batch), [(key, bytes, numFragments)] (poll),
    [(eventNum, dataId, numFragments)] (lost_poll), items collected (gc), the stats dict
    (stats), items in progress (compact)."""
    r = O.Reassembler(True, queue_capacity)
    out = []
    for st in s.steps:
        if st[0] == "batch":
            _, a, b, now = st
            r.set_time(now)
            if b > a:
                r.push_batch(s.pk[a:b], s.ln[a:b])
            out.append(None)
        elif st[0] == "poll":
            out.append([((e, d), by, nf) for by, e, d, nf in r.pop_all_frags(1 << 20)])
        elif st[0] == "lost_poll":
            out.append(r.lost_pop_all())
        elif st[0] == "gc":
            r.set_time(st[1])
            out.append(r.gc(st[2]))
        elif st[0] == "stats":
            out.append(r.stats())
        else:
            out.append(int(r.stats()["inProgress"]))
    return out


# ----------------------------------------------------------------------------------
# clean family: offset 0 first per event, tails shuffled, no duplicates -- the default
# (order-insensitive) mode and the reference agree on every such stream

EDGE_SIZES = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4097]


def _spread(rnd, seq, nb):
    """seq cut into nb consecutive non-empty parts when it is long enough (the last part is
    never empty: the withheld last fragment)."""
    if nb <= 1 or len(seq) < 2:
        return [seq]
    nb = min(nb, len(seq))
    cuts = sorted(rnd.sample(range(1, len(seq)), nb - 1))
    return [seq[a:b] for a, b in zip([0] + cuts, cuts + [len(seq)])]


def clean_schedule(seed: int) -> Schedule:
    """12 to 40 interleaved events over six batches at clock 100, 200, ... ms.  Kinds: whole
    (one batch), straddle (last fragment withheld for one or two batches: completes, across
    compactions), never (last fragment never sent: collected, or live to the end), late (last
    fragment withheld from batch 0 to batch 4: the GC at 400 ms takes the item first, so the
    fragment starts a new one, which no later GC is old enough to take -- the reference logs a
    key's loss once, hpp:262-279, the device on every collection).
    After every batch: poll by 3; odd batches add gc(250 ms) and lost_poll by 2 and compact
    twice, back to back."""
    rnd = random.Random(0xC1EA0 + seed)
    mtu = (80, 200)[seed % 2]
    mp = O.max_pld_len(mtu)
    stride = (36 + mp + 15) // 16 * 16
    nev = rnd.randint(12, 40)
    parts = [[] for _ in range(N_BATCHES)]          # per batch: one fragment list per event
    for k in range(nev):
        kind = ("late", "never", "straddle")[k] if k < 3 else rnd.choice(["whole"] * 3 + ["straddle"] * 3 + ["never"])
        if k < 3 or (kind != "whole" and rnd.random() < 0.5):
            size = rnd.randint(2 * mp + 1, 40 * mp)
        else:
            size = rnd.choice(EDGE_SIZES) if rnd.random() < 0.5 else rnd.randint(1, 40 * mp)
        ev = np.random.default_rng(seed * 977 + k).integers(0, 256, size, dtype=np.uint8)
        pk, ln = O.segment_event(ev, (500 + k) * rnd.choice([1, 1 << 33]), rnd.choice([1, 4321]), 7, 99, 2, mp, stride)
        tail = list(range(1, len(ln)))
        rnd.shuffle(tail)
        seq = [(pk[i].copy(), int(ln[i])) for i in [0] + tail]
        if len(seq) < 2:
            kind = "whole"
        if kind == "whole":
            parts[rnd.randrange(N_BATCHES)].append(seq)
        elif kind == "late":
            parts[0].append(seq[:-1])
            parts[4].append(seq[-1:])
        else:
            start = {1: 2, 2: 3}.get(k, rnd.randrange(N_BATCHES - 1))
            nb = min(rnd.randint(2, 3), N_BATCHES - start)
            if kind == "never":
                seq = seq[:-1]
            for j, part in enumerate(_spread(rnd, seq, nb)):
                parts[start + j].append(part)
    out, steps = [], []
    for k in range(N_BATCHES):
        a = len(out)
        streams = [p for p in parts[k] if p]
        while streams:
            s_ = rnd.choice(streams)
            out.append(s_.pop(0))
            if not s_:
                streams.remove(s_)
        now = 100 * (k + 1)
        steps += [("batch", a, len(out), now), ("poll", 3)]
        if k % 2:
            steps += [("gc", now, TIMEOUT_MS), ("lost_poll", 2), ("stats",), ("compact",), ("compact",)]
        else:
            steps += [("stats",), ("compact",)]
    steps += [("poll", 3), ("lost_poll", 2), ("stats",)]
    return Schedule(np.stack([p for p, _ in out]), np.array([L for _, L in out], np.uint32), stride, steps)


# ----------------------------------------------------------------------------------
# dirty family: any arrival order (REFERENCE_ORDER mode)


def dirty_schedule(seed: int) -> Schedule:
    """test_gpu_reference_order._draw's streams (duplicates, late offset 0, drops, replays,
    bad headers) cut into six equal batches at clock 100, 200, ... ms; after every batch poll,
    compact (the GC then reads `created` from the moved slots), gc(250 ms), lost_poll, stats.
    Redrawn until no event completes with a hole,
    with the items each GC removes taken into account."""
    from test_gpu_reference_order import _draw
    for sub in range(1000):
        pk, ln, stride, _ = _draw(seed * 1000 + sub)
        n = len(ln)
        steps = []
        for k in range(N_BATCHES):
            now = 100 * (k + 1)
            steps += [("batch", n * k // N_BATCHES, n * (k + 1) // N_BATCHES, now), ("poll", 0), ("compact",),
                      ("gc", now, TIMEOUT_MS), ("lost_poll", 0), ("stats",)]
        s = Schedule(pk, ln, stride, steps, redraws=sub)
        if not trace(s).hole:
            return s
    raise AssertionError("no hole-free schedule drawn")
