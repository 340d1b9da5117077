"""Host model of a receive graph that runs without end -- TEST INFRASTRUCTURE
(tests/test_turn_ref_cpu.py, tests/test_gpu_turn.py).

`stream()` builds a datagram stream cut into K batches whose events straddle the batches;
`run(s, max_carries)` says what `reassemble -> collect_next -> turn(marks all 0)` must leave
after every batch: the events delivered, d_status, the cursor, the occupancy, and at the end
every counter and the lost records.  `replay_oracle` drives the CPU oracle with the turn as
its clock: set_time(e) before a batch's pushes, e the turns that ran so far, and set_time(k),
gc(timeout = max_carries) at the k-th turn.  An event created in epoch e has been carried
k - 1 - e times at turn k; the oracle loses it iff k - e > timeout, which is carries >=
max_carries.  tests/test_turn_ref_cpu.py pins the model to the oracle.

One difference is the reference's own: it logs and counts a key's loss once
(hpp:262-279), the device at every collection.  With max_carries below 2 a straddling event
is lost at its first turn, its later fragments start a new item, and that is lost in turn: the
model counts both (`reassemblyLoss`, `lost`) and states the de-duplicated view beside them
(`reassemblyLossOnce`, `lost_once`: a key's first record), which is what the oracle holds.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

import oracle_ffi as O

MTU = 200
K_BATCHES = 12
BATCH_MAX = 256
N_EVENTS = 140
SEED = 53                      # chosen so that test_turn_ref_cpu.py's conditions hold
NEVER = 0xFFFFFFFF
ARENA = 64 << 10
SLOTS = 64
QCAP = 64
NO_BUF = -1


def max_pld() -> int:
    return O.max_pld_len(MTU)


def stride() -> int:
    return (36 + max_pld() + 15) // 16 * 16


def lengths():
    mp = max_pld()
    return [1, mp - 1, mp, mp + 1, 255, 256, 257, 4095, 4097, 9999]


def need(n: int) -> int:
    """Arena bytes of one event buffer: its length rounded up to 256, at least 256."""
    return max(256, (n + 255) // 256 * 256)


def slot_hash(ev: int, d: int, mask: int) -> int:
    """reas_table.hpp's slot_hash."""
    M = (1 << 64) - 1
    h = ev ^ (d | d << 16 | d << 32 | d << 48)
    h &= M
    h ^= h >> 33
    h = h * 0xff51afd7ed558ccd & M
    h ^= h >> 33
    return h & 0xFFFFFFFF & mask


@dataclass
class Frag:
    key: tuple          # (eventNum, dataId)
    off: int
    plen: int
    blen: int


@dataclass
class Stream:
    pk: np.ndarray                      # [n, stride] datagram slots
    ln: np.ndarray                      # [n] datagram lengths
    stride: int
    cuts: list                          # batch b = datagrams [cuts[b], cuts[b + 1])
    frags: list                         # Frag per datagram
    events: dict                        # key -> payload bytes
    cls: dict                           # key -> index into lengths()
    missing: set = field(default_factory=set)     # keys that lack one fragment


def _cut(rnd, seq, nb):
    nb = max(1, min(nb, len(seq)))
    cuts = sorted(rnd.sample(range(1, len(seq)), nb - 1)) if nb > 1 else []
    return [seq[a:b] for a, b in zip([0] + cuts, cuts + [len(seq)])]


def stream(seed: int = SEED, n_events: int = N_EVENTS) -> Stream:
    """n_events events whose lengths cycle through lengths(), each one's datagrams in order,
    offset 0 first, no duplicates (the default mode equals the reference), cut
    across 1 to 3 consecutive batches and interleaved with the other events'.  About one in
    eight lacks one fragment that is not its first (the next event of two fragments or more
    after every eighth) and never completes."""
    rnd = random.Random(0x7E4B + seed)
    mp, st, L = max_pld(), stride(), lengths()
    parts = [[] for _ in range(K_BATCHES)]
    events, cls, missing = {}, {}, set()
    pending = False
    for k in range(n_events):
        size = L[k % len(L)]
        key = ((1000 + k) << (33 if k % 5 == 0 else 0), 4321 if k % 3 else 1)
        body = np.random.default_rng(seed * 7919 + k).integers(0, 256, size, dtype=np.uint8)
        pk, ln = O.segment_event(body, key[0], key[1], 7, 99, 2, mp, st)
        seq = [(pk[i].copy(), int(ln[i]), Frag(key, i * mp, int(ln[i]) - 36, size)) for i in range(len(ln))]
        pending = pending or k % 8 == 2
        if pending and len(seq) >= 2:
            del seq[rnd.randrange(1, len(seq))]
            missing.add(key)
            pending = False
        events[key], cls[key] = body.tobytes(), k % len(L)
        nb = min(rnd.choice([1, 1, 1, 2, 2, 3]), len(seq))
        start = min(k * K_BATCHES // n_events, K_BATCHES - nb)
        for j, part in enumerate(_cut(rnd, seq, nb)):
            parts[start + j].append(part)
    out, cuts = [], [0]
    for b in range(K_BATCHES):
        live = [p for p in parts[b] if p]
        while live:
            p = rnd.choice(live)
            out.append(p.pop(0))
            if not p:
                live.remove(p)
        cuts.append(len(out))
    return Stream(np.stack([p for p, _, _ in out]), np.array([n for _, n, _ in out], np.uint32), st, cuts,
                  [f for _, _, f in out], events, cls, missing)


@dataclass
class Step:
    """What one batch -> collect_next -> turn leaves behind."""
    delivered: dict             # key -> (bytes, numFragments) completed by this batch
    after_batch: dict           # arenaUsed, tableUsed, inProgress, completedPending
    status: list                # d_status of the turn
    after_turn: dict
    carried: list               # keys the turn carried
    lost: list                  # (eventNum, dataId, numFragments, 0) the turn aged out
    created: list               # keys whose item this batch created


@dataclass
class Run:
    steps: list
    stats: dict                 # every counter of stats() at the end
    lost: list                  # every lost record, in turn order (sorted within a turn)
    lost_once: list             # a key's first record only: the reference's log
    stats_once: dict            # stats with reassemblyLoss counted once per key
    completed_carried: set      # keys that completed after having been carried
    twice: bool                 # a key was collected twice


def run(s: Stream, max_carries: int, arena: int = ARENA) -> Run:
    items, top, used = {}, 0, 0            # key -> item; arena top and slots claimed this epoch
    hist = dict(eventSuccess=0, totalPackets=0, totalBytes=0, badHeaderDiscards=0, dataErrCnt=0, enqueueLoss=0,
                reassemblyLoss=0)
    steps, lost_all, carried_done = [], [], set()
    for b in range(K_BATCHES):
        delivered, created = {}, []
        for p in range(s.cuts[b], s.cuts[b + 1]):
            f = s.frags[p]
            hist["totalPackets"] += 1
            hist["totalBytes"] += int(s.ln[p])
            it = items.get(f.key)
            if f.off == 0 or it is None:
                assert it is None, "a clean stream sends offset 0 once"
                buf = top if top + f.blen <= arena else NO_BUF
                top += need(f.blen)
                used += 1
                it = items[f.key] = dict(blen=f.blen, cur=0, frags=0, carries=0, buf=buf)
                created.append(f.key)
            it["cur"] += f.plen
            it["frags"] += 1
            if it["cur"] == it["blen"]:
                assert it["buf"] != NO_BUF, "the stream fits its arena"
                hist["eventSuccess"] += 1
                delivered[f.key] = (s.events[f.key], it["frags"])
                if it["carries"]:
                    carried_done.add(f.key)
                del items[f.key]
        after_batch = dict(arenaUsed=top, tableUsed=used, inProgress=len(items), completedPending=len(delivered))
        lost = sorted((k[0], k[1], it["frags"], 0) for k, it in items.items() if it["carries"] >= max_carries
                      and max_carries != NEVER)
        for ev, d, _, _ in lost:
            del items[(ev, d)]
        hist["reassemblyLoss"] += len(lost)
        lost_all += lost
        top = 0
        for it in items.values():
            it["carries"] += 1
            it["buf"] = top
            top += need(it["blen"])
        used = len(items)
        after_turn = dict(arenaUsed=top, tableUsed=used, inProgress=used, completedPending=0)
        steps.append(Step(delivered, after_batch, [1, used, len(lost), top], after_turn, sorted(items), lost, created))
    seen, once = set(), []
    for r in lost_all:
        if r[:2] not in seen:
            seen.add(r[:2])
            once.append(r)
    stats = dict(hist, inProgress=len(items))
    return Run(steps, stats, lost_all, once, dict(stats, reassemblyLoss=len(once)), carried_done,
               len(once) != len(lost_all))


def replay_oracle(s: Stream, max_carries: int):
    """-> (per batch: {key: (bytes, numFragments)} delivered, per turn: items collected,
    stats at the end, lost records at the end), the turn as the oracle's clock."""
    r = O.Reassembler(True, 0)
    delivered, collected = [], []
    for b in range(K_BATCHES):
        r.set_time(b)
        a, e = s.cuts[b], s.cuts[b + 1]
        if e > a:
            r.push_batch(s.pk[a:e], s.ln[a:e])
        delivered.append({(ev, d): (by, nf) for by, ev, d, nf in r.pop_all_frags(1 << 16)})
        r.set_time(b + 1)
        collected.append(r.gc(max_carries))
    return delivered, collected, r.stats(), r.lost_pop_all()
