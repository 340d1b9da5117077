"""Host model of e2sar_hip_rows_ready over rows_ref.Window -- TEST INFRASTRUCTURE
(tests/test_rows_ready_cpu.py, tests/test_gpu_rows_ready.py).

Restates the definitions of include/e2sar_hip.h in plain Python integers, one event after the
other; it knows nothing of summaries, workgroups or pieces.  Also the random streams both test
files draw from, so that what the CPU test asserts of the family holds for what the GPU runs.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import reas_cuts as RC
import rows_ref as RR

READY_ZERO = 1
EV_COMPLETE, EV_GIVEN_UP, EV_TRUNCATED = 1, 2, 4
NEVER = 0xFFFFFFFF

Rule = namedtuple("Rule", "required_mask slack k_max flags", defaults=(0, NEVER, 0, 0))
# eventNum, presentMask, openMask, row, flags: e2sar_hip_rows_event
Event = namedtuple("Event", "eventNum presentMask openMask row flags")


def check_rule(window, rule):
    """What a PARAMETER status refuses of a rule."""
    return rule.flags & ~READY_ZERO == 0 and rule.required_mask >> len(window.ids) == 0


def masks(window, i):
    """-> (present, open, truncated) of the event i behind the base."""
    nid = len(window.ids)
    r = (window.base + i) & (window.n_events - 1)
    present = opened = 0
    trunc = False
    for j in range(nid):
        c = r * nid + j
        if window.flags[c] & RR.COMPLETE:
            present |= 1 << j
        if window.bytes[c] != 0:
            opened |= 1 << j
        if window.flags[c] & RR.TRUNCATED:
            trunc = True
    return present, opened, trunc


def ready(window, rule):
    """-> (ready[8], [Event] * k, the bytes `out` holds after the call).  The window is not changed."""
    assert check_rule(window, rule)
    N, nid = window.n_events, len(window.ids)
    R = rule.required_mask or (1 << nid) - 1
    H = 0
    for i in range(N):
        if masks(window, i)[1]:
            H = i + 1
    words = [0] * 8
    events = []
    out = window.out.copy()
    k = 0
    while k < min(rule.k_max, N):
        present, opened, trunc = masks(window, k)
        complete = present & R == R
        given_up = not complete and k < H and H - 1 - k >= rule.slack
        if not complete and not given_up:
            break
        row = (window.base + k) & (N - 1)
        events.append(Event((window.base + k) & RR.M64, present, opened, row,
                            (EV_COMPLETE if complete else EV_GIVEN_UP) | (EV_TRUNCATED if trunc else 0)))
        words[1] += complete
        words[2] += given_up
        words[4] += bin(present).count("1")
        words[5] += bin(opened & ~present).count("1")
        if rule.flags & READY_ZERO:
            for j in range(nid):
                keep = min(window.bytes[row * nid + j], window.pitch) if present >> j & 1 else 0
                out[row, j, keep:] = 0
        k += 1
    words[0], words[3] = k, H
    return words, events, out


# ----------------------------------------------------------------------------------
# the random family

SEEDS = range(40)
STRIDE, MAX_PLD, PITCH = 80, 36, 512        # MTU 100: 36 bytes of payload behind 64 of headers


def random_family(seed):
    """-> (ids, n_events, base, slack, k_max, batches): a stream of consecutive events of random
    length on 1..3 ids, cut into batches of [(row, len)] datagrams, with dropped fragments and
    some held back for the next batch.  No fragment comes twice."""
    rng = np.random.default_rng([0xead, seed])
    n_events = (8, 64)[seed % 2]
    ids = [7, 9, 300][: 1 + seed % 3]
    base = int(rng.integers(0, 1 << 40))
    slack = int(rng.integers(1, 6))
    k_max = int(rng.integers(1, 8)) if seed % 4 else n_events
    batches, held = [], []
    ev = base
    for _ in range(6):
        dgrams, held = held, []
        for _ in range(int(rng.integers(2, 6))):
            for d in ids:
                size = int(rng.choice([1, 35, 36, 37, 100, 300, 511, 512, 517, 700]))
                data = rng.integers(1, 256, size, dtype=np.uint8)
                frags = [RC.dgram(ev, d, off, size, data[off:off + MAX_PLD], STRIDE, True) for off in range(0, size, MAX_PLD)]
                for f in frags:
                    u = rng.random()
                    if u < 0.06:
                        continue                                    # lost
                    (held if u < 0.16 else dgrams).append(f)        # late by a batch
            ev += 1
        order = rng.permutation(len(dgrams))
        batches.append([dgrams[q] for q in order])
    return ids, n_events, base, slack, k_max, batches


def run_family(seed, step):
    """The loop reassemble -> ready(zero) -> advance(count = ready[0]) on the model; step(window,
    rule, batch, words, events, out) sees every step before the advance.  A held-back fragment
    of an event the window has let go meanwhile is counted late, one of an event the window has
    not reached yet early, by the kernel and the model alike."""
    ids, n_events, base, slack, k_max, batches = random_family(seed)
    w = RR.Window(ids, n_events, PITCH, base)
    rule = Rule(0, slack, k_max, READY_ZERO)
    for batch in batches:
        pk = np.stack([r for r, _ in batch]) if batch else np.zeros((1, STRIDE), np.uint8)
        ln = np.array([n for _, n in batch], np.uint32)
        w.apply(pk[: len(ln)], ln, STRIDE)
        words, events, out = ready(w, rule)
        step(w, rule, batch, words, events, out)
        w.out[:] = out
        w.advance(rule.k_max, words[0])
