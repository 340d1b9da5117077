"""A rows window on a lattice (e2sar_hip_rows.eventStep S > 1, eventPhase P) in terms of the
consecutive window -- TEST INFRASTRUCTURE (tests/test_rows_strided_cpu.py,
tests/test_gpu_rows_strided.py).

The yardstick is rows_ref.Window, which knows nothing of lattices.  A stream T is turned into
T': the datagrams that pass rule 1 (header validation) and carry an event the window owns, with
the RE header's eventNum (its bytes 12..19) rewritten to q(ev) = ev // S; the datagrams rule 1
stops stay as they are, since rule 1 comes before rule 1b and counts them whatever their event
number.  A window (S, P) fed T must then equal a consecutive window fed T', with counts[10] the
number of datagrams of T that pass rule 1 and are not owned, and the device base the model's
base * S + P.
"""
from __future__ import annotations

import numpy as np

import rows_ref as RR

C_NOT_OWNED = 10


def q(ev: int, step: int) -> int:
    return (ev & RR.M64) // step


def owned(ev: int, step: int, phase: int) -> bool:
    return (ev & RR.M64) % step == phase


def event_of(ev_index: int, step: int, phase: int) -> int:
    """The event number of an index of the lattice: the inverse of q on owned events."""
    return ev_index * step + phase


def header_valid(slot, length: int, stride: int, with_lb=True) -> bool:
    """Rule 1 of e2sar_hip_rows_reassemble passes the datagram (rows_ref.Window.push's first three tests)."""
    hl = 36 if with_lb else 20
    if length < hl or length > stride:
        return False
    return slot[hl - 20] == 0x10 and slot[hl - 19] == 0


def event_num(slot, with_lb=True) -> int:
    hl = 36 if with_lb else 20
    return int.from_bytes(bytes(slot[hl - 8:hl]), "big")


def renumber(dgrams, step: int, phase: int, stride: int, with_lb=True):
    """dgrams: [(slot uint8[stride], len)] -> (T', the number of rule-1-valid datagrams that are
    not owned).  The slots of T' are copies; T is not changed."""
    hl = 36 if with_lb else 20
    out, not_owned = [], 0
    for slot, length in dgrams:
        if not header_valid(slot, length, stride, with_lb):
            out.append((slot, length))
            continue
        ev = event_num(slot, with_lb)
        if not owned(ev, step, phase):
            not_owned += 1
            continue
        new = np.array(slot, np.uint8, copy=True)
        new[hl - 8:hl] = np.frombuffer(q(ev, step).to_bytes(8, "big"), np.uint8)
        out.append((new, length))
    return out, not_owned
