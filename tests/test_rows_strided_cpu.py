"""A rows window on a lattice, without a GPU: the renumbering helper of tests/rows_strided_ref.py
against the oracle's segmenter, the layout of e2sar_hip_rows as the C compiler and ctypes see it,
and RowWindow.first_owned."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O
import rows_ref as RR
import rows_strided_ref as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------
# 1. the helper


@pytest.mark.parametrize("step,phase", [(2, 0), (2, 1), (3, 2), (4, 1), (5, 0), (8, 7)])
@pytest.mark.parametrize("mtu", [100, 1500])
def test_renumber_is_the_segmenter_on_the_index(mtu, step, phase):
    """renumber(segment(ev)) equals segment(q(ev)) in the RE header and the payload, for owned
    events; every datagram of another event is dropped and counted."""
    max_pld = O.max_pld_len(mtu)
    stride = (36 + max_pld + 15) // 16 * 16
    rng = np.random.default_rng([mtu, step, phase])
    for base in (0, 3 * 2 ** 40 + 5, 2 ** 63 + 2 ** 33 + 7, 2 ** 64 - 64 * step):
        for ev in range(base, base + 2 * step):
            data = rng.integers(0, 256, 2 * max_pld + 3, dtype=np.uint8)
            pk, ln = O.segment_event(data, ev, 9, 77, 1234, 2, max_pld, stride)
            got, not_owned = RS.renumber([(pk[i], int(ln[i])) for i in range(len(ln))], step, phase, stride)
            if ev % step != phase:
                assert got == [] and not_owned == len(ln) == 3
                continue
            assert not_owned == 0 and len(got) == len(ln)
            assert RS.event_of(RS.q(ev, step), step, phase) == ev
            want, wl = O.segment_event(data, ev // step, 9, 77, 1234, 2, max_pld, stride)
            for i, (slot, length) in enumerate(got):
                assert length == int(wl[i])
                assert slot[16:length].tobytes() == want[i][16:length].tobytes()      # RE header and payload
                assert slot[:16].tobytes() == pk[i][:16].tobytes()                    # the LB header stays


def test_renumber_keeps_what_rule_1_stops():
    """A datagram that header validation stops stays in the stream, owned or not: rule 1 comes
    before rule 1b."""
    stride = 64
    pk, ln = O.segment_event(np.arange(10, dtype=np.uint8), 7, 9, 0, 0, 2, 28, stride)
    bad = pk[0].copy()
    bad[16] = 0x20
    dgrams = [(pk[0], int(ln[0])), (bad, int(ln[0])), (pk[0], 35), (pk[0], stride + 1)]
    got, not_owned = RS.renumber(dgrams, 2, 0, stride)
    assert not_owned == 1 and [n for _, n in got] == [int(ln[0]), 35, stride + 1]
    assert all(g is d for (g, _), (d, _) in zip(got, dgrams[1:]))
    w = RR.Window([9], 8, 256)
    for slot, n in got:
        w.push(slot.tobytes(), n, stride)
    assert (w.counts[RR.C_BAD_HEADER], w.counts[RR.C_DATA_ERR], w.counts[RR.C_ACCEPTED]) == (2, 1, 0)


# ----------------------------------------------------------------------------------
# 2. the struct

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "e2sar_hip.h"
_Static_assert(sizeof(e2sar_hip_rows) == 64, "e2sar_hip_rows is 64 bytes");
_Static_assert(offsetof(e2sar_hip_rows, eventStep) == 56, "eventStep follows withLBHeader");
_Static_assert(offsetof(e2sar_hip_rows, eventPhase) == 60, "eventPhase is the last word");
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(e2sar_hip_rows), offsetof(e2sar_hip_rows, eventStep),
           offsetof(e2sar_hip_rows, eventPhase), offsetof(e2sar_hip_rows, withLBHeader), offsetof(e2sar_hip_rows, nIds),
           offsetof(e2sar_hip_rows, dataIds));
    return 0;
}
"""


def test_struct_layout(tmp_path):
    from e2sar_amd import _capi
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = _capi.Rows
    assert got == [C.sizeof(R), R.eventStep.offset, R.eventPhase.offset, R.withLBHeader.offset, R.nIds.offset,
                   R.dataIds.offset] == [64, 56, 60, 52, 40, 32]
    # built positionally, as the callers from before the lattice build it: both fields 0
    w = R(1, 2, 3, 4, (C.c_uint16 * 1)(7), 1, 8, 256, 1)
    assert (w.eventStep, w.eventPhase) == (0, 0)


# ----------------------------------------------------------------------------------
# 3. first_owned


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_first_owned(world):
    from e2sar_amd.sar import RowWindow
    firsts = [0, 1, world - 1, world, 5 * world - 1, 5 * world, 2 ** 63 + 11, 2 ** 63 + 8 * world - 1, 2 ** 64 - 3 * world - 1]
    for first in firsts:
        for rank in range(world):
            got = RowWindow.first_owned(first, world, rank)
            want = next(e for e in range(first, first + world) if e % world == rank)
            assert got == want and isinstance(got, int)
    assert RowWindow.first_owned(0, world, world - 1) == world - 1
    with pytest.raises(ValueError):
        RowWindow.first_owned(0, world, world)
