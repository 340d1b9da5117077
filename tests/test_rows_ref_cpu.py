"""The host model of the rows family (tests/rows_ref.py) against the oracle, and its window,
wrap, truncation and ring rules on small cases of their own (CPU only)."""
import random

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC
import rows_ref as RR

IDS = [7, 9, 300]


def _events(rng, sizes, ev0, ids, max_pld, stride):
    """One event per (size, id): -> ([(row, len)], {(ev, id): bytes})."""
    dgrams, events = [], {}
    for k, s in enumerate(sizes):
        ev, d = ev0 + k // len(ids), ids[k % len(ids)]
        data = rng.integers(0, 256, s, dtype=np.uint8)
        pk, ln = O.segment_event(data, ev, d, ev & 0xFFFF, ev, 2, max_pld, stride)
        dgrams += [(pk[i], int(ln[i])) for i in range(len(ln))]
        events[(ev, d)] = data.tobytes()
    return dgrams, events


def _stack(dgrams):
    return np.stack([r for r, _ in dgrams]), np.array([n for _, n in dgrams], np.uint32)


@pytest.mark.parametrize("mtu,seed", [(100, 0), (100, 1), (1499, 2), (1500, 3)])
def test_model_agrees_with_oracle_on_shuffled_streams(mtu, seed):
    max_pld = O.max_pld_len(mtu)
    stride = (36 + max_pld + 15) // 16 * 16
    rng = np.random.default_rng([mtu, seed])
    sizes = [1, 15, 16, 17, max_pld - 1, max_pld, max_pld + 1, 3 * max_pld + 5, 4097, 700, 33, 2 * max_pld]
    ev0 = 5 * 2 ** 33 + 3
    dgrams, events = _events(rng, sizes, ev0, IDS, max_pld, stride)
    # an event ahead of the window, one of a foreign id: the oracle completes both, the window takes neither
    extra, _ = _events(rng, [300], ev0 + 8, [7], max_pld, stride)
    foreign, _ = _events(rng, [300], ev0, [8], max_pld, stride)
    # bad headers and fragments that overrun their own length
    bad = RC.dgram(ev0, 7, 0, 64, bytes(16), stride, True)
    bad[0][16] = 0x20
    short = (np.zeros(stride, np.uint8), 35)
    over = RC.dgram(ev0 + 1, 9, 50, 60, bytes(16), stride, True)
    stream = dgrams + extra + foreign + [bad, short, over, over]
    random.Random(seed).shuffle(stream)
    pk, ln = _stack(stream)

    ref = O.Reassembler(True)
    ref.push_batch(pk, ln)
    done = ref.pop_all_frags()
    st = ref.stats()

    w = RR.Window(IDS, 8, 8192, ev0)
    half = len(ln) // 2
    w.apply(pk[:half], ln[:half], stride)                      # the cut does not matter
    w.apply(pk[half:], ln[half:], stride)
    assert w.counts[RR.C_BAD_HEADER] == st["badHeaderDiscards"] == 2
    assert w.counts[RR.C_DATA_ERR] == st["dataErrCnt"] == 2
    assert w.counts[RR.C_EARLY] == len(extra) and w.counts[RR.C_FOREIGN] == len(foreign) and w.counts[RR.C_LATE] == 0
    cells = w.cells()
    seen = 0
    for data, ev, d, frags in done:
        if d not in IDS or not ev0 <= ev < ev0 + 8:
            continue
        seen += 1
        acc, nbytes, flags = cells[w.cell_index(ev, d)]
        assert flags == RR.COMPLETE and nbytes == len(data)
        assert acc == (frags << RR.ACC_SHIFT) | len(data)
        assert w.out.reshape(-1, w.pitch)[w.cell_index(ev, d)][:len(data)].tobytes() == data == events[(ev, d)]
    assert seen >= 4                                            # the one-datagram events at least
    # arrival order does not matter to the model: every event of the stream is complete, not
    # only those whose offset 0 came first
    assert w.counts[RR.C_COMPLETE] == len(sizes)
    assert w.counts[RR.C_ACCEPTED] == len(dgrams) and w.counts[RR.C_BYTES] == sum(sizes)
    for (ev, d), data in events.items():
        c = w.cell_index(ev, d)
        assert cells[c][2] == RR.COMPLETE
        row = w.out.reshape(-1, w.pitch)[c]
        assert row[:len(data)].tobytes() == data and (row[len(data):] == RR.FILL).all()


def _one(ev, d, off, blen, n, stride=64, byte=0x11):
    return RC.dgram(ev, d, off, blen, bytes([byte]) * n, stride, True)


def test_window_edges_and_wrap():
    for base in (2 ** 64 - 3, 7 * 2 ** 33, 0):
        w = RR.Window([7], 8, 256, base)
        evs = [(base - 1) & RR.M64, base, (base + 7) & RR.M64, (base + 8) & RR.M64]
        pk, ln = _stack([_one(e, 7, 0, 16, 16) for e in evs])
        w.apply(pk, ln)
        assert w.counts[RR.C_LATE] == 1 and w.counts[RR.C_EARLY] == 1 and w.counts[RR.C_COMPLETE] == 2
        open_rows = [c for c, (_, b, _) in enumerate(w.cells()) if b]
        assert open_rows == sorted({evs[1] & 7, evs[2] & 7})


def test_truncation():
    w = RR.Window([7], 2, 256, 0)
    stream = [_one(0, 7, 0, 300, 28), _one(0, 7, 240, 300, 28, byte=0x22), _one(0, 7, 268, 300, 28, byte=0x33)]
    pk, ln = _stack(stream)
    w.apply(pk, ln)
    acc, nbytes, flags = w.cells()[0]
    assert nbytes == 300 and flags == RR.TRUNCATED and acc == (3 << RR.ACC_SHIFT) | 84
    assert w.counts[RR.C_BYTES] == 84                           # payloads count in full
    assert (w.out[0, 0, 240:256] == 0x22).all() and (w.out[0, 0, 28:240] == RR.FILL).all()
    assert not (w.out == 0x33).any()
    assert (w.out[1] == RR.FILL).all()


def test_lengths_and_zero():
    w = RR.Window([7], 2, 256, 0)
    pk, ln = _stack([_one(0, 7, 16, 64, 16), _one(0, 7, 0, 0, 0), _one(0, 7, 0, 200, 16), _one(0, 7, 60, 200, 16, byte=0xEE),
                     _one(0, 7, 100, 50, 16, byte=0xEE), _one(1, 7, 0, 0, 0)])
    w.apply(pk, ln)
    # length 0 is a data error and opens nothing; the joiner of another length lies inside S = 64
    assert w.counts[RR.C_DATA_ERR] == 4 and w.counts[RR.C_ACCEPTED] == 2
    assert w.cells()[0] == ((2 << RR.ACC_SHIFT) | 32, 64, 0) and w.cells()[1] == (0, 0, 0)
    assert not (w.out == 0xEE).any()


def test_ring():
    w = RR.Window([7, 9], 4, 256, 10)
    dg = [_one(10 + e, d, 0, 16, 16) for e in range(4) for d in (7, 9)]
    dg[3] = _one(11, 9, 0, 32, 16)                              # event 11 of id 9 stays incomplete
    pk, ln = _stack(dg)
    w.apply(pk, ln)
    w.advance(4, 0)
    assert w.base == 10 and w.counts[RR.C_RELEASED] == 0
    w.advance(4, 2)
    assert w.base == 12 and w.counts[RR.C_RELEASED] == 1 and w.counts[RR.C_RELEASED_COMPLETE] == 3
    assert [b for _, b, _ in w.cells()] == [16, 16, 16, 16, 0, 0, 0, 0]     # rows 12 & 3 = 0, 13 & 3 = 1 ... kept
    pk, ln = _stack([_one(10, 7, 0, 16, 16), _one(14, 7, 0, 8, 8, byte=0x44)])
    w.apply(pk, ln)
    assert w.counts[RR.C_LATE] == 1
    assert w.out[2, 0, :8].tolist() == [0x44] * 8 and w.out[2, 0, 8:16].tolist() == [0x11] * 8   # the old event's bytes
    w.advance(100)
    assert w.base == 16 and all(c == (0, 0, 0) for c in w.cells())
    w.clear(5)
    assert w.base == 5 and w.counts == [0] * 16


def test_descriptor_rules():
    assert RR.check_descriptor([1], 8, 256)
    assert not RR.check_descriptor([], 8, 256) and not RR.check_descriptor(range(65), 8, 256)
    assert not RR.check_descriptor([1, 1], 8, 256) and not RR.check_descriptor([1], 6, 256)
    assert not RR.check_descriptor([1], 0, 256) and not RR.check_descriptor([1], 8, 128) and not RR.check_descriptor([1], 8, 0)
