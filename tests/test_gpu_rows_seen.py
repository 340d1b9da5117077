"""The seen calls (e2sar_hip_rows_reassemble_seen / _advance_seen / _clear_seen, sar.RowWindow with
frag_bytes) against the host model tests/rows_seen_ref.py, in full: the whole `out` tensor
(pre-filled with 0xA5), every cell, all 16 counts, the base and every word of the bits.  Copies of
a fragment inside one launch carry the same bytes, so that the result is determinate whichever
copy is taken; copies in different launches carry different bytes, and the first must stay."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC
import rows_ready_ref as M
import rows_ref as RR
import rows_seen_ref as SR
import rows_strided_ref as RS

pytestmark = pytest.mark.gpu


def _stride(max_pld):
    return (36 + max_pld + 15) // 16 * 16


def _segment(rng, ev, d, size, max_pld, stride):
    data = rng.integers(0, 256, size, dtype=np.uint8)
    pk, ln = O.segment_event(data, ev & RR.M64, d, ev & 0xFFFF, ev & RR.M64, 2, max_pld, stride)
    return [(pk[i], int(ln[i])) for i in range(len(ln))]


def _frag(ev, d, f, blen, fb=16, byte=None, n=None, stride=64):
    """Fragment f of a hand-cut event of blen bytes in fragments of fb: its bytes say which it is."""
    n = min(fb, blen - f * fb) if n is None else n
    return RC.dgram(ev & RR.M64, d, f * fb, blen, bytes([(0x20 + f) & 0xFF if byte is None else byte]) * n, stride, True)


def _upload(hip, dgrams, stride):
    import torch
    pk = np.stack([r for r, _ in dgrams]) if dgrams else np.zeros((1, stride), np.uint8)
    ln = np.array([n for _, n in dgrams] or [0], np.uint32)
    dev = hip.torch_device
    return torch.from_numpy(pk).to(dev).view(-1), torch.from_numpy(ln.view(np.int32).copy()).to(dev), len(dgrams)


class Pair:
    """A device window with bits and its model, fed the same batches; on a lattice the model is the
    consecutive one fed the renumbered stream."""

    def __init__(self, hip, ids, n_events, pitch, frag_bytes, max_frags=None, base=0, step=1, phase=0):
        from e2sar_amd import sar
        self.hip, self.step, self.phase = hip, step, phase
        self.win = sar.RowWindow(hip, ids, n_events, pitch, base, True, step=step, phase=phase, frag_bytes=frag_bytes,
                                 max_frags=max_frags)
        self.win.out.fill_(RR.FILL)
        self.ref = SR.SeenWindow(ids, n_events, pitch, frag_bytes, self.win.max_frags, RS.q(base, step) if step > 1 else base)
        self.not_owned = 0

    def model(self, dgrams, stride, count=None):
        if count is not None:
            dgrams = dgrams[:count]
        if self.step > 1:
            dgrams, not_owned = RS.renumber(dgrams, self.step, self.phase, stride)
            self.not_owned += not_owned
        for slot, n in dgrams:
            self.ref.push(slot.tobytes(), n, stride)

    def send(self, dgrams, stride, what="", count=None):
        import torch
        d_pk, d_ln, n = _upload(self.hip, dgrams, stride)
        d_count = None if count is None else torch.tensor([count], dtype=torch.int32, device=self.hip.torch_device)
        self.win.reassemble(d_pk, stride, d_ln, n, d_count)
        self.model(dgrams, stride, count)
        self.check(what)

    def advance(self, k, k_dev=None, what="advance"):
        import torch
        count = None if k_dev is None else torch.tensor([k_dev], dtype=torch.int32, device=self.hip.torch_device)
        self.win.advance(k, count)
        self.ref.advance(k, k_dev)
        self.check(what)

    def check(self, what=""):
        counts, base = self.win.parse_counts()
        cells = self.win.parse_cells().reshape(-1)
        want = list(self.ref.counts)
        want[RS.C_NOT_OWNED] = self.not_owned
        print(f"{what}: counts {counts} model {want}; base {base}")
        assert counts == want, what
        assert base == (RS.event_of(self.ref.base, self.step, self.phase) if self.step > 1 else self.ref.base), what
        assert [(int(c["acc"]), int(c["bytes"]), int(c["flags"])) for c in cells] == self.ref.cells(), what
        bits = self.win.parse_seen()
        assert bits.shape == (self.win.n_events, len(self.win.ids), self.win.max_frags // 32)
        assert bits.reshape(-1, bits.shape[2]).tolist() == self.ref.seen_words(), what
        out = self.win.out.cpu().numpy()
        diff = np.argwhere(out != self.ref.out)
        assert diff.size == 0, f"{what}: {len(diff)} bytes differ, first at {diff[:4].tolist()}"

    def flags(self, ev, d):
        return self.ref.cells()[self.ref.cell_index(ev, d)][2]


# ----------------------------------------------------------------------------------
# 1. the hole


def test_hole_example(hip):
    """Fragment 0 twice, fragment 1 never, fragment 2 once: the plain call marks the cell COMPLETE."""
    p = Pair(hip, [7], 8, 256, 16)
    assert p.win.max_frags == 128
    f = [_frag(3, 7, j, 48) for j in range(3)]
    p.send([f[0], f[0], f[2]], 64, "duplicate and loss")
    assert p.flags(3, 7) == 0 and p.ref.counts[SR.C_DUPLICATE] == 1 and p.ref.counts[RR.C_COMPLETE] == 0
    assert (p.ref.out[3, 0, 16:32] == RR.FILL).all()
    p.send([f[1]], 64, "the lost fragment")
    assert p.flags(3, 7) == RR.COMPLETE and p.ref.counts[RR.C_COMPLETE] == 1


# ----------------------------------------------------------------------------------
# 2. where the copies stand in a launch


def test_duplicates_adjacent_in_a_run(hip):
    p = Pair(hip, [7], 8, 256, 16)
    order = [0, 1, 1, 2, 3, 3, 3, 4, 5, 6, 6, 7, 8, 9, 9]
    p.send([_frag(1, 7, f, 160) for f in order], 64)
    assert p.flags(1, 7) == RR.COMPLETE and p.ref.counts[SR.C_DUPLICATE] == 5
    # descending and repeated: every stretch is one lane long
    order = [5, 4, 4, 3, 2, 2, 1, 0, 0, 5]
    p.send([_frag(2, 7, f, 96) for f in order], 64)
    assert p.flags(2, 7) == RR.COMPLETE and p.ref.counts[SR.C_DUPLICATE] == 9


def test_duplicates_in_one_wave_around_another_run(hip):
    p = Pair(hip, [7, 9], 8, 256, 16)
    a = lambda f: _frag(4, 7, f, 128)
    b = lambda f: _frag(4, 9, f, 80)
    p.send([a(0), a(1), a(2), b(0), b(1), a(1), a(2), a(3), b(1), b(2), a(4), a(5), b(3), b(4), a(5), a(6), a(7), b(0)], 64)
    assert p.flags(4, 7) == p.flags(4, 9) == RR.COMPLETE and p.ref.counts[SR.C_DUPLICATE] == 5
    assert p.ref.counts[RR.C_COMPLETE] == 2


def test_duplicates_in_different_workgroups(hip):
    """The whole stream sent twice and shuffled, MTU 100 and an event of 65 539 bytes among short ones."""
    max_pld = O.max_pld_len(100)
    stride = _stride(max_pld)
    rng = np.random.default_rng(22)
    events = [(10, 7, 65539), (11, 7, 3 * max_pld + 5), (12, 7, 1), (13, 7, max_pld)]
    dgrams = [dg for e, d, s in events for dg in _segment(rng, e, d, s, max_pld, stride)]
    twice = dgrams + dgrams
    random.Random(22).shuffle(twice)
    p = Pair(hip, [7], 8, 65792, max_pld, base=8)
    p.send(twice, stride)
    assert all(p.flags(e, d) == RR.COMPLETE for e, d, _ in events)
    assert p.ref.counts[SR.C_DUPLICATE] == len(dgrams) == p.ref.counts[RR.C_ACCEPTED]


def test_duplicates_in_a_later_launch(hip):
    """The later copies carry other bytes: the first stay."""
    p = Pair(hip, [7, 9], 8, 256, 16)
    p.send([_frag(5, d, f, 112) for d in (7, 9) for f in (0, 2, 3, 6)], 64, "first launch")
    again = [_frag(5, d, f, 112, byte=0xEE) for d in (7, 9) for f in (0, 2, 3, 6)]
    rest = [_frag(5, d, f, 112) for d in (7, 9) for f in (1, 4, 5)]
    both = again + rest
    random.Random(5).shuffle(both)
    p.send(both, 64, "second launch")
    assert p.flags(5, 7) == p.flags(5, 9) == RR.COMPLETE and p.ref.counts[SR.C_DUPLICATE] == 8
    assert not (p.win.out == 0xEE).any().item()
    p.send(again + rest, 64, "third launch: all duplicates")
    assert p.ref.counts[SR.C_DUPLICATE] == 8 + 14 and p.ref.counts[RR.C_COMPLETE] == 2


@pytest.mark.parametrize("order", [0, "in order"])
def test_word_boundaries(hip, order):
    """Copies of fragments 31, 32, 63, 64 and 127: the ends of the bits' 32-bit words and 16-byte stores."""
    marks = [31, 32, 63, 64, 127]
    p = Pair(hip, [7, 9], 8, 2048, 16, 128)
    dgrams = [_frag(6, 7, f, 2048) for f in range(128)] + [_frag(6, 7, f, 2048) for f in marks]
    dgrams += [_frag(6, 9, f, 2048) for f in marks + marks]
    if order != "in order":
        random.Random(order).shuffle(dgrams)
    p.send(dgrams, 64, "first launch")
    assert p.flags(6, 7) == RR.COMPLETE and p.ref.counts[SR.C_DUPLICATE] == 10
    c = p.ref.cell_index(6, 9)
    assert p.ref.seen_words()[c] == [1 << 31, 1 | 1 << 31, 1, 1 << 31] and p.ref.seen_words()[c - 1] == [0xFFFFFFFF] * 4
    p.send([_frag(6, 7, f, 2048, byte=0xEE) for f in marks], 64, "later copies")
    assert p.ref.counts[SR.C_DUPLICATE] == 15


# ----------------------------------------------------------------------------------
# 3. whole streams with copies of the first, a middle and the last fragment

BASE_RT = 3 * 2 ** 40 + 5
_RT = {}


def _round_trip_stream(mtu, n_ids):
    """tests/test_gpu_rows.py's stream -- every length on every id once at least, in passes of at
    most 8 events -- with fragments 0, n // 2 and n - 1 of every event sent twice.
    -> (ids, stride, max_pld, passes of datagrams in event order, copies per pass)."""
    key = (mtu, n_ids)
    if key not in _RT:
        max_pld = O.max_pld_len(mtu)
        stride = _stride(max_pld)
        sizes = [1, 15, 16, 17, max_pld - 1, max_pld, max_pld + 1, 3 * max_pld + 5, 65539]
        ids = [7, 9, 300][:n_ids]
        rng = np.random.default_rng([mtu, n_ids, 3])
        cells = [(k // n_ids, ids[k % n_ids], sizes[k % len(sizes)]) for k in range(-(-len(sizes) // n_ids) * n_ids)]
        passes, copies = [], []
        for first in range(0, cells[-1][0] + 1, 8):
            dgrams, extra = [], 0
            for e, d, s in cells:
                if first <= e < first + 8:
                    fr = _segment(rng, BASE_RT + e, d, s, max_pld, stride)
                    twice = sorted({0, len(fr) // 2, len(fr) - 1})
                    extra += len(twice)
                    for k, dg in enumerate(fr):
                        dgrams += [dg, dg] if k in twice else [dg]
            passes.append(dgrams)
            copies.append(extra)
        _RT[key] = (ids, stride, max_pld, passes, copies)
    return _RT[key]


@pytest.mark.parametrize("order", [0, 1, 2, "in order"])
@pytest.mark.parametrize("n_ids", [1, 3])
@pytest.mark.parametrize("mtu", [100, 1499, 1500, 9000])
def test_round_trip_with_copies(hip, mtu, n_ids, order):
    ids, stride, max_pld, passes, copies = _round_trip_stream(mtu, n_ids)
    p = Pair(hip, ids, 8, 65792, max_pld, base=BASE_RT)
    dup = 0
    for k, dgrams in enumerate(passes):
        dgrams = list(dgrams)
        if order != "in order":
            random.Random(order * 100 + k).shuffle(dgrams)
        p.send(dgrams, stride, f"pass {k}")
        dup += copies[k]
        assert p.ref.counts[SR.C_DUPLICATE] == dup
        assert all(fl == RR.COMPLETE for _, b, fl in p.ref.cells() if b)
        p.advance(8, what=f"advance {k}")
        assert not any(p.ref.seen)


# ----------------------------------------------------------------------------------
# 4. the grid


def test_grid_rules_and_empty_fragment(hip):
    """Rule 4b's three refusals open no cell and set no bit, in more than one wave; a fragment of no
    bytes is accepted off the grid, twice, and sets no bit."""
    p = Pair(hip, [7, 9], 8, 256, 16, 128)
    bad = [RC.dgram(1, 7, 8, 4000, b"a" * 8, 64, True),              # off the grid
           RC.dgram(1, 9, 16, 4000, b"a" * 17, 64, True),            # longer than fragBytes
           RC.dgram(2, 7, 128 * 16, 4000, b"a" * 16, 64, True),      # f == maxFrags
           RC.dgram(2, 9, 0xFFFFFFF0, 0xFFFFFFFF, b"a" * 15, 64, True)]
    p.send(bad * 20, 64, "refused")
    assert p.ref.counts[RR.C_DATA_ERR] == 80 and all(c == (0, 0, 0) for c in p.ref.cells()) and not any(p.ref.seen)
    empty = RC.dgram(1, 7, 5, 4000, b"", 64, True)
    p.send([empty, _frag(1, 7, 127, 4000), empty, bad[0], _frag(1, 7, 127, 4000)], 64, "no bytes")
    c = p.ref.cell_index(1, 7)
    assert p.ref.cells()[c] == ((3 << RR.ACC_SHIFT) | 16, 4000, RR.TRUNCATED) and p.ref.seen[c] == 1 << 127
    assert p.ref.counts[SR.C_DUPLICATE] == 1 and p.ref.counts[RR.C_ACCEPTED] == 3 and p.ref.counts[RR.C_DATA_ERR] == 81


@pytest.mark.parametrize("order", [0, "in order"])
def test_longer_than_the_pitch(hip, order):
    """400 bytes into a pitch of 256: max_frags, not the pitch, bounds the event; copies on either side
    of the pitch and across it."""
    p = Pair(hip, [7], 8, 256, 16, 128)
    dgrams = [_frag(2, 7, f, 400) for f in list(range(25)) + [15, 16, 20, 24]]
    if order != "in order":
        random.Random(order).shuffle(dgrams)
    p.send(dgrams, 64)
    assert p.flags(2, 7) == RR.COMPLETE | RR.TRUNCATED and p.ref.counts[SR.C_DUPLICATE] == 4
    assert p.ref.cells()[p.ref.cell_index(2, 7)][0] == (25 << RR.ACC_SHIFT) | 400
    # an odd fragment length: 28 bytes, the pitch inside fragment 9
    max_pld = O.max_pld_len(92)
    stride = _stride(max_pld)
    q = Pair(hip, [7], 8, 256, max_pld)
    fr = _segment(np.random.default_rng(4), 3, 7, 700, max_pld, stride)
    dgrams = fr + [fr[9], fr[9], fr[24]]
    if order != "in order":
        random.Random(order).shuffle(dgrams)
    q.send(dgrams, stride)
    assert max_pld == 28 and q.flags(3, 7) == RR.COMPLETE | RR.TRUNCATED and q.ref.counts[SR.C_DUPLICATE] == 3


# ----------------------------------------------------------------------------------
# 5. a lattice


@pytest.mark.parametrize("phase", [0, 2])
def test_lattice_with_copies(hip, phase):
    """Step 3, fed the events of all three ranks, every fourth datagram twice."""
    max_pld = O.max_pld_len(100)
    stride = _stride(max_pld)
    rng = np.random.default_rng([5, phase])
    base = 3 * 1000 + phase
    dgrams = []
    for ev in range(3000, 3000 + 3 * 8):
        for d in (7, 9):
            dgrams += _segment(rng, ev, d, 40 + 13 * (ev % 11), max_pld, stride)
    owned = sum(1 for s, n in dgrams if RS.owned(RS.event_num(s), 3, phase))
    dgrams = [dg for k, dg in enumerate(dgrams) for _ in range(2 if k % 4 == 0 else 1)]
    random.Random(phase).shuffle(dgrams)
    p = Pair(hip, [7, 9], 8, 256, max_pld, base=base, step=3, phase=phase)
    p.send(dgrams, stride)
    assert p.ref.counts[RR.C_ACCEPTED] == owned and p.ref.counts[RR.C_COMPLETE] == 16
    assert p.ref.counts[SR.C_DUPLICATE] > 8 and p.not_owned > 2 * owned
    p.advance(3, what="advance on the lattice")
    assert p.ref.base == 1003 and sum(1 for s in p.ref.seen if s) == 10


# ----------------------------------------------------------------------------------
# 6. the count on the device


@pytest.mark.parametrize("count", [0, 1, 64, 65, 130, 1000])
def test_device_count(hip, count):
    """Datagrams at or past n leave no trace, bits included: a copy past n is no duplicate."""
    max_pld, stride, n = 28, 64, 130
    rng = np.random.default_rng(7)
    dgrams = [dg for e in range(8) for dg in _segment(rng, 50 + e, 7, 15 * max_pld - 3, max_pld, stride)]
    dgrams = [dg for k, dg in enumerate(dgrams) for _ in range(2 if k % 10 == 3 else 1)][:n]
    assert len(dgrams) == n
    p = Pair(hip, [7], 8, 512, max_pld, base=50)
    p.send(dgrams, stride, count=count)
    assert p.ref.counts[RR.C_ACCEPTED] + p.ref.counts[SR.C_DUPLICATE] == min(count, n)
    if count == 0:
        assert p.ref.counts == [0] * 16 and not any(p.ref.seen)
    if count >= n:
        assert p.ref.counts[SR.C_DUPLICATE] == 12


# ----------------------------------------------------------------------------------
# 7. the ring


def test_ring(hip):
    p = Pair(hip, [7, 9], 4, 256, 16)
    first = [_frag(e, d, f, 96) for e in range(4) for d in (7, 9) for f in range(6) if (e, d, f) != (1, 9, 5)]
    p.send(first + first[:7], 64, "first lap")
    assert p.ref.counts[SR.C_DUPLICATE] == 7 and p.ref.counts[RR.C_COMPLETE] == 7
    p.advance(4, 2, "a partial advance")                         # events 0 and 1 go, the bits of 2 and 3 stay
    assert p.ref.base == 2 and [bool(s) for s in p.ref.seen] == [False] * 4 + [True] * 4
    # events 4 and 5 land in the rows of 0 and 1: none of their fragments is a duplicate; a copy of event 2's is
    second = [_frag(e, d, f, 96, byte=0x60 + f) for e in (4, 5) for d in (7, 9) for f in range(6)]
    p.send(second + [_frag(2, 7, 3, 96, byte=0xEE), first[0]], 64, "second lap")
    assert p.ref.counts[SR.C_DUPLICATE] == 8 and p.ref.counts[RR.C_LATE] == 1 and p.ref.counts[RR.C_COMPLETE] == 11
    p.advance(1000, what="k above nEvents")
    assert p.ref.base == 6 and not any(p.ref.seen)
    p.send([_frag(6, 7, 0, 96), _frag(9, 9, 5, 96)], 64, "before clear")
    p.win.clear(1 << 40)
    p.ref.clear(1 << 40)
    p.check("clear")
    assert not any(p.ref.seen) and p.win.parse_seen().sum() == 0
    p.send([_frag((1 << 40) + 2, 7, f, 96) for f in (0, 0, 5)], 64, "after clear")
    assert p.ref.counts[SR.C_DUPLICATE] == 1


# ----------------------------------------------------------------------------------
# 8. one captured graph


def test_one_captured_graph(hip):
    """reassemble -> ready(zero) -> advance(ready's k), captured once on one stream, replayed three
    times with fresh datagrams: copies, and a loss that the newer events give up."""
    import torch
    stride, cap_n, slack = 64, 200, 2
    dev = hip.torch_device
    p = Pair(hip, [7, 9], 4, 256, 16)
    p.win.alloc_ready(4)
    d_pk = torch.zeros(cap_n * stride, dtype=torch.uint8, device=dev)
    d_ln = torch.zeros(cap_n, dtype=torch.int32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        p.win.reassemble(d_pk, stride, d_ln, cap_n, d_count, stream=s)
        p.win.ready(slack, zero=True, stream=s)
        p.win.advance(4, p.win.ready_words[0:1], stream=s)
    p.check("capture launches nothing")
    # replay 0: events 0, 1 whole with copies, 2 loses fragment 1 and has fragment 0 twice -- the plain call's hole;
    # replay 1: events 3, 4 -- two newer than 2, which is given up with zeros in its row; replay 2: 5, 6, 7 and a
    # copy of 5's fragment inside the batch
    batches = [[(0, range(6)), (1, range(6)), (2, (0, 0, 2, 3, 4, 5))], [(3, range(6)), (4, (0, 1, 1, 2, 3, 4, 5))],
               [(5, (0, 1, 2, 2, 3, 4, 5)), (6, range(6)), (7, (5, 4, 3))]]
    rule = M.Rule(0, slack, 4, M.READY_ZERO)
    total_k = 0
    for replay, events in enumerate(batches):
        dgrams = [_frag(e, d, f, 96, byte=0x10 * replay + f) for e, fs in events for d in (7, 9) for f in fs]
        random.Random(replay).shuffle(dgrams)
        n = len(dgrams)
        pk, ln, _ = _upload(hip, dgrams, stride)
        d_pk[: n * stride].copy_(pk)
        d_ln[:n].copy_(ln)
        d_count.fill_(n)
        torch.cuda.synchronize()
        graph.replay()
        p.model(dgrams, stride)
        words, evs, out = M.ready(p.ref, rule)
        p.ref.out[...] = out
        p.ref.advance(4, words[0])
        got, _ = p.win.parse_ready()
        assert got == words, replay
        p.check(f"replay {replay}")
        total_k += words[0]
        assert p.ref.base == total_k
        if replay == 1:                                           # the given-up event's row went out as zeros
            assert words[2] == 1 and (p.ref.out[2, :, :] == 0).all()
    assert total_k == 7 and p.ref.counts[RR.C_RELEASED] == 2 and p.ref.counts[RR.C_RELEASED_COMPLETE] == 12
    assert p.ref.counts[SR.C_DUPLICATE] == 2 + 2 + 2


# ----------------------------------------------------------------------------------
# 9. statuses


def test_statuses(hip):
    import torch
    from e2sar_amd import _capi
    L = _capi.lib()
    stride = 64
    p = Pair(hip, [7, 9], 4, 256, 16)
    p.send([_frag(1, 7, f, 48) for f in (0, 0, 2)], stride)       # something to lose
    d_pk, d_ln, n = _upload(hip, [_frag(2, 9, 0, 16)] * 4, stride)
    ids = (C.c_uint16 * 2)(7, 9)
    w0, s0 = p.win._w, p.win._seen

    def desc(**kw):
        w = _capi.Rows(w0.d_out, w0.d_cells, w0.d_base, w0.d_counts, ids, 2, 4, 256, 1)
        for k, v in kw.items():
            setattr(w, k, v)
        return w

    def bits(**kw):
        z = _capi.RowsSeen(s0.d_seen, 16, 128)
        for k, v in kw.items():
            setattr(z, k, v)
        return z

    ref = lambda x: C.byref(x) if x is not None else None
    h, P, R = hip.handle, _capi.ERR_PARAMETER, _capi.ERR_OUT_OF_RANGE

    def reas(ctx, w, z, pk=d_pk.data_ptr(), st=stride, ln=d_ln.data_ptr(), mx=n):
        return L.e2sar_hip_rows_reassemble_seen(ctx, ref(w), ref(z), pk, st, ln, None, mx, None)

    def adv(ctx, w, z, k=1):
        return L.e2sar_hip_rows_advance_seen(ctx, ref(w), ref(z), None, k, None)

    def clr(ctx, w, z, base=0):
        return L.e2sar_hip_rows_clear_seen(ctx, ref(w), ref(z), base, None)

    calls = []
    for f in (reas, adv, clr):
        calls += [(P, lambda f=f: f(None, desc(), bits())), (P, lambda f=f: f(h, None, bits())),
                  (P, lambda f=f: f(h, desc(), None))]
        # the plain calls' descriptor rules, one of each kind
        for w in (desc(d_cells=0), desc(nIds=0), desc(nEvents=6), desc(pitch=128), desc(d_out=w0.d_out + 128),
                  desc(eventStep=2, eventPhase=2)):
            calls.append((P, lambda f=f, w=w: f(h, w, bits())))
        for z in (bits(d_seen=0), bits(fragBytes=0), bits(maxFrags=0), bits(maxFrags=64), bits(maxFrags=192),
                  bits(maxFrags=129), bits(d_seen=s0.d_seen + 4), bits(d_seen=s0.d_seen + 8)):
            calls.append((P, lambda f=f, z=z: f(h, desc(), z)))
    calls += [(P, lambda: reas(h, desc(), bits(), pk=0)), (P, lambda: reas(h, desc(), bits(), ln=0)),
              (P, lambda: reas(h, desc(), bits(), st=72)), (P, lambda: reas(h, desc(), bits(), pk=d_pk.data_ptr() + 8)),
              (R, lambda: reas(h, desc(), bits(), mx=(1 << 30) + 1)), (R, lambda: reas(h, desc(nEvents=1 << 31), bits())),
              (P, lambda: clr(h, desc(eventStep=2, eventPhase=1), bits(), base=4)),
              # 2^30 cells of 2^32 - 128 bits each: more than 2^31 - 1 workgroups of 256 16-byte words
              (R, lambda: adv(h, desc(nEvents=1 << 29), bits(maxFrags=0xFFFFFF80), k=1 << 29))]
    for k, (want, call) in enumerate(calls):
        assert call() == want, (k, L.e2sar_hip_last_error())
    p.check("failing calls")
    assert reas(h, desc(), bits(), mx=0) == _capi.OK                # nothing launched
    assert adv(h, desc(), bits(), k=0) == _capi.OK
    p.check("maxPackets 0, kMax 0")
    assert L.e2sar_hip_rows_seen_bytes(4, 2, 128) == p.win.seen.numel() * 4
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------
# 10. a plain window beside it


def test_plain_window_beside(hip):
    """A window without frag_bytes in the same process is the plain family's, bit for bit: the same
    stream, copies and all, gives rows_ref's result there -- the hole included."""
    from e2sar_amd import sar
    max_pld = O.max_pld_len(100)
    stride = _stride(max_pld)
    rng = np.random.default_rng(10)
    dgrams = [dg for e in range(8) for d in (7, 9) for dg in _segment(rng, e, d, 30 + 50 * e, max_pld, stride)]
    holed = [_frag(8, 7, f, 48) for f in (0, 0, 2)]
    p = Pair(hip, [7, 9], 16, 512, max_pld)
    plain = sar.RowWindow(hip, [7, 9], 16, 512)
    assert plain.seen is None and plain.max_frags == 0
    with pytest.raises(ValueError):
        plain.parse_seen()
    plain.out.fill_(RR.FILL)
    ref = RR.Window([7, 9], 16, 512)
    for k, batch in enumerate([dgrams[:50], dgrams[50:], holed]):
        st = 64 if batch is holed else stride
        if batch is not holed:
            batch = list(batch)
            random.Random(k).shuffle(batch)
        d_pk, d_ln, n = _upload(hip, batch, st)
        plain.reassemble(d_pk, st, d_ln, n)
        for slot, ln in batch:
            ref.push(slot.tobytes(), ln, st)
        if batch is not holed:
            p.send(batch, st, f"seen {k}")
        counts, base = plain.parse_counts()
        cells = [(int(c["acc"]), int(c["bytes"]), int(c["flags"])) for c in plain.parse_cells().reshape(-1)]
        assert counts == ref.counts and base == ref.base and cells == ref.cells()
        assert (plain.out.cpu().numpy() == ref.out).all()
    assert ref.cells()[ref.cell_index(8, 7)][2] == RR.COMPLETE     # the plain contract: complete with a hole
    plain.advance(4)
    ref.advance(4)
    assert plain.parse_counts() == (ref.counts, ref.base) and ref.counts[SR.C_DUPLICATE] == 0
    assert p.ref.counts[RR.C_COMPLETE] == 16
