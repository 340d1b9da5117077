"""e2sar_hip_rows_ready (sar.RowWindow.ready) against the host model tests/rows_ready_ref.py, word
for word: d_ready, the k records, the whole `out` tensor, the cells, the counts and the base.
`out`, d_events, d_ready and the work buffer are pre-filled with a fill byte, so that what must
never be written is checked as well as what must be."""
import ctypes as C
import random

import numpy as np
import pytest

import reas_cuts as RC
import rows_ready_ref as M
import rows_ref as RR

pytestmark = pytest.mark.gpu

FILL = 0xC3                  # d_ready, d_events and the work buffer before a call
FILL32 = int.from_bytes(bytes([FILL]) * 4, "little")


def _one(ev, d, off, blen, n, stride=64, byte=0x11):
    return RC.dgram(ev & RR.M64, d, off, blen, bytes([byte]) * n, stride, True)


def _cell(ev, d, size, stride=64, byte=0x11, drop=()):
    """The fragments of one cell of `size` bytes, without those whose index is in `drop`."""
    pl = stride - 36
    return [_one(ev, d, off, size, min(pl, size - off), stride, byte) for q, off in enumerate(range(0, size, pl)) if q not in drop]


def _whole(ev, ids, size=16, stride=64):
    return [f for j, d in enumerate(ids) for f in _cell(ev, d, size, stride, 0x20 + j)]


class Pair:
    """A device window with its ready buffers and the model, fed the same batches."""

    def __init__(self, hip, ids, n_events, pitch, base=0, k_alloc=None):
        import torch
        from e2sar_amd import sar
        self.hip, self.torch = hip, torch
        self.win = sar.RowWindow(hip, ids, n_events, pitch, base)
        self.win.out.fill_(RR.FILL)
        self.win.alloc_ready(n_events + 8 if k_alloc is None else k_alloc)
        self.ref = RR.Window(ids, n_events, pitch, base)
        self.words = None

    def upload(self, dgrams, stride):
        dev = self.hip.torch_device
        pk = np.stack([r for r, _ in dgrams]) if dgrams else np.zeros((1, stride), np.uint8)
        ln = np.array([n for _, n in dgrams] or [0], np.uint32)
        return (self.torch.from_numpy(pk).to(dev).view(-1), self.torch.from_numpy(ln.view(np.int32).copy()).to(dev),
                pk, ln, len(dgrams))

    def feed(self, dgrams, stride=64):
        d_pk, d_ln, pk, ln, n = self.upload(dgrams, stride)
        self.win.reassemble(d_pk, stride, d_ln, n)
        self.ref.apply(pk[:n], ln[:n], stride)

    def prefill(self):
        self.win.ready_words.fill_(FILL32 - (1 << 32))
        self.win.events.fill_(FILL)
        self.win.ready_work.fill_(FILL)

    def ready(self, slack, k_max, required=None, zero=False, null_events=False, what=""):
        """One call, checked in full against the model; -> (words, events) of the model."""
        from e2sar_amd import _capi
        self.prefill()
        mask = sum(1 << self.ref.ids.index(d) for d in required or ())
        rule = M.Rule(mask, slack, k_max, M.READY_ZERO if zero else 0)
        if null_events:
            w = self.win
            crule = _capi.RowsReadyRule(mask, slack, k_max, rule.flags, 0)
            rc = _capi.lib().e2sar_hip_rows_ready(self.hip.handle, C.byref(w._w), C.byref(crule), w.ready_words.data_ptr(), None,
                                                  w.ready_work.data_ptr(), w.ready_work.numel(), None)
            assert rc == _capi.OK, _capi.lib().e2sar_hip_last_error()
        else:
            self.win.ready(slack, k_max, required, zero)
        words, events, out = M.ready(self.ref, rule)
        self.ref.out[:] = out
        self.words = words
        self.check(words, [] if null_events else events, what)
        return words, events

    def check(self, words, events, what=""):
        """`ready_words`, the records and the fill behind them, and the window's state."""
        got_words, got = self.win.parse_ready()
        raw = self.win.events.cpu().numpy()
        print(f"{what}: ready {got_words} model {words}")
        assert got_words == words, what
        n = len(events)
        if n:
            assert len(got) == n
            assert [M.Event(*(int(v) for v in e)) for e in got.tolist()] == events, what
        assert (raw[n * 32:] == FILL).all(), f"{what}: a record at or past k was written"
        self.check_window(what)

    def check_window(self, what=""):
        counts, base = self.win.parse_counts()
        cells = self.win.parse_cells().reshape(-1)
        assert counts == self.ref.counts, what
        assert base == self.ref.base, what
        assert [(int(c["acc"]), int(c["bytes"]), int(c["flags"])) for c in cells] == self.ref.cells(), what
        out = self.win.out.cpu().numpy()
        diff = np.argwhere(out != self.ref.out)
        assert diff.size == 0, f"{what}: {len(diff)} bytes of out differ, first at {diff[:4].tolist()}"

    def advance(self, k_max, what="advance"):
        self.win.advance(k_max, count=self.win.ready_words[0:1])
        self.ref.advance(k_max, self.words[0])
        self.check_window(what)


# ----------------------------------------------------------------------------------
# 1. edges, hand-cut


def test_empty_window(hip):
    p = Pair(hip, [7, 9], 8, 256, 5)
    for zero in (False, True):
        words, _ = p.ready(0, 8, zero=zero, what=f"empty, zero {zero}")
        assert words == [0] * 8


@pytest.mark.parametrize("base", [0, 13, 2 ** 64 - 3])
def test_all_complete(hip, base):
    """Every event whole: k = N, H = N with the last row open; a base that is no multiple of N
    wraps the ring, one at 2^64 - 3 the event numbers."""
    ids = [7, 9]
    p = Pair(hip, ids, 8, 256, base)
    p.feed([f for e in range(8) for f in _whole(base + e, ids)])
    words, events = p.ready(3, 1000, zero=True, what="all complete")          # kMax above N
    assert words == [8, 8, 0, 8, 16, 0, 0, 0]
    assert [e.eventNum for e in events] == [(base + e) & RR.M64 for e in range(8)]
    assert [e.row for e in events] == [(base + e) & 7 for e in range(8)]
    for k_max in (0, 1):
        words, _ = p.ready(3, k_max, zero=True, what=f"kMax {k_max}")
        assert words[0] == k_max and words[3] == 8
    p.ready(3, 8)
    p.advance(8)
    assert p.ref.counts[RR.C_RELEASED_COMPLETE] == 16 and p.ref.base == (base + 8) & RR.M64
    assert p.ready(3, 8, what="after the advance")[0] == [0] * 8


@pytest.mark.parametrize("slack", [0, 1, 4, 5, 6, 0xFFFFFFFF])
def test_hole_at_event_0(hip, slack):
    """Event 0 lost a fragment, 1 .. 5 are whole: the newest is 5 events on.  At distance
    slack - 1 (slack 6) k = 0; at slack (5) and beyond it is given up.  Event 6 is empty: only
    the horizon, 6, is ahead of it, and slack 0 stops there as every other."""
    ids = [7, 9]
    p = Pair(hip, ids, 8, 256, 40)
    p.feed(_cell(40, 7, 100, drop=(1,)) + _cell(40, 9, 100) + [f for e in range(41, 46) for f in _whole(e, ids)])
    words, events = p.ready(slack, 8, zero=True, what=f"slack {slack}")
    if slack <= 5:
        assert words == [6, 5, 1, 6, 11, 1, 0, 0] and events[0].flags == M.EV_GIVEN_UP
        assert events[0].presentMask == 2 and events[0].openMask == 3
    else:
        assert words == [0, 0, 0, 6, 0, 0, 0, 0]


def test_required_subset_and_truncated(hip):
    """Only id 9 is required and id 7 never arrives; event 1's cell passes the pitch."""
    ids = [7, 9, 11]
    p = Pair(hip, ids, 4, 256, 0)
    p.feed(_cell(0, 9, 50) + _cell(0, 11, 60, drop=(0,)) + _cell(1, 9, 300) + _cell(2, 11, 20))
    words, events = p.ready(0xFFFFFFFF, 4, required=[9], zero=True, what="required subset")
    assert words == [2, 2, 0, 3, 2, 1, 0, 0]
    assert [e.flags for e in events] == [M.EV_COMPLETE, M.EV_COMPLETE | M.EV_TRUNCATED]
    assert events[0].presentMask == 2 and events[0].openMask == 6
    assert p.ready(0xFFFFFFFF, 4, what="all required")[0][0] == 0


def test_sixty_four_ids(hip):
    ids = list(range(1000, 1064))
    p = Pair(hip, ids, 2, 256, 8)
    p.feed([f for d in ids for f in _cell(8, d, 40)] + _cell(9, 1063, 40) + _cell(9, 1000, 40, drop=(0,)))
    words, events = p.ready(0xFFFFFFFF, 2, zero=True, what="64 ids")
    assert words == [1, 1, 0, 2, 64, 0, 0, 0] and events[0].presentMask == 2 ** 64 - 1
    words, events = p.ready(0xFFFFFFFF, 2, required=[1063], zero=True, what="bit 63 alone")
    assert words == [2, 2, 0, 2, 65, 1, 0, 0] and events[1].presentMask == 1 << 63 and events[1].openMask == (1 << 63) | 1


def test_events_null(hip):
    ids = [7]
    p = Pair(hip, ids, 8, 256, 3)
    p.feed([f for e in (3, 4, 6) for f in _whole(e, ids)])
    words, _ = p.ready(1, 8, zero=True, null_events=True, what="d_events NULL")
    assert words == [4, 3, 1, 4, 3, 0, 0, 0]
    p.advance(8)


# ----------------------------------------------------------------------------------
# 2. zeroing


@pytest.mark.parametrize("pitch", [256, 768])
def test_zeroing(hip, pitch):
    """Whole cells of every length around a 16-byte chunk and the pitch, an open incomplete
    cell and an empty one in a ready event, and the event at index k, which keeps every byte."""
    ids = [7, 9]
    sizes = [1, 15, 16, 17, pitch - 1, pitch, pitch + 5]
    dg = [f for e, s in enumerate(sizes) for f in _cell(e, 7, s, byte=0x31 + e) + _cell(e, 9, sizes[-1 - e], byte=0x51 + e)]
    dg += _cell(7, 7, 200, byte=0x61, drop=(2,))                   # event 7: an open incomplete cell and an empty one
    dg += _cell(8, 7, 100, byte=0x62) + _cell(8, 9, 100, byte=0x63, drop=(0,))   # index k: waited for
    dg += _whole(12, ids)
    for zero in (False, True):
        p = Pair(hip, ids, 16, pitch, 0)
        p.feed(dg)
        before = p.ref.out.copy()
        words, events = p.ready(5, 16, zero=zero, what=f"pitch {pitch} zero {zero}")
        assert words[0] == 8 and words[2] == 1 and events[7].openMask == 1 and events[7].presentMask == 0
        if not zero:
            assert (p.ref.out == before).all()
            continue
        assert (p.ref.out[8:] == before[8:]).all() and (p.ref.out[7] == 0).all()
        for e, s in enumerate(sizes):
            assert (p.ref.out[e, 0, :min(s, pitch)] == 0x31 + e).all() and (p.ref.out[e, 0, s:] == 0).all()
        p.advance(16)


def test_zeroing_two_pieces(hip):
    """pitch 16384: a cell spans two pieces, with the event's end in the first, in the second,
    at their boundary and at the pitch."""
    ids, stride, pitch = [7], 1472, 16384
    sizes = [100, 8191, 8192, 8193, 12345, 16383, 16384, 20000]
    dg = [f for e, s in enumerate(sizes) for f in _cell(e, 7, s, stride, 0x41 + e)] + _cell(8, 7, 9000, stride, 0x4a, drop=(3,))
    p = Pair(hip, ids, 16, pitch, 0)
    p.feed(dg, stride)
    before = p.ref.out.copy()
    p.ready(0xFFFFFFFF, 16, what="flag off")
    assert (p.ref.out == before).all()
    words, _ = p.ready(0xFFFFFFFF, 16, zero=True, what="two pieces")
    assert words[0] == 8 and (p.ref.out[8:] == before[8:]).all()
    for e, s in enumerate(sizes):
        assert (p.ref.out[e, 0, :min(s, pitch)] == 0x41 + e).all() and (p.ref.out[e, 0, s:] == 0).all()


# ----------------------------------------------------------------------------------
# 3. more than one workgroup of events


@pytest.mark.parametrize("lost,slack,want_k", [((5, 300, 301, 777, 1010), 20, 1010), ((), 20, 1024), ((0,), 1024, 0),
                                               ((255, 256, 511, 512), 0, 1024)])
def test_many_events(hip, lost, slack, want_k):
    ids, N, base = [7, 9, 11], 1024, 5 * 2 ** 40 + 777
    dg = []
    for e in range(N):
        for j, d in enumerate(ids):
            if not (e in lost and j == e % 3):
                dg.append(_one(base + e, d, 0, 16, 16, byte=1 + (e + j) % 250))
    random.Random(3).shuffle(dg)
    p = Pair(hip, ids, N, 256, base)
    p.feed(dg)
    words, events = p.ready(slack, 2000, zero=True, what=f"lost {lost}")
    assert words[0] == want_k and words[3] == N and words[2] == sum(e < want_k for e in lost)
    p.advance(2000)
    assert p.ref.base == base + want_k


# ----------------------------------------------------------------------------------
# 4. random streams


@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_streams(hip, seed):
    ids, n_events, base, slack, k_max, batches = M.random_family(seed)
    p = Pair(hip, ids, n_events, M.PITCH, base)
    for step, batch in enumerate(batches):
        p.feed(batch, M.STRIDE)
        p.check_window(f"seed {seed} step {step}: reassembly")
        p.ready(slack, k_max, zero=True, what=f"seed {seed} step {step}")
        p.advance(k_max, f"seed {seed} step {step}: advance")


# ----------------------------------------------------------------------------------
# 5. one captured graph


def test_one_captured_graph(hip):
    """reassemble -> ready -> advance, captured once and replayed over six batches with losses;
    the host reads only between replays."""
    import torch
    stride, cap_n, slack, k_max = 64, 400, 2, 3
    dev = hip.torch_device
    ids = [7, 9]
    p = Pair(hip, ids, 8, 512, 0)
    d_pk = torch.zeros(cap_n * stride, dtype=torch.uint8, device=dev)
    d_ln = torch.zeros(cap_n, dtype=torch.int32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        p.win.reassemble(d_pk, stride, d_ln, cap_n, d_count, stream=s)
        p.win.ready(slack, k_max, zero=True, stream=s)
        p.win.advance(k_max, count=p.win.ready_words[0:1], stream=s)
    p.check_window("capture launches nothing")
    rng = random.Random(5)
    rule = M.Rule(0, slack, k_max, M.READY_ZERO)
    ev, ks = 0, []
    for replay in range(6):
        dgrams = []
        for _ in range(3):
            for j, d in enumerate(ids):
                frags = _cell(ev, d, rng.choice([30, 200, 512, 600]), byte=1 + (7 * ev + j) % 250)
                if rng.random() < 0.3:
                    frags.pop(rng.randrange(len(frags)))
                dgrams += frags
            ev += 1
        rng.shuffle(dgrams)
        d_pkn, d_lnn, pk, ln, n = p.upload(dgrams, stride)
        assert 0 < n <= cap_n
        d_pk[: n * stride].copy_(d_pkn)
        d_ln[:n].copy_(d_lnn)
        d_count.fill_(n)
        p.prefill()
        torch.cuda.synchronize()
        graph.replay()
        p.ref.apply(pk, ln, stride, n)
        words, events, out = M.ready(p.ref, rule)
        p.ref.out[:] = out
        p.ref.advance(k_max, words[0])
        p.check(words, events, f"replay {replay}")
        ks.append(words[0])
    assert p.ref.base == sum(ks) and max(ks) == k_max
    assert p.ref.counts[RR.C_RELEASED] > 0 and p.ref.counts[RR.C_RELEASED_COMPLETE] > 0


# ----------------------------------------------------------------------------------
# 6. statuses


def test_statuses(hip):
    import torch
    from e2sar_amd import _capi
    L = _capi.lib()
    ids = [7, 9]
    p = Pair(hip, ids, 4, 256, 0)
    p.feed(_whole(0, ids) + _cell(1, 7, 50))
    words, events = p.ready(0, 4, what="before the failing calls")
    w, w0 = p.win, p.win._w
    c_ids = (C.c_uint16 * 2)(7, 9)
    work, nwork = w.ready_work.data_ptr(), w.ready_work.numel()
    assert nwork == L.e2sar_hip_rows_ready_work_bytes(4) and nwork % 256 == 0 and nwork >= 4 * 20

    def desc(**kw):
        d = _capi.Rows(w0.d_out, w0.d_cells, w0.d_base, w0.d_counts, c_ids, 2, 4, 256, 1)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def rule(mask=0, slack=0, k_max=4, flags=1, reserved=0):
        return _capi.RowsReadyRule(mask, slack, k_max, flags, reserved)

    def call(ctx=hip.handle, d=desc(), r=rule(), ready=w.ready_words.data_ptr(), ev=w.events.data_ptr(), wk=work, nb=nwork):
        return L.e2sar_hip_rows_ready(ctx, C.byref(d) if d is not None else None, C.byref(r) if r is not None else None,
                                      ready, ev, wk, nb, None)

    P, R = _capi.ERR_PARAMETER, _capi.ERR_OUT_OF_RANGE
    big = torch.empty(L.e2sar_hip_rows_ready_work_bytes(1 << 20), dtype=torch.uint8, device=hip.torch_device)
    calls = [(P, b"ctx is NULL", lambda: call(ctx=None)), (P, b"descriptor is NULL", lambda: call(d=None)),
             (P, b"NULL device buffer", lambda: call(d=desc(d_cells=0))), (P, b"power of two", lambda: call(d=desc(nEvents=6))),
             (P, b"multiple of 256", lambda: call(d=desc(pitch=128))), (P, b"nIds", lambda: call(d=desc(nIds=65))),
             (R, b"cells", lambda: call(d=desc(nEvents=1 << 31))),
             (P, b"rule is NULL", lambda: call(r=None)), (P, b"NULL device buffer", lambda: call(ready=0)),
             (P, b"NULL device buffer", lambda: call(wk=0)), (P, b"reserved", lambda: call(r=rule(reserved=1))),
             (P, b"unknown rule flags", lambda: call(r=rule(flags=2))), (P, b"unknown rule flags", lambda: call(r=rule(flags=0x80000001))),
             (P, b"requiredMask", lambda: call(r=rule(mask=4))), (P, b"requiredMask", lambda: call(r=rule(mask=1 << 63))),
             (P, b"too small", lambda: call(nb=nwork - 1)), (P, b"too small", lambda: call(nb=0)),
             (P, b"256-byte aligned", lambda: call(wk=work + 128, nb=nwork)),
             (P, b"d_ready not 4-byte", lambda: call(ready=w.ready_words.data_ptr() + 2)),
             (P, b"d_events not 8-byte", lambda: call(ev=w.events.data_ptr() + 4)),
             # 2^20 events of 2 cells of 2^24 / 8192 pieces: 2^32 workgroups
             (R, b"zero launch too large", lambda: call(d=desc(nEvents=1 << 20, pitch=1 << 24), r=rule(k_max=1 << 20),
                                                        wk=big.data_ptr(), nb=big.numel()))]
    p.prefill()
    for k, (want, msg, fn) in enumerate(calls):
        assert fn() == want, (k, L.e2sar_hip_last_error())
        assert msg in L.e2sar_hip_last_error(), (k, L.e2sar_hip_last_error())
    # a failing call launches nothing: every buffer holds its fill, the window what it held
    torch.cuda.synchronize()
    assert (w.ready_words.cpu().numpy().view(np.uint8) == FILL).all() and (w.events.cpu().numpy() == FILL).all()
    assert (w.ready_work.cpu().numpy() == FILL).all()
    p.check_window("failing calls")
    with pytest.raises(ValueError):
        Pair(hip, ids, 4, 256, 0, k_alloc=2).win.ready(0, 3)      # more records than alloc_ready made room for
    # kMax 0 succeeds: k = 0 and H, nothing zeroed
    assert p.ready(0, 0, zero=True, what="kMax 0")[0] == [0, 0, 0, 2, 0, 0, 0, 0]
    assert p.ready(0, 4, zero=True, what="the same rule again")[0] == words
