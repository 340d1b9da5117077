"""Reassembly straight into a tensor (e2sar_hip_rows_reassemble / _advance / _clear, sar.RowWindow)
against the host model tests/rows_ref.py, in full: the whole `out` tensor -- pre-filled with
0xA5, so an unwritten byte is checked as well as a written one -- every cell, all 16 counts
and the base.  The streams send no fragment twice and keep every cell's opener determinate
within a launch, the proviso under which the result holds for any order and any cut."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC
import rows_ref as RR

pytestmark = pytest.mark.gpu

MARK = 0xEE                  # payload byte of every fragment that must be dropped


def _stride(max_pld):
    return (36 + max_pld + 15) // 16 * 16


def _stack(dgrams, stride):
    if not dgrams:
        return np.zeros((1, stride), np.uint8), np.zeros(1, np.uint32), 0
    return np.stack([r for r, _ in dgrams]), np.array([n for _, n in dgrams], np.uint32), len(dgrams)


def _segment(rng, ev, d, size, max_pld, stride):
    data = rng.integers(0, 256, size, dtype=np.uint8)
    pk, ln = O.segment_event(data, ev & RR.M64, d, ev & 0xFFFF, ev & RR.M64, 2, max_pld, stride)
    return [(pk[i], int(ln[i])) for i in range(len(ln))]


class Pair:
    """A device window and its model, fed the same batches."""

    def __init__(self, hip, ids, n_events, pitch, base=0, with_lb=True):
        import torch
        from e2sar_amd import sar
        self.hip, self.torch = hip, torch
        self.win = sar.RowWindow(hip, ids, n_events, pitch, base, with_lb)
        self.win.out.fill_(RR.FILL)
        self.ref = RR.Window(ids, n_events, pitch, base, with_lb)

    def upload(self, dgrams, stride):
        pk, ln, n = _stack(dgrams, stride)
        dev = self.hip.torch_device
        return (self.torch.from_numpy(pk).to(dev).view(-1), self.torch.from_numpy(ln.view(np.int32).copy()).to(dev),
                pk, ln, n)

    def send(self, dgrams, stride, count=None, max_packets=None):
        d_pk, d_ln, pk, ln, n = self.upload(dgrams, stride)
        d_count = None
        if count is not None:
            d_count = self.torch.tensor([count], dtype=self.torch.int32, device=self.hip.torch_device)
        self.win.reassemble(d_pk, stride, d_ln, n if max_packets is None else max_packets, d_count)
        self.ref.apply(pk[:n], ln[:n], stride, count)
        self.check()

    def check(self, what=""):
        counts, base = self.win.parse_counts()
        cells = self.win.parse_cells().reshape(-1)
        got = [(int(c["acc"]), int(c["bytes"]), int(c["flags"])) for c in cells]
        assert counts == self.ref.counts, what
        assert base == self.ref.base, what
        assert got == self.ref.cells(), what
        out = self.win.out.cpu().numpy()
        diff = np.argwhere(out != self.ref.out)
        assert diff.size == 0, f"{what}: {len(diff)} bytes differ, first at {diff[:4].tolist()}"


# ----------------------------------------------------------------------------------
# 1. round trip

_RT = {}


def _round_trip_stream(mtu, n_ids):
    """Passes of at most 8 events: every length on every id once at least; -> (ids, stride, pitch, passes)."""
    key = (mtu, n_ids)
    if key not in _RT:
        max_pld = O.max_pld_len(mtu)
        stride = _stride(max_pld)
        sizes = [1, 15, 16, 17, max_pld - 1, max_pld, max_pld + 1, 3 * max_pld + 5, 65539]
        ids = [7, 9, 300][:n_ids]
        rng = np.random.default_rng([mtu, n_ids])
        cells = [(k // n_ids, ids[k % n_ids], sizes[k % len(sizes)]) for k in range(-(-len(sizes) // n_ids) * n_ids)]
        passes = []
        for first in range(0, cells[-1][0] + 1, 8):
            passes.append([_segment(rng, BASE_RT + e, d, s, max_pld, stride) for e, d, s in cells if first <= e < first + 8])
        _RT[key] = (ids, stride, 65792, passes)
    return _RT[key]


BASE_RT = 3 * 2 ** 40 + 5


@pytest.mark.parametrize("order", [0, 1, 2, "in order"])
@pytest.mark.parametrize("n_ids", [1, 3])
@pytest.mark.parametrize("mtu", [100, 1499, 1500, 9000])
def test_round_trip(hip, mtu, n_ids, order):
    ids, stride, pitch, passes = _round_trip_stream(mtu, n_ids)
    p = Pair(hip, ids, 8, pitch, BASE_RT)
    for k, events in enumerate(passes):
        dgrams = [dg for ev in events for dg in ev]
        if order != "in order":
            random.Random(order * 100 + k).shuffle(dgrams)
        p.send(dgrams, stride)
        assert p.ref.counts[RR.C_ACCEPTED] == sum(len(ev) for ps in passes[:k + 1] for ev in ps)
        assert all(fl == RR.COMPLETE for _, b, fl in p.ref.cells() if b)
        p.win.advance(8)
        p.ref.advance(8)
        p.check("advance")
    assert p.ref.counts[RR.C_RELEASED_COMPLETE] == p.ref.counts[RR.C_COMPLETE] == sum(len(ps) for ps in passes)


# ----------------------------------------------------------------------------------
# 2. window edges


def _one(ev, d, off, blen, n, stride=64, byte=0x11, with_lb=True):
    return RC.dgram(ev & RR.M64, d, off, blen, bytes([byte]) * n, stride, with_lb)


@pytest.mark.parametrize("base", [2 ** 64 - 3, 7 * 2 ** 33, 0])
def test_window_edges(hip, base):
    p = Pair(hip, [7], 8, 256, base)
    evs = [base - 1, base, base + 7, base + 8]
    p.send([_one(e, 7, 0, 16, 16, byte=0x20 + k) for k, e in enumerate(evs)] +
           [_one(base + j, 7, 16, 40, 12, byte=0x30 + j) for j in range(1, 7)], 64)
    assert p.ref.counts[RR.C_LATE] == 1 and p.ref.counts[RR.C_EARLY] == 1 and p.ref.counts[RR.C_COMPLETE] == 2


# ----------------------------------------------------------------------------------
# 3. rejected datagrams


@pytest.mark.parametrize("with_lb", [True, False])
def test_rejected_datagrams(hip, with_lb):
    """Foreign ids, a wrong RE version, datagrams too short for their headers, a length above
    the stride, and a header-only datagram that announces length 0: counts move, nothing is
    written, no cell opens.  (A header-only datagram of an event of at least a byte is an
    accepted fragment of no bytes by rule 6; it comes last, in a launch of its own.)"""
    stride, hl = 64, 36 if with_lb else 20
    p = Pair(hip, [7, 9], 8, 256, 100, with_lb)
    bad = _one(101, 7, 0, 16, 16, with_lb=with_lb)
    bad[0][hl - 20] = 0x20
    bad2 = _one(101, 7, 0, 16, 16, with_lb=with_lb)
    bad2[0][hl - 19] = 0x01
    ok = _one(102, 9, 0, 16, 16, with_lb=with_lb)
    dgrams = [_one(101, 8, 0, 16, 16, with_lb=with_lb), _one(101, 0, 0, 16, 16, with_lb=with_lb), bad, bad2,
              (ok[0], 0), (ok[0], hl - 1), _one(103, 7, 0, 0, 0, with_lb=with_lb), (ok[0], stride + 1), (ok[0], 1 << 31)]
    p.send(dgrams * 9, stride)                                  # more than one wave
    c = p.ref.counts
    assert (c[RR.C_FOREIGN], c[RR.C_BAD_HEADER], c[RR.C_DATA_ERR]) == (18, 36, 27) and c[RR.C_ACCEPTED] == 0
    assert all(cell == (0, 0, 0) for cell in p.ref.cells()) and (p.ref.out == RR.FILL).all()
    p.send([_one(103, 7, 0, 5, 0, with_lb=with_lb)], stride)
    assert p.ref.cells()[p.ref.cell_index(103, 7)] == (1 << RR.ACC_SHIFT, 5, 0)


# ----------------------------------------------------------------------------------
# 4. truncation


@pytest.mark.parametrize("order", [0, "in order"])
def test_truncation(hip, order):
    max_pld = O.max_pld_len(100)
    stride = _stride(max_pld)
    rng = np.random.default_rng(4)
    dgrams = [dg for k, s in enumerate([255, 256, 257, 700]) for dg in _segment(rng, 40 + k, 7, s, max_pld, stride)]
    if order != "in order":
        random.Random(order).shuffle(dgrams)
    p = Pair(hip, [7], 4, 256, 40)
    p.send(dgrams, stride)
    flags = [fl for _, _, fl in p.ref.cells()]
    assert flags == [RR.COMPLETE, RR.COMPLETE, RR.COMPLETE | RR.TRUNCATED, RR.COMPLETE | RR.TRUNCATED]
    assert p.ref.counts[RR.C_BYTES] == 255 + 256 + 257 + 700


# ----------------------------------------------------------------------------------
# 5. lengths that disagree


@pytest.mark.parametrize("stride,pl", [(64, 28), (1472, 64)])
def test_lengths_that_disagree(hip, stride, pl):
    rng = np.random.default_rng([5, stride])
    S = 8 * pl
    keys = [(200 + e, d) for e in range(4) for d in (7, 9)]
    data = {k: rng.integers(0, 0xEE, S, dtype=np.uint8) for k in keys}

    def frag(k, j, blen):
        return RC.dgram(k[0], k[1], j * pl, blen, data[k][j * pl:(j + 1) * pl], stride, True)

    p = Pair(hip, [7, 9], 4, 4096, 200)
    p.send([frag(k, 3, S) for k in keys], stride)               # the openers, not at offset 0
    second = []
    for k in keys:
        second += [frag(k, 0, S + 1000), frag(k, 1, S - pl), frag(k, 2, S)]                       # joiners
        second += [RC.dgram(k[0], k[1], S - pl + 1, S + 1000, bytes([MARK]) * pl, stride, True),      # ends past S
                   RC.dgram(k[0], k[1], S + 512, S + 2000, bytes([MARK]) * pl, stride, True),
                   RC.dgram(k[0], k[1], 100, 50, bytes([MARK]) * pl, stride, True)]                   # its own length
        second += [frag(k, j, S) for j in range(4, 8)]
    random.Random(stride).shuffle(second)
    p.send(second, stride)
    assert p.ref.counts[RR.C_DATA_ERR] == 3 * len(keys) and p.ref.counts[RR.C_COMPLETE] == len(keys)
    assert not (p.win.out == MARK).any().item()
    for k in keys:
        assert p.ref.out.reshape(-1, 4096)[p.ref.cell_index(*k)][:S].tobytes() == data[k].tobytes()


# ----------------------------------------------------------------------------------
# 6. an event split over two calls


@pytest.mark.parametrize("mtu", [100, 1500])
def test_event_split_over_two_calls(hip, mtu):
    max_pld = O.max_pld_len(mtu)
    stride = _stride(max_pld)
    dgrams = _segment(np.random.default_rng(mtu), 77, 9, 20 * max_pld + 3, max_pld, stride)
    random.Random(6).shuffle(dgrams)
    p = Pair(hip, [7, 9], 2, 32768, 76)
    p.send(dgrams[:13], stride)
    assert p.ref.cells()[p.ref.cell_index(77, 9)][2] == 0
    p.send(dgrams[13:], stride)
    assert p.ref.cells()[p.ref.cell_index(77, 9)][2] == RR.COMPLETE


# ----------------------------------------------------------------------------------
# 7. device count


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 130, 1000])
def test_device_count(hip, count):
    """Slots and lengths at or past n hold well-formed datagrams of events inside the window:
    they leave no trace."""
    max_pld, stride, n = 28, 64, 130
    rng = np.random.default_rng(7)
    dgrams = [dg for e in range(8) for dg in _segment(rng, 50 + e, 7, 17 * max_pld - 3, max_pld, stride)][:n]
    assert len(dgrams) == n
    p = Pair(hip, [7], 8, 512, 50)
    p.send(dgrams, stride, count=count, max_packets=n)
    assert p.ref.counts[RR.C_ACCEPTED] == min(count, n)
    if count == 0:
        assert p.ref.counts == [0] * 16 and (p.ref.out == RR.FILL).all()


# ----------------------------------------------------------------------------------
# 8. ring


def test_ring(hip):
    import torch
    stride, max_pld = 64, 28
    rng = np.random.default_rng(8)
    p = Pair(hip, [7, 9], 4, 256, 0)
    first = []
    for e in range(4):
        for d in (7, 9):
            dg = _segment(rng, e, d, 100, max_pld, stride)
            first += dg[:-1] if (e, d) == (1, 9) else dg          # one left incomplete
    straggler = first[0]
    assert RR.Window([7, 9], 4, 256).cell_index(0, 7) == 0
    p.send(first, stride)
    k = torch.tensor([2], dtype=torch.int32, device=hip.torch_device)
    p.win.advance(4, k)
    p.ref.advance(4, 2)
    p.check("advance by a device word")
    assert p.ref.base == 2 and p.ref.counts[RR.C_RELEASED] == 1 and p.ref.counts[RR.C_RELEASED_COMPLETE] == 3
    old = p.ref.out[0, 0, 40:100].copy()
    # events 4 and 5 land in rows 0 and 1; they are shorter, so the bytes past them are the old events'
    p.send([straggler] + [dg for e in (4, 5) for d in (7, 9) for dg in _segment(rng, e, d, 40, max_pld, stride)], stride)
    assert p.ref.counts[RR.C_LATE] == 1
    assert (p.ref.out[0, 0, 40:100] == old).all() and p.ref.cells()[0][1] == 40
    k.fill_(0)
    p.win.advance(4, k)
    p.ref.advance(4, 0)
    p.check("k = 0")
    p.win.advance(1000)
    p.ref.advance(1000)
    p.check("k above nEvents")
    assert p.ref.base == 6 and all(c == (0, 0, 0) for c in p.ref.cells())


# ----------------------------------------------------------------------------------
# 9. one captured graph


def test_one_captured_graph(hip):
    import torch
    stride, max_pld, cap_n = 64, 28, 200
    dev = hip.torch_device
    p = Pair(hip, [7, 9], 4, 512, 0)
    d_pk = torch.zeros(cap_n * stride, dtype=torch.uint8, device=dev)
    d_ln = torch.zeros(cap_n, dtype=torch.int32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    d_k = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        p.win.reassemble(d_pk, stride, d_ln, cap_n, d_count, stream=s)
        p.win.advance(4, d_k, stream=s)
    clear = torch.cuda.CUDAGraph()
    with torch.cuda.graph(clear, stream=s):
        p.win.clear(1 << 40, stream=s)
    p.check("capture launches nothing")
    rng = np.random.default_rng(9)
    base = 0
    # no event is sent twice: event 7 is early, 2 stays complete in the window over a replay, the
    # second replay's count cuts fragments off (5 stays incomplete and is released so), 8 is early
    for replay, (events, count_over, k) in enumerate([([0, 1, 2, 7], 0, 2), ([3, 4, 5], 5, 1), ([6, 8], 0, 4)]):
        dgrams = [dg for e in events for d in (7, 9) for dg in _segment(rng, e, d, 60 + 37 * e, max_pld, stride)]
        random.Random(replay).shuffle(dgrams)
        pk, ln, n = _stack(dgrams, stride)
        assert n <= cap_n
        d_pk[: n * stride].copy_(torch.from_numpy(pk).to(dev).view(-1))
        d_ln[:n].copy_(torch.from_numpy(ln.view(np.int32).copy()).to(dev))
        count = n - count_over
        d_count.fill_(count)
        d_k.fill_(k)
        torch.cuda.synchronize()
        graph.replay()
        p.ref.apply(pk, ln, stride, count)
        p.ref.advance(4, k)
        p.check(f"replay {replay}")
        base += k
        assert p.ref.base == base
    assert p.ref.counts[RR.C_EARLY] > 0 and p.ref.counts[RR.C_RELEASED] > 0 and p.ref.counts[RR.C_RELEASED_COMPLETE] > 0
    for _ in range(2):
        clear.replay()
        p.ref.clear(1 << 40)
        p.check("captured clear")
        p.send(_segment(rng, (1 << 40) + 1, 9, 50, max_pld, stride), stride)


# ----------------------------------------------------------------------------------
# 10. statuses


def test_statuses(hip):
    import torch
    from e2sar_amd import _capi
    L = _capi.lib()
    stride = 64
    p = Pair(hip, [7, 9], 4, 256, 0)
    p.send(_segment(np.random.default_rng(10), 1, 7, 50, 28, stride), stride)      # something to lose
    d_pk, d_ln, _, _, n = p.upload([_one(2, 9, 0, 16, 16)] * 4, stride)
    ids = (C.c_uint16 * 65)(*range(1, 66))
    w0 = p.win._w

    def desc(**kw):
        w = _capi.Rows(w0.d_out, w0.d_cells, w0.d_base, w0.d_counts, ids, 2, 4, 256, 1)
        for k, v in kw.items():
            setattr(w, k, v)
        return w

    def reas(ctx, w, pk=d_pk.data_ptr(), st=stride, ln=d_ln.data_ptr(), mx=n):
        return L.e2sar_hip_rows_reassemble(ctx, C.byref(w) if w is not None else None, pk, st, ln, None, mx, None)

    h, P, R = hip.handle, _capi.ERR_PARAMETER, _capi.ERR_OUT_OF_RANGE
    bad_desc = [desc(d_out=0), desc(d_cells=0), desc(d_base=0), desc(d_counts=0),
                desc(dataIds=C.POINTER(C.c_uint16)()), desc(nIds=0), desc(nIds=65), desc(dataIds=(C.c_uint16 * 2)(5, 5)),
                desc(nEvents=0), desc(nEvents=6), desc(pitch=0), desc(pitch=128), desc(pitch=257), desc(d_out=w0.d_out + 128)]
    calls = [(P, lambda: reas(None, desc())), (P, lambda: reas(h, None)), (P, lambda: reas(h, desc(), pk=0)),
             (P, lambda: reas(h, desc(), ln=0)), (P, lambda: reas(h, desc(), st=72)), (P, lambda: reas(h, desc(), st=48)),
             (P, lambda: reas(h, desc(), pk=d_pk.data_ptr() + 8)),
             (R, lambda: reas(h, desc(), mx=(1 << 30) + 1)), (R, lambda: reas(h, desc(nEvents=1 << 31))),
             (P, lambda: L.e2sar_hip_rows_advance(None, C.byref(desc()), None, 1, None)),
             (P, lambda: L.e2sar_hip_rows_advance(h, None, None, 1, None)),
             (P, lambda: L.e2sar_hip_rows_clear(None, C.byref(desc()), 0, None)),
             (P, lambda: L.e2sar_hip_rows_clear(h, None, 0, None))]
    for w in bad_desc:
        calls += [(P, lambda w=w: reas(h, w)), (P, lambda w=w: L.e2sar_hip_rows_advance(h, C.byref(w), None, 1, None)),
                  (P, lambda w=w: L.e2sar_hip_rows_clear(h, C.byref(w), 0, None))]
    for k, (want, call) in enumerate(calls):
        assert call() == want, (k, L.e2sar_hip_last_error())
        p.check(f"failing call {k}")
    assert reas(h, desc(), mx=0) == _capi.OK                      # nothing launched
    p.check("maxPackets 0")
    torch.cuda.synchronize()


def test_sixty_four_ids(hip):
    """The largest id list: the first, the last and a middle column."""
    ids = list(range(1000, 1064))
    p = Pair(hip, ids, 2, 256, 8)
    rng = np.random.default_rng(64)
    p.send([dg for d in (1000, 1031, 1063) for e in (8, 9) for dg in _segment(rng, e, d, 100, 28, 64)] +
           [_one(8, 999, 0, 16, 16), _one(9, 1064, 0, 16, 16)], 64)
    assert p.ref.counts[RR.C_COMPLETE] == 6 and p.ref.counts[RR.C_FOREIGN] == 2
