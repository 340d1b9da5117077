"""A rows window on a lattice (e2sar_hip_rows.eventStep S > 1, eventPhase P; sar.RowWindow(step,
phase)) against the consecutive window's host model.  The yardstick is tests/rows_ref.py fed the
renumbered stream of tests/rows_strided_ref.py: `out` byte for byte (pre-filled, so an unwritten
byte is checked as well as a written one), every cell, counts[0..9], counts[10] = the rule-1-valid
datagrams of other ranks' events, counts[11..15] = 0 and the device base = model base * S + P."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC
import rows_ready_ref as M
import rows_ref as RR
import rows_strided_ref as RS

pytestmark = pytest.mark.gpu

LATTICES = [(2, 0), (2, 1), (3, 2), (4, 1), (5, 0), (8, 7)]


def _stride(max_pld):
    return (36 + max_pld + 15) // 16 * 16


def _segment(rng, ev, d, size, max_pld, stride):
    data = rng.integers(0, 256, size, dtype=np.uint8)
    pk, ln = O.segment_event(data, ev & RR.M64, d, ev & 0xFFFF, ev & RR.M64, 2, max_pld, stride)
    return [(pk[i], int(ln[i])) for i in range(len(ln))]


def _one(ev, d, off, blen, n, stride=64, byte=0x11):
    return RC.dgram(ev & RR.M64, d, off, blen, bytes([byte]) * n, stride, True)


def _base(b, step, phase):
    """b rounded down to the lattice; the lattice's first event where that would pass below 0."""
    r = b - (b - phase) % step
    return r if r >= 0 else phase


def _upload(hip, dgrams, stride):
    import torch
    pk = np.stack([r for r, _ in dgrams]) if dgrams else np.zeros((1, stride), np.uint8)
    ln = np.array([n for _, n in dgrams] or [0], np.uint32)
    dev = hip.torch_device
    return torch.from_numpy(pk).to(dev).view(-1), torch.from_numpy(ln.view(np.int32).copy()).to(dev), len(dgrams)


class Pair:
    """A device window on the lattice (step, phase) fed T, and the consecutive model fed T'."""

    def __init__(self, hip, ids, n_events, pitch, base, step, phase, k_alloc=None, win=None):
        from e2sar_amd import sar
        assert base % step == phase
        self.hip, self.step, self.phase = hip, step, phase
        self.win = win or sar.RowWindow(hip, ids, n_events, pitch, base, True, step=step, phase=phase)
        self.win.out.fill_(RR.FILL)
        if k_alloc:
            self.win.alloc_ready(k_alloc)
        self.ref = RR.Window(ids, n_events, pitch, RS.q(base, step))
        self.not_owned = 0

    def model(self, dgrams, stride):
        tp, not_owned = RS.renumber(dgrams, self.step, self.phase, stride)
        self.not_owned += not_owned
        if tp:
            self.ref.apply(np.stack([r for r, _ in tp]), np.array([n for _, n in tp], np.uint32), stride)

    def send(self, dgrams, stride, what=""):
        d_pk, d_ln, n = _upload(self.hip, dgrams, stride)
        self.win.reassemble(d_pk, stride, d_ln, n)
        self.model(dgrams, stride)
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
        print(f"{what}: counts {counts} model {self.ref.counts[:10]} not owned {self.not_owned}; base {base}")
        assert counts[:10] == self.ref.counts[:10], what
        assert counts[RS.C_NOT_OWNED] == self.not_owned, what
        assert counts[11:] == [0] * 5, what
        assert base == RS.event_of(self.ref.base, self.step, self.phase), what
        assert [(int(c["acc"]), int(c["bytes"]), int(c["flags"])) for c in cells] == self.ref.cells(), what
        out = self.win.out.cpu().numpy()
        diff = np.argwhere(out != self.ref.out)
        assert diff.size == 0, f"{what}: {len(diff)} bytes differ, first at {diff[:4].tolist()}"


# ----------------------------------------------------------------------------------
# 1. equivalence

BASES = [0, 3 * 2 ** 40 + 5, 2 ** 63 + 2 ** 33 + 7, "top"]          # top: 2^64 - 64 S
_STREAMS = {}


def _stream(mtu, step, phase, base):
    """Two passes of 8 window positions, 8 S consecutive event numbers each, on two ids.  The
    owned events take every size on every id; the events of other ranks, which stand between
    them in every batch, are short.  Each pass ends with datagrams that rules 1 and 2 stop,
    carrying an owned event number of the window and one of another rank.
    -> (ids, stride, pitch, passes of datagrams in event order)."""
    key = (mtu, step, phase, base)
    if key not in _STREAMS:
        max_pld = O.max_pld_len(mtu)
        stride = _stride(max_pld)
        sizes = [1, 17, max_pld, max_pld + 1, 3 * max_pld + 5, 65539]
        ids = [7, 9]
        rng = np.random.default_rng([mtu, step, phase, base % 1000])
        passes = []
        for first in (0, 8):
            dgrams = []
            for e in range(base + first * step, base + (first + 8) * step):
                i = (e - base) // step
                for j, d in enumerate(ids):
                    size = sizes[(i + 3 * j) % 6] if RS.owned(e, step, phase) else sizes[(e + j) % 5]
                    dgrams += _segment(rng, e, d, size, max_pld, stride)
            for e in (base + (first + 2) * step, base + (first + 2) * step + 1):          # owned, not owned
                bad = _one(e, 7, 0, 16, 16, stride)
                bad[0][16] = 0x20                                                       # rule 1: RE version
                ok = _one(e, 9, 0, 16, 16, stride)
                dgrams += [bad, (ok[0], 35), (ok[0], stride + 1),                       # rule 1: too short, over-long
                           _one(e, 8, 0, 16, 16, stride)]                               # rule 2, unless 1b comes first
            passes.append(dgrams)
        _STREAMS[key] = (ids, stride, 65792, passes)
    return _STREAMS[key]


@pytest.mark.parametrize("order", [0, 1, 2, "in order"])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("mtu", [100, 1500])
@pytest.mark.parametrize("step,phase", LATTICES)
def test_equivalence(hip, step, phase, mtu, base, order):
    base = _base(2 ** 64 - 64 * step if base == "top" else base, step, phase)
    ids, stride, pitch, passes = _stream(mtu, step, phase, base)
    p = Pair(hip, ids, 8, pitch, base, step, phase)
    for k, dgrams in enumerate(passes):
        dgrams = list(dgrams)
        if order != "in order":
            random.Random(order * 100 + k).shuffle(dgrams)
        p.send(dgrams, stride, f"pass {k}")
        c = p.ref.counts
        # rule 1 before 1b before 2: per pass 2 bad versions, 2 short, 2 over-long, whatever the event;
        # the foreign dataId counts as foreign on the owned event only
        assert (c[RR.C_BAD_HEADER], c[RR.C_DATA_ERR], c[RR.C_FOREIGN]) == (4 * (k + 1), 2 * (k + 1), k + 1)
        assert c[RR.C_COMPLETE] == 16 * (k + 1) and c[RR.C_LATE] == c[RR.C_EARLY] == 0
        assert p.not_owned > 0
        p.advance(8)
    assert p.ref.counts[RR.C_RELEASED_COMPLETE] == 32 and p.ref.base == RS.q(base, step) + 16


# ----------------------------------------------------------------------------------
# 2. edges in index space


@pytest.mark.parametrize("base", [3 * 8 * 1000 + 1, 2 ** 63 + 2 ** 33 + 7 - (2 ** 63 + 2 ** 33 + 7 - 1) % 3])
def test_edges_in_index_space(hip, base):
    S, P, N = 3, 1, 8
    p = Pair(hip, [7], N, 256, base, S, P)
    evs = [base - S, base + (N - 1) * S, base + N * S, base + 1, base + N * S + 1]
    p.send([_one(e, 7, 0, 16, 16, byte=0x20 + k) for k, e in enumerate(evs)], 64, "edges")
    counts, _ = p.win.parse_counts()
    assert (counts[RR.C_LATE], counts[RR.C_EARLY], counts[RS.C_NOT_OWNED], counts[RR.C_ACCEPTED]) == (1, 1, 2, 1)
    row = (RS.q(base, S) + N - 1) & (N - 1)
    cells = p.win.parse_cells()
    assert int(cells[row, 0]["bytes"]) == 16 and int(cells[row, 0]["flags"]) == RR.COMPLETE
    assert sum(int(c["bytes"]) != 0 for c in cells.reshape(-1)) == 1
    if base == 3 * 8 * 1000 + 1:
        assert row == N - 1                                       # the last row of the tensor
    assert (p.win.out[row, 0, :16] == 0x21).all().item()


# ----------------------------------------------------------------------------------
# 3. delivery


def _delivery_batches(base, step, stride=64):
    """Three batches of 4 S consecutive events, two ids, cells of 100 bytes in 4 fragments; one
    fragment lost in some events, owned ones among them."""
    rng = random.Random(step)
    ids, batches = [7, 9], []
    lost = {(0, 1): 7, (0, 3): 9, (1, 2): 7, (2, 0): 9}          # (batch, position in the batch): the id that loses
    for b in range(3):
        dgrams = []
        for e in range(base + 4 * b * step, base + 4 * (b + 1) * step):
            pos = (e - base) // step - 4 * b
            for j, d in enumerate(ids):
                frags = [_one(e, d, off, 100, min(28, 100 - off), stride, 1 + (5 * e + j) % 250) for off in range(0, 100, 28)]
                if lost.get((b, pos)) == d:
                    frags.pop(1 + (e + j) % 3)
                dgrams += frags
        rng.shuffle(dgrams)
        batches.append(dgrams)
    return ids, batches


def _check_ready(p, rule, what):
    """ready() of the device window against the model's on the renumbered window."""
    words, events, out = M.ready(p.ref, rule)
    got_words, got = p.win.parse_ready()
    print(f"{what}: ready {got_words} model {words}")
    assert got_words == words, what
    want = [M.Event(RS.event_of(e.eventNum, p.step, p.phase), e.presentMask, e.openMask, e.row, e.flags) for e in events]
    assert [M.Event(*(int(v) for v in e)) for e in got.tolist()] == want, what
    p.ref.out[:] = out
    return words


@pytest.mark.parametrize("step,phase", [(2, 1), (3, 2)])
def test_delivery(hip, step, phase):
    """reassemble -> ready(zero) -> advance(count = ready[0]) over three batches with losses,
    eager and as one captured graph replayed three times: both end in the model's state."""
    import torch
    stride, slack, k_max, cap_n = 64, 2, 4, 512
    base = _base(3 * 2 ** 40 + 5, step, phase)
    ids, batches = _delivery_batches(base, step)
    rule = M.Rule(0, slack, k_max, M.READY_ZERO)

    p = Pair(hip, ids, 8, 256, base, step, phase, k_alloc=k_max)
    ks = []
    for b, dgrams in enumerate(batches):
        p.send(dgrams, stride, f"batch {b}")
        p.win.ready(slack, k_max, zero=True)
        words = _check_ready(p, rule, f"batch {b}")
        p.win.advance(k_max, count=p.win.ready_words[0:1])
        p.ref.advance(k_max, words[0])
        p.check(f"batch {b}: advance")
        ks.append(words[0])
    assert p.ref.counts[RR.C_RELEASED] > 0 and p.ref.counts[RR.C_RELEASED_COMPLETE] > 0 and 0 < min(ks) < k_max

    # the same chain, linear, captured once with a device count
    g = Pair(hip, ids, 8, 256, base, step, phase, k_alloc=k_max)
    dev = hip.torch_device
    d_pk = torch.zeros(cap_n * stride, dtype=torch.uint8, device=dev)
    d_ln = torch.zeros(cap_n, dtype=torch.int32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g.win.reassemble(d_pk, stride, d_ln, cap_n, d_count, stream=s)
        g.win.ready(slack, k_max, zero=True, stream=s)
        g.win.advance(k_max, count=g.win.ready_words[0:1], stream=s)
    for b, dgrams in enumerate(batches):
        d_pkn, d_lnn, n = _upload(hip, dgrams, stride)
        assert 0 < n <= cap_n
        d_pk[: n * stride].copy_(d_pkn)
        d_ln[:n].copy_(d_lnn)
        d_count.fill_(n)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert (g.win.parse_ready()[0][0]) == ks[b]
    g.ref, g.not_owned = p.ref, p.not_owned
    g.check("the graph's end state")
    assert torch.equal(g.win.out, p.win.out) and torch.equal(g.win.cells, p.win.cells)
    assert torch.equal(g.win.counts, p.win.counts) and torch.equal(g.win.base, p.win.base)


# ----------------------------------------------------------------------------------
# 4. two and three ranks on one GPU


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_on_one_gpu(hip, world):
    """Every rank lands a random share of one shuffled batch, reassembles it where it landed,
    routes the other ranks' datagrams (PacketRouter, foreign only), and every owner reassembles
    the spans it is handed: no process group, the spans are read where the router packed them."""
    import torch
    from e2sar_amd import sar
    from e2sar_amd.dist import PacketRouter
    max_pld = O.max_pld_len(100)
    stride, first, ids, N = _stride(max_pld), 1000 * world + 1, [7, 9], 8
    rng = np.random.default_rng(world)
    sizes = [1, 17, max_pld, max_pld + 1, 3 * max_pld + 5, 700]
    batch = [dg for e in range(first, first + N * world) for j, d in enumerate(ids)
             for dg in _segment(rng, e, d, sizes[(e + j) % 6], max_pld, stride)]
    random.Random(world).shuffle(batch)
    landed_at = rng.integers(0, world, len(batch))
    pairs = []
    for r in range(world):
        win = sar.RowWindow.for_rank(hip, ids, N, 768, world, r, first_event=first)
        b = sar.RowWindow.first_owned(first, world, r)
        assert (win.step, win.phase) == (world, r) and b % world == r and first <= b < first + world
        pairs.append(Pair(hip, ids, N, 768, b, world, r, win=win))
    landed_not_owned = []
    for r, p in enumerate(pairs):
        share = [dg for dg, at in zip(batch, landed_at) if at == r]
        d_pk, d_ln, n = _upload(hip, share, stride)
        p.win.reassemble(d_pk, stride, d_ln, n)
        landed_not_owned.append(sum(not RS.owned(RS.event_num(s), world, r) for s, _ in share))
        router = PacketRouter(hip, stride, n, world, r)
        spk, sln, cnt = router.route(d_pk, d_ln, n, foreign_only=True)
        cnt = [int(c) for c in cnt.tolist()]
        assert cnt[r] == 0 and sum(cnt) == landed_not_owned[r]
        at = 0
        for d in range(world):
            if cnt[d]:
                pairs[d].win.reassemble(spk[at * stride:], stride, sln[at:], cnt[d])
            at += cnt[d]
        torch.cuda.synchronize()
    accepted = 0
    for r, p in enumerate(pairs):
        p.model(batch, stride)                                     # all of the rank's datagrams, wherever they landed
        p.not_owned = landed_not_owned[r]                          # the owners' spans hold owned datagrams only
        p.check(f"rank {r} of {world}")
        assert p.ref.counts[RR.C_COMPLETE] == N * len(ids)
        accepted += p.ref.counts[RR.C_ACCEPTED]
    assert accepted == len(batch)


# ----------------------------------------------------------------------------------
# 5. arguments


def test_arguments(hip):
    import torch
    from e2sar_amd import _capi, sar
    L = _capi.lib()
    stride, ids = 64, [7, 9]
    p = Pair(hip, ids, 4, 256, 5, 2, 1, k_alloc=4)
    p.send(_segment(np.random.default_rng(5), 7, 7, 50, 28, stride), stride, "something to lose")
    d_pk, d_ln, n = _upload(hip, [_one(9, 9, 0, 16, 16)] * 4, stride)
    w0, win = p.win._w, p.win
    c_ids = (C.c_uint16 * 2)(*ids)

    def desc(step, phase):
        return _capi.Rows(w0.d_out, w0.d_cells, w0.d_base, w0.d_counts, c_ids, 2, 4, 256, 1, step, phase)

    rule = _capi.RowsReadyRule(0, 2, 4, 0, 0)
    h, P = hip.handle, _capi.ERR_PARAMETER
    calls = {
        "reassemble": lambda w, base=5: L.e2sar_hip_rows_reassemble(h, C.byref(w), d_pk.data_ptr(), stride, d_ln.data_ptr(), None, n, None),
        "advance": lambda w, base=5: L.e2sar_hip_rows_advance(h, C.byref(w), None, 1, None),
        "clear": lambda w, base=5: L.e2sar_hip_rows_clear(h, C.byref(w), base, None),
        "ready": lambda w, base=5: L.e2sar_hip_rows_ready(h, C.byref(w), C.byref(rule), win.ready_words.data_ptr(), win.events.data_ptr(),
                                                          win.ready_work.data_ptr(), win.ready_work.numel(), None),
    }
    for step, phase in [(2, 2), (2, 3), (5, 5), (0, 1), (1, 1), (2 ** 32 - 1, 2 ** 32 - 1)]:
        for name, call in calls.items():
            assert call(desc(step, phase)) == P, (name, step, phase, L.e2sar_hip_last_error())
            p.check(f"{name} refuses step {step} phase {phase}")
    for base in (4, 0, 2 ** 64 - 2):
        assert calls["clear"](desc(2, 1), base) == P, base
        p.check(f"clear refuses base {base}")
    assert calls["clear"](desc(0, 0), 4) == _capi.OK and calls["clear"](desc(2, 1), 5) == _capi.OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        sar.RowWindow(hip, ids, 4, 256, 5, True, step=3, phase=1)
    with pytest.raises(ValueError):
        sar.RowWindow(hip, ids, 4, 256, 4, True, step=2, phase=2)


def test_step_one_spelled_out(hip):
    """step=1, phase=0 is the default window, with its 64-bit wrap: the model is fed the stream as it is."""
    base, stride = 2 ** 64 - 3, 64
    rng = np.random.default_rng(11)
    dgrams = [dg for e in range(base - 1, base + 9) for d in (7, 9) for dg in _segment(rng, e, d, 100, 28, stride)]
    random.Random(11).shuffle(dgrams)
    from e2sar_amd import sar
    p = Pair(hip, [7, 9], 8, 256, base, 1, 0)
    q = Pair(hip, [7, 9], 8, 256, base, 1, 0, win=sar.RowWindow(hip, [7, 9], 8, 256, base))
    for pair in (p, q):
        pair.send(dgrams, stride, "step 1")
        assert pair.not_owned == 0 and pair.ref.counts[RR.C_LATE] == 8 and pair.ref.counts[RR.C_EARLY] == 8
        pair.advance(5)
        assert pair.ref.base == 2
