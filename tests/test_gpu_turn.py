"""A receive graph that runs without end: e2sar_hip_reas_collect_next and e2sar_hip_reas_turn
(reas_turn.hpp, the cursor kernels of reas_collect.hpp) against tests/turn_ref.py's model, which
tests/test_turn_ref_cpu.py pins to the CPU oracle with the turn as its clock.

Every reassembler here is the small one the model's preconditions are stated for: 64 slots, a
64-KiB arena, 64 completed and 64 lost records, LB headers, COMPACTABLE.

Lost records: the device logs every collection of a key, the reference its first (DESIGN.md
5.3).  With max_carries of 2 or more the model shows no key collected twice and the device's
records and counters are compared with the oracle's outright; below that the comparison is
with the model's full list, and with the oracle's after a host's de-duplication (a key's first
record; reassemblyLoss counted once per key)."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
import turn_ref as T

pytestmark = pytest.mark.gpu

SENT = 0xC3
HISTORY = ("eventSuccess", "totalPackets", "totalBytes", "badHeaderDiscards", "dataErrCnt", "enqueueLoss",
           "reassemblyLoss")
OCC = ("arenaUsed", "tableUsed", "inProgress", "completedPending")
FAR = dict(arena_mark=1 << 62, record_mark=0xFFFFFFFF, table_mark=0xFFFFFFFF)      # marks never reached


@pytest.fixture(scope="module")
def s():
    return T.stream()


@pytest.fixture(scope="module")
def models(s):
    """max_carries -> (the model's run, the oracle's stats and lost records): computed once."""
    out = {}
    for m in (0, 1, 2, T.NEVER):
        _, _, stats, lost = T.replay_oracle(s, m)
        out[m] = (T.run(s, m), {f: int(v) for f, v in stats.items()}, sorted(lost))
    return out


def _reas(hip, flags=0, compactable=True):
    from e2sar_amd import sar
    return sar.DeviceReassembler(hip, with_lb_header=True, table_slots=T.SLOTS, queue_capacity=T.QCAP, lost_capacity=64,
                                 arena_bytes=T.ARENA, compactable=compactable, flags=flags)


def _upload(hip, pk, ln):
    import torch
    dpk = torch.from_numpy(np.ascontiguousarray(pk).reshape(-1)).to(hip.torch_device)
    dln = torch.from_numpy(np.ascontiguousarray(ln, np.uint32).view(np.int32).copy()).to(hip.torch_device)
    return dpk, dln


def _stats(R):
    st = R.stats()
    return {f: int(getattr(st, f)) for f in HISTORY + OCC + ("lostPending", "errorFlags")}


def _lost(R):
    return [(r.eventNum, r.dataId, r.numFragments, r.enqueueLoss) for r in R.lost_poll()]


class Bufs:
    """The caller's side of collect_next and turn: output, index, counts, cursor, status."""

    def __init__(self, hip, R, out_bytes=T.ARENA, max_events=T.QCAP):
        import torch
        from e2sar_amd import sar
        dev = hip.torch_device
        self.out = torch.full((out_bytes,), SENT, dtype=torch.uint8, device=dev)
        self.index = torch.zeros(max_events * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
        self.counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
        self.status = torch.full((4,), -1, dtype=torch.int64, device=dev)
        self.cursor = R.new_cursor()
        self.max_events = max_events

    def cur(self):
        return int(self.cursor.cpu()[0])

    def stat(self):
        return [int(x) for x in self.status.cpu().tolist()]

    def cnt(self):
        return [int(x) for x in self.counts.cpu().tolist()]

    def delivered(self, pitch=0):
        """{key: (bytes, numFragments)} of the last collect_next, read from `out`."""
        from e2sar_amd import sar
        rows = sar.parse_collect(self.index, self.counts)
        o = self.out.cpu().numpy()
        got = {}
        for r in rows:
            off, n = int(r["outOffset"]), int(r["bytes"])
            assert not pitch or n <= pitch
            got[(int(r["eventNum"]), int(r["dataId"]))] = (o[off:off + n].tobytes(), int(r["numFragments"]))
            if pitch:
                assert not o[off + n:off + pitch].any(), "row not zero-filled"
        assert len(got) == len(rows), "an event delivered twice in one call"
        return got


def _end_checks(R, run, ostats, olost, lost):
    """Every counter of stats() and the sorted lost records, against the model and the oracle."""
    st = _stats(R)
    assert {f: st[f] for f in HISTORY + ("inProgress",)} == run.stats
    assert sorted(lost) == sorted(run.lost)
    seen, once = set(), []
    for r in lost:                                  # a host's de-duplication: a key's first record
        if r[:2] not in seen:
            seen.add(r[:2])
            once.append(r)
    assert sorted(r[:3] for r in once) == olost and all(r[3] == 0 for r in lost)
    assert {**{f: st[f] for f in ostats}, "reassemblyLoss": len(once)} == ostats
    if not run.twice:
        assert {f: st[f] for f in ostats} == ostats and sorted(r[:3] for r in lost) == olost
    assert st["errorFlags"] == 0


# ----------------------------------------------------------------------------------
# 1: eager, turn by turn


@pytest.mark.parametrize("m", [0, 1, 2, T.NEVER])
def test_eager_turn_by_turn(hip, s, models, m):
    run, ostats, olost = models[m]
    R = _reas(hip)
    B = Bufs(hip, R)
    dpk, dln = _upload(hip, s.pk, s.ln)
    base, lost, seen = R.arena_ptr, [], set()
    for b, step in enumerate(run.steps):
        a, e = s.cuts[b], s.cuts[b + 1]
        R.reassemble(dpk[a * s.stride:], s.stride, dln[a:], e - a)
        st = _stats(R)
        assert {f: st[f] for f in OCC} == step.after_batch and st["errorFlags"] == 0, (b, st)
        R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
        got = B.delivered()
        assert got == step.delivered, b
        assert not seen & set(got), "an event delivered twice over the run"
        seen |= set(got)
        assert B.cur() == len(got) and B.cnt()[0] == len(got) and B.cnt()[2] == 0, b
        R.turn(B.cursor, B.status, max_carries=m)
        assert B.stat() == step.status and B.cur() == 0, (b, B.stat(), step.status)
        st = _stats(R)
        assert {f: st[f] for f in OCC} == step.after_turn and st["errorFlags"] == 0, (b, st)
        now = _lost(R)
        assert sorted(now) == step.lost, b
        lost += now
    assert R.arena_ptr == base
    _end_checks(R, run, ostats, olost, lost)
    R.close()


# ----------------------------------------------------------------------------------
# 2: one graph, twelve replays


def test_one_graph_twelve_replays(hip, s, models):
    """reassemble_dev(count word) -> collect_next (rows) -> turn, captured once and replayed for
    batches 2..12 with each batch's datagrams, lengths and count written into the same device
    buffers: no host read of the reassembler between the capture and the end, only of the
    outputs.  Events begin in one replay and end in a later one."""
    import torch
    from e2sar_amd import _capi
    m = 2
    run, ostats, olost = models[m]
    dev = hip.torch_device
    pitch = 10000
    R = _reas(hip)
    B = Bufs(hip, R, out_bytes=T.QCAP * pitch)
    d_pk = torch.zeros(T.BATCH_MAX * s.stride, dtype=torch.uint8, device=dev)
    d_ln = torch.zeros(T.BATCH_MAX, dtype=torch.int32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    h_pk = torch.from_numpy(s.pk.reshape(-1))
    h_ln = torch.from_numpy(s.ln.view(np.int32).copy())

    def load(b):
        a, e = s.cuts[b], s.cuts[b + 1]
        d_pk[:(e - a) * s.stride].copy_(h_pk[a * s.stride:e * s.stride])
        d_ln[:e - a].copy_(h_ln[a:e])
        d_n.fill_(e - a)

    def chain(stream):
        R.reassemble_dev(d_pk, s.stride, d_ln, d_n, max_packets=T.BATCH_MAX, stream=stream)
        R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP, pitch, stream=stream)
        R.turn(B.cursor, B.status, max_carries=m, stream=stream)

    def check(b, seen):
        step = run.steps[b]
        got = B.delivered(pitch)
        assert got == step.delivered, b
        assert not seen & set(got)
        seen |= set(got)
        assert B.stat() == step.status and B.cur() == 0, (b, B.stat(), step.status)

    base = int(_capi.lib().e2sar_hip_reas_arena(R.handle))
    seen = set()
    load(0)
    chain(torch.cuda.current_stream())                          # internal buffers exist before the capture
    torch.cuda.synchronize()
    check(0, seen)
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        chain(cap)
    for b in range(1, T.K_BATCHES):
        load(b)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(b, seen)
    assert seen == set(s.events) - s.missing
    assert int(_capi.lib().e2sar_hip_reas_arena(R.handle)) == base == R.arena_ptr
    st = _stats(R)
    assert {f: st[f] for f in OCC} == run.steps[-1].after_turn
    _end_checks(R, run, ostats, olost, _lost(R))
    R.close()


# ----------------------------------------------------------------------------------
# 3: skips change nothing


def _fed(hip, s, max_events=T.QCAP):
    """A reassembler after the stream's first batch and one collect_next of max_events."""
    R = _reas(hip)
    B = Bufs(hip, R)
    dpk, dln = _upload(hip, s.pk[:s.cuts[1]], s.ln[:s.cuts[1]])
    R.reassemble(dpk, s.stride, dln, s.cuts[1])
    R.collect_next(B.out, B.index, B.counts, B.cursor, max_events)
    return R, B


def _snapshot(hip, R, B):
    """The whole arena, the completed records (as relay_plan states them: addresses, keys,
    lengths), stats() and the cursor."""
    import torch
    from e2sar_amd import sar
    desc = torch.zeros(T.QCAP * sar.SEG_EVENT_BYTES, dtype=torch.uint8, device=hip.torch_device)
    cnt = torch.zeros(2, dtype=torch.int32, device=hip.torch_device)
    R.relay_plan(desc, cnt, 0, T.QCAP, T.max_pld(), 0, 0)
    return (R.arena_tensor().cpu().numpy().tobytes(), desc.cpu().numpy().tobytes(), cnt.cpu().tolist(), _stats(R),
            B.cur())


def test_skipped_turns_change_nothing(hip, s, models):
    step = models[T.NEVER][0].steps[0]
    done, live = len(step.delivered), step.after_batch["inProgress"]
    assert done >= 2 and live >= 1
    # (a) a record is not collected yet
    R, B = _fed(hip, s, max_events=1)
    assert B.cur() == 1 and B.cnt()[2] == done - 1
    before = _snapshot(hip, R, B)
    assert before[2][0] == done and before[3]["completedPending"] == done
    R.turn(B.cursor, B.status, max_carries=0)
    assert B.stat() == [2, 0, 0, step.after_batch["arenaUsed"]]
    assert _snapshot(hip, R, B) == before
    # (b) everything collected, every mark one above the current use
    R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
    assert B.cur() == done
    before = _snapshot(hip, R, B)
    use = step.after_batch
    R.turn(B.cursor, B.status, arena_mark=use["arenaUsed"] + 1, record_mark=done + 1, table_mark=use["tableUsed"] + 1,
           max_carries=0)
    assert B.stat() == [0, 0, 0, use["arenaUsed"]]
    assert _snapshot(hip, R, B) == before
    R.close()


@pytest.mark.parametrize("mark", ["arena_mark", "record_mark", "table_mark"])
def test_a_mark_at_the_current_value_runs_the_turn(hip, s, models, mark):
    step = models[T.NEVER][0].steps[0]
    use = {"arena_mark": step.after_batch["arenaUsed"], "record_mark": len(step.delivered),
           "table_mark": step.after_batch["tableUsed"]}[mark]
    R, B = _fed(hip, s)
    before = _snapshot(hip, R, B)
    R.turn(B.cursor, B.status, **{**FAR, mark: use + 1})
    assert B.stat() == [0, 0, 0, step.after_batch["arenaUsed"]] and _snapshot(hip, R, B) == before
    R.turn(B.cursor, B.status, **{**FAR, mark: use})
    assert B.stat() == step.status and B.cur() == 0
    st = _stats(R)
    assert {f: st[f] for f in OCC} == step.after_turn and st["errorFlags"] == 0
    R.close()


# ----------------------------------------------------------------------------------
# 4: collect_next alone

EIGHT = [1, 135, 137, 255, 256, 257, 4095, 4097]


def _eight(hip):
    """Eight events, one launch each: the record order is the launch order, on any reassembler."""
    evs = [np.random.default_rng(800 + k).integers(0, 256, n, dtype=np.uint8) for k, n in enumerate(EIGHT)]
    fr = [O.segment_event(e, 50 + k, 4321, 7, 99, 2, T.max_pld(), T.stride()) for k, e in enumerate(evs)]

    def feed(R):
        for pk, ln in fr:
            dpk, dln = _upload(hip, pk, ln)
            R.reassemble(dpk, T.stride(), dln, len(ln))
    return evs, feed


@pytest.mark.parametrize("pitch", [0, 1024])
def test_collect_next_is_collect_behind_a_cursor(hip, pitch):
    import torch
    from e2sar_amd import sar
    evs, feed = _eight(hip)
    R, twin = _reas(hip), _reas(hip)
    feed(R)
    feed(twin)
    A, W = Bufs(hip, R, max_events=3), Bufs(hip, twin, max_events=3)
    for call, first in enumerate((0, 3, 6)):
        for X in (A, W):
            X.out.fill_(SENT)
            X.index.zero_()
        R.collect_next(A.out, A.index, A.counts, A.cursor, 3, pitch)
        twin.collect(W.out, W.index, W.counts, first, 3, pitch)
        n = min(3, 8 - first)
        assert A.cur() == first + n and A.cnt() == W.cnt() and A.cnt()[0] == n
        rows = sar.parse_collect(A.index, A.counts)
        assert [int(r["eventNum"]) for r in rows] == [50 + first + i for i in range(n)]
        assert torch.equal(A.index, W.index) and torch.equal(A.out, W.out), call
        o = A.out.cpu().numpy()
        for r in rows:
            e, off = evs[int(r["eventNum"]) - 50], int(r["outOffset"])
            cp = min(len(e), pitch) if pitch else len(e)
            assert np.array_equal(o[off:off + cp], e[:cp])
            assert int(r["flags"]) == (sar._capi.COLLECT_TRUNCATED if pitch and len(e) > pitch else 0)
    # a fourth call takes nothing and writes nothing
    A.out.fill_(SENT)
    R.collect_next(A.out, A.index, A.counts, A.cursor, 3, pitch)
    assert A.cnt() == [0, 0, 0, 0] and A.cur() == 8 and bool((A.out == SENT).all())
    assert _stats(R)["completedPending"] == 8 and _stats(R)["errorFlags"] == 0
    R.close()
    twin.close()


def test_collect_next_stops_in_front_of_an_event_that_does_not_fit(hip):
    evs, feed = _eight(hip)
    R = _reas(hip)
    feed(R)
    B = Bufs(hip, R)
    room = sum(T.need(n) for n in EIGHT[:6]) + EIGHT[6] - 1          # event 6 lacks one byte of room
    R.collect_next(B.out[:room], B.index, B.counts, B.cursor, T.QCAP)
    assert B.cur() == 6 and B.cnt() == [6, sum(T.need(n) for n in EIGHT[:6]), 2, sum(EIGHT[:6])]
    assert sorted(B.delivered()) == [(50 + k, 4321) for k in range(6)]
    assert bool((B.out[sum(T.need(n) for n in EIGHT[:6]):] == SENT).all())
    # no room at all: nothing taken, the cursor stays
    from e2sar_amd import sar
    sar._call("e2sar_hip_reas_collect_next", R.handle, B.cursor.data_ptr(), T.QCAP, B.out.data_ptr(), 0, 0, 0,
              B.index.data_ptr(), B.counts.data_ptr(), sar._s(None))
    assert B.cur() == 6 and B.cnt() == [0, 0, 2, 0]
    R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
    assert B.cur() == 8 and B.cnt()[0] == 2
    assert B.delivered() == {(50 + k, 4321): (evs[k].tobytes(), O.num_packets(EIGHT[k], T.max_pld())) for k in (6, 7)}
    R.close()


# ----------------------------------------------------------------------------------
# 5: edges of the move


def _frags(ev, evnum, did=4321):
    pk, ln = O.segment_event(ev, evnum, did, 7, 99, 2, T.max_pld(), T.stride())
    return [(pk[i], int(ln[i])) for i in range(len(ln))]


def _send(hip, R, frags):
    dpk, dln = _upload(hip, np.stack([p for p, _ in frags]), np.array([n for _, n in frags], np.uint32))
    R.reassemble(dpk, T.stride(), dln, len(frags))


def test_survivors_cross_a_turn_through_a_wrapping_probe_chain(hip):
    """40 events in progress whose keys hash to the table's last eight slots: the chain wraps
    past slot 63, in the current table and again in the alternate one."""
    nums = [ev for ev in range(1, 100000) if T.slot_hash(ev, 4321, T.SLOTS - 1) >= T.SLOTS - 8][:40]
    assert len(nums) == 40 and len({T.slot_hash(ev, 4321, T.SLOTS - 1) for ev in nums}) <= 8
    evs = [np.random.default_rng(ev).integers(0, 256, 137 + k, dtype=np.uint8) for k, ev in enumerate(nums)]
    fr = [_frags(e, ev) for e, ev in zip(evs, nums)]
    R = _reas(hip)
    B = Bufs(hip, R)
    _send(hip, R, [f[0] for f in fr])
    assert _stats(R)["inProgress"] == 40
    R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
    for turn in (1, 2):                                        # the second from a table a turn filled
        R.turn(B.cursor, B.status, max_carries=2)
        assert B.stat() == [1, 40, 0, sum(T.need(len(e)) for e in evs)], turn
    st = _stats(R)
    assert st["tableUsed"] == st["inProgress"] == 40 and st["errorFlags"] == 0
    _send(hip, R, [f[1] for f in fr])
    R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
    assert B.delivered() == {(ev, 4321): (e.tobytes(), 2) for e, ev in zip(evs, nums)}
    R.turn(B.cursor, B.status, max_carries=2)
    assert B.stat() == [1, 0, 0, 0]
    st = _stats(R)
    assert st["eventSuccess"] == 40 and st["reassemblyLoss"] == 0 and st["tableUsed"] == 0 and st["errorFlags"] == 0
    R.close()


def test_a_survivor_without_a_buffer(hip):
    """Six events of 9999 bytes leave 4096 bytes of the arena: an event of 4097 bytes created
    then has no buffer.  It is carried as such, completes as an enqueue loss and sets error
    bit 1 and no other."""
    big = [np.random.default_rng(900 + k).integers(0, 256, 9999, dtype=np.uint8) for k in range(6)]
    odd = np.random.default_rng(990).integers(0, 256, 4097, dtype=np.uint8)
    fb, fo = [_frags(e, 10 + k) for k, e in enumerate(big)], _frags(odd, 77)
    R = _reas(hip)
    B = Bufs(hip, R)
    _send(hip, R, [f[0] for f in fb])
    _send(hip, R, fo[:1])                                      # created last: the arena is full
    st = _stats(R)
    assert st["errorFlags"] == 2 and st["inProgress"] == 7 and st["arenaUsed"] == 6 * 10240 + 4352
    R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
    R.turn(B.cursor, B.status)
    assert B.stat() == [1, 7, 0, 6 * 10240]
    st = _stats(R)
    assert st["tableUsed"] == st["inProgress"] == 7 and st["arenaUsed"] == 6 * 10240 and st["errorFlags"] == 2
    _send(hip, R, [f for fr in fb for f in fr[1:]] + fo[1:])
    R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
    assert B.delivered() == {(10 + k, 4321): (e.tobytes(), len(fb[k])) for k, e in enumerate(big)}
    assert _lost(R) == [(77, 4321, len(fo), 1)]
    st = _stats(R)
    assert st["eventSuccess"] == 7 and st["enqueueLoss"] == 1 and st["reassemblyLoss"] == 0 and st["inProgress"] == 0
    assert st["errorFlags"] == 2
    R.close()


def test_survivors_with_one_fragment_and_with_all_but_the_last_byte(hip):
    first = np.random.default_rng(41).integers(0, 256, 9999, dtype=np.uint8)
    last = np.random.default_rng(42).integers(0, 256, 30 * T.max_pld() + 1, dtype=np.uint8)
    ff, fl = _frags(first, 5), _frags(last, 6, 1)
    assert fl[-1][1] == 36 + 1
    R = _reas(hip)
    B = Bufs(hip, R)
    _send(hip, R, ff[:1] + fl[:-1])
    R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
    R.turn(B.cursor, B.status, max_carries=1)
    assert B.stat() == [1, 2, 0, T.need(len(first)) + T.need(len(last))]
    _send(hip, R, fl[-1:] + ff[1:])
    R.collect_next(B.out, B.index, B.counts, B.cursor, T.QCAP)
    assert B.delivered() == {(5, 4321): (first.tobytes(), len(ff)), (6, 1): (last.tobytes(), len(fl))}
    st = _stats(R)
    assert st["eventSuccess"] == 2 and st["inProgress"] == 0 and st["errorFlags"] == 0
    R.close()


# ----------------------------------------------------------------------------------
# 6: statuses


def _code(call):
    from e2sar_amd._capi import E2SARHipError
    with pytest.raises(E2SARHipError) as e:
        call()
    return e.value.code


def test_statuses_and_a_failing_call_launches_nothing(hip, s):
    from e2sar_amd import _capi
    L = _capi.lib()
    R, B = _fed(hip, s, max_events=1)
    before = _stats(R)
    cur = B.cur()
    ok = _capi.TurnMarks(0, 0, 0, 0, 0)
    bad = _capi.TurnMarks(0, 0, 0, 0, 1)
    h, c, st, stream = R.handle, B.cursor.data_ptr(), B.status.data_ptr(), None
    turn = lambda *a: _capi.check(L.e2sar_hip_reas_turn(*a))
    for args in [(None, c, C.byref(ok), st, stream), (h, None, C.byref(ok), st, stream), (h, c, None, st, stream),
                 (h, c, C.byref(ok), None, stream), (h, c, C.byref(bad), st, stream)]:
        assert _code(lambda: turn(*args)) == _capi.ERR_PARAMETER
        assert _stats(R) == before and B.cur() == cur
    nxt = lambda *a: _capi.check(L.e2sar_hip_reas_collect_next(*a))
    o, i, n = B.out.data_ptr(), B.index.data_ptr(), B.counts.data_ptr()
    for args in [(None, c, 4, o, 4096, 0, 0, i, n, stream), (h, None, 4, o, 4096, 0, 0, i, n, stream),
                 (h, c, 0, o, 4096, 0, 0, i, n, stream), (h, c, 4, o + 16, 4096, 0, 0, i, n, stream),
                 (h, c, 4, o, 4096, 24, 0, i, n, stream), (h, c, 4, o, 4096, 0, 48, i, n, stream)]:
        assert _code(lambda: nxt(*args)) == _capi.ERR_PARAMETER
        assert _stats(R) == before and B.cur() == cur
    R.close()
    # LOGIC: no alternate table; reference-order mode
    for kw in (dict(compactable=False), dict(flags=_capi.REAS_REFERENCE_ORDER)):
        Q = _reas(hip, **kw)
        Bq = Bufs(hip, Q)
        dpk, dln = _upload(hip, s.pk[:s.cuts[1]], s.ln[:s.cuts[1]])
        Q.reassemble(dpk, s.stride, dln, s.cuts[1])
        before = _stats(Q)
        assert _code(lambda: Q.turn(Bq.cursor, Bq.status)) == _capi.ERR_LOGIC
        assert _stats(Q) == before and Bq.stat() == [-1] * 4
        Q.close()
