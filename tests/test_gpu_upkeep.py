"""The reassembler's upkeep path against the oracle: GC, compaction, recycle, partial polls,
ring overflow, reset_stats and the relay plan -- what keeps a long-running reassembler alive
(reas_upkeep.hpp, recycle_slots in reas_table.hpp, the poll / recycle / compact / reset
entry points of capi.cpp).

A schedule (tests/upkeep_schedule.py) is applied to a DeviceReassembler and to the oracle;
at every poll, lost_poll and stats step the two must agree bit-exactly: event bytes,
numFragments, keys, lost records, every counter.  tests/test_upkeep_schedule_cpu.py shows on
the oracle alone that the schedules reach the states these tests are about.

Lost-event de-duplication (hpp:262-279) is the host's job when it drains the lost records
(DESIGN.md 5.3): the device logs every collection, the oracle a key's first one only.  The
schedules therefore let no key be collected twice (Trace.twice); the one case that is about
a second collection takes its expectation from an oracle that saw only the second item.
"""
import ctypes as C
import os
import random

import numpy as np
import pytest

import oracle_ffi as O
import upkeep_schedule as U
from test_gpu_golden import STATS
from test_gpu_parity import _pipelined

pytestmark = pytest.mark.gpu

MP = 16                       # payload bytes at MTU 80
STRIDE = 64
FORMS = ["fused", "split", "pipelined"]
HISTORY = ("eventSuccess", "totalPackets", "totalBytes", "badHeaderDiscards", "dataErrCnt", "enqueueLoss",
           "reassemblyLoss")
STATE = ("inProgress", "tableUsed", "arenaUsed", "completedPending", "lostPending")


def _ro():
    from e2sar_amd import _capi
    return _capi.REAS_REFERENCE_ORDER


def _reas(hip, flags=0, slots=64, arena=4 << 20, qcap=4096, lcap=4096):
    from e2sar_amd import sar
    return sar.DeviceReassembler(hip, with_lb_header=True, table_slots=slots, queue_capacity=qcap, lost_capacity=lcap,
                                 arena_bytes=arena, compactable=True, flags=flags)


def _upload(hip, pk, ln):
    import torch
    dpk = torch.from_numpy(np.ascontiguousarray(pk).reshape(-1)).to(hip.torch_device)
    dln = torch.from_numpy(np.ascontiguousarray(ln, np.uint32).view(np.int32).copy()).to(hip.torch_device)
    return dpk, dln


def _launch(R, dpk, dln, stride, a, b, now, form):
    if b <= a:
        return
    if form == "fused":
        R.reassemble(dpk[a * stride:], stride, dln[a:], b - a, now_ms=now)
    elif form == "split":
        w = R.alloc_work(b - a)
        R.classify(dpk[a * stride:], stride, dln[a:], b - a, w, now_ms=now)
        R.scatter(dpk[a * stride:], stride, b - a, w)
    else:
        # the batch in up to three parts, scatter of part k beside classify of part k + 1; the
        # chain ends before the next upkeep step (a classified part holds arena addresses)
        cuts = sorted({a, a + (b - a) // 3, a + 2 * (b - a) // 3, b})
        _pipelined(R, dpk, dln, stride, list(zip(cuts[:-1], cuts[1:])), now)


def _poll_calls(R, cap, lost=False):
    """Drain through the C entry point, `cap` records per call (0: the ring's capacity, one
    call); one list of records per call that returned any."""
    from e2sar_amd import _capi
    if cap == 0:
        recs = R.lost_poll() if lost else R.poll()
        return [recs] if recs else []
    typ = _capi.LostRec if lost else _capi.EventRec
    fn = _capi.lib().e2sar_hip_reas_lost_poll if lost else _capi.lib().e2sar_hip_reas_poll
    calls = []
    while True:
        buf = (typ * cap)()
        n = C.c_uint32(12345)
        _capi.check(fn(R.handle, buf, cap, C.byref(n)))
        assert n.value <= cap
        if n.value == 0:
            return calls
        calls.append([typ.from_buffer_copy(bytes(buf[k])) for k in range(n.value)])


def _events(R, cap=0):
    """Drain the completed events: [(key, bytes, numFragments)], bytes read before anything
    can move them."""
    return [((r.eventNum, r.dataId), R.event_bytes(r), r.numFragments) for call in _poll_calls(R, cap) for r in call]


def _lost(R, cap=0):
    return [(r.eventNum, r.dataId, r.numFragments, r.enqueueLoss) for call in _poll_calls(R, cap, lost=True)
            for r in call]


def _stats(R):
    st = R.stats()
    return {f: int(getattr(st, f)) for f in HISTORY + STATE + ("errorFlags",)}


def _compact(R, bases):
    """Compact; the arena base alternates between exactly two addresses."""
    from e2sar_amd import _capi
    R.compact()
    base = int(_capi.lib().e2sar_hip_reas_arena(R.handle))
    assert base == R.arena_ptr
    if len(bases) == 1:
        assert base != bases[0]
    else:
        assert base == bases[len(bases) % 2]
    bases.append(base)


def _run(hip, s, form, flags=0, R=None, **kw):
    """Apply schedule s to a device reassembler and to the oracle, step by step."""
    R = R or _reas(hip, flags, **kw)
    ref, T = U.replay_oracle(s), U.trace(s)
    assert not T.twice
    live = iter(T.live)
    dpk, dln = _upload(hip, s.pk, s.ln)
    bases = [R.arena_ptr]
    for k, (st, want) in enumerate(zip(s.steps, ref)):
        if st[0] == "batch":
            _launch(R, dpk, dln, s.stride, st[1], st[2], st[3], form)
        elif st[0] == "poll":
            assert sorted(_events(R, st[1])) == sorted(want), (k, form)
        elif st[0] == "lost_poll":
            assert sorted(_lost(R, st[1])) == sorted(r + (0,) for r in want), (k, form)
        elif st[0] == "gc":
            R.gc(st[1], st[2])
        elif st[0] == "stats":
            got = _stats(R)
            assert {f: got[f] for f in STATS} == {f: int(want[f]) for f in STATS}, (k, form)
            assert got["errorFlags"] == 0
        else:
            _compact(R, bases)
            got = _stats(R)
            assert got["tableUsed"] == got["inProgress"] == want, (k, form, got)
            assert got["arenaUsed"] == U.arena_need(next(live)), (k, form)
            assert got["errorFlags"] == 0
    return R, ref


# ----------------------------------------------------------------------------------
# a, b: lifecycles


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("seed", range(3))
def test_lifecycle_default_mode(hip, seed, form):
    """Clean schedules: partial polls, compaction after every batch (twice back to back after
    the odd ones, into the table just left), GC and partial lost polls between batches."""
    _run(hip, U.clean_schedule(seed), form)[0].close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("E2SAR_RANDOM_SEEDS", "12"))))
def test_lifecycle_reference_order(hip, seed):
    """Dirty schedules: a reference-order item's state lives only in its slot (bufOff, bytes,
    acc, created, bvalid) and crosses a compaction after every batch, then a GC."""
    _run(hip, U.dirty_schedule(seed), FORMS[seed % 3], flags=_ro())[0].close()


# ----------------------------------------------------------------------------------
# hand-built schedules at MTU 80


def _frags(ev, evnum, did=4321):
    pk, ln = O.segment_event(ev, evnum, did, 7, 99, 2, MP, STRIDE)
    return [(pk[i], int(ln[i])) for i in range(len(ln))]


def _bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _schedule(steps):
    """steps with ("batch", [fragments], now) -> Schedule"""
    out, conv = [], []
    for st in steps:
        if st[0] == "batch":
            conv.append(("batch", len(out), len(out) + len(st[1]), st[2]))
            out += st[1]
        else:
            conv.append(st)
    return U.Schedule(np.stack([p for p, _ in out]), np.array([L for _, L in out], np.uint32), STRIDE, conv)


# c
@pytest.mark.parametrize("slots,nev", [(64, 48), (32768, 5)])
def test_compaction_under_collisions(hip, slots, nev):
    """48 live events re-inserted into a 64-slot table three times in a row (every compaction
    block probes past slots other blocks claimed), then again between the two batches that
    finish them; 5 events in 32768 slots: nearly every block leaves at once."""
    per = O.num_packets(3000, MP)
    assert per == 188
    evs = [_bytes(9100 + k, 3000) for k in range(nev)]
    fr = [_frags(e, k) for k, e in enumerate(evs)]
    held = [1 + k * 186 // (nev - 1) for k in range(nev)]              # 1 .. 187, one count per event
    assert len(set(held)) == nev and held[0] == 1 and held[-1] == 187
    rnd = random.Random(9)
    early = [f for k in range(nev) for f in fr[k][1:per - held[k]]]
    rnd.shuffle(early)
    late = [f for k in range(nev) for f in fr[k][per - held[k]:]]
    rnd.shuffle(late)
    cut = len(late) // 2
    s = _schedule([("batch", [fr[k][0] for k in range(nev)] + early, 0), ("poll", 0), ("stats",),
                   ("compact",), ("compact",), ("compact",), ("stats",),
                   ("batch", late[:cut], 0), ("poll", 0), ("compact",),
                   ("batch", late[cut:], 0), ("poll", 0), ("stats",)])
    R, ref = _run(hip, s, "fused", slots=slots, arena=1 << 20)
    done = [ev for st, r in zip(s.steps, ref) if st[0] == "poll" for ev in r]
    assert sorted(done) == sorted(((k, 4321), evs[k].tobytes(), per) for k in range(nev))
    assert ref[-1]["eventSuccess"] == nev and ref[-1]["inProgress"] == 0
    R.close()


# d
EDGE_LENGTHS = [17, 31, 32, 33, 255, 256, 257, 4095, 4097, 65537]


def test_compaction_copy_edges(hip):
    """reas_compact_kernel's 16-byte loop and byte tail at lengths around 16, 256 and 4096:
    every byte of the live buffers moves (the received part and the not yet written rest,
    which holds a known fill), and nothing lands outside them."""
    import torch
    from e2sar_amd import _capi
    R = _reas(hip, arena=1 << 18)
    rng = np.random.default_rng(404)
    fill = rng.integers(0, 256, R.arena_bytes, dtype=np.uint8)
    first = R.arena_ptr
    R.arena_tensor().copy_(torch.from_numpy(fill).to(hip.torch_device))
    evs = [_bytes(4000 + n, n) for n in EDGE_LENGTHS]
    fr = [_frags(e, k) for k, e in enumerate(evs)]
    pk = np.stack([p for f in fr for p, _ in f])
    ln = np.array([L for f in fr for _, L in f], np.uint32)
    dpk, dln = _upload(hip, pk, ln)
    at = np.cumsum([0] + [len(f) for f in fr])
    old = []                       # arena offsets in creation order: one launch per event
    for k, f in enumerate(fr):
        old.append(U.arena_need(EDGE_LENGTHS[:k]))
        _launch(R, dpk, dln, STRIDE, int(at[k]), int(at[k + 1]) - 1, 100, "fused")     # all but the last
    st = _stats(R)
    assert st["inProgress"] == len(evs) and st["arenaUsed"] == U.arena_need(EDGE_LENGTHS) and st["errorFlags"] == 0
    bases = [first]
    _compact(R, bases)
    # the first arena is free now: mark all of it, then compact back into it
    _capi.check(_capi.lib().e2sar_hip_memset_d(hip.handle, C.c_void_p(first), 0xA5, R.arena_bytes))
    _compact(R, bases)
    assert R.arena_ptr == first
    st = _stats(R)
    assert st["tableUsed"] == st["inProgress"] == len(evs) and st["arenaUsed"] == U.arena_need(EDGE_LENGTHS)
    used = st["arenaUsed"]
    # (the issue's form of the check: the unused part, refilled right after the compaction)
    _capi.check(_capi.lib().e2sar_hip_memset_d(hip.handle, C.c_void_p(first + used), 0x5A, R.arena_bytes - used))
    moved = R.arena_tensor().cpu().numpy().copy()
    for k in range(len(evs)):
        _launch(R, dpk, dln, STRIDE, int(at[k + 1]) - 1, int(at[k + 1]), 200, "fused")
    recs = [r for call in _poll_calls(R, 0) for r in call]
    after = R.arena_tensor().cpu().numpy()
    assert sorted(r.eventNum for r in recs) == list(range(len(evs)))
    outside = np.ones(R.arena_bytes, bool)
    for r in recs:
        k, n, off = r.eventNum, EDGE_LENGTHS[r.eventNum], r.arenaOffset
        assert r.bytes == n and r.numFragments == len(fr[k]) and off % 256 == 0 and off + n <= used
        got = n - (int(ln[at[k + 1] - 1]) - 36)                    # bytes received before the compactions
        assert np.array_equal(moved[off:off + got], evs[k][:got]), n
        assert np.array_equal(moved[off + got:off + n], fill[old[k] + got:old[k] + n]), n
        assert np.array_equal(after[off:off + n], evs[k]), n
        outside[off:off + n] = False
    # between an event's end and the next 256-aligned start, and past the last buffer: what
    # the test wrote there, before the second batch and after it
    want = np.where(np.arange(R.arena_bytes) < used, 0xA5, 0x5A).astype(np.uint8)
    assert np.array_equal(moved[outside], want[outside])
    assert np.array_equal(after[outside], want[outside])
    assert _stats(R)["errorFlags"] == 0
    R.close()


# e
def _gc_log(s, ref):
    """What the oracle collected at every GC and handed out at every lost poll, in step order."""
    return [sorted(r) if st[0] == "lost_poll" else r for st, r in zip(s.steps, ref) if st[0] in ("gc", "lost_poll")]


@pytest.mark.parametrize("mode", ["default", "reference_order"])
def test_created_and_acc_survive_a_compaction(hip, mode):
    flags = _ro() if mode == "reference_order" else 0
    a = [_frags(_bytes(50 + k, 400), 10 + k)[:3 + k] for k in range(3)]          # 3, 4, 5 fragments
    b = [_frags(_bytes(60 + k, 400), 20 + k)[:7 + k] for k in range(3)]          # 7, 8, 9 fragments
    A = sorted((10 + k, 4321, 3 + k) for k in range(3))
    B = sorted((20 + k, 4321, 7 + k) for k in range(3))
    flat = lambda c: [f for ev in c for f in ev]
    # the issue's case: two cohorts, one compaction, one GC that is between their ages
    s = _schedule([("batch", flat(a), 100), ("batch", flat(b), 400), ("poll", 0), ("compact",),
                   ("gc", 700, 500), ("lost_poll", 0), ("stats",),
                   ("gc", 700, 500), ("lost_poll", 0), ("stats",)])
    R, ref = _run(hip, s, "fused", flags)
    assert _gc_log(s, ref) == [3, A, 0, []]
    R.close()
    # the boundary, a strict > on now - created (cpp:262), before and after a compaction
    c = [_frags(_bytes(70, 400), 30)[:2]]
    s = _schedule([("batch", flat(a), 100), ("batch", flat(b), 400),
                   ("gc", 600, 500), ("lost_poll", 0), ("poll", 0), ("compact",),
                   ("gc", 600, 500), ("lost_poll", 0), ("gc", 601, 500), ("lost_poll", 0), ("stats",),
                   ("gc", 601, 500), ("lost_poll", 0),
                   ("gc", 900, 500), ("lost_poll", 0), ("gc", 901, 500), ("lost_poll", 0), ("stats",),
                   ("batch", flat(c), 1000),                         # created in the table in use: no move before its GC
                   ("gc", 1500, 500), ("lost_poll", 0), ("gc", 1501, 500), ("lost_poll", 0), ("stats",)])
    R, ref = _run(hip, s, "fused", flags)
    assert _gc_log(s, ref) == [0, [], 0, [], 3, A, 0, [], 0, [], 3, B, 0, [], 1, [(30, 4321, 2)]]
    R.close()


# f
@pytest.mark.parametrize("mode", ["default", "reference_order"])
def test_fragments_after_gc_start_a_new_item(hip, mode):
    flags = _ro() if mode == "reference_order" else 0
    ev, other = _bytes(81, 160), _bytes(82, 100)
    fr, fo = _frags(ev, 77), _frags(other, 78)                # 10 and 7 fragments
    s = _schedule([("batch", fr[:4] + fo[:3], 100), ("gc", 400, 250), ("lost_poll", 0), ("stats",),
                   ("batch", fr[4:9] + fo[3:], 500), ("poll", 0), ("stats",), ("compact",), ("stats",)])
    R, ref = _run(hip, s, "fused", flags)
    # both items were collected with 4 and 3 fragments; the rest of each starts a new item:
    # event 78's never completes (4 of 7 fragments), like event 77's (5 of 10)
    assert sorted(ref[2]) == [(77, 4321, 4), (78, 4321, 3)] and ref[5] == [] and ref[-1]["inProgress"] == 2
    # the second collection.  The reference logs a key's loss once (hpp:262-279), so the
    # oracle that saw the first collection stays silent here, while the device leaves that
    # de-duplication to the host.  The expectation comes from an oracle that
    # sees what the device's table holds after the first GC: the second batch alone.
    fresh = O.Reassembler(True, 0)
    fresh.set_time(500)
    a, b = s.steps[4][1:3]
    fresh.push_batch(s.pk[a:b], s.ln[a:b])
    fresh.set_time(800)
    assert fresh.gc(250) == 2
    want = sorted(fresh.lost_pop_all())
    assert want == [(77, 4321, 5), (78, 4321, 4)]
    R.gc(800, 250)
    assert sorted(_lost(R)) == [w + (0,) for w in want]
    st = _stats(R)
    assert st["reassemblyLoss"] == 4 and st["inProgress"] == 0 == fresh.stats()["inProgress"]
    assert st["eventSuccess"] == 0 and st["errorFlags"] == 0
    R.close()


# g
@pytest.mark.parametrize("mode", ["default", "reference_order"])
def test_event_without_a_buffer_crosses_a_compaction(hip, mode):
    """An arena too small for the last event: its item has no buffer (bufOff == kNoBuf, error
    bit 1), stays in progress through a compaction and completes as an enqueue loss."""
    flags = _ro() if mode == "reference_order" else 0
    evs = [_bytes(90 + k, 1000) for k in range(4)]
    fr = [_frags(e, k) for k, e in enumerate(evs)]            # 63 fragments each
    R = _reas(hip, flags, arena=3 * 1024 + 512)
    pk = np.stack([p for f in fr for p, _ in f])
    ln = np.array([L for f in fr for _, L in f], np.uint32)
    dpk, dln = _upload(hip, pk, ln)
    ref = O.Reassembler(True, 0)
    for k in range(4):                                        # one launch per event: event 3 is created last
        _launch(R, dpk, dln, STRIDE, 63 * k, 63 * k + 62, 100, "fused")
        ref.push_batch(pk[63 * k:63 * k + 62], ln[63 * k:63 * k + 62])
    st = _stats(R)
    assert st["errorFlags"] == 2 and st["inProgress"] == 4 and st["tableUsed"] == 4
    _compact(R, [R.arena_ptr])
    st = _stats(R)
    assert st["tableUsed"] == st["inProgress"] == 4 and st["arenaUsed"] == 3 * 1024 and st["errorFlags"] == 2
    last = [63 * k + 62 for k in range(4)]
    dl, dn = _upload(hip, pk[last], ln[last])
    _launch(R, dl, dn, STRIDE, 0, 4, 200, "fused")
    ref.push_batch(pk[last], ln[last])
    assert sorted(_events(R)) == sorted(((e, d), b, nf) for b, e, d, nf in ref.pop_all_frags(1 << 16)
                                        if e != 3)
    assert _lost(R) == [(3, 4321, 63, 1)]
    st, rst = _stats(R), ref.stats()
    assert rst["eventSuccess"] == 4 and rst["enqueueLoss"] == 0
    # the oracle has no arena to run out of: its enqueueLoss + 1, everything else equal
    assert {f: st[f] for f in STATS} == {f: int(rst[f]) + (f == "enqueueLoss") for f in STATS}
    assert st["completedPending"] == 0 and st["lostPending"] == 0
    R.close()


# h
def _raises_logic(call):
    from e2sar_amd._capi import ERR_LOGIC, E2SARHipError
    with pytest.raises(E2SARHipError) as e:
        call()
    assert e.value.code == ERR_LOGIC


def test_compact_and_recycle_contracts(hip):
    from e2sar_amd import _capi
    evs = [_bytes(120 + k, 100 + 16 * k) for k in range(4)]
    fr = [_frags(e, k) for k, e in enumerate(evs)]
    R = _reas(hip)
    # events 0, 1 complete (unpolled), 2 in progress, 3 collected (one lost record pending)
    s1 = fr[0] + fr[1] + fr[2][:3]
    pk = np.stack([p for p, _ in s1 + fr[3][:2] + fr[2][3:]])
    ln = np.array([L for _, L in s1 + fr[3][:2] + fr[2][3:]], np.uint32)
    dpk, dln = _upload(hip, pk, ln)
    n1 = len(s1)
    _launch(R, dpk, dln, STRIDE, n1, n1 + 2, 0, "fused")
    R.gc(1000, 500)
    _launch(R, dpk, dln, STRIDE, 0, n1, 1000, "fused")
    before, base = _stats(R), R.arena_ptr
    assert before["completedPending"] == 2 and before["inProgress"] == 1 and before["lostPending"] == 1
    # compact / recycle(force=0) with unpolled records: LOGIC, nothing changes
    _raises_logic(R.compact)
    _raises_logic(lambda: R.recycle(force=False))
    assert int(_capi.lib().e2sar_hip_reas_arena(R.handle)) == base and _stats(R) == before
    assert sorted(_events(R)) == [((k, 4321), evs[k].tobytes(), len(fr[k])) for k in range(2)]
    # recycle(force=0) with an item in progress: LOGIC likewise
    polled = _stats(R)
    assert polled == {**before, "completedPending": 0}
    _raises_logic(lambda: R.recycle(force=False))
    assert _stats(R) == polled
    # event 2 completes and stays unpolled, event 3's rest starts an item: force drops both
    _launch(R, dpk, dln, STRIDE, n1 + 2, len(ln), 1000, "fused")
    _launch(R, dpk, dln, STRIDE, n1, n1 + 1, 1000, "fused")
    full = _stats(R)
    assert full["completedPending"] == 1 and full["inProgress"] == 1 and full["lostPending"] == 1
    R.recycle(force=True)
    after = _stats(R)
    assert {f: after[f] for f in ("inProgress", "tableUsed", "arenaUsed", "completedPending")} == \
        {"inProgress": 0, "tableUsed": 0, "arenaUsed": 0, "completedPending": 0}
    assert {f: after[f] for f in HISTORY + ("lostPending", "errorFlags")} == \
        {f: full[f] for f in HISTORY + ("lostPending", "errorFlags")}          # no lost record written
    assert _poll_calls(R, 0) == []
    assert _lost(R) == [(3, 4321, 2, 0)]
    # the same keys again reassemble from scratch
    every = [f for k in range(4) for f in fr[k]]
    dpk, dln = _upload(hip, np.stack([p for p, _ in every]), np.array([L for _, L in every], np.uint32))
    _launch(R, dpk, dln, STRIDE, 0, len(every), 2000, "fused")
    assert sorted(_events(R)) == [((k, 4321), evs[k].tobytes(), len(fr[k])) for k in range(4)]
    st = _stats(R)
    assert st["inProgress"] == 0 and st["tableUsed"] == 4 and st["eventSuccess"] == full["eventSuccess"] + 4
    R.recycle(force=False)                                  # drained: legal
    R.close()


# i
@pytest.mark.parametrize("cap", [1, 3, 7])
def test_partial_polls(hip, cap):
    """Polls with a cap below what is queued: the records that stay are moved down the ring
    (slide_down's chunked device-to-device copies); none is lost, repeated or reordered."""
    from e2sar_amd import _capi
    L = _capi.lib()
    evs = [_bytes(200 + k, 40 + k) for k in range(20)]             # 3 to 4 fragments each
    fr = [_frags(e, k) for k, e in enumerate(evs)]
    every = [f for f_ in fr for f in f_]
    dpk, dln = _upload(hip, np.stack([p for p, _ in every]), np.array([L_ for _, L_ in every], np.uint32))
    n12 = sum(len(f) for f in fr[:12])
    R = _reas(hip)
    _launch(R, dpk, dln, STRIDE, 0, n12, 0, "fused")
    assert _stats(R)["completedPending"] == 12
    _launch(R, dpk, dln, STRIDE, n12, len(every), 0, "fused")
    n = C.c_uint32(99)
    _capi.check(L.e2sar_hip_reas_poll(R.handle, None, 0, C.byref(n)))
    assert n.value == 0 and _stats(R)["completedPending"] == 20
    got, left = [], 20
    while left:
        buf = (_capi.EventRec * cap)()
        _capi.check(L.e2sar_hip_reas_poll(R.handle, buf, cap, C.byref(n)))
        assert n.value == min(cap, left)
        left -= n.value
        assert _stats(R)["completedPending"] == left
        got += [((buf[k].eventNum, buf[k].dataId), R.event_bytes(buf[k]), buf[k].numFragments) for k in range(n.value)]
    _capi.check(L.e2sar_hip_reas_poll(R.handle, buf, cap, C.byref(n)))
    assert n.value == 0
    assert sorted(got) == [((k, 4321), evs[k].tobytes(), len(fr[k])) for k in range(20)]
    assert sorted(k[0] for k, _, _ in got[:12]) == list(range(12))          # first batch first
    # the lost ring: 6 items collected by one GC, 4 by a later one
    firsts = np.cumsum([0] + [len(f) for f in fr])[:10]
    for k, a in enumerate(firsts):                                           # two fragments of events 0 .. 9
        _launch(R, dpk, dln, STRIDE, int(a), int(a) + 2, 100 if k < 6 else 200, "fused")
    R.gc(400, 250)
    assert _stats(R)["lostPending"] == 6
    R.gc(1000, 250)
    _capi.check(L.e2sar_hip_reas_lost_poll(R.handle, None, 0, C.byref(n)))
    assert n.value == 0 and _stats(R)["lostPending"] == 10
    lost, left = [], 10
    while left:
        lb = (_capi.LostRec * cap)()
        _capi.check(L.e2sar_hip_reas_lost_poll(R.handle, lb, cap, C.byref(n)))
        assert n.value == min(cap, left)
        left -= n.value
        assert _stats(R)["lostPending"] == left
        lost += [(lb[k].eventNum, lb[k].dataId, lb[k].numFragments, lb[k].enqueueLoss) for k in range(n.value)]
    assert sorted(lost) == [(k, 4321, 2, 0) for k in range(10)]
    assert sorted(r[0] for r in lost[:6]) == list(range(6))
    st = _stats(R)
    assert st["reassemblyLoss"] == 10 and st["inProgress"] == 0 and st["errorFlags"] == 0
    R.close()


# j
def test_completed_ring_overflow(hip):
    evs = [_bytes(300 + k, 40 + k) for k in range(20)]
    fr = [_frags(e, k) for k, e in enumerate(evs)]
    every = [f for f_ in fr for f in f_]
    pk, ln = np.stack([p for p, _ in every]), np.array([L for _, L in every], np.uint32)
    dpk, dln = _upload(hip, pk, ln)
    n12 = sum(len(f) for f in fr[:12])
    R = _reas(hip, qcap=8)
    ref = O.Reassembler(True, 8)
    _launch(R, dpk, dln, STRIDE, 0, n12, 0, "fused")
    ref.push_batch(pk[:n12], ln[:n12])
    st, rst = _stats(R), ref.stats()
    assert rst["eventSuccess"] == 12 and rst["enqueueLoss"] == 4
    assert {f: st[f] for f in STATS} == {f: int(rst[f]) for f in STATS}
    assert st["completedPending"] == 8 and st["lostPending"] == 4
    got, lost = _events(R), _lost(R)
    # which 8 of the 12 fit is the device's completion order: every event is
    # in exactly one of the two lists, whole
    assert len(got) == 8 and len(lost) == 4
    assert sorted([k[0] for k, _, _ in got] + [r[0] for r in lost]) == list(range(12))
    assert all(b == evs[k[0]].tobytes() and nf == len(fr[k[0]]) and k[1] == 4321 for k, b, nf in got)
    assert all(r == (r[0], 4321, len(fr[r[0]]), 1) for r in lost)
    assert len(ref.pop_all()) == 8 and len(ref.lost_pop_all()) == 4
    # drained: the ring takes 8 more
    _launch(R, dpk, dln, STRIDE, n12, len(ln), 0, "fused")
    ref.push_batch(pk[n12:], ln[n12:])
    st, rst = _stats(R), ref.stats()
    assert rst["eventSuccess"] == 20 and rst["enqueueLoss"] == 4
    assert {f: st[f] for f in STATS} == {f: int(rst[f]) for f in STATS}
    assert sorted(_events(R)) == [((k, 4321), evs[k].tobytes(), len(fr[k])) for k in range(12, 20)]
    assert _lost(R) == [] and _stats(R)["errorFlags"] == 0
    R.close()


def test_lost_ring_overflow(hip):
    fr = [_frags(_bytes(400 + k, 100), k)[:1 + k % 5] for k in range(11)]
    every = [f for f_ in fr for f in f_]
    pk, ln = np.stack([p for p, _ in every]), np.array([L for _, L in every], np.uint32)
    dpk, dln = _upload(hip, pk, ln)
    n10 = sum(len(f) for f in fr[:10])
    R = _reas(hip, lcap=4)
    ref = O.Reassembler(True, 0)
    _launch(R, dpk, dln, STRIDE, 0, n10, 100, "fused")
    ref.set_time(100)
    ref.push_batch(pk[:n10], ln[:n10])
    R.gc(1000, 500)
    ref.set_time(1000)
    assert ref.gc(500) == 10
    st, rst = _stats(R), ref.stats()
    assert rst["reassemblyLoss"] == 10
    assert {f: st[f] for f in STATS} == {f: int(rst[f]) for f in STATS}
    assert st["lostPending"] == 4
    got, want = _lost(R), ref.lost_pop_all()
    assert len(want) == 10 and len(got) == len(set(got)) == 4
    assert set(got) <= {w + (0,) for w in want}
    assert _stats(R)["lostPending"] == 0
    # drained: a later loss is recorded again
    _launch(R, dpk, dln, STRIDE, n10, len(ln), 2000, "fused")
    ref.set_time(2000)
    ref.push_batch(pk[n10:], ln[n10:])
    R.gc(3000, 500)
    ref.set_time(3000)
    assert ref.gc(500) == 1
    assert _lost(R) == [w + (0,) for w in ref.lost_pop_all()] == [(10, 4321, 1, 0)]
    st, rst = _stats(R), ref.stats()
    assert {f: st[f] for f in STATS} == {f: int(rst[f]) for f in STATS} and st["errorFlags"] == 0
    R.close()


# k
def test_reset_stats_zeroes_history_and_keeps_state(hip):
    evs = [_bytes(500 + k, 200) for k in range(6)]
    fr = [_frags(e, k) for k, e in enumerate(evs)]             # 13 fragments each
    bad = fr[0][0][0].copy()
    bad[16] = 0x20                                            # RE version 2: badHeaderDiscards
    over = np.zeros(STRIDE, np.uint8)
    over[:36] = np.frombuffer(O.lbre_hdr(2, 7, 99, 4321, 100, 50, 999), np.uint8)   # offset + 16 > 50: dataErrCnt
    s1 = fr[0] + fr[1] + [f for k in (2, 3, 4) for f in fr[k][:5]] + [(bad, 52), (over, 52)]
    s2 = fr[5][:2]
    s3 = [f for k in (2, 3, 4) for f in fr[k][5:]]
    pk = np.stack([p for p, _ in s1 + s2 + s3])
    ln = np.array([L for _, L in s1 + s2 + s3], np.uint32)
    dpk, dln = _upload(hip, pk, ln)
    # five buffers fill the arena; event 5, created last at an earlier clock, gets none (error
    # bit 1) and is the one the GC collects
    R = _reas(hip, arena=5 * 256)
    _launch(R, dpk, dln, STRIDE, 0, len(s1), 500, "fused")
    _launch(R, dpk, dln, STRIDE, len(s1), len(s1) + 2, 100, "fused")
    R.gc(500, 250)
    before = _stats(R)
    assert {f: before[f] for f in STATE} == {"inProgress": 3, "tableUsed": 6, "arenaUsed": 6 * 256,
                                             "completedPending": 2, "lostPending": 1}
    assert before["errorFlags"] == 2
    assert all(before[f] > 0 for f in HISTORY if f != "enqueueLoss"), before
    R.reset_stats()
    after = _stats(R)
    assert {f: after[f] for f in HISTORY + ("errorFlags",)} == {f: 0 for f in HISTORY + ("errorFlags",)}
    assert {f: after[f] for f in STATE} == {f: before[f] for f in STATE}
    assert sorted(_events(R)) == [((k, 4321), evs[k].tobytes(), 13) for k in range(2)]
    assert _lost(R) == [(5, 4321, 2, 0)]
    # the three items complete and count from zero
    a = len(s1) + 2
    _launch(R, dpk, dln, STRIDE, a, len(ln), 600, "fused")
    assert sorted(_events(R)) == [((k, 4321), evs[k].tobytes(), 13) for k in (2, 3, 4)]
    st = _stats(R)
    assert {f: st[f] for f in HISTORY} == {"eventSuccess": 3, "totalPackets": len(s3), "totalBytes": int(ln[a:].sum()),
                                          "badHeaderDiscards": 0, "dataErrCnt": 0, "enqueueLoss": 0,
                                          "reassemblyLoss": 0}
    assert st["inProgress"] == 0 and st["errorFlags"] == 0
    R.close()


@pytest.mark.parametrize("form", FORMS + ["reference_order"])
def test_a_fragment_that_overruns_its_own_length_creates_no_item(hip, form):
    """offset + payload > bufferLength in a fragment's own header: dropped and counted before
    the table lookup, as the oracle does (cpp:391 has no check).  The default
    mode used to create an item for such a fragment when its key had none -- a slot, a buffer
    and an in-progress count that only the GC freed, as a lost event of 0 fragments
    (test_reset_stats_zeroes_history_and_keeps_state found it)."""
    over = np.zeros(STRIDE, np.uint8)
    over[:36] = np.frombuffer(O.lbre_hdr(2, 7, 99, 4321, 100, 50, 999), np.uint8)
    fr = _frags(_bytes(650, 100), 998)                        # 7 fragments
    flags = _ro() if form == "reference_order" else 0
    s = _schedule([("batch", [(over, 52)] + fr[:3] + [(over, 52)], 100), ("poll", 0), ("stats",), ("compact",),
                   ("batch", [(over, 52)], 200), ("stats",), ("gc", 1000, 500), ("lost_poll", 0), ("stats",)])
    R, ref = _run(hip, s, "fused" if flags else form, flags)
    assert ref[2]["dataErrCnt"] == 2 and ref[2]["inProgress"] == 1 and ref[5]["dataErrCnt"] == 3
    assert ref[7] == [(998, 4321, 3)]
    st = _stats(R)
    assert st["tableUsed"] == 1 and st["arenaUsed"] == 256     # the one real item, after the compaction
    R.close()


# l
SEG_EVENT =np.dtype([("data", "<u8"), ("eventNum", "<u8"), ("lbTick", "<u8"), ("bytes", "<u4"),
                      ("pktBase", "<u4"), ("dataId", "<u2"), ("entropy", "<u2"), ("reserved", "<u4")])
PLAN_CASES = [(0, 600), (0, 256), (0, 257), (1, 600), (255, 2), (256, 344), (300, 1000), (600, 5), (700, 5)]


def test_relay_plan_beyond_one_scan_step(hip):
    """relay_plan_kernel scans 256 records per step: the carry across steps, a non-zero
    firstRecord, and maxEvents below and above what is stored."""
    import torch
    from e2sar_amd import sar
    rnd = np.random.default_rng(600)
    sizes = [int(x) for x in rnd.integers(1, 49, 600)]
    evs = [_bytes(7000 + k, n) for k, n in enumerate(sizes)]
    fr = [_frags(e, 5000 + k, 4000 + k % 7) for k, e in enumerate(evs)]
    every = [f for f_ in fr for f in f_]
    dpk, dln = _upload(hip, np.stack([p for p, _ in every]), np.array([L for _, L in every], np.uint32))
    R = _reas(hip, slots=1024, qcap=1024)
    _launch(R, dpk, dln, STRIDE, 0, len(every), 0, "fused")
    seg = sar.DeviceSegmenter(hip, mtu=80, lb_hdr_version=2)
    assert seg.max_pld == MP and seg.stride == STRIDE
    tick, ent0 = 0x0123456789ABCDEF, 0xFF00                   # entropies wrap past 0xFFFF
    plans = {}
    for first, cap in PLAN_CASES:
        desc = torch.full((cap * sar.SEG_EVENT_BYTES,), 0xEE, dtype=torch.uint8, device=hip.torch_device)
        cnt = torch.full((2,), -1, dtype=torch.int32, device=hip.torch_device)
        R.relay_plan(desc, cnt, first, cap, MP, tick, ent0)
        out = None
        if (first, cap) == (256, 344):
            opk, oln = seg.alloc_packets(cap * 3)
            seg.segment_device(desc, cnt, cap, 3, opk, oln)
            out = (opk, oln)
        plans[(first, cap)] = (desc, cnt, out)
    torch.cuda.synchronize()
    arena = R.arena_ptr
    recs = R.poll()
    assert len(recs) == 600 and sorted(r.eventNum for r in recs) == list(range(5000, 5600))
    by_key = {(5000 + k, 4000 + k % 7): e for k, e in enumerate(evs)}
    for (first, cap), (desc, cnt, out) in plans.items():
        n = min(cap, max(0, 600 - first))
        want = recs[first:first + n]
        npk = [(r.bytes + MP - 1) // MP for r in want]
        assert [int(x) for x in cnt.cpu().tolist()] == [n, sum(npk)], (first, cap)
        raw = desc.cpu().numpy()
        table = np.frombuffer(raw.tobytes(), SEG_EVENT)
        assert (raw[n * 40:] == 0xEE).all(), (first, cap)     # nothing written past descriptor n
        base = 0
        for i, (t, r) in enumerate(zip(table[:n], want)):
            assert int(t["data"]) == arena + r.arenaOffset
            assert (int(t["eventNum"]), int(t["dataId"]), int(t["bytes"])) == (r.eventNum, r.dataId, r.bytes)
            assert int(t["lbTick"]) == tick and int(t["entropy"]) == (ent0 + i) & 0xFFFF
            assert int(t["pktBase"]) == base and int(t["reserved"]) == 0, (first, cap, i)
            base += npk[i]
        if out is not None:
            assert n > 256
            total = sum(npk)
            gp = out[0][: total * STRIDE].view(total, STRIDE).cpu().numpy()
            gl = out[1][:total].cpu().numpy().astype(np.uint32)
            base = 0
            for i, r in enumerate(want):
                op, ol = O.segment_event(by_key[(r.eventNum, r.dataId)], r.eventNum, r.dataId, (ent0 + i) & 0xFFFF,
                                         tick, 2, MP, STRIDE)
                np.testing.assert_array_equal(gl[base:base + len(ol)], ol)
                for k in range(len(ol)):
                    assert np.array_equal(gp[base + k, :int(ol[k])], op[k, :int(ol[k])]), (i, k)
                base += len(ol)
            assert base == total
    assert _stats(R)["errorFlags"] == 0
    R.close()
