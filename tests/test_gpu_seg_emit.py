"""e2sar_hip_seg_emit against the host models of tests/seg_emit_ref.py (the plan) and
tests/seg_ref.py (the datagrams): events whose count, lengths and offsets live in device memory.

Every case runs the call over canary-filled packet, lens, descriptor and count buffers and
compares them whole: the datagram bytes and the zero fill, the canary in every slot, lens
entry and descriptor the contract leaves alone, the descriptors field for field (`reserved`
is the library's) and d_counts[0..3].  The source holds random non-zero bytes, so a byte
read from outside an event shows in a slot.  Most calls go through the C ABI itself because
the stride, maxPackets and the source's extent must be settable.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import seg_emit_ref as E
import seg_ref as M

pytestmark = pytest.mark.gpu

SEG_EVENT = np.dtype([("data", "<u8"), ("eventNum", "<u8"), ("lbTick", "<u8"), ("bytes", "<u4"), ("pktBase", "<u4"),
                      ("dataId", "<u2"), ("entropy", "<u2"), ("reserved", "<u4")])
FIELDS = ("data", "eventNum", "lbTick", "bytes", "pktBase", "dataId", "entropy")
CANARY_COUNT = 0x5A5A5A5A
NUM = E.Numbering(event_num_base=0x0102030405060000, lb_tick_base=0x0123456789AB0000, lb_tick_step=1, data_id=4321,
                  entropy_base=0xBEEF)


class _Emit:
    """One e2sar_hip_seg_emit call over fresh canary buffers, and what it left.

    arena: the device region's bytes; lengths (and offsets) name max_events source events;
    slots: the packet buffer's size in slots (default: max_packets); count: *d_count, None =
    NULL; base_off: d_data = the arena's address + base_off."""

    def __init__(self, hip, arena, lengths, max_pld, stride, ver, *, offsets=None, pitch=0, count=None, max_packets=None,
                 slots=None, data_bytes=None, num=NUM, hint=0, base_off=0):
        import torch
        from e2sar_amd import _capi
        from e2sar_amd._capi import check, lib
        dev = hip.torch_device
        lengths = np.asarray(lengths, np.uint32)
        self.max_events = len(lengths)
        total = int(M.num_packets(lengths, max_pld).sum())
        self.max_packets = total if max_packets is None else max_packets
        slots = max(self.max_packets, 1) if slots is None else slots
        self.data_bytes = arena.size - base_off if data_bytes is None else data_bytes
        self.args = dict(pitch=pitch, offsets=offsets, count=count, num=num)
        self.lengths, self.max_pld, self.stride, self.ver, self.arena_np, self.base_off = lengths, max_pld, stride, ver, arena, base_off
        self.pk0, self.ln0 = M.canary_buffers(slots, stride)
        t = lambda a: torch.from_numpy(a).to(dev)
        self.arena = t(arena)
        assert self.arena.data_ptr() % 16 == 0
        self.d_len = t(lengths.view(np.int32))
        self.d_off = t(np.asarray(offsets, np.uint64).view(np.int64)) if offsets is not None else None
        self.d_count = t(np.array([count], np.uint32).view(np.int32)) if count is not None else None
        self.d_nums = t(num.event_nums.view(np.int64)) if num.event_nums is not None else None
        self.pkts, self.lens = t(self.pk0), t(self.ln0.view(np.int32))
        self.events = torch.full(((self.max_events + 2) * 40,), M.CANARY, dtype=torch.uint8, device=dev)
        self.counts = torch.full((8 + 2,), CANARY_COUNT, dtype=torch.int32, device=dev)
        ptr = lambda x, o=0: (x.data_ptr() + o) if x is not None else 0
        self.src = _capi.SegSource(ptr(self.arena, base_off), self.data_bytes, ptr(self.d_len), ptr(self.d_count),
                                   ptr(self.d_off), pitch, hint)
        self.num = _capi.SegNumbering(ptr(self.d_nums), num.event_num_base, num.lb_tick_base, num.lb_tick_step, num.data_id,
                                      num.entropy_base, _capi.SEG_TICKS_AS_EVENTNUM if num.ticks_as_event_num else 0)
        self.call = lambda stream: check(lib().e2sar_hip_seg_emit(
            hip.handle, C.byref(self.src), C.byref(self.num), self.max_events, ver, max_pld,
            C.c_void_p(ptr(self.pkts, M.GUARD)), stride, self.max_packets, C.c_void_p(ptr(self.lens, 4 * M.GUARD_LENS)),
            C.c_void_p(ptr(self.events, 40)), C.c_void_p(ptr(self.counts, 4)), C.c_void_p(int(stream.cuda_stream))))

    def run(self):
        import torch
        self.call(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return self

    def plan(self, lengths=None, count="same"):
        a = self.args
        return E.plan(self.lengths if lengths is None else lengths, self.max_pld, self.max_packets, self.data_bytes,
                      pitch=a["pitch"], offsets=a["offsets"], count=a["count"] if count == "same" else count,
                      max_events=self.max_events, num=a["num"])

    def check(self, what, plan=None, pk0=None, ln0=None):
        """The buffers against the model's plan; -> (packet bytes, lens) as the device left them."""
        plan = self.plan() if plan is None else plan
        counts = self.counts.cpu().numpy().view(np.uint32)
        assert counts[[0, 9]].tolist() == [CANARY_COUNT] * 2, f"{what}: a word beside d_counts was written"
        assert counts[1:5].tolist() == plan.counts, f"{what}: d_counts[0..3] {counts[1:5].tolist()}, want {plan.counts}"
        desc = self.events.cpu().numpy()
        got = desc[40:40 + 40 * plan.n].view(SEG_EVENT)
        rest = np.delete(desc, np.s_[40:40 + 40 * plan.n])
        assert (rest == M.CANARY).all(), f"{what}: a descriptor at or past n = {plan.n} (or beside the table) was written"
        base = self.arena.data_ptr() + self.base_off
        for f in FIELDS:
            want = plan.events["off"] + np.uint64(base) if f == "data" else plan.events[f]
            np.testing.assert_array_equal(got[f], want, err_msg=f"{what}: descriptor field {f}")
        arena = self.arena_np[self.base_off:]
        want_pk, want_ln = M.expected(arena, plan.events, self.max_pld, self.stride, self.ver,
                                      self.pk0 if pk0 is None else pk0, self.ln0 if ln0 is None else ln0)
        got_ln = self.lens.cpu().numpy().view(np.uint32)
        bad = np.nonzero(got_ln != want_ln)[0]
        assert bad.size == 0, (f"{what}: {bad.size} lens entries differ, first at slot {int(bad[0]) - M.GUARD_LENS}: "
                               f"got {int(got_ln[bad[0]]):#x}, want {int(want_ln[bad[0]]):#x}")
        got_pk = self.pkts.cpu().numpy()
        diff = M.first_difference(got_pk, want_pk, self.stride)
        assert diff is None, f"{what}: {diff}"
        return got_pk, got_ln


def _subset_lengths(max_pld):
    return [n for n in (1, 5, 12, 13, 17, max_pld - 1, max_pld, max_pld + 1, 3 * max_pld - 1, 3 * max_pld + 1) if n > 0]


@functools.lru_cache(maxsize=None)
def _ragged(max_pld):
    """-> (arena, offsets, lengths): the subset matrix at every residue mod 16, one empty event."""
    offs, lens, need = M.pack_events(M.matrix_cases(max_pld, _subset_lengths(max_pld)))
    return M.random_arena(need, 3000 + max_pld), offs, lens


# ----------------------------------------------------------------------------------
# 1. parity, ragged


@pytest.mark.parametrize("ver", [2, 3])
@pytest.mark.parametrize("max_pld", [1, 12, 1436, 8936])
def test_parity_ragged(hip, max_pld, ver):
    arena, offs, lens = _ragged(max_pld)
    call = _Emit(hip, arena, lens, max_pld, M.min_stride(max_pld), ver, offsets=offs).run()
    plan = call.plan()
    assert plan.counts == [len(lens), M.total_packets(M.make_events(offs, lens, max_pld), max_pld), 0, 0]
    assert (plan.events["pktBase"] == M.make_events(offs, lens, max_pld)["pktBase"]).all()
    call.check(f"maxPld {max_pld} v{ver}", plan)


# ----------------------------------------------------------------------------------
# 2. parity, rows


@pytest.mark.parametrize("base_off", [0, 1, 2, 3])
@pytest.mark.parametrize("pitch,max_pld,ver", [(100, 12, 2), (1437, 1436, 3)])
def test_parity_rows(hip, pitch, max_pld, ver, base_off):
    """64 rows: with the four base offsets the rows of either pitch start at every residue
    mod 16, each with every length of 0, 1, pitch - 1, pitch."""
    rows = 64
    starts = {(base_off + i * pitch) % 16 for i in range(rows)}
    assert len(starts) == (16 if pitch % 2 else 4)
    lens = [(0, 1, pitch - 1, pitch)[(i // 16) % 4] for i in range(rows)]
    arena = M.random_arena(base_off + rows * pitch + 64, 40 + pitch)
    call = _Emit(hip, arena, lens, max_pld, M.min_stride(max_pld), ver, pitch=pitch, base_off=base_off,
                 data_bytes=rows * pitch).run()
    assert call.plan().counts[0] == rows
    call.check(f"pitch {pitch} base {base_off}")


# ----------------------------------------------------------------------------------
# 3. unit boundaries, both instantiations


@functools.lru_cache(maxsize=None)
def _unit_batch(max_pld, stride):
    """Events of 256 * U * m - 1, that, and + 1 chunks for U = 2, 4 and m = 1, 2 (the nearest
    reachable counts where spc does not divide it), ending in a 1-byte and in a full last
    datagram; empty events first, between them and last."""
    spc = stride // 16
    npks = sorted({n for U in (2, 4) for m in (1, 2) for t in (-1, 0, 1) for n in M.npk_near(256 * U * m + t, spc)})
    cases = [(0, 0), (7, 0)]
    for k, (n, tail) in enumerate((n, tail) for n in npks for tail in (1, max_pld)):
        cases.append(((4 * k + (3 if k % 5 == 4 else 0)) % 16, (n - 1) * max_pld + tail))
        if k % 3 == 0:
            cases.append((k % 16, 0))
    cases += [(9, 0), (0, 0)]
    offs, lens, need = M.pack_events(cases)
    return M.random_arena(need, 91 + max_pld), offs, lens


@pytest.mark.parametrize("ver", [2, 3])
@pytest.mark.parametrize("max_pld,stride", [(12, 48), (1436, 1472)])
def test_unit_boundaries(hip, max_pld, stride, ver):
    arena, offs, lens = _unit_batch(max_pld, stride)
    assert lens[0] == 0 and lens[-1] == 0
    out = {}
    for U, hint in ((4, 0xFFFFFFFF), (2, 1)):               # the hint selects the instantiation only
        assert U == (2 if -(-hint // max_pld) * (stride // 16) <= 1 << 18 else 4)
        out[U] = _Emit(hip, arena, lens, max_pld, stride, ver, offsets=offs, hint=hint).run().check(f"maxPld {max_pld} U {U}")
    assert np.array_equal(out[2][0], out[4][0]) and np.array_equal(out[2][1], out[4][1])
    # hint 0 = unknown: U = 4's launch
    _Emit(hip, arena, lens, max_pld, stride, ver, offsets=offs, hint=0).run().check(f"maxPld {max_pld} no hint")


# ----------------------------------------------------------------------------------
# 4. the plan across its 256-event steps


@functools.lru_cache(maxsize=None)
def _many():
    lens = np.random.default_rng(600).integers(0, 41, 600).astype(np.uint32)
    lens[[0, 100, 255, 256, 257, 300, 511, 512, 513, 599]] = [0, 5, 40, 7, 0, 40, 13, 25, 0, 40]
    cases = [((5 * i) % 16, int(n)) for i, n in enumerate(lens)]
    offs, lens, need = M.pack_events(cases)
    return M.random_arena(need, 601), offs, lens


@pytest.mark.parametrize("cut", [None, 100, 255, 256, 300, 511, 512, 599])
def test_plan_across_steps(hip, cut):
    """600 events of 0..40 bytes at maxPld 12: the carries across the scan steps, and capacity
    cuts in the first, second and third step and on their edges."""
    arena, offs, lens = _many()
    npk = M.num_packets(lens, 12)
    cap = None
    if cut is not None:
        assert npk[cut] > 0
        cap = int(npk[:cut + 1].sum()) - 1                  # event `cut` is one slot short
    call = _Emit(hip, arena, lens, 12, 48, 2, offsets=offs, max_packets=cap, slots=int(npk.sum())).run()
    plan = call.plan()
    assert plan.counts[0] == (600 if cut is None else cut) and plan.counts[3] == (0 if cut is None else 1)
    call.check(f"cut {cut}", plan)


def test_plan_source_cut_in_second_step(hip):
    arena, offs, lens = _many()
    lens = lens.copy()
    offs = offs.copy()
    offs[300] = arena.size - int(lens[300]) + 1             # ends one byte past the region
    call = _Emit(hip, arena, lens, 12, 48, 3, offsets=offs).run()
    plan = call.plan()
    assert plan.counts[0] == 300 and plan.counts[2:] == [300, 2]
    call.check("outside at 300", plan)


# ----------------------------------------------------------------------------------
# 5. the device-side count


@pytest.mark.parametrize("count", [0, 1, "n-1", "n", "n+5", 0xFFFFFFFF, None])
def test_device_count(hip, count):
    arena, offs, lens = _ragged(1436)
    n = len(lens)
    count = {"n-1": n - 1, "n": n, "n+5": n + 5}.get(count, count)
    call = _Emit(hip, arena, lens, 1436, 1472, 2, offsets=offs, count=count).run()
    plan = call.plan()
    assert plan.counts[0] == (n if count is None else min(count, n)) and plan.counts[2:] == [0, 0]
    call.check(f"count {count}", plan)                      # descriptors and slots past n keep the canary


# ----------------------------------------------------------------------------------
# 6. packet capacity


@pytest.mark.parametrize("short", [0, 1, 2, "all"])
def test_capacity(hip, short):
    """maxPackets of total, total - 1, total - 2 and 0.  The batch ends with a 3-datagram event
    and a 1-byte event: at total - 1 only the last does not fit; at total - 2 the 3-datagram
    event is cut and the 1-byte event behind it, which would fit, is not taken."""
    arena, offs, lens = _ragged(12)
    offs = np.concatenate((offs[:-2], [offs[-2], offs[-2] + 30])).astype(np.uint64)
    lens = np.concatenate((lens[:-2], [30, 1])).astype(np.uint32)
    total = int(M.num_packets(lens, 12).sum())
    cap = 0 if short == "all" else total - short
    call = _Emit(hip, arena, lens, 12, 48, 3, offsets=offs, max_packets=cap, slots=total).run()
    plan = call.plan()
    n = len(lens)
    assert plan.counts == {0: [n, total, 0, 0], 1: [n - 1, total - 1, 1, 1], 2: [n - 2, total - 4, 2, 1],
                           "all": [0, 0, n, 1]}[short]
    call.check(f"maxPackets {cap}", plan)


def test_capacity_zero_takes_leading_empty_events(hip):
    arena = M.random_arena(256, 9)
    call = _Emit(hip, arena, [0, 0, 5, 0], 12, 48, 2, offsets=np.array([3, 3, 3, 9], np.uint64), max_packets=0, slots=4).run()
    assert call.plan().counts == [2, 0, 2, 1]
    call.check("maxPackets 0")


# ----------------------------------------------------------------------------------
# 7. source bounds


def test_row_longer_than_pitch(hip):
    pitch = 100
    lens = [100, 7, 101, 3, 0]
    arena = M.random_arena(5 * pitch + 64, 70)
    call = _Emit(hip, arena, lens, 12, 48, 2, pitch=pitch, data_bytes=5 * pitch, slots=64, max_packets=64).run()
    assert call.plan().counts == [2, 10, 3, 2]
    call.check("row of pitch + 1")


def test_ragged_end_past_the_source(hip):
    arena = M.random_arena(1024, 71)
    offs = np.array([0, 500, 990, 16], np.uint64)
    ok = _Emit(hip, arena, [40, 60, 10, 5], 12, 48, 3, offsets=offs, data_bytes=1000, slots=64, max_packets=64).run()
    assert ok.plan().counts == [4, 11, 0, 0]
    ok.check("end at dataBytes")
    bad = _Emit(hip, arena, [40, 60, 11, 5], 12, 48, 3, offsets=offs, data_bytes=1000, slots=64, max_packets=64).run()
    assert bad.plan().counts == [2, 9, 2, 2]
    bad.check("end at dataBytes + 1")
    far = _Emit(hip, arena, [40, 60], 12, 48, 3, offsets=np.array([0, 2**64 - 8], np.uint64), data_bytes=1000, slots=64,
                max_packets=64).run()
    assert far.plan().counts == [1, 4, 1, 2]
    far.check("offset + bytes wraps in 64 bits")


@pytest.mark.parametrize("count", [None, 8, 5])
def test_fewer_rows_than_the_count(hip, count):
    pitch = 100
    arena = M.random_arena(8 * pitch + 64, 72)
    call = _Emit(hip, arena, [9] * 8, 12, 48, 2, pitch=pitch, data_bytes=5 * pitch + 99, count=count, slots=16,
                 max_packets=16).run()
    assert call.plan().counts == [5, 5, 0, 0 if count == 5 else 2]
    call.check(f"5 rows of data, count {count}")


# ----------------------------------------------------------------------------------
# 8. numbering


@pytest.mark.parametrize("kind", ["wrap", "array", "ticks"])
@pytest.mark.parametrize("ver", [2, 3])
def test_numbering(hip, kind, ver):
    arena, offs, lens = _ragged(12)
    num = {"wrap": E.Numbering(event_num_base=2**64 - 2, lb_tick_base=2**64 - 700, lb_tick_step=7, data_id=0xFFFF,
                               entropy_base=0xFFFE),
           "array": E.Numbering(event_nums=np.random.default_rng(8).integers(0, 2**64, len(lens), dtype=np.uint64),
                                event_num_base=5, lb_tick_base=1 << 40, data_id=7, entropy_base=3),
           "ticks": E.Numbering(event_num_base=99, lb_tick_base=0x0123456789ABCDEF, lb_tick_step=0x100000001,
                                data_id=1, entropy_base=0x8000, ticks_as_event_num=True)}[kind]
    call = _Emit(hip, arena, lens, 12, 48, ver, offsets=offs, num=num).run()
    plan = call.plan()
    if kind == "wrap":
        assert plan.events["eventNum"][:3].tolist() == [2**64 - 2, 2**64 - 1, 0]
        assert plan.events["entropy"][:3].tolist() == [0xFFFE, 0xFFFF, 0]
        assert plan.events["lbTick"][99:101].tolist() == [2**64 - 7, 0]
    call.check(kind, plan)


# ----------------------------------------------------------------------------------
# 9. capture


def test_graph_replay(hip):
    """One emit captured into a HIP graph (a linear chain of two kernel nodes) and replayed
    twice, with the lengths and the count rewritten in place between the replays."""
    import torch
    arena, offs, lens = _ragged(1436)
    n = len(lens)
    call = _Emit(hip, arena, lens, 1436, 1472, 2, offsets=offs, count=n).run()
    call.check("uncaptured")
    pk0, ln0 = torch.from_numpy(call.pk0).to(hip.torch_device), torch.from_numpy(call.ln0.view(np.int32)).to(hip.torch_device)
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        call.call(cap)
    results = []
    for replay, (count, scale) in enumerate([(n, 1), (n - 3, 0)]):
        new = lens if scale else np.where(np.arange(n) % 2 == 0, np.minimum(lens, 1437), 0).astype(np.uint32)
        call.d_len.copy_(torch.from_numpy(new.view(np.int32)))
        call.d_count.fill_(count)
        call.pkts.copy_(pk0)
        call.lens.copy_(ln0)
        call.events.fill_(M.CANARY)
        call.counts.fill_(CANARY_COUNT)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        plan = call.plan(new, count)
        assert plan.counts[0] == count
        results.append(call.check(f"replay {replay}", plan))
    assert not np.array_equal(results[0][0], results[1][0])


# ----------------------------------------------------------------------------------
# 10. round trip through the Python API


def test_round_trip_rows(hip):
    """emit_rows -> counts -> DeviceReassembler.reassemble -> collect_rows gives the source rows back."""
    import torch
    from e2sar_amd import sar
    rows_n, pitch = 37, 5008
    host = M.random_arena(rows_n * pitch, 11).reshape(rows_n, pitch)
    lens = np.random.default_rng(12).integers(1, pitch + 1, rows_n).astype(np.int32)
    lens[[0, 5, 36]] = [pitch, 1, pitch - 1]
    dev = hip.torch_device
    rows = torch.from_numpy(host).to(dev)
    d_len = torch.from_numpy(lens).to(dev)
    count = torch.tensor([rows_n - 4], dtype=torch.int32, device=dev)
    seg = sar.DeviceSegmenter(hip, mtu=1500, lb_hdr_version=2)
    packets, plens, events, counts = seg.emit_rows(rows, d_len, count, event_num_base=1000, data_id=77, entropy_base=5,
                                                  lb_tick_base=9, lb_tick_step=1)
    desc = sar.parse_emit(events, counts)
    n, ndg, left, why = counts.cpu().tolist()[:4]
    assert (n, left, why) == (rows_n - 4, 0, 0) and len(desc) == n
    assert ndg == int(M.num_packets(lens[:n].astype(np.uint32), seg.max_pld).sum())
    assert desc["eventNum"].tolist() == list(range(1000, 1000 + n)) and desc["bytes"].tolist() == lens[:n].tolist()
    R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=256, queue_capacity=256, arena_bytes=1 << 22)
    R.reassemble(packets, seg.stride, plens, ndg)
    out, index, ccounts = R.collect_rows(rows_n, pitch)
    got = sar.parse_collect(index, ccounts)
    assert len(got) == n and R.stats().errorFlags == 0
    out = out.cpu().numpy()
    for r, g in enumerate(got):                             # completion order is the device's
        i = int(g["eventNum"]) - 1000
        assert int(g["bytes"]) == lens[i] and int(g["dataId"]) == 77
        assert np.array_equal(out[r, :lens[i]], host[i, :lens[i]]), f"row {i}"
        assert not out[r, lens[i]:].any()
    assert sorted(int(g["eventNum"]) for g in got) == list(range(1000, 1000 + n))
    R.close()


# ----------------------------------------------------------------------------------
# 11. argument statuses


def test_argument_statuses(hip):
    """Return code and message of every check, in the order they fire; no failing call
    reaches a launch."""
    import torch
    from e2sar_amd import _capi
    from e2sar_amd._capi import ERR_OUT_OF_RANGE, ERR_PARAMETER, E2SARHipError, check, lib
    buf = torch.zeros(1 << 14, dtype=torch.uint8, device=hip.torch_device)
    base = (buf.data_ptr() + 255) & ~255
    pk, ln, ev, cnt, data, nb, offs = base, base + 0x1000, base + 0x1400, base + 0x1800, base + 0x2000, base + 0x2800, base + 0x2C00
    NULL = C.c_void_p(0)
    p = C.c_void_p

    def src(d_data=data, d_bytes=nb, pitch=64, d_offsets=0, hint=0):
        return C.byref(_capi.SegSource(d_data, 1024, d_bytes, 0, d_offsets, pitch, hint))

    def num(flags=0):
        return C.byref(_capi.SegNumbering(0, 0, 0, 0, 0, 0, flags))

    def fails(code, msg, rc):
        with pytest.raises(E2SARHipError) as ei:
            check(rc)
        assert (ei.value.code, ei.value.msg) == (code, msg)

    L, P, h = lib(), ERR_PARAMETER, hip.handle
    emit = L.e2sar_hip_seg_emit
    fails(P, "ctx is NULL", emit(NULL, src(), num(), 4, 2, 100, p(pk), 144, 8, p(ln), p(ev), p(cnt), NULL))
    # maxEvents 0: success before any other check, nothing launched
    assert emit(h, None, None, 0, 2, 0, NULL, 0, 0, NULL, NULL, NULL, NULL) == 0
    fails(P, "NULL source or numbering", emit(h, None, num(), 4, 2, 100, p(pk), 144, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, "NULL source or numbering", emit(h, src(), None, 4, 2, 100, p(pk), 144, 8, p(ln), p(ev), p(cnt), NULL))
    for bad in (dict(d_data=0), dict(d_bytes=0)):
        fails(P, "NULL device buffer", emit(h, src(**bad), num(), 4, 2, 100, p(pk), 144, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, "NULL device buffer", emit(h, src(), num(), 4, 2, 100, NULL, 144, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, "NULL device buffer", emit(h, src(), num(), 4, 2, 100, p(pk), 144, 8, p(ln), NULL, p(cnt), NULL))
    fails(P, "NULL device buffer", emit(h, src(), num(), 4, 2, 100, p(pk), 144, 8, p(ln), p(ev), NULL, NULL))
    both = "give a pitch (rows) or d_offsets (ragged), not both"
    fails(P, both, emit(h, src(pitch=64, d_offsets=offs), num(), 4, 2, 100, p(pk), 144, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, both, emit(h, src(pitch=0, d_offsets=0), num(), 4, 2, 100, p(pk), 144, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, "unknown numbering flags", emit(h, src(), num(2), 4, 2, 100, p(pk), 144, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, "maxPldLen is 0 (MTU too small)", emit(h, src(), num(), 4, 2, 0, p(pk), 144, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, "maxPldLen above a UDP datagram", emit(h, src(), num(), 4, 2, 65536, p(pk), 65600, 8, p(ln), p(ev), p(cnt), NULL))
    stride = "stride must be a multiple of 16 and hold 36 + maxPldLen"
    fails(P, stride, emit(h, src(), num(), 4, 2, 100, p(pk), 128, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, stride, emit(h, src(), num(), 4, 2, 100, p(pk), 150, 8, p(ln), p(ev), p(cnt), NULL))
    fails(P, "packet buffer not 16-byte aligned", emit(h, src(), num(), 4, 2, 100, p(pk + 8), 144, 8, p(ln), p(ev), p(cnt), NULL))
    R = ERR_OUT_OF_RANGE
    fails(R, "batch too large", emit(h, src(), num(), 4, 2, 100, p(pk), 144, 0xFFFFFFFF, p(ln), p(ev), p(cnt), NULL))
    # 2^32 - 1 chunks in units of 512 (U = 2 by the pitch) is 2^23 workgroups; + 2^31 events passes 2^31 - 1
    big = "launch too large (units of maxPackets slots + maxEvents)"
    fails(R, big, emit(h, src(), num(), 1 << 31, 2, 12, p(pk), 48, 0xFFFFFFFF // 3, p(ln), p(ev), p(cnt), NULL))
    fails(R, big, emit(h, src(), num(), 0x7FFFFFFF, 2, 12, p(pk), 48, 1, p(ln), p(ev), p(cnt), NULL))
    # d_lens and d_count are optional; a legal call on an empty source runs and takes nothing
    torch.cuda.synchronize()
    assert emit(h, C.byref(_capi.SegSource(data, 0, nb, 0, 0, 64, 0)), num(), 4, 2, 100, p(pk), 144, 8, NULL, p(ev), p(cnt),
                C.c_void_p(int(torch.cuda.current_stream().cuda_stream))) == 0
    torch.cuda.synchronize()
    assert buf[0x1800 + (base - buf.data_ptr()):][:20].view(torch.int32).tolist() == [0, 0, 0, 2, 0]
