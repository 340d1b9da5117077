"""e2sar_hip_reassemble_batch_dev against the oracle: a batch whose datagram count the
kernels read from device memory, min(*d_count, maxPackets) datagrams of it reassembled.

The batches are segmented in order (offset 0 first, no duplicates), so the oracle defines the
outcome however a launch is cut into groups.  The expected result of a call
is the oracle fed the first n = min(count, bound) rows: events, bytes, numFragments, every
counter, errorFlags 0.  The rows at and past n are live datagrams -- the remaining fragments
of events begun before n, and whole events with eventNums of their own -- so a kernel that
reads one of them changes a counter, opens an item or delivers an event the oracle does not
have.  The arena is prefilled with a sentinel: where n falls on an event boundary no byte
outside the delivered records may differ from it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC
import sar_inputs as SI
import seg_emit_ref as E

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SLACK = 4096
COUNTERS = ("eventSuccess", "totalPackets", "totalBytes", "badHeaderDiscards", "dataErrCnt", "enqueueLoss",
            "reassemblyLoss", "inProgress")
STATS = COUNTERS + ("completedPending", "lostPending", "arenaUsed", "tableUsed", "errorFlags")
U32 = 0xFFFFFFFF


class _Batch:
    """Events of nfr[k] fragments each, segmented by the oracle in order into slots of
    `stride` bytes: rows, lens, the event of every row, the rows at which an event starts.
    with_lb False: the datagrams as a receiver behind the load balancer sees them, the LB
    header stripped (a slot of 48 bytes holds RE header + 12 bytes, not LB + RE + 16)."""

    def __init__(self, stride, max_pld, nfr, tail=None, with_lb=True):
        rng = np.random.default_rng([stride, len(nfr)])
        pks, lns, self.events, self.owner = [], [], {}, []
        for k, f in enumerate(nfr):
            size = (f - 1) * max_pld + (int(rng.integers(1, max_pld + 1)) if tail is None else tail)
            data = rng.integers(0, 256, size, dtype=np.uint8)
            ev = RC.EV0 + k
            self.events[(ev, SI.DATA_ID)] = data.tobytes()
            p, l = O.segment_event(data, ev, SI.DATA_ID, SI.entropy(k), SI.lb_tick(k), 2, max_pld,
                                   stride if with_lb else 36 + max_pld)
            assert len(l) == f
            if not with_lb:
                q = np.zeros((f, stride), np.uint8)
                q[:, :20 + max_pld] = p[:, 16:]
                p, l = q, l - 16
            pks.append(p)
            lns.append(l)
            self.owner += [ev] * f
        self.stride, self.with_lb = stride, with_lb
        self.rows, self.lens = np.concatenate(pks), np.concatenate(lns).astype(np.uint32)
        self.owner = np.array(self.owner, np.uint64)
        self.B = len(self.lens)
        self.boundaries = set(np.concatenate(([0], np.cumsum(nfr))).tolist())
        self.sizes = [len(b) for b in self.events.values()]
        self._ref = {}

    def arena_bytes(self):
        return sum(max(256, (n + 255) // 256 * 256) for n in self.sizes) + SLACK

    def ref(self, n, keep=None):
        """The oracle over rows [0, n) (of those, the rows keep selects): ({key: (bytes, frags)}, stats)."""
        key = (n, None if keep is None else keep.tobytes())
        if key not in self._ref:
            sel = np.arange(n) if keep is None else np.nonzero(keep[:n])[0]
            r = O.Reassembler(self.with_lb)
            if sel.size:
                r.push_batch(self.rows[sel], self.lens[sel])
            ref = {}
            for b, e, d, nf in r.pop_all_frags():
                assert (e, d) not in ref
                ref[(e, d)] = (b, nf)
            self._ref[key] = (ref, r.stats())
        return self._ref[key]


def _upload(ctx, rows, lens):
    """Datagram rows as one device buffer and their lengths, with 256 spare bytes behind the
    last slot and one spare length, so that the views advanced past the whole batch still
    have an address."""
    import torch
    flat = np.concatenate([np.ascontiguousarray(rows).reshape(-1), np.zeros(256, np.uint8)])
    dpk = torch.from_numpy(flat).to(ctx.torch_device)
    spare = np.concatenate([np.ascontiguousarray(lens, np.uint32), np.array([U32], np.uint32)])
    dln = torch.from_numpy(spare.view(np.int32).copy()).to(ctx.torch_device)
    return dpk, dln


def _counts(ctx, values):
    import torch
    return torch.from_numpy(np.array(values, np.uint32).view(np.int32).copy()).to(ctx.torch_device)


def _records(R, recs, arena, label, into=None):
    """{key: (bytes, frags)} of the polled records, none twice."""
    got = {} if into is None else into
    for rec in recs:
        key = (rec.eventNum, rec.dataId)
        assert key not in got, f"{label}: {key} delivered twice"
        assert rec.arenaOffset % 256 == 0 and rec.arenaOffset + rec.bytes <= arena.size, label
        got[key] = (arena[rec.arenaOffset:rec.arenaOffset + rec.bytes].tobytes(), rec.numFragments, rec.arenaOffset)
    return got


def _check(got, st, ref, rst, label, arena=None):
    """arena: also, no byte of it outside the delivered records differs from the sentinel."""
    assert set(got) == set(ref), (label, sorted(set(got) ^ set(ref))[:4])
    for k, (b, nf) in ref.items():
        assert got[k][0] == b, f"{label}: event {k} of {len(b)} bytes differs"
        assert got[k][1] == nf, (label, k, got[k][1], nf)
    for f in COUNTERS:
        assert getattr(st, f) == rst[f], (label, f, getattr(st, f), rst[f])
    assert st.errorFlags == 0, (label, st.errorFlags)
    if arena is not None:
        outside = np.ones(arena.size, bool)
        for b, _, off in got.values():
            outside[off:off + len(b)] = False
        stray = np.nonzero(outside & (arena != SENTINEL))[0]
        assert stray.size == 0, f"{label}: {stray.size} arena bytes outside the delivered events written, at {stray[:12]}"


def _stats_tuple(st):
    return tuple(getattr(st, f) for f in STATS)


# ----------------------------------------------------------------------------------
# 1. counts around every group edge


def _auto_group(stride):
    """reas_group_size's budget rule, which stands for a batch far below one residency wave:
    at most 9216 16-byte chunks of slots per workgroup, at most 64 datagrams."""
    G = 64
    while G > 1 and G * (stride // 16) > 9216:
        G >>= 1
    return G


@functools.lru_cache(maxsize=None)
def _small(stride):
    # 48: a reassembler of LB + RE datagrams refuses a slot below 36 + 16 bytes, so the slots
    # of maxPld 12 are read as a receiver behind the load balancer gets them, RE header first
    with_lb = stride != 48
    return _Batch(stride, 12 if stride == 48 else stride - 36, [1 + (5 * k) % 9 for k in range(40)], with_lb=with_lb)


_dev = {}


def _small_on_device(ctx, stride):
    if _dev.get("key") != stride:
        _dev.clear()
        M = _small(stride)
        _dev.update(key=stride, value=(M,) + _upload(ctx, M.rows, M.lens))
    return _dev["value"]


@pytest.mark.parametrize("group_size", [1, 7, 64, 0])
@pytest.mark.parametrize("stride", [48, 1472, 9008])
def test_counts_around_group_edges(hip, stride, group_size):
    import torch
    from e2sar_amd import sar
    M, dpk, dln = _small_on_device(hip, stride)
    B = M.B
    G = min(group_size, 64) if group_size else _auto_group(stride)
    assert B == 196 and 3 * G < B - 1
    values = sorted({0, 1, G - 1, G, G + 1, 3 * G, B - 1, B, B + 5, U32})
    assert any(min(v, B) not in M.boundaries for v in values) and 1 in M.boundaries
    first = _counts(hip, values)
    second = _counts(hip, [B - min(v, B) for v in values])
    whole_ref, whole_st = M.ref(B)
    assert {k: v[0] for k, v in whole_ref.items()} == M.events and whole_st["inProgress"] == 0
    for i, v in enumerate(values):
        n = min(v, B)
        label = f"stride {stride} G {group_size} count {v:#x}"
        R = sar.DeviceReassembler(hip, with_lb_header=M.with_lb, table_slots=4096, arena_bytes=M.arena_bytes(),
                                  group_size=group_size)
        R.arena_tensor().fill_(SENTINEL)
        R.reassemble_dev(dpk, stride, dln, first[i:i + 1], max_packets=B)
        torch.cuda.synchronize()
        recs, st = R.poll(), R.stats()
        arena = R.arena_tensor().cpu().numpy()
        got = _records(R, recs, arena, label)
        ref, rst = M.ref(n)
        _check(got, st, ref, rst, label, arena if n in M.boundaries else None)
        if n == 0:
            assert _stats_tuple(st) == (0,) * len(STATS), (label, _stats_tuple(st))
        # the rest: pointers advanced by n, count B - n; together the whole stream
        R.reassemble_dev(dpk[n * stride:], stride, dln[n:], second[i:i + 1], max_packets=B - n)
        torch.cuda.synchronize()
        recs, st = R.poll(), R.stats()
        arena = R.arena_tensor().cpu().numpy()
        got = _records(R, recs, arena, label + " + rest", {k: (arena[o:o + len(b)].tobytes(), nf, o)
                                                            for k, (b, nf, o) in got.items()})
        _check(got, st, whole_ref, whole_st, label + " + rest", arena)
        R.close()


# ----------------------------------------------------------------------------------
# 2. a word beside the count


@pytest.mark.parametrize("words", [(0, 65, U32), (U32, 65, 0)])
def test_a_word_beside_the_count(hip, words):
    import torch
    from e2sar_amd import sar
    M, dpk, dln = _small_on_device(hip, 1472)
    three = _counts(hip, list(words))
    R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=4096, arena_bytes=M.arena_bytes())
    R.arena_tensor().fill_(SENTINEL)
    R.reassemble_dev(dpk, 1472, dln, three[1:2], max_packets=M.B)
    torch.cuda.synchronize()
    recs, st = R.poll(), R.stats()
    arena = R.arena_tensor().cpu().numpy()
    ref, rst = M.ref(65)
    assert 0 < rst["eventSuccess"] < len(M.events)
    _check(_records(R, recs, arena, "beside"), st, ref, rst, f"count between {words[0]:#x} and {words[2]:#x}")
    R.close()


# ----------------------------------------------------------------------------------
# 3. the split form chosen by the bound

BIG_STRIDE, BIG_PLD, BIG_BOUND, BIG_ROWS = 9008, 8936, 37_300, 2304


@pytest.fixture(scope="module")
def big(hip):
    """37,300 slots of 9008 bytes (more than 320 MiB) in one uninitialised buffer; the first
    2304 hold the 8,936-byte fragments of 768 events of 2, 3 and 4 fragments."""
    import torch
    assert BIG_BOUND * BIG_STRIDE > 320 << 20
    M = _Batch(BIG_STRIDE, BIG_PLD, [2, 3, 4] * (BIG_ROWS // 9), tail=BIG_PLD)
    assert M.B == BIG_ROWS and (M.lens == 36 + BIG_PLD).all()
    dpk = torch.empty(BIG_BOUND * BIG_STRIDE, dtype=torch.uint8, device=hip.torch_device)
    dln = torch.empty(BIG_BOUND, dtype=torch.int32, device=hip.torch_device)
    dpk[:M.rows.size].copy_(torch.from_numpy(M.rows.reshape(-1)))
    dln[:M.B].copy_(torch.from_numpy(M.lens.view(np.int32)))
    yield M, dpk, dln
    del dpk, dln
    torch.cuda.empty_cache()


@pytest.mark.parametrize("count", [0, 1, 1023, 1024, 1025, 2049])
def test_split_form_by_the_bound(hip, big, count):
    """At this stride the scatter has one datagram per workgroup: the counts sit on both
    sides of xcd_runs' window of 1024 groups, whose permutation must be that of the groups
    there are (cdiv(n, G)), not of the grid."""
    import torch
    from e2sar_amd import sar
    M, dpk, dln = big
    R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=4096, arena_bytes=M.arena_bytes())
    R.reassemble_dev(dpk, BIG_STRIDE, dln, _counts(hip, [count]), max_packets=BIG_BOUND)
    torch.cuda.synchronize()
    recs, st = R.poll(), R.stats()
    arena = R.arena_tensor()[:st.arenaUsed].cpu().numpy()
    ref, rst = M.ref(count)
    assert rst["totalPackets"] == count and (count in M.boundaries or rst["inProgress"] == 1)
    _check(_records(R, recs, arena, f"split {count}"), st, ref, rst, f"split form, count {count}")
    R.close()


# ----------------------------------------------------------------------------------
# 4. one graph, different counts


def test_one_graph_different_counts(hip):
    """recycle(force) -> emit -> reassemble_dev(count = emit's counts[1:2]) -> collect (rows),
    captured once on one stream and replayed with the source lengths and the source count
    rewritten in place: no host read between the capture and the end of a replay.

    An empty event has no datagram (e2sar_hip_seg_emit), so the reassembler never hears of
    it: the rows collected are the taken events of at least one byte, in the model's plan."""
    import torch
    from e2sar_amd import sar
    rows_n, pitch = 37, 5008
    dev = hip.torch_device
    host = np.random.default_rng(21).integers(1, 256, (rows_n, pitch), dtype=np.uint8)
    all_lens = np.random.default_rng(22).integers(1, pitch + 1, rows_n).astype(np.uint32)
    all_lens[[0, 5, 36]] = [pitch, 1, pitch - 1]
    half_lens = np.where(np.arange(rows_n) % 4 == 2, 0, np.minimum(all_lens, 1437)).astype(np.uint32)
    seg = sar.DeviceSegmenter(hip, mtu=1500, lb_hdr_version=2)
    max_packets = rows_n * sar.num_packets(pitch, seg.max_pld)
    rows = torch.from_numpy(host).to(dev)
    d_len = torch.from_numpy(all_lens.view(np.int32).copy()).to(dev)
    d_count = torch.tensor([rows_n], dtype=torch.int32, device=dev)
    packets, plens = seg.alloc_packets(max_packets)
    events = torch.empty(rows_n * sar.SEG_EVENT_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int32, device=dev)
    out = torch.empty((rows_n, pitch), dtype=torch.uint8, device=dev)
    index = torch.empty(rows_n * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
    ccounts = torch.empty(4, dtype=torch.int64, device=dev)
    R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=256, queue_capacity=256, arena_bytes=1 << 22)

    def chain(stream):
        R.recycle(force=True, stream=stream)
        seg.emit(rows.view(-1), d_len, packets, plens, events, counts, pitch=pitch, count=d_count, max_events=rows_n,
                 event_num_base=1000, data_id=77, entropy_base=5, lb_tick_base=9, lb_tick_step=1, stream=stream)
        R.reassemble_dev(packets, seg.stride, plens, counts[1:2], stream=stream)
        R.collect(out.view(-1), index, ccounts, 0, rows_n, pitch, stream=stream)

    def check(lens, count, label):
        plan = E.plan(lens, seg.max_pld, max_packets, rows_n * pitch, pitch=pitch, count=count, max_events=rows_n,
                      num=E.Numbering(event_num_base=1000, data_id=77, entropy_base=5, lb_tick_base=9, lb_tick_step=1))
        assert plan.n == count and counts.cpu().tolist()[:4] == plan.counts, label
        want = [int(e) - 1000 for e, b in zip(plan.events["eventNum"], plan.events["bytes"]) if b > 0]
        got = sar.parse_collect(index, ccounts)
        st = R.stats()
        assert int(ccounts[0].item()) == len(want) == len(got), (label, int(ccounts[0].item()), len(want))
        assert st.errorFlags == 0 and st.eventSuccess == len(want) and st.inProgress == 0, label
        assert st.totalPackets == plan.datagrams, (label, st.totalPackets, plan.datagrams)
        o = out.cpu().numpy()
        for r, g in enumerate(got):                             # completion order is the device's
            i = int(g["eventNum"]) - 1000
            assert int(g["bytes"]) == lens[i] and int(g["dataId"]) == 77, (label, i)
            assert np.array_equal(o[r, :lens[i]], host[i, :lens[i]]), f"{label}: row {i}"
            assert not o[r, lens[i]:].any(), f"{label}: row {i} not zero-filled"
        assert sorted(int(g["eventNum"]) - 1000 for g in got) == want, label
        return o, len(want)

    chain(torch.cuda.current_stream())                          # internal buffers exist before the capture
    torch.cuda.synchronize()
    check(all_lens, rows_n, "uncaptured")
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        chain(cap)
    taken = []
    for label, lens, count in [("all rows", all_lens, rows_n), ("half, some empty", half_lens, 19), ("count 0", half_lens, 0)]:
        d_len.copy_(torch.from_numpy(lens.view(np.int32).copy()))
        d_count.fill_(count)
        out.fill_(SENTINEL)
        R.reset_stats()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        o, n = check(lens, count, label)
        taken.append(n)
        if count == 0:
            assert (o == SENTINEL).all(), "count 0: the row buffer was written"
    assert taken == [rows_n, 19 - 5, 0]
    R.close()


# ----------------------------------------------------------------------------------
# 5. relay without the host


def test_relay_without_the_host(hip):
    """R1 reassembles a batch with a host count; relay_plan -> segment_device re-segment its
    events, and R2 takes their datagram count from relay_plan's counts[1] on the device."""
    import torch
    from e2sar_amd import sar
    M, dpk, dln = _small_on_device(hip, 1472)
    dev = hip.torch_device
    R1 = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=256, queue_capacity=256, arena_bytes=M.arena_bytes())
    R2 = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=256, queue_capacity=256, arena_bytes=M.arena_bytes())
    seg = sar.DeviceSegmenter(hip, mtu=1000, lb_hdr_version=3)
    nev = len(M.events)
    maxpk = max(sar.num_packets(n, seg.max_pld) for n in M.sizes)
    desc = torch.zeros(nev * sar.SEG_EVENT_BYTES, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    opk, oln = seg.alloc_packets(nev * maxpk)
    R1.reassemble(dpk, 1472, dln, M.B)
    R1.relay_plan(desc, cnt, 0, nev, seg.max_pld, 0x0123456789ABCDEF, 0xFFFD)
    seg.segment_device(desc, cnt, nev, maxpk, opk, oln)
    R2.reassemble_dev(opk, seg.stride, oln, cnt[1:2])
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [nev, sum(sar.num_packets(n, seg.max_pld) for n in M.sizes)]
    a, b = R1.poll(), R2.poll()
    one = {(r.eventNum, r.dataId): R1.event_bytes(r) for r in a}
    two = {(r.eventNum, r.dataId): R2.event_bytes(r) for r in b}
    assert len(a) == len(b) == nev and one == M.events
    assert two == one
    s2 = R2.stats()
    assert s2.errorFlags == 0 and s2.totalPackets == int(cnt[1].item()) and s2.inProgress == 0
    R1.close()
    R2.close()


# ----------------------------------------------------------------------------------
# 6. ownership


@pytest.mark.parametrize("count", [70, U32])
def test_ownership(hip, count):
    import torch
    from e2sar_amd import sar
    M, dpk, dln = _small_on_device(hip, 1472)
    n = min(count, M.B)
    R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=4096, arena_bytes=M.arena_bytes())
    R.arena_tensor().fill_(SENTINEL)
    R.set_owner(2, 1)
    R.reassemble_dev(dpk, 1472, dln, _counts(hip, [count]), max_packets=M.B)
    torch.cuda.synchronize()
    recs, st = R.poll(), R.stats()
    arena = R.arena_tensor().cpu().numpy()
    mine = M.owner % np.uint64(2) == 1
    ref, rst = M.ref(n, mine)
    assert 0 < rst["totalPackets"] == int(mine[:n].sum()) < n
    _check(_records(R, recs, arena, "owner"), st, ref, rst, f"owner 1 of 2, count {count:#x}",
           arena if n in M.boundaries else None)
    R.close()


# ----------------------------------------------------------------------------------
# 7. statuses


def test_statuses(hip):
    """Return code and message of every check; no failing call changes a statistic."""
    import torch
    from e2sar_amd import _capi, sar
    from e2sar_amd._capi import ERR_LOGIC, ERR_OUT_OF_RANGE, ERR_PARAMETER, E2SARHipError, check, lib
    M, dpk, dln = _small_on_device(hip, 1472)
    cnt = _counts(hip, [5])
    R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=256, queue_capacity=256, arena_bytes=M.arena_bytes())
    RO = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=256, queue_capacity=256, arena_bytes=M.arena_bytes(),
                               flags=_capi.REAS_REFERENCE_ORDER)
    R.reassemble_dev(dpk, 1472, dln, cnt, max_packets=M.B)        # some history for the statistics
    before = _stats_tuple(R.stats())
    assert before[STATS.index("totalPackets")] == 5
    p, NULL = C.c_void_p, C.c_void_p(0)
    call = lib().e2sar_hip_reassemble_batch_dev
    r, pk, ln, ct = R.handle, p(dpk.data_ptr()), p(dln.data_ptr()), p(cnt.data_ptr())

    def fails(code, msg, rc):
        with pytest.raises(E2SARHipError) as ei:
            check(rc)
        assert (ei.value.code, ei.value.msg) == (code, msg)
        assert _stats_tuple(R.stats()) == before and _stats_tuple(RO.stats()) == (0,) * len(STATS), msg

    P = ERR_PARAMETER
    fails(P, "reas is NULL", call(NULL, pk, 1472, ln, ct, M.B, 0, NULL))
    fails(P, "NULL device buffer", call(r, NULL, 1472, ln, ct, M.B, 0, NULL))
    fails(P, "NULL device buffer", call(r, pk, 1472, NULL, ct, M.B, 0, NULL))
    fails(P, "d_count is NULL", call(r, pk, 1472, ln, NULL, M.B, 0, NULL))
    fails(P, "d_count is NULL", call(r, pk, 1472, ln, NULL, 0, 0, NULL))       # NULL never means "all"
    stride = "stride must be a multiple of 16 and > header + 16"
    fails(P, stride, call(r, pk, 1470, ln, ct, M.B, 0, NULL))
    fails(P, stride, call(r, pk, 48, ln, ct, M.B, 0, NULL))                     # 36 + 16 does not fit
    fails(P, "packet buffer not 16-byte aligned", call(r, p(dpk.data_ptr() + 8), 1472, ln, ct, M.B, 0, NULL))
    fails(ERR_OUT_OF_RANGE, "batch too large", call(r, pk, 1472, ln, ct, U32 // 92 + 1, 0, NULL))
    with pytest.raises(E2SARHipError) as ei:
        check(call(RO.handle, pk, 1472, ln, ct, M.B, 0, NULL))
    assert ei.value.code == ERR_LOGIC and "REFERENCE_ORDER" in ei.value.msg
    assert _stats_tuple(RO.stats()) == (0,) * len(STATS)
    # maxPackets 0: success, nothing launched
    assert call(r, pk, 1472, ln, ct, 0, 0, NULL) == 0
    torch.cuda.synchronize()
    assert _stats_tuple(R.stats()) == before
    R.close()
    RO.close()
