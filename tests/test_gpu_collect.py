"""Device-side delivery (e2sar_hip_reas_collect): the events a reassembler completed, packed
into a caller's device buffer by collect_plan_kernel + collect_copy_kernel, against the
host model of tests/collect_ref.py and the events' own bytes.  Bit-exact throughout.

Inputs as in test_gpu_relay.py: the oracle's segmentation of every event (LB header kept),
reassembled by DeviceReassembler.reassemble.  Every output buffer starts as the non-zero
pattern of test_gpu_copy_spans.py with a guard area behind it, and is compared whole: each
byte the contract leaves alone -- padding between ragged events, rows past the last, the
guard -- must still hold the pattern.  The model gets the records poll() returns after the
collects (they stay queued), so index row i is checked against polled record i.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import collect_ref as M
import oracle_ffi as O

pytestmark = pytest.mark.gpu

# sub-dword; one byte either side of a 16-byte chunk, of a payload (1436 at MTU 1500) and of an
# 8-KiB copy piece; two pieces plus one byte; many pieces
SIZES = [1, 3, 15, 16, 17, 67, 1435, 1436, 1437, 8191, 8192, 8193, 16385, 100001, (1 << 20) + 7]
ROW_SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 20000]
GUARD = 8192
FIELDS = ("eventNum", "outOffset", "bytes", "dataId", "flags", "numFragments")


def _pattern(n):
    return (np.arange(n) * 37 % 251 + 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _datagrams(sizes, mtu, seed):
    """-> (sources by (eventNum, dataId), packets[n, stride], lens[n], stride), built once per argument set."""
    rnd = np.random.default_rng(seed)
    mp = O.max_pld_len(mtu)
    stride = (36 + mp + 15) // 16 * 16
    src, pks, lns = {}, [], []
    for k, b in enumerate(sizes):
        data, ev, did = rnd.integers(0, 256, b, dtype=np.uint8), 5000 + 3 * k, 4321 + (k % 3)
        p, l = O.segment_event(data, ev, did, 0x100 + k, 0xABC00 + k, 2, mp, stride)
        src[(ev, did)] = data
        pks.append(p)
        lns.append(l)
    return src, np.concatenate(pks), np.concatenate(lns).astype(np.uint32), stride


def _reassembled(hip, sizes, mtu, seed, queue_capacity=256, table_slots=256, split=None):
    """A reassembler that has completed the events of _datagrams (in `split` launches, cut at those datagram counts)."""
    import torch
    from e2sar_amd import sar
    src, pk, ln, stride = _datagrams(tuple(sizes), mtu, seed)
    R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=table_slots, queue_capacity=queue_capacity,
                              lost_capacity=64, arena_bytes=sum(sizes) + 256 * (len(sizes) + 1))
    cuts = [0] + list(split or []) + [len(ln)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        dpk = torch.from_numpy(pk[a:b].reshape(-1).copy()).to(hip.torch_device)
        dln = torch.from_numpy(ln[a:b].view(np.int32).copy()).to(hip.torch_device)
        R.reassemble(dpk, stride, dln, b - a)
    return R, src


class _Call:
    """One collect call over a fresh pattern buffer of out_bytes + GUARD bytes, and what it left."""

    def __init__(self, hip, R, out_bytes, first=0, max_events=64, pitch=0, align=256):
        import torch
        from e2sar_amd import sar
        from e2sar_amd._capi import check, lib
        self.args = (first, max_events, out_bytes, pitch, align)
        self.before = _pattern(out_bytes + GUARD)
        buf = torch.from_numpy(self.before).to(hip.torch_device)
        index = torch.full((max_events * sar.COLLECT_REC_BYTES,), 0xEE, dtype=torch.uint8, device=hip.torch_device)
        counts = torch.full((4,), -1, dtype=torch.int64, device=hip.torch_device)
        if out_bytes:
            R.collect(buf[:out_bytes], index, counts, first, max_events, pitch, align)
        else:                       # an empty tensor has no address: the C call itself
            check(lib().e2sar_hip_reas_collect(R.handle, first, max_events, C.c_void_p(buf.data_ptr()), 0, pitch, align,
                                               C.c_void_p(index.data_ptr()), C.c_void_p(counts.data_ptr()),
                                               C.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
        self.rows = sar.parse_collect(index, counts)
        self.counts = [int(x) for x in counts.cpu().tolist()]
        self.after = buf.cpu().numpy()
        self.index_tail = index[len(self.rows) * sar.COLLECT_REC_BYTES:].cpu().numpy()

    def check(self, polled, src):
        """Against the model over the polled records: rows, counts, every byte of the buffer."""
        first, max_events, out_bytes, pitch, align = self.args
        rows, counts = M.layout(M.records_of(polled), first, max_events, out_bytes, pitch, align)
        assert self.counts == counts, (self.args, self.counts, counts)
        assert len(self.rows) == counts[0]
        for f in FIELDS:
            np.testing.assert_array_equal(self.rows[f], rows[f], err_msg=f"{f} {self.args}")
        assert (self.index_tail == 0xEE).all(), "index rows past n were written"
        sources = [src[(int(r["eventNum"]), int(r["dataId"]))] for r in rows]
        want = M.expected_out(self.before, rows, sources, pitch)
        bad = np.nonzero(self.after != want)[0]
        assert bad.size == 0, f"{self.args}: {bad.size} bytes differ, first at {bad[:8].tolist()}"
        return rows, counts


@pytest.mark.parametrize("align", [16, 64, 256, 4096])
@pytest.mark.parametrize("mtu", [1500, 9000])
def test_ragged_parity(hip, mtu, align):
    R, src = _reassembled(hip, SIZES, mtu, 17 + mtu)
    call = _Call(hip, R, len(SIZES) * 4096 + sum(SIZES) + 4096, align=align)
    polled = R.poll()
    assert len(polled) == len(SIZES)
    rows, counts = call.check(polled, src)
    assert counts[0] == len(SIZES) and counts[2] == 0 and counts[3] == sum(SIZES)
    for row, rec in zip(call.rows, polled):             # index row i is polled record i
        assert (int(row["eventNum"]), int(row["dataId"]), int(row["bytes"]), int(row["numFragments"])) == \
               (rec.eventNum, rec.dataId, rec.bytes, rec.numFragments)
    R.close()


@pytest.mark.parametrize("mtu", [1500, 9000])
def test_capacity_cut_and_resume(hip, mtu):
    R, src = _reassembled(hip, SIZES, mtu, 17 + mtu)
    big = len(SIZES) * 256 + sum(SIZES) + 256
    order = _Call(hip, R, big)                         # the record order, which is the device's
    assert len(order.rows) == len(SIZES)
    calls = [order]
    for k in (len(SIZES) // 2, len(SIZES) - 1):
        end = int(order.rows["outOffset"][k]) + int(order.rows["bytes"][k])
        for out_bytes, n in ((end, k + 1), (end - 1, k)):
            a = _Call(hip, R, out_bytes)
            assert a.counts[0] == n and a.counts[2] == len(SIZES) - n, (k, out_bytes, a.counts)
            b = _Call(hip, R, big, first=n)
            assert b.counts[0] == len(SIZES) - n and b.counts[2] == 0
            keys = [(int(r["eventNum"]), int(r["dataId"])) for r in np.concatenate([a.rows, b.rows])]
            assert sorted(keys) == sorted(src) and len(set(keys)) == len(keys)       # every event once
            calls += [a, b]
    empty = _Call(hip, R, 0)
    assert empty.counts == [0, 0, len(SIZES), 0]
    calls.append(empty)
    polled = R.poll()
    for c in calls:
        c.check(polled, src)
    R.close()


@pytest.mark.parametrize("pitch", [16, 4096])
def test_row_mode(hip, pitch):
    import torch
    from e2sar_amd import sar
    R, src = _reassembled(hip, ROW_SIZES, 1500, 23)
    n = len(ROW_SIZES)
    full = _Call(hip, R, (n + 2) * pitch, max_events=16, pitch=pitch)          # two rows more than events
    five = _Call(hip, R, 5 * pitch + 15, max_events=16, pitch=pitch)
    rows_t, index_t, counts_t = R.collect_rows(n + 2, pitch)
    got = sar.parse_collect(index_t, counts_t)
    tensor = rows_t.cpu().numpy()
    polled = R.poll()
    rows, counts = full.check(polled, src)
    assert counts == [n, n * pitch, 0, sum(min(b, pitch) for b in ROW_SIZES)]
    assert [int(f) for f in rows["flags"]] == [1 if r.bytes > pitch else 0 for r in polled]
    assert sorted(int(b) for b in rows["bytes"]) == sorted(ROW_SIZES)
    _, counts5 = five.check(polled, src)
    assert counts5[0] == 5 and counts5[2] == n - 5
    # collect_rows: a [max_events, pitch] tensor whose row i is event i
    assert rows_t.shape == (n + 2, pitch) and rows_t.dtype == torch.uint8 and len(got) == n
    for i, row in enumerate(got):
        data = src[(int(row["eventNum"]), int(row["dataId"]))][:pitch]
        assert int(row["outOffset"]) == i * pitch
        assert np.array_equal(tensor[i, :len(data)], data) and not tensor[i, len(data):].any(), i
    R.close()


def test_more_records_than_a_scan_step(hip):
    """601 events: three 256-record steps of the plan's scan (a lost carry shows in every later
    offset), ten levels of the copy's search, and a 3-piece event between single-piece ones
    (a search off by one lands a piece in a neighbour)."""
    rnd = np.random.default_rng(99)
    small = [int(x) for x in rnd.integers(1, 301, 600)]
    sizes = small[:300] + [2 * 8192 + 100] + small[300:]
    mp = O.max_pld_len(1500)
    at = 300 + O.num_packets(sizes[300], mp)           # launches: 300 events, the large one, 300 events
    R, src = _reassembled(hip, sizes, 1500, 99, queue_capacity=1024, table_slots=2048, split=[300, at])
    total = sum((b + 15) // 16 * 16 for b in sizes)
    ragged = _Call(hip, R, total + 64, max_events=1024, align=16)
    rows304 = _Call(hip, R, 700 * 304, max_events=1024, pitch=304)
    polled = R.poll()
    assert len(polled) == 601
    rows, counts = ragged.check(polled, src)
    assert counts == [601, total, 0, sum(sizes)]
    assert 256 < int(np.nonzero(rows["bytes"] > 8192)[0][0]) < 345        # the large event, with events behind it
    rows, counts = rows304.check(polled, src)
    assert counts == [601, 601 * 304, 0, sum(sizes) - sizes[300] + 304] and int(rows["flags"].sum()) == 1
    R.close()


def test_graph_replay(hip):
    """segment(recycle) -> reassemble -> collect captured once on a side stream and replayed
    with new event bytes: no allocation, no memset node, no wait inside the collect."""
    import torch
    from e2sar_amd import sar
    sizes = [5000, 8192, 3, 20001, 70000]
    offs = np.cumsum([0] + [(b + 255) // 256 * 256 for b in sizes])
    dev = hip.torch_device
    source = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=dev)
    seg = sar.DeviceSegmenter(hip, mtu=1500, lb_hdr_version=2)
    plan = seg.plan([(source.data_ptr() + int(offs[k]), b, 70 + k, 9, 1 + k, 5) for k, b in enumerate(sizes)])
    pk, ln = seg.alloc_packets(plan.total_packets)
    R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=64, queue_capacity=64, arena_bytes=1 << 20)
    out_bytes = int(offs[-1]) + 1024
    before = _pattern(out_bytes + GUARD)
    pattern = torch.from_numpy(before).to(dev)
    buf = torch.empty_like(pattern)
    index = torch.empty(8 * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)

    def body(stream):
        seg.segment(plan, pk, ln, stream=stream, recycle=R, force=True)
        R.reassemble(pk, seg.stride, ln, plan.total_packets, stream=stream)
        R.collect(buf[:out_bytes], index, counts, first_record=0, max_events=8, stream=stream)

    def fresh(seed):
        host = np.random.default_rng(seed).integers(0, 256, int(offs[-1]), dtype=np.uint8)
        source.copy_(torch.from_numpy(host).to(dev))
        buf.copy_(pattern)
        index.fill_(0xEE)
        counts.fill_(-1)
        torch.cuda.synchronize()
        return {(70 + k, 9): host[int(offs[k]):int(offs[k]) + b] for k, b in enumerate(sizes)}

    def verify(src, what):
        rows = sar.parse_collect(index, counts)
        polled = R.poll()
        want_rows, want_counts = M.layout(M.records_of(polled), 0, 8, out_bytes)
        assert [int(x) for x in counts.cpu().tolist()] == want_counts and want_counts[0] == len(sizes), what
        for f in FIELDS:
            np.testing.assert_array_equal(rows[f], want_rows[f], err_msg=f"{f} {what}")
        want = M.expected_out(before, want_rows, [src[(int(r["eventNum"]), int(r["dataId"]))] for r in want_rows])
        assert np.array_equal(buf.cpu().numpy(), want), what

    cap = torch.cuda.Stream()
    src = fresh(1)
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        body(cap)
    torch.cuda.synchronize()
    verify(src, "uncaptured step")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        body(cap)
    for replay in range(3):
        src = fresh(10 + replay)
        graph.replay()
        torch.cuda.synchronize()
        verify(src, f"replay {replay}")
    R.close()


def test_cursor_past_the_end(hip):
    R, src = _reassembled(hip, ROW_SIZES, 1500, 23)
    n = len(ROW_SIZES)
    calls = [_Call(hip, R, 1 << 16, first=n), _Call(hip, R, 1 << 16, first=n + 5),
             _Call(hip, R, 1 << 16, first=n, pitch=4096), _Call(hip, R, 1 << 16, first=2**32 - 1)]
    polled = R.poll()
    assert len(polled) == n
    for c in calls:
        assert c.counts == [0, 0, 0, 0]
        c.check(polled, src)
    R.close()


def test_arguments(hip):
    """Each PARAMETER case returns ERR_PARAMETER with a message and launches nothing."""
    import torch
    from e2sar_amd import sar
    from e2sar_amd._capi import ERR_PARAMETER, lib
    R, _ = _reassembled(hip, ROW_SIZES, 1500, 23)
    before = _pattern(1 << 16)
    buf = torch.from_numpy(before).to(hip.torch_device)
    index = torch.full((8 * sar.COLLECT_REC_BYTES,), 0xEE, dtype=torch.uint8, device=hip.torch_device)
    counts = torch.full((4,), -1, dtype=torch.int64, device=hip.torch_device)
    assert buf.data_ptr() % 256 == 0
    good = dict(r=R.handle, first=0, max_events=8, out=buf.data_ptr(), out_bytes=1 << 16, pitch=0, align=256,
                index=index.data_ptr(), counts=counts.data_ptr())
    bad = [dict(r=None), dict(out=None), dict(index=None), dict(counts=None), dict(max_events=0),
           dict(out=buf.data_ptr() + 16), dict(out=buf.data_ptr() + 128), dict(pitch=24), dict(pitch=8),
           dict(align=8), dict(align=48), dict(align=8192), dict(align=1)]
    for change in bad:
        a = dict(good, **change)
        rc = lib().e2sar_hip_reas_collect(a["r"], a["first"], a["max_events"], C.c_void_p(a["out"]), a["out_bytes"],
                                          a["pitch"], a["align"], C.c_void_p(a["index"]), C.c_void_p(a["counts"]),
                                          C.c_void_p(int(torch.cuda.current_stream().cuda_stream)))
        assert rc == ERR_PARAMETER, change
        assert lib().e2sar_hip_last_error(), change
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before)
    assert (index.cpu().numpy() == 0xEE).all() and counts.cpu().tolist() == [-1] * 4
    # align 0 means 256, and the same arguments unchanged are accepted
    R.collect(buf, index, counts, max_events=8, align=0)
    assert len(sar.parse_collect(index, counts)) == 8 and len(R.poll()) == 8
    R.close()
