"""Offsets past 32 bits: an arena above 4 GiB, bufferOffsets from 2^31 up, datagram slots
past 4 GiB of their batch, routed output past 4 GiB.

bufferOffset and bufferLength are u32 on the wire; arenaOffset, PktInfo.dst, p * stride and
outOffset are 64-bit, each by a cast in the kernel that computes it.  One cast dropped would
pass every other test here: no other arena reaches 4 GiB, no other batch 2^32 bytes.

Both situations are sparse.  Arena: two lone fragments that announce lengths of 2^32 - 1 and
3 * 2^30 take the first 7 GiB, so every whole event lies above; nothing but the stated
fragments is written there.  Slots: 67 600 datagrams of 100 bytes in slots of 65 520.
Expected values come from construction (the host never holds the big buffers), except for the
one reference-order case, which asks the oracle over the compact rows.
"""
import random

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC
import reas_lengths as RL
import route_ref as RR
from test_gpu_golden import STATS

pytestmark = pytest.mark.gpu

G = 1 << 30
FILL = 0xA5
NOW = 100

# ----------------------------------------------------------------------------------
# the arena above 4 GiB

ARENA = 7 * G + (64 << 20)
A_LEN, B_LEN = 0xFFFFFFFF, 3 * G
KEY_A, KEY_B = ((0xA << 32) + 0xA, 9), ((0xB << 32) + 0xB, 9)
A_BASE, B_BASE = 0, 1 << 32                      # where the two items lie: A's length rounds up to 2^32
MTU = 1500
IDS = (4321, 4322, 4323)
ARENA_FORMS = ["fused", "split", "pipelined", "reforder", "dev"]


class _Arena:
    """The three launches, the writes they must make below 7 GiB, the whole events."""

    def __init__(self):
        mp = O.max_pld_len(MTU)
        self.mp = mp
        self.stride = stride = (36 + mp + 15) // 16 * 16
        rng = np.random.default_rng(0xFA12)
        pay = lambda n: rng.integers(1, 256, n, dtype=np.uint8)        # noqa: E731  (never 0: A's gaps read 0xA5)
        self.writes = []                                               # (arena offset, bytes) below 7 GiB

        def frag(key, base, off, blen, n, taken=True):
            p = pay(n)
            if taken:
                self.writes.append((base + off, p))
            return RC.dgram(key[0], key[1], off, blen, p, stride, True)

        l1 = [frag(KEY_A, A_BASE, 0, A_LEN, 64)]
        l2 = [frag(KEY_B, B_BASE, 0, B_LEN, 64)]
        l3 = [frag(KEY_A, A_BASE, 1 << 31, A_LEN, 1000),
              frag(KEY_A, A_BASE, A_LEN - 64, A_LEN, 64),              # ends exactly at the length
              frag(KEY_A, A_BASE, 0xFFFFFFF0, A_LEN, 32, taken=False),  # off + pl wraps 32 bits: dropped
              frag(KEY_B, B_BASE, B_LEN - 1000, B_LEN, 1000)]
        rows = [r for r, _ in l1 + l2 + l3]
        lens = [n for _, n in l1 + l2 + l3]
        sizes = [1, 15, 16, 17, 67, mp, mp + 1, 100_000, 1 << 20]
        self.events = {}
        for k in range(24):
            key = (100 + k // 3, IDS[k % 3])
            data = rng.integers(0, 256, sizes[k % 9], dtype=np.uint8)
            self.events[key] = data
            pk, ln = O.segment_event(data, key[0], key[1], k, 7000 + k, 2, mp, stride)
            rows += list(pk)
            lens += [int(x) for x in ln]
        self.rows, self.lens = np.stack(rows), np.array(lens, np.uint32)
        self.launches = [(0, 1), (1, 1), (2, len(lens) - 2)]
        self.frags = {k: O.num_packets(len(b), mp) for k, b in self.events.items()}
        # the windows compared byte for byte: each write with 16 bytes either side; the last ends
        # with B's item (the whole events begin there)
        self.windows = [(0, 64 + 16), ((1 << 31) - 16, (1 << 31) + 1000 + 16),
                        (A_LEN - 64 - 16, B_BASE + 64 + 16), (B_BASE + B_LEN - 1000 - 16, B_BASE + B_LEN)]
        self.stats = dict(eventSuccess=24, totalPackets=len(lens), totalBytes=int(self.lens.sum()), badHeaderDiscards=0,
                          dataErrCnt=1, enqueueLoss=0, reassemblyLoss=0, inProgress=2)

    def window(self, lo, hi):
        w = np.full(hi - lo, FILL, np.uint8)
        for at, b in self.writes:
            a, z = max(at, lo), min(at + len(b), hi)
            if a < z:
                w[a - lo:z - lo] = b[a - at:z - at]
        return w


_arena = {}


def _arena_case():
    if not _arena:
        _arena["case"] = _Arena()
    return _arena["case"]


def _arena_run(ctx, form):
    """The three launches in one form -> the reassembler, records still queued."""
    import torch
    from e2sar_amd import _capi, sar
    c = _arena_case()
    R = sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=256, queue_capacity=256, lost_capacity=64,
                              arena_bytes=ARENA, flags=_capi.REAS_REFERENCE_ORDER if form == "reforder" else 0)
    arena = R.arena_tensor()
    assert arena.numel() == ARENA
    for lo, hi in c.windows:
        arena[lo:hi].fill_(FILL)
    dpk = torch.from_numpy(np.concatenate([c.rows.reshape(-1), np.zeros(256, np.uint8)])).to(ctx.torch_device)
    dln = torch.from_numpy(c.lens.view(np.int32).copy()).to(ctx.torch_device)
    st = c.stride
    args = [(dpk[a * st:], dln[a:], n) for a, n in c.launches]
    if form in ("fused", "reforder"):
        for pk, ln, n in args:
            R.reassemble(pk, st, ln, n, now_ms=NOW)
    elif form == "dev":
        for pk, ln, n in args:
            R.reassemble_dev(pk, st, ln, torch.tensor([n], dtype=torch.int32, device=ctx.torch_device), now_ms=NOW)
    elif form == "split":
        for pk, ln, n in args:
            w = R.alloc_work(n)
            R.classify(pk, st, ln, n, w, now_ms=NOW)
            R.scatter(pk, st, n, w)
    else:
        works = [R.alloc_work(len(c.lens)) for _ in range(2)]
        R.classify(args[0][0], st, args[0][1], args[0][2], works[0], now_ms=NOW)
        for k, (pk, ln, n) in enumerate(args):
            if k + 1 < len(args):
                cpk, cln, cn = args[k + 1]
                R.scatter_classify(st, pk, n, works[k % 2], cpk, cln, cn, works[(k + 1) % 2], now_ms=NOW)
            else:
                R.scatter(pk, st, n, works[k % 2])
    torch.cuda.synchronize()
    return R


def _check_arena(R, recs, label):
    c = _arena_case()
    st = R.stats()
    assert {k: int(getattr(st, k)) for k in STATS} == c.stats, (label, st)
    assert st.errorFlags == 0, label
    assert sorted((r.eventNum, r.dataId) for r in recs) == sorted(c.events), label
    for rec in recs:
        key = (rec.eventNum, rec.dataId)
        assert rec.arenaOffset >= 7 * G and rec.arenaOffset % 256 == 0, (label, key, rec.arenaOffset)
        assert rec.bytes == len(c.events[key]) and rec.numFragments == c.frags[key], (label, key)
        assert R.event_bytes(rec) == c.events[key].tobytes(), (label, key)
    arena = R.arena_tensor()
    for lo, hi in c.windows:
        got = arena[lo:hi].cpu().numpy()
        bad = np.nonzero(got != c.window(lo, hi))[0]
        assert bad.size == 0, f"{label}: arena [{lo:#x}, {hi:#x}) differs at {[hex(lo + int(x)) for x in bad[:8]]}"


def _lost(R):
    R.gc(now_ms=NOW + 1000, timeout_ms=500)
    return sorted((r.eventNum, r.dataId, r.numFragments) for r in R.lost_poll())


@pytest.mark.parametrize("form", ARENA_FORMS)
def test_arena_above_4gib(hip, form):
    R = _arena_run(hip, form)
    _check_arena(R, R.poll(), form)
    # A took its creator, the fragment at 2^31 and the one that ends at its length; B two
    assert _lost(R) == [KEY_A + (3,), KEY_B + (2,)]
    st = R.stats()
    assert st.reassemblyLoss == 2 and st.inProgress == 0 and st.dataErrCnt == 1
    R.close()


def test_delivery_from_above_4gib(hip):
    """collect (ragged and rows), build with ids, relay_plan -> segment_device and copy_spans
    over records whose arenaOffset is above 7 GiB."""
    import torch
    from e2sar_amd import sar
    import test_gpu_build as TB
    import test_gpu_collect as TC
    c = _arena_case()
    R = _arena_run(hip, "fused")
    total = sum(len(b) for b in c.events.values())
    ragged = TC._Call(hip, R, total + 25 * 256, max_events=64)
    rows = TC._Call(hip, R, 24 * 4096, max_events=64, pitch=4096)
    built = TB._Call(hip, R, total + 25 * 256, ids=[IDS[2], IDS[0], IDS[1]], max_records=64)
    seg = sar.DeviceSegmenter(hip, mtu=MTU, lb_hdr_version=2)
    assert seg.max_pld == c.mp and seg.stride == c.stride
    nev, maxpk = 24, max(c.frags.values())
    desc = torch.zeros(nev * sar.SEG_EVENT_BYTES, dtype=torch.uint8, device=hip.torch_device)
    cnt = torch.zeros(2, dtype=torch.int32, device=hip.torch_device)
    opk, oln = seg.alloc_packets(nev * maxpk)
    tick, ent0 = 0x0123456789ABCDEF, 0xFFF0
    R.relay_plan(desc, cnt, 0, nev, seg.max_pld, tick, ent0)
    seg.segment_device(desc, cnt, nev, maxpk, opk, oln)
    torch.cuda.synchronize()
    recs = R.poll()
    _check_arena(R, recs, "delivery")
    src = c.events
    assert ragged.check(recs, src)[1][0] == 24
    assert rows.check(recs, src)[1][0] == 24
    w = built.check(recs, TB._by_key(src))
    assert w.counts[0] == 8 and w.counts[1] == 24 and all(int(m) == 0b111 for m in built.groups["presentMask"])
    # relay: descriptor i is record i, its datagrams the oracle's segmentation of the event
    n, tot = (int(x) for x in cnt.cpu().tolist())
    assert n == nev and tot == sum(c.frags.values())
    table = np.frombuffer(desc.cpu().numpy().tobytes(), sar.SEG_EVENT)[:n]
    gp = opk[: tot * seg.stride].view(tot, seg.stride).cpu().numpy()
    gl = oln[:tot].cpu().numpy().astype(np.uint32)
    base = 0
    for i, (t, rec) in enumerate(zip(table, recs)):
        assert int(t["data"]) == R.arena_ptr + rec.arenaOffset and int(t["pktBase"]) == base
        op, ol = O.segment_event(src[(rec.eventNum, rec.dataId)], rec.eventNum, rec.dataId, (ent0 + i) & 0xFFFF, tick, 2,
                                 seg.max_pld, seg.stride)
        np.testing.assert_array_equal(gl[base:base + len(ol)], ol)
        for k in range(len(ol)):
            assert np.array_equal(gp[base + k, :int(ol[k])], op[k, :int(ol[k])]), (i, k)
        base += len(ol)
    # copy_spans out of the arena, back to back
    out = torch.full((total + 64,), FILL, dtype=torch.uint8, device=hip.torch_device)
    spans, at = [], 0
    for rec in recs:
        spans.append((R.arena_ptr + rec.arenaOffset, out.data_ptr() + at, rec.bytes))
        at += rec.bytes
    hip.copy_spans(spans)
    torch.cuda.synchronize()
    want = np.concatenate([src[(r.eventNum, r.dataId)] for r in recs] + [np.full(64, FILL, np.uint8)])
    assert np.array_equal(out.cpu().numpy(), want)
    assert _lost(R) == [KEY_A + (3,), KEY_B + (2,)]
    R.close()


# ----------------------------------------------------------------------------------
# datagram slots above 4 GiB

STRIDE = 65520
NEV, NFR, PL = 4225, 16, 64
N = NEV * NFR                                    # 67 600 slots: 4.43 GB
FIRST_FAR = -(-(1 << 32) // STRIDE)              # the first slot wholly past 2^32
EV_BASE = 1 << 40
SLOT_ID = 5
SLOT_FORMS = ["fused", "split", "pipelined", "fused_cold", "split_cold", "dev"]


class _Slots:
    def __init__(self):
        rng = np.random.default_rng(0x51075)
        self.data = rng.integers(0, 256, (NEV, NFR * PL), dtype=np.uint8)
        rows = np.zeros((N, 128), np.uint8)
        for e in range(NEV):
            for j in range(NFR):
                rows[e * NFR + j] = RC.dgram(EV_BASE + e, SLOT_ID, j * PL, NFR * PL, self.data[e, j * PL:(j + 1) * PL],
                                             128, True)[0]
        self.rows = rows
        self.lens = np.full(N, 36 + PL, np.uint32)
        self.stats = dict(eventSuccess=NEV, totalPackets=N, totalBytes=N * (36 + PL), badHeaderDiscards=0, dataErrCnt=0,
                          enqueueLoss=0, reassemblyLoss=0, inProgress=0)


def _spread(ctx, rows):
    """[n, 128] host rows -> a device batch of n slots of STRIDE bytes, only the first 128 of each written."""
    import torch
    big = torch.empty(len(rows) * STRIDE + 256, dtype=torch.uint8, device=ctx.torch_device)
    big[: len(rows) * STRIDE].view(len(rows), STRIDE)[:, :128].copy_(torch.from_numpy(rows).to(ctx.torch_device))
    return big


@pytest.fixture(scope="module")
def slots(hip):
    import torch
    # slot 65 552 straddles 2^32; more than 2 000 slots lie wholly past it
    assert STRIDE * 65553 > 1 << 32 > STRIDE * 65552 and FIRST_FAR == 65553 and N - FIRST_FAR > 2000
    s = _Slots()
    s.dpk = _spread(hip, s.rows)
    s.dln = torch.from_numpy(s.lens.view(np.int32).copy()).to(hip.torch_device)
    yield s
    del s.dpk
    torch.cuda.empty_cache()


def _slot_reassembler(ctx, flags=0):
    from e2sar_amd import sar
    return sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=16384, queue_capacity=8192, lost_capacity=256,
                                 arena_bytes=(NEV + 64) * NFR * PL, flags=flags)


@pytest.mark.parametrize("form", SLOT_FORMS)
def test_slots_above_4gib(hip, slots, form):
    import torch
    kind, _, load = form.partition("_")
    R = _slot_reassembler(hip)
    if load:
        R.set_cold(True)
    dpk, dln = slots.dpk, slots.dln
    if kind == "fused":
        R.reassemble(dpk, STRIDE, dln, N, now_ms=NOW)               # split internally above 320 MiB
    elif kind == "dev":
        R.reassemble_dev(dpk, STRIDE, dln, torch.tensor([N], dtype=torch.int32, device=hip.torch_device), now_ms=NOW)
    elif kind == "split":
        w = R.alloc_work(N)
        R.classify(dpk, STRIDE, dln, N, w, now_ms=NOW)
        R.scatter(dpk, STRIDE, N, w)
    else:
        # the second batch is still addressed past 2^32 from its own first slot
        a = 1000
        assert N - a > FIRST_FAR + 1000
        works = [R.alloc_work(N) for _ in range(2)]
        R.classify(dpk, STRIDE, dln, a, works[0], now_ms=NOW)
        R.scatter_classify(STRIDE, dpk, a, works[0], dpk[a * STRIDE:], dln[a:], N - a, works[1], now_ms=NOW)
        R.scatter(dpk[a * STRIDE:], STRIDE, N - a, works[1])
    torch.cuda.synchronize()
    recs, st = R.poll(), R.stats()
    assert {k: int(getattr(st, k)) for k in STATS} == slots.stats, (form, st)
    assert st.errorFlags == 0
    arena = R.arena_tensor().cpu().numpy()
    seen = set()
    for rec in recs:
        e = rec.eventNum - EV_BASE
        assert 0 <= e < NEV and e not in seen and rec.dataId == SLOT_ID
        seen.add(e)
        assert rec.bytes == NFR * PL and rec.numFragments == NFR, (form, e, rec.numFragments)
        if not np.array_equal(arena[rec.arenaOffset:rec.arenaOffset + rec.bytes], slots.data[e]):
            raise AssertionError(f"{form}: event {e} (slots {e * NFR}..) differs")
    assert len(seen) == NEV
    R.close()


def test_slots_above_4gib_reference_order(hip, slots):
    """The slots past 2^32 shuffled; the last three hold second copies of fragments of events
    that are whole by then (each starts an item of its own), and the fragments they displace
    leave three events in progress.  Expected: the oracle over the compact rows."""
    import torch
    from e2sar_amd import _capi
    rnd = random.Random(4225)
    far = -(-FIRST_FAR // NFR) * NFR                         # the first event wholly past 2^32
    order = list(range(far, N))
    rnd.shuffle(order)
    first = {}
    for i, p in enumerate(order):                            # each event's offset 0 ahead of its other fragments
        first.setdefault(p // NFR, i)
    for i, p in enumerate(order):
        if p % NFR == 0 and first[p // NFR] != i:
            j = first[p // NFR]
            order[i], order[j] = order[j], order[i]
    rows = slots.rows.copy()
    rows[far:] = slots.rows[order]
    for k, e in enumerate((4200, 4210, 4220)):               # events wholly past 2^32
        rows[N - 1 - k] = slots.rows[e * NFR + 3 + k]
    assert all(e * NFR >= far for e in (4200, 4210, 4220))
    assert not RL.model(rows, slots.lens)[0]                 # no event completes with a hole
    r = O.Reassembler(True)
    r.set_time(NOW)
    r.push_batch(rows, slots.lens)
    ref = sorted((e, d, nf, b) for b, e, d, nf in r.pop_all_frags(1 << 12))
    rst = r.stats()
    r.set_time(NOW + 1000)
    r.gc(500)
    rlost = sorted(r.lost_pop_all())
    assert rst["eventSuccess"] == len(ref) >= NEV - 3 and rst["inProgress"] == len(rlost) >= 3
    dpk = _spread(hip, rows)
    R = _slot_reassembler(hip, flags=_capi.REAS_REFERENCE_ORDER)
    R.reassemble(dpk, STRIDE, slots.dln, N, now_ms=NOW)
    torch.cuda.synchronize()
    recs, st = R.poll(), R.stats()
    assert {k: int(getattr(st, k)) for k in STATS} == {k: int(rst[k]) for k in STATS}
    assert st.errorFlags == 0
    arena = R.arena_tensor().cpu().numpy()
    got = sorted((rec.eventNum, rec.dataId, rec.numFragments, arena[rec.arenaOffset:rec.arenaOffset + rec.bytes].tobytes())
                 for rec in recs)
    assert got == ref
    assert _lost(R) == rlost
    R.close()
    del dpk


def _index_of(rows):
    """Which datagram of the stream a routed slot holds, from its header."""
    ev = RR.event_nums_of(rows).astype(np.int64) - EV_BASE
    off = np.ascontiguousarray(rows[:, 20:24]).view(">u4")[:, 0].astype(np.int64)
    return ev * NFR + off // PL


def test_route_above_4gib(hip, slots):
    """route_batch, route_foreign and route_append at world 2: source slots and packed output
    both pass 4 GiB; compared slot by slot (the datagram's 100 bytes) with route_ref."""
    import torch
    from e2sar_amd.dist import PacketRouter, RegionRouter
    world, me = 2, 1
    ln = slots.lens
    dests = RR.route_dests(slots.rows, ln, STRIDE, world, me)
    assert sorted(np.unique(dests).tolist()) == [0, 1]
    L = 36 + PL
    router = PacketRouter(hip, STRIDE, N, world, me)
    for foreign_only in (False, True):
        router.send_ln.fill_(0x5A5A5A5A)
        router.counts.fill_(-1)
        spk, sln, cnt = router.route(slots.dpk, slots.dln, N, foreign_only=foreign_only)
        torch.cuda.synchronize()
        rpk, rln, rcounts = RR.stable_pack(slots.rows, ln, dests, world, me, foreign_only)
        k = len(rln)
        assert cnt.cpu().tolist() == rcounts and (k == N or foreign_only)
        got_ln = sln.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_ln[:k], rln) and (got_ln[k:] == 0x5A5A5A5A).all()
        got = spk[: N * STRIDE].view(N, STRIDE)[:k, :L].cpu().numpy()
        bad = np.nonzero((got != rpk[:, :L]).any(axis=1))[0]
        assert bad.size == 0, f"foreign_only={foreign_only}: {bad.size} packed slots differ, first {bad[:8].tolist()}"
    del router, spk
    torch.cuda.empty_cache()
    # route_append: region 1 begins at slot `cap` and ends past 2^32
    runs = RR.append_model(dests, world, me, False)
    cap = 34000
    assert max(len(np.concatenate(r)) for r in runs) <= cap and (cap + len(np.concatenate(runs[1]))) * STRIDE > 1 << 32
    reg = RegionRouter(hip, STRIDE, cap, N, world, me, foreign_only=False)
    reg.send_ln.fill_(0x5A5A5A5A)
    reg.route(slots.dpk, slots.dln, N)
    torch.cuda.synchronize()
    running = reg.running.cpu().tolist()
    for d in range(world):
        want = np.concatenate(runs[d])
        assert running[d] == len(want), (d, running)
        got = reg.send_pk[d * cap * STRIDE:(d * cap + running[d]) * STRIDE].view(running[d], STRIDE)[:, :128].cpu().numpy()
        idx = _index_of(got)
        assert sorted(idx.tolist()) == sorted(want.tolist()), f"region {d}"
        assert np.array_equal(got[:, :L], slots.rows[idx][:, :L]), f"region {d} slots"
        gl = reg.send_ln[d * cap:(d + 1) * cap].cpu().numpy().view(np.uint32)
        assert (gl[:running[d]] == L).all() and (gl[running[d]:] == 0x5A5A5A5A).all(), f"region {d} lens"
        at = {int(s): i for i, s in enumerate(idx)}
        for g in runs[d]:                                   # every block's run contiguous, in landing order
            i = at[int(g[0])]
            assert idx[i:i + len(g)].tolist() == g.tolist(), f"region {d}"
