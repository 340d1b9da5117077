"""The route kernels (e2sar_amd/csrc/route.hpp) against the host model in route_ref.py, at
the shapes where routing is more than the identity: many workgroups, the scan's tile loop
(above 65 536 datagrams), worlds up to 64, both header forms, datagrams that stay home,
64-bit event numbers, slots wider than a pack slice, and route_append's region contract
with and without overflow.

Every comparison is exact.  Send buffers and lens are filled with a sentinel before each
launch and every slot the model leaves unused must still hold it afterwards.
"""
import numpy as np
import pytest

import oracle_ffi as O
import route_ref as RR

pytestmark = pytest.mark.gpu

SENT_B = 0xA5
SENT_L = 0x5A5A5A5A


def _torch():
    import torch
    return torch


def _upload(ctx, pk, ln):
    torch = _torch()
    dpk = torch.from_numpy(np.ascontiguousarray(pk).reshape(-1)).to(ctx.torch_device)
    dln = torch.from_numpy(np.ascontiguousarray(ln, np.uint32).view(np.int32)).to(ctx.torch_device)
    return dpk, dln


def _same_rows(got, want, what):
    """Exact equality of two [slots, width] arrays; names the first wrong slots."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} slots differ, first {bad[:8].tolist()}")


def _random_lens(n, stride, with_lb, seed):
    hl = 36 if with_lb else 20
    return np.random.default_rng(seed).integers(hl, stride + 1, n).astype(np.uint32)


def _events_for(dests, world, seed):
    """Event numbers spread over all 64 bits whose owner is dests[k]."""
    hi = np.random.default_rng(seed).integers(0, (2**64 - world) // world, len(dests), dtype=np.uint64,
                                              endpoint=True)
    return hi * np.uint64(world) + np.asarray(dests).astype(np.uint64)


def _check_packed(ctx, pk, ln, stride, world, self_rank, with_lb=True):
    """route_batch and route_foreign of one batch == stable_pack: counts, lens, whole slots,
    and the sentinel everywhere behind the packed spans."""
    from e2sar_amd.dist import PacketRouter
    torch = _torch()
    n = len(ln)
    dests = RR.route_dests(pk, ln, stride, world, self_rank, with_lb)
    dpk, dln = _upload(ctx, pk, ln)
    for foreign_only in (False, True):
        router = PacketRouter(ctx, stride, n, world, self_rank, with_lb)
        router.send_pk.fill_(SENT_B)
        router.send_ln.fill_(SENT_L)
        router.counts.fill_(-1)
        spk, sln, cnt = router.route(dpk, dln, n, foreign_only=foreign_only)
        torch.cuda.synchronize()
        rpk, rln, rcounts = RR.stable_pack(pk, ln, dests, world, self_rank, foreign_only)
        k = len(rln)
        assert k == (n - int((dests == self_rank).sum()) if foreign_only else n)
        assert cnt.cpu().tolist() == rcounts, ("foreign" if foreign_only else "batch")
        want_ln = np.full(n, SENT_L, np.uint32)
        want_ln[:k] = rln
        _same_rows(sln.cpu().numpy().view(np.uint32).reshape(n, 1), want_ln.reshape(n, 1),
                   f"lens (foreign_only={foreign_only})")
        want_pk = np.full((n, stride), SENT_B, np.uint8)
        want_pk[:k] = rpk
        _same_rows(spk.cpu().numpy().reshape(n, stride), want_pk, f"slots (foreign_only={foreign_only})")
    _same_rows(dpk.cpu().numpy().reshape(n, stride), pk, "the landed batch itself")
    return dests


# ----------------------------------------------------------------------------------
# a. route_batch / route_foreign against stable_pack

def _pack_cases():
    cases = []
    # around one workgroup, and several: every small world, both kinds of event numbers
    for i, n in enumerate([1, 255, 256, 257, 1000]):
        for j, world in enumerate([2, 3, 8]):
            cases.append((n, 48, world, (i + 2 * j) % world, True, "edge" if (i + j) % 2 else "uniform"))
    # 258 blocks = one full scan tile + 2, and 513 = two full tiles + 1
    for n in (65793, 131073):
        for world in (7, 64):
            for self_rank in (0, world // 2, world - 1):
                cases.append((n, 48, world, self_rank, True, "uniform" if self_rank else "edge"))
    # wide slots (MTU 1500 and jumbo: 92 and 561 chunks), where div_recip sees its largest
    # operands.  The pack slice boundary nch / 2 falls inside a datagram only in a block
    # with an odd number of datagrams: 700 and 600 end in even blocks, 701 and 601 in odd ones
    cases.append((700, 1472, 3, 1, True, "uniform"))
    cases.append((600, 8976, 3, 2, True, "edge"))
    cases.append((701, 1472, 3, 0, True, "edge"))
    cases.append((601, 8976, 3, 1, True, "uniform"))
    # RE header at offset 0
    cases.append((1000, 48, 3, 1, False, "edge"))
    cases.append((700, 1472, 7, 4, False, "uniform"))
    return cases


@pytest.mark.parametrize("n,stride,world,self_rank,with_lb,events", _pack_cases())
def test_route_pack_matches_model(hip, n, stride, world, self_rank, with_lb, events):
    ev = RR.edge_event_nums(n) if events == "edge" else RR.uniform_event_nums(n, seed=n + world)
    pk, ln = RR.make_datagrams(n, stride, ev, with_lb, seed=n ^ stride ^ world,
                               ln=_random_lens(n, stride, with_lb, seed=n + 1))
    dests = _check_packed(hip, pk, ln, stride, world, self_rank, with_lb)
    if n >= 1000:                                     # the case routes to every rank
        assert len(np.unique(dests)) == world
    if n in (701, 601):                               # the last block's slice boundary splits a datagram
        assert (n % RR.BLOCK * (stride // 16) // 2) % (stride // 16) != 0


# ----------------------------------------------------------------------------------
# b. skewed and degenerate batches

def _skewed(kind, n, world):
    rng = np.random.default_rng(21)
    if kind == "one_destination":
        return np.full(n, 5)
    if kind == "one_rank_gets_nothing":
        d = rng.integers(0, world - 1, n)
        return np.where(d >= 3, d + 1, d)                         # every rank but 3
    if kind == "per_wave":
        return np.repeat(rng.integers(0, world, (n + 63) // 64), 64)[:n]
    if kind == "per_datagram":
        return np.arange(n) % world
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["one_destination", "one_rank_gets_nothing", "per_wave", "per_datagram"])
def test_route_skewed_batches(hip, kind):
    n, stride, world, self_rank = 2000, 48, 8, 2
    dests = _skewed(kind, n, world)
    pk, ln = RR.make_datagrams(n, stride, _events_for(dests, world, seed=5), seed=6,
                               ln=_random_lens(n, stride, True, seed=7))
    got = _check_packed(hip, pk, ln, stride, world, self_rank)
    assert got.tolist() == dests.tolist()
    counts = np.bincount(got, minlength=world)
    if kind == "one_destination":
        assert counts[5] == n
    if kind == "one_rank_gets_nothing":
        assert counts[3] == 0 and (np.delete(counts, 3) > 0).all()
    if kind == "per_wave":
        waves = got[: n // 64 * 64].reshape(-1, 64)
        assert (waves == waves[:, :1]).all() and len(np.unique(waves[:, 0])) == world


def test_route_nothing_parses(hip):
    # everything stays on self: route_batch is the identity, route_foreign packs and writes nothing
    n, stride, world, self_rank = 2000, 48, 8, 6
    pk, ln = RR.make_datagrams(n, stride, RR.uniform_event_nums(n, 9), seed=10)
    pk[:, 16] = 0x20
    dests = _check_packed(hip, pk, ln, stride, world, self_rank)
    assert (dests == self_rank).all()


# ----------------------------------------------------------------------------------
# c. datagrams that stay home

def test_route_unparsable_datagrams_stay_home(hip):
    from e2sar_amd.dist import PacketRouter
    n, stride, world, self_rank = 600, 48, 5, 3
    ev = RR.edge_event_nums(n)
    ev[n // 2:] = RR.uniform_event_nums(n - n // 2, 31)
    pk, ln = RR.make_datagrams(n, stride, ev, seed=32, ln=_random_lens(n, stride, True, seed=33))
    cand = np.arange(3, n, 7)
    for j, k in enumerate(cand):
        kind = j % 5
        if kind == 0:
            ln[k] = 35
        elif kind == 1:
            ln[k] = 0
        elif kind == 2:
            ln[k] = stride + 1
        elif kind == 3:
            pk[k, 16] = 0x20                          # version nibble
        else:
            pk[k, 17] = 0x01                          # reserved byte
    # every one of them would go elsewhere if it parsed, so the test sees it stay
    foreign = (RR.event_nums_of(pk) % np.uint64(world)).astype(np.int64) != self_rank
    home = cand[foreign[cand]]
    assert len(home) > 50 and set((np.arange(len(cand)) % 5)[foreign[cand]].tolist()) == {0, 1, 2, 3, 4}
    dests = _check_packed(hip, pk, ln, stride, world, self_rank)
    assert (dests[home] == self_rank).all()
    # said once more without the model's packing: counted for self, absent from the foreign spans
    torch = _torch()
    dpk, dln = _upload(hip, pk, ln)
    router = PacketRouter(hip, stride, n, world, self_rank)
    spk, sln, cnt = router.route(dpk, dln, n)
    torch.cuda.synchronize()
    counts = cnt.cpu().tolist()
    owned = int((~foreign).sum())
    assert counts[self_rank] == owned + len(home)
    a = sum(counts[:self_rank])
    span = RR.stamp_of(spk.cpu().numpy().reshape(n, stride)[a:a + counts[self_rank]])
    assert set(home.tolist()) <= set(span.tolist())
    spk, sln, cnt = router.route(dpk, dln, n, foreign_only=True)
    torch.cuda.synchronize()
    counts = cnt.cpu().tolist()
    assert counts[self_rank] == 0 and sum(counts) == n - owned - len(home)
    packed = RR.stamp_of(spk.cpu().numpy().reshape(n, stride)[: sum(counts)])
    assert not set(home.tolist()) & set(packed.tolist())


# ----------------------------------------------------------------------------------
# d / e. route_append: the region contract, and overflow

def _append(ctx, pk, ln, cuts, stride, cap, world, self_rank, foreign_only):
    """Route pk[cuts[i]:cuts[i+1]] as successive batches into one RegionRouter (sentinel
    filled); -> (rows[world, cap, stride], lens[world, cap], running)."""
    from e2sar_amd.dist import RegionRouter
    torch = _torch()
    dpk, dln = _upload(ctx, pk, ln)
    router = RegionRouter(ctx, stride, cap, max(b - a for a, b in zip(cuts[:-1], cuts[1:])), world, self_rank,
                          foreign_only=foreign_only)
    router.send_pk.fill_(SENT_B)
    router.send_ln.fill_(SENT_L)
    assert router.running.cpu().tolist() == [0] * world
    for a, b in zip(cuts[:-1], cuts[1:]):
        router.route(dpk[a * stride:], dln[a:], b - a)          # raises unless the status is 0
    torch.cuda.synchronize()
    return (router.send_pk.cpu().numpy().reshape(world, cap, stride),
            router.send_ln.cpu().numpy().view(np.uint32).reshape(world, cap), router.running.cpu().tolist())


def _check_region(rows, lens, count, want, pk, ln, batch_of, block_of, what):
    """A region that did not overflow: its first `count` slots are exactly the datagrams
    `want` (indices), whole, lens slot by slot; each (batch, block) run contiguous and
    ascending; batches in order; the sentinel behind."""
    st = RR.stamp_of(rows[:count])
    assert sorted(st.tolist()) == sorted(want.tolist()), what
    _same_rows(rows[:count], pk[st], what + " slots")
    assert lens[:count].tolist() == ln[st].tolist(), what
    g = batch_of[st] * (1 << 20) + block_of[st]
    if count:
        assert int((g[1:] != g[:-1]).sum()) + 1 == len(np.unique(g)), what + ": a block's run is split"
        assert (st[1:] > st[:-1])[g[1:] == g[:-1]].all(), what + ": order lost inside a block's run"
        assert (np.diff(batch_of[st]) >= 0).all(), what + ": batches out of order"
    assert (rows[count:] == SENT_B).all(), what + ": store past the appended datagrams"
    assert (lens[count:] == SENT_L).all(), what + ": lens store past the appended datagrams"


def _batches(cuts, n):
    batch_of = np.zeros(n, np.int64)
    block_of = np.zeros(n, np.int64)
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        batch_of[a:b] = i
        block_of[a:b] = np.arange(b - a) // RR.BLOCK
    return batch_of, block_of


@pytest.mark.parametrize("foreign_only", [True, False])
@pytest.mark.parametrize("world,self_rank", [(2, 1), (5, 2), (64, 40)])
def test_route_append_contract(hip, world, self_rank, foreign_only):
    stride, cuts = 48, [0, 700, 701, 2001]
    n = cuts[-1]
    cap = n + 7
    ev = RR.uniform_event_nums(n, seed=world)
    ev[::3] = RR.edge_event_nums(n)[::3]
    pk, ln = RR.make_datagrams(n, stride, ev, seed=40 + world, ln=_random_lens(n, stride, True, seed=41))
    dests = RR.route_dests(pk, ln, stride, world, self_rank)
    rows, lens, running = _append(hip, pk, ln, cuts, stride, cap, world, self_rank, foreign_only)
    batch_of, block_of = _batches(cuts, n)
    # the model's runs, batch by batch
    runs = [[] for _ in range(world)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        for d, groups in enumerate(RR.append_model(dests[a:b], world, self_rank, foreign_only)):
            runs[d] += [a + g for g in groups]
    for d in range(world):
        want = np.concatenate(runs[d]) if runs[d] else np.zeros(0, np.int64)
        assert running[d] == len(want), (d, running)
        _check_region(rows[d], lens[d], running[d], want, pk, ln, batch_of, block_of, f"region {d}")
        # every run of the model is one of the region's runs
        st = RR.stamp_of(rows[d][: running[d]])
        at = {int(s): i for i, s in enumerate(st)}
        for g in runs[d]:
            i = at[int(g[0])]
            assert st[i:i + len(g)].tolist() == g.tolist(), f"region {d}"
    assert (running[self_rank] == 0) == foreign_only
    assert sum(running) == n - (int((dests == self_rank).sum()) if foreign_only else 0)


@pytest.mark.parametrize("self_rank,foreign_only", [(0, False), (3, True)])
def test_route_append_overflow_is_counted_not_written(hip, self_rank, foreign_only):
    # region 2 overflows in the first batch; regions 1 and 3 on either side of it do not.
    # With (3, True) region 3 stays empty, so a single store one slot past region 2 shows.
    stride, world, cap, cuts = 48, 4, 300, [0, 2000, 2500]
    n = cuts[-1]
    rng = np.random.default_rng(50)
    dests = np.concatenate([rng.permutation(np.repeat([0, 1, 2, 3], [270, 265, 1200, 265])),
                            rng.permutation(np.repeat([0, 1, 2, 3], [20, 20, 440, 20]))])
    pk, ln = RR.make_datagrams(n, stride, _events_for(dests, world, seed=51), seed=52,
                               ln=_random_lens(n, stride, True, seed=53))
    assert RR.route_dests(pk, ln, stride, world, self_rank).tolist() == dests.tolist()
    rows, lens, running = _append(hip, pk, ln, cuts, stride, cap, world, self_rank, foreign_only)
    batch_of, block_of = _batches(cuts, n)
    want = [290, 285, 1640, 285]
    if foreign_only:
        want[self_rank] = 0
    assert running == want and running[2] > cap
    # the region that overflowed: cap distinct datagrams of rank 2, all from the first batch
    st = RR.stamp_of(rows[2])
    assert ((st >= 0) & (st < cuts[1])).all(), "region 2 holds something that is no first-batch datagram"
    assert len(set(st.tolist())) == cap
    assert (dests[st] == 2).all()
    _same_rows(rows[2], pk[st], "region 2 slots")
    assert lens[2].tolist() == ln[st].tolist()
    # the others: exactly their own datagrams, the sentinel behind them
    for d in (0, 1, 3):
        own = np.nonzero(dests == d)[0] if want[d] else np.zeros(0, np.int64)
        _check_region(rows[d], lens[d], running[d], own, pk, ln, batch_of, block_of, f"region {d}")


# ----------------------------------------------------------------------------------
# f. the router and the reassembler agree on who owns an event

def _owner_batch():
    """15 events of sizes around the fragment boundaries, event numbers at and above 2^32,
    segmented by the oracle; each event's first fragment first, the rest shuffled; one
    datagram made unparsable."""
    sizes = [1, 1436, 1437, 5000, 20000] * 3
    nums = [2**32 - 1, 2**32] + [2**40 + k for k in range(6)] + [2**64 - 1 - k for k in range(7)]
    mp = O.max_pld_len(1500)
    stride = (36 + mp + 15) // 16 * 16
    rng = np.random.default_rng(60)
    pks, lns, starts, at = [], [], [], 0
    for i, (size, ev) in enumerate(zip(sizes, nums)):
        p, l = O.segment_event(rng.integers(0, 256, size, dtype=np.uint8), ev, 4321, 1 + i, (1 << 48) + i, 2, mp, stride)
        pks.append(p)
        lns.append(l)
        starts.append(at)
        at += len(l)
    pk, ln = np.concatenate(pks), np.concatenate(lns)
    rest = [k for k in range(at) if k not in starts]
    rng.shuffle(rest)
    order = starts + rest
    pk, ln = pk[order].copy(), ln[order].copy()
    pk[at // 2, 16] = 0x20
    return pk, ln, stride


@pytest.mark.parametrize("world", [3, 7, 64])
def test_router_and_reassembler_agree_on_ownership(hip, world):
    from e2sar_amd import sar
    from e2sar_amd.dist import PacketRouter
    from test_gpu_parity import _check_reas, _reas_oracle
    torch = _torch()
    pk, ln, stride = _owner_batch()
    n = len(ln)
    owners = set((RR.event_nums_of(pk) % np.uint64(world)).tolist())
    dpk, dln = _upload(hip, pk, ln)
    # an owner of some event, the last rank, and a rank in between
    for r in sorted({min(owners), world // 2, world - 1}):
        dests = RR.route_dests(pk, ln, stride, world, r)
        keep = dests == r
        ref, rst, _ = _reas_oracle(pk[keep], ln[keep], True)
        R = sar.DeviceReassembler(hip, with_lb_header=True, table_slots=256, arena_bytes=1 << 24)
        R.set_owner(world, r)
        R.reassemble(dpk, stride, dln, n)
        router = PacketRouter(hip, stride, n, world, r)
        router.send_pk.fill_(SENT_B)
        router.send_ln.fill_(SENT_L)
        spk, sln, cnt = router.route(dpk, dln, n, foreign_only=True)
        torch.cuda.synchronize()
        got = {(x.eventNum, x.dataId): (R.event_bytes(x), x.numFragments) for x in R.poll()}
        st = R.stats()
        _check_reas(got, st, ref, rst)
        assert st.badHeaderDiscards == 1 and st.errorFlags == 0
        counts = cnt.cpu().tolist()
        rpk, rln, rcounts = RR.stable_pack(pk, ln, dests, world, r, True)
        assert counts == rcounts
        k = sum(counts)
        _same_rows(spk.cpu().numpy().reshape(n, stride)[:k], rpk, f"rank {r} foreign spans")
        assert (spk.cpu().numpy().reshape(n, stride)[k:] == SENT_B).all()
        # kept and packed datagrams partition the batch.  totalPackets counts every datagram
        # the reassembler took, the unparsable one among them (as the reference does,
        # e2sarDPReassembler.cpp:332), so badHeaderDiscards is part of it, not beside it
        assert st.totalPackets + k == n
        assert st.totalPackets == int(keep.sum()) and k == int((~keep).sum())
        assert st.totalPackets - st.badHeaderDiscards == int((keep & (np.arange(n) != n // 2)).sum())