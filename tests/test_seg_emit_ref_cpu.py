"""The host model of e2sar_hip_seg_emit's plan (tests/seg_emit_ref.py), pinned on hand-cut
cases and against seg_ref's packet counts and make_events' pktBase prefix.  CPU only."""
import numpy as np
import pytest

import seg_emit_ref as E
import seg_ref as M


def test_all_taken_by_hand():
    # maxPld 10: 0, 1, 10, 11, 25 bytes -> 0, 1, 1, 2, 3 datagrams
    p = E.plan([0, 1, 10, 11, 25], 10, 7, 1000, pitch=100)
    assert p.counts == [5, 7, 0, 0]
    assert p.events["pktBase"].tolist() == [0, 0, 1, 2, 4]
    assert p.events["off"].tolist() == [0, 100, 200, 300, 400]


def test_capacity_cut_by_hand():
    # one slot short: the 25-byte event does not fit, and the 1-byte event behind it is not taken
    p = E.plan([0, 1, 10, 11, 25, 1], 10, 6, 1000, pitch=100)
    assert p.counts == [4, 4, 2, 1]
    # no slot at all: leading empty events are taken, they need none
    assert E.plan([0, 0, 3, 0], 10, 0, 1000, pitch=100).counts == [2, 0, 2, 1]
    assert E.plan([3], 10, 0, 1000, pitch=100).counts == [0, 0, 1, 1]


def test_source_bounds_by_hand():
    # a row longer than its pitch ends the batch, whatever follows
    assert E.plan([5, 101, 5], 10, 99, 1000, pitch=100).counts == [1, 1, 2, 2]
    assert E.plan([5, 100, 5], 10, 99, 1000, pitch=100).counts == [3, 12, 0, 0]
    # ragged: the end of an event may touch dataBytes, not pass it
    offs = np.array([0, 40, 90], np.uint64)
    assert E.plan([40, 50, 10], 10, 99, 100, offsets=offs).counts == [3, 10, 0, 0]
    assert E.plan([40, 50, 11], 10, 99, 100, offsets=offs).counts == [2, 9, 1, 2]
    # an offset near 2^64 must not wrap into the source
    offs = np.array([0, 2**64 - 4], np.uint64)
    assert E.plan([8, 8], 10, 99, 100, offsets=offs).counts == [1, 1, 1, 2]
    # rows past the end of the source: the available count is cut, the reason says why
    assert E.plan([5, 5, 5, 5], 10, 99, 250, pitch=100).counts == [2, 2, 0, 2]
    assert E.plan([5, 5, 5, 5], 10, 99, 250, pitch=100, count=2).counts == [2, 2, 0, 0]
    # an earlier cut keeps its own reason
    assert E.plan([5, 5, 5, 5], 10, 1, 250, pitch=100).counts == [1, 1, 1, 1]


def test_count_by_hand():
    L = [5, 5, 5, 5]
    assert E.plan(L, 10, 99, 1000, pitch=100, count=0).counts == [0, 0, 0, 0]
    assert E.plan(L, 10, 99, 1000, pitch=100, count=3).counts == [3, 3, 0, 0]
    assert E.plan(L, 10, 99, 1000, pitch=100, count=9).counts == [4, 4, 0, 0]       # clamped to maxEvents
    assert E.plan(L, 10, 99, 1000, pitch=100, count=9, max_events=2).counts == [2, 2, 0, 0]
    assert E.plan(L, 10, 99, 1000, pitch=100, count=None).counts == [4, 4, 0, 0]


def test_numbering_by_hand():
    num = E.Numbering(event_num_base=2**64 - 2, lb_tick_base=2**64 - 5, lb_tick_step=3, data_id=0x1234,
                      entropy_base=0xFFFE)
    ev = E.plan([1, 1, 1, 1], 10, 99, 1000, pitch=100, num=num).events
    assert ev["eventNum"].tolist() == [2**64 - 2, 2**64 - 1, 0, 1]
    assert ev["lbTick"].tolist() == [2**64 - 5, 2**64 - 2, 1, 4]
    assert ev["entropy"].tolist() == [0xFFFE, 0xFFFF, 0, 1]
    assert ev["dataId"].tolist() == [0x1234] * 4
    num.ticks_as_event_num = True
    ev = E.plan([1, 1, 1, 1], 10, 99, 1000, pitch=100, num=num).events
    assert ev["eventNum"].tolist() == ev["lbTick"].tolist()
    nums = np.array([7, 2**63, 9, 2**64 - 1], np.uint64)
    ev = E.plan([1, 1, 1, 1], 10, 99, 1000, pitch=100, num=E.Numbering(event_nums=nums)).events
    assert ev["eventNum"].tolist() == nums.tolist()


@pytest.mark.parametrize("max_pld", [1, 12, 1436, 8936])
def test_against_seg_ref(max_pld):
    """Over the subset matrix: the datagram total is seg_ref.num_packets' sum, and pktBase is
    make_events' prefix, for every capacity cut."""
    lens = [1, 5, 12, 13, 17, max_pld - 1, max_pld, max_pld + 1, 3 * max_pld - 1, 3 * max_pld + 1]
    cases = M.matrix_cases(max_pld, [n for n in lens if n > 0])
    offs, lengths, need = M.pack_events(cases)
    want = M.make_events(offs, lengths, max_pld)
    npk = M.num_packets(lengths, max_pld)
    total = int(npk.sum())
    p = E.plan(lengths, max_pld, total, need, offsets=offs)
    assert p.counts == [len(cases), total, 0, 0]
    assert (p.events["pktBase"] == want["pktBase"]).all() and (p.events["off"] == offs).all()
    ends = np.cumsum(npk)
    for cap in (0, 1, total // 2, total - 1):
        p = E.plan(lengths, max_pld, cap, need, offsets=offs)
        n = int(np.searchsorted(ends, cap, side="right"))          # events whose end is <= cap
        assert p.counts == [n, int(ends[n - 1]) if n else 0, len(cases) - n, 1]
        assert (p.events["pktBase"] == want["pktBase"][:n]).all()


def test_unit_search_never_picks_an_empty_event():
    rng = np.random.default_rng(5)
    for spc, uc in ((3, 512), (92, 512), (92, 1024)):
        lengths = rng.integers(0, 3000, 300) * (rng.random(300) < 0.6)      # 40 % empty, also first and last
        lengths[[0, 1, 150, 298, 299]] = 0
        first = E.first_units(lengths, 12, spc, uc)
        npk = M.num_packets(lengths, 12)
        seen = np.zeros(len(lengths), np.int64)
        for p in range(int(first[-1])):
            e = E.event_of_unit(first, p)
            assert lengths[e] > 0 and first[e] <= p < first[e + 1]
            assert (p - int(first[e])) * uc < int(npk[e]) * spc
            seen[e] += 1
        assert (seen == np.diff(first.astype(np.int64))).all()             # every unit of every event, once
