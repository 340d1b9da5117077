"""The host model of e2sar_hip_rows_ready (tests/rows_ready_ref.py) on hand cases, and the
random family the GPU test runs: it must hold the steps it is there for (CPU only)."""
import numpy as np

import oracle_ffi as O
import reas_cuts as RC
import rows_ready_ref as M
import rows_ref as RR


def _one(ev, d, off, blen, n, byte=0x11):
    return RC.dgram(ev & RR.M64, d, off, blen, bytes([byte]) * n, 64, True)


def _window(dgrams, ids=(7, 9), n_events=8, pitch=256, base=0):
    w = RR.Window(ids, n_events, pitch, base)
    if dgrams:
        w.apply(np.stack([r for r, _ in dgrams]), np.array([n for _, n in dgrams], np.uint32), 64)
    return w


def _whole(ev, ids=(7, 9), n=16):
    return [_one(ev, d, 0, n, n) for d in ids]


def test_empty_window():
    w = _window([])
    words, events, out = M.ready(w, M.Rule(0, 0, 8, M.READY_ZERO))
    assert words == [0] * 8 and events == [] and (out == RR.FILL).all()


def test_prefix_of_complete_events_and_the_hole_behind_it():
    base = 2 ** 64 - 3
    w = _window(_whole(base) + _whole(base + 1) + [_one(base + 2, 7, 0, 16, 16)] + _whole(base + 3), base=base)
    words, events, _ = M.ready(w, M.Rule(0, M.NEVER, 8))
    assert words == [2, 2, 0, 4, 4, 0, 0, 0]
    assert [e.eventNum for e in events] == [2 ** 64 - 3, 2 ** 64 - 2] and [e.row for e in events] == [5, 6]
    assert all(e.flags == M.EV_COMPLETE and e.presentMask == e.openMask == 3 for e in events)
    # the hole is one event behind the horizon's last: slack 1 gives it up, slack 2 waits
    assert M.ready(w, M.Rule(0, 2, 8))[0][0] == 2
    words, events, _ = M.ready(w, M.Rule(0, 1, 8))
    assert words == [4, 3, 1, 4, 7, 0, 0, 0]
    assert events[2] == M.Event(2 ** 64 - 1, 1, 1, 7, M.EV_GIVEN_UP) and events[3].eventNum == 0 and events[3].row == 0
    # only id 7 required: the hole is whole
    assert M.ready(w, M.Rule(1, M.NEVER, 8))[0][:3] == [4, 4, 0]
    # kMax cuts
    assert M.ready(w, M.Rule(0, 1, 3))[0][:3] == [3, 2, 1] and M.ready(w, M.Rule(0, 1, 0))[0] == [0, 0, 0, 4, 0, 0, 0, 0]


def test_slack_distances():
    # events 0..3 empty, 4 open and incomplete: H = 5; event i is 4 - i behind the newest, and
    # event 4 itself 0 behind: only slack 0 gives it up
    for slack, want in [(0, 5), (3, 2), (4, 1), (5, 0), (M.NEVER, 0)]:
        w = _window([_one(4, 7, 0, 32, 16)], ids=(7,))
        words, events, _ = M.ready(w, M.Rule(0, slack, 8))
        assert words[0] == want and words[3] == 5, (slack, words)
        assert words[5] == (1 if want == 5 else 0)
        assert all(e.flags == M.EV_GIVEN_UP for e in events)


def test_zeroing_and_what_is_kept():
    dg = [_one(0, 7, 0, 17, 17, byte=0x21), _one(0, 9, 0, 300, 28, byte=0x22),      # short whole cell; open incomplete cell
          _one(1, 7, 0, 16, 16, byte=0x23)]                                           # event 1: id 9 empty -> waited for
    w = _window(dg)
    before = w.out.copy()
    words, events, out = M.ready(w, M.Rule(0, 1, 8, M.READY_ZERO))
    assert words == [1, 0, 1, 2, 1, 1, 0, 0] and events[0].flags == M.EV_GIVEN_UP
    assert (out[0, 0, :17] == 0x21).all() and (out[0, 0, 17:] == 0).all() and (out[0, 1] == 0).all()
    assert (out[1:] == before[1:]).all() and (w.out == before).all()
    assert (M.ready(w, M.Rule(0, 1, 8))[2] == before).all()
    # a truncated whole cell keeps its pitch bytes
    w = _window([_one(0, 7, 0, 300, 28), _one(0, 7, 28, 300, 28)] + [_one(0, 7, o, 300, min(28, 300 - o)) for o in range(56, 300, 28)],
                ids=(7,))
    words, events, out = M.ready(w, M.Rule(0, M.NEVER, 8, M.READY_ZERO))
    assert words[:2] == [1, 1] and events[0].flags == M.EV_COMPLETE | M.EV_TRUNCATED and (out[0] == 0x11).all()


def test_rule_checks():
    w = _window([])
    assert M.check_rule(w, M.Rule(3, 0, 1, 1)) and not M.check_rule(w, M.Rule(4, 0, 1, 0)) and not M.check_rule(w, M.Rule(0, 0, 1, 2))


def test_random_family_holds_what_it_is_for():
    assert O.max_pld_len(100) == M.MAX_PLD and M.STRIDE == (36 + M.MAX_PLD + 15) // 16 * 16
    seen = dict.fromkeys(["k0 behind a hole within slack", "given up in the prefix", "cut by kMax", "short whole cell",
                          "open incomplete cell in a ready event"], 0)

    def step(w, rule, batch, words, events, out):
        k, H = words[0], words[3]
        N = w.n_events
        if k == 0 and H > 0 and H - 1 < rule.slack:
            seen["k0 behind a hole within slack"] += 1
        if words[2]:
            seen["given up in the prefix"] += 1
        if k == rule.k_max < N:
            nxt = M.ready(w, rule._replace(k_max=N))[0][0]
            seen["cut by kMax"] += nxt > k
        nid = len(w.ids)
        for e in events:
            for j in range(nid):
                if e.presentMask >> j & 1 and w.bytes[e.row * nid + j] < w.pitch:
                    seen["short whole cell"] += 1
            if e.openMask & ~e.presentMask:
                seen["open incomplete cell in a ready event"] += 1

    for seed in M.SEEDS:
        M.run_family(seed, step)
    assert all(seen.values()), seen
