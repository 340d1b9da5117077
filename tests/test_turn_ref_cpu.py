"""tests/turn_ref.py against the CPU oracle, and the preconditions tests/test_gpu_turn.py leans
on: that the stream fits the GPU test's small arena, table and queue only because it is turned,
that events straddle the turns, age out, and complete after having been carried.  No GPU.

These are conditions on the inputs, not measurements: if a seed fails one, the seed changes,
not the bound."""
import pytest

import turn_ref as T

CARRIES = [0, 1, 2, T.NEVER]


@pytest.fixture(scope="module")
def s():
    return T.stream()


@pytest.fixture(scope="module")
def runs(s):
    return {m: T.run(s, m) for m in CARRIES}


def test_stream_shape(s):
    mp = T.max_pld()
    assert mp == 136 and T.lengths() == [1, 135, 136, 137, 255, 256, 257, 4095, 4097, 9999]
    assert len(s.cuts) == T.K_BATCHES + 1 and s.cuts[-1] == len(s.ln) == len(s.frags)
    assert all(0 < b - a <= T.BATCH_MAX for a, b in zip(s.cuts, s.cuts[1:]))
    seen, batches = {}, {}
    for b in range(T.K_BATCHES):
        for p in range(s.cuts[b], s.cuts[b + 1]):
            f = s.frags[p]
            assert (f.off == 0) == (f.key not in seen), "offset 0 first"
            assert f.off > seen.get(f.key, -1), "in order, no duplicates"
            seen[f.key] = f.off
            batches.setdefault(f.key, set()).add(b)
    assert set(seen) == set(s.events) and len(s.events) == T.N_EVENTS
    for key, bs in batches.items():
        assert 1 <= len(bs) <= 3 and max(bs) - min(bs) == len(bs) - 1, "1 to 3 consecutive batches"
    assert {len(bs) for bs in batches.values()} == {1, 2, 3}
    # about one in eight lacks a fragment
    assert T.N_EVENTS // 10 <= len(s.missing) <= T.N_EVENTS // 6
    for key in s.missing:
        got = sum(f.plen for f in s.frags if f.key == key)
        assert 0 < len(s.events[key]) - got <= mp


def test_slot_hash_spreads():
    # the copy of reas_table.hpp's slot_hash: pinned values (a 64-bit finaliser of pair_hash)
    assert T.slot_hash(0, 0, 63) == 0
    assert [T.slot_hash(ev, 4321, 63) for ev in (1, 2, 3)] == [T.slot_hash(ev, 4321, 0xFFFFFFFF) & 63 for ev in (1, 2, 3)]
    assert len({T.slot_hash(ev, 1, 63) for ev in range(1000, 1064)}) > 32


@pytest.mark.parametrize("m", CARRIES)
def test_model_equals_oracle(s, runs, m):
    run = runs[m]
    delivered, collected, stats, lost = T.replay_oracle(s, m)
    for b, step in enumerate(run.steps):
        assert step.delivered == delivered[b], b
        assert len(step.lost) == collected[b], b
        assert step.status == [1, len(step.carried), len(step.lost), step.after_turn["arenaUsed"]]
    assert {f: int(v) for f, v in stats.items()} == run.stats_once
    assert sorted(lost) == sorted(r[:3] for r in run.lost_once)
    # with two carries or more no key is collected twice: the device and the reference agree outright
    assert run.twice == (m < 2)
    if not run.twice:
        assert run.stats == run.stats_once and run.lost == run.lost_once
    # each event delivered once over the run
    keys = [k for step in run.steps for k in step.delivered]
    assert len(keys) == len(set(keys))
    if m >= 2:
        assert set(keys) == set(s.events) - s.missing


@pytest.mark.parametrize("m", CARRIES)
def test_the_run_fits_the_gpu_tests_reassembler(s, runs, m):
    for b, step in enumerate(runs[m].steps):
        # in-progress events plus the epoch's completed events, in 256-rounded bytes; slots
        # claimed in the epoch, live plus tombstones; completed records of the epoch
        assert step.after_batch["arenaUsed"] <= T.ARENA, (m, b)
        assert step.after_batch["tableUsed"] <= 48, (m, b)
        assert step.after_batch["completedPending"] <= T.QCAP, (m, b)
        assert step.after_turn["arenaUsed"] == sum(T.need(len(s.events[k])) for k in step.carried)


def test_the_run_needs_its_turns(s, runs):
    assert sum(len(e) for e in s.events.values()) >= 4 * T.ARENA
    assert sum(T.need(len(e)) for e in s.events.values()) > 4 * T.ARENA


def test_events_straddle_age_out_and_complete_carried(s, runs):
    assert len(runs[T.NEVER].completed_carried) >= 10
    assert sum(len(step.lost) for step in runs[2].steps) >= 3
    assert all(r[:2] in s.missing for r in runs[2].lost)
    # one event per length class completes after having been carried.  A class of one datagram
    # (1, maxPld - 1, maxPld bytes) cannot: its event completes in the launch that creates it.
    # Those complete uncarried, every other class carried.
    L = T.lengths()
    for m in (2, T.NEVER):
        carried = {s.cls[k] for k in runs[m].completed_carried}
        assert carried == {c for c, n in enumerate(L) if n > T.max_pld()}, m
        done = {s.cls[k] for step in runs[m].steps for k in step.delivered}
        assert done == set(range(len(L)))
    # with max_carries 1 an event cut across three batches is lost at its second turn
    assert any(r[:2] not in s.missing for r in runs[1].lost)
