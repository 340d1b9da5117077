"""The upkeep schedules (tests/upkeep_schedule.py) on the oracle alone: they exercise what
tests/test_gpu_upkeep.py is there to check.  Without these conditions the GPU tests could
pass vacuously -- a compaction of an empty table, a GC that collects nothing."""
import os

import pytest

import upkeep_schedule as U

CLEAN_SEEDS = range(3)
DIRTY_SEEDS = range(int(os.environ.get("E2SAR_RANDOM_SEEDS", "12")))


@pytest.fixture(scope="module")
def schedules():
    out = {("clean", s): U.clean_schedule(s) for s in CLEAN_SEEDS}
    out.update({("dirty", s): U.dirty_schedule(s) for s in DIRTY_SEEDS})
    return {k: (s, U.trace(s), U.replay_oracle(s)) for k, s in out.items()}


def test_the_trace_model_is_the_oracle(schedules):
    """trace() supplies what the oracle does not expose; everything the two share is equal."""
    for name, (s, T, ref) in schedules.items():
        gcs = iter(T.gcs)
        live = iter(T.live)
        done = lost = 0
        pending = []
        for st, r in zip(s.steps, ref):
            if st[0] == "poll":
                done += len(r)
            elif st[0] == "gc":
                keys, survivors = next(gcs)
                assert r == len(keys), name
                pending = sorted((k[0], k[1], nf) for k, nf in keys)
            elif st[0] == "lost_poll":
                assert sorted(r) == pending, name          # keys and fragment counts of the last GC
                lost += len(r)
                pending = []
            elif st[0] == "compact":
                assert r == len(next(live)), name
            elif st[0] == "stats":
                assert r["reassemblyLoss"] == lost, name
        assert done == len(T.completions), name
        assert not T.hole and not T.twice, name


def test_every_compaction_moves_a_live_item(schedules):
    for name, (s, T, _) in schedules.items():
        assert T.live and all(T.live), (name, [len(x) for x in T.live])


def test_an_event_completes_with_fragments_from_both_sides_of_a_compaction(schedules):
    for name, (s, T, _) in schedules.items():
        if name[0] == "clean":
            assert any(len(ep) > 1 for _, ep in T.completions), name
    assert any(len(ep) > 1 for n, (_, T, _) in schedules.items() if n[0] == "dirty" for _, ep in T.completions)


def test_a_mid_stream_gc_loses_one_item_and_spares_another(schedules):
    for name, (s, T, _) in schedules.items():
        mid = T.gcs[:-1]                               # the last GC of a schedule has no batch after it
        if name[0] == "clean":
            assert any(lost and survivors for lost, survivors in mid), name
    assert any(lost and survivors for n, (_, T, _) in schedules.items() if n[0] == "dirty"
               for lost, survivors in T.gcs[:-1])


def test_clean_keys_get_fragments_after_their_item_was_collected(schedules):
    for name, (s, T, _) in schedules.items():
        if name[0] == "clean":
            assert T.after_collect, name


def test_dirty_seeds_need_few_redraws(schedules):
    redraws = {name[1]: s.redraws for name, (s, _, _) in schedules.items() if name[0] == "dirty"}
    print("redraws per dirty seed:", redraws)
    assert all(r < 999 for r in redraws.values())
