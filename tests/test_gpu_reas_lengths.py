"""Fragments of one key that disagree on bufferLength, against the guarded oracle.

An item's length S is the bufferLength of the fragment that creates it.  A later fragment
with another length joins when it lies inside S; one that fits its own length but ends past
S is dropped and counted in dataErrCnt (classify_wave's "bounds against the event's length"
in the default path, `viol` in ro_walk_chunk in the reference order; DESIGN.md 5.3 Bounds).
If either test were wrong the fragment would be stored past the item, into its arena
neighbour, or counted into curBytes.

Default path (tests/reas_lengths.py, conditions asserted by test_reas_lengths_cpu.py): for
every launch form the completed events, their bytes and numFragments, every counter and the
GC's lost records equal the oracle's; the whole arena, prefilled with 0xA5, equals the host
image (completed events at their arenaOffset, the taken fragments of the item that stays in
progress in the one gap, 0xA5 elsewhere); the payload byte of the dropped fragments is nowhere
in the arena.

Case (a) streams run in every launch form.  Case (b) streams run only where a key's block is
one kernel group: fused and reassemble_dev at group size 7 or 64, split and pipelined (64-lane
classify waves).  fused1, fused0 and dev0 are deliberately absent for (b): there the run head
is not the item's creator for certain.  Within (b) the own-length control ends the first run,
so the item is created by one of two run heads of the same wave; both carry S.

Reference order: test_gpu_reference_order's random streams with bufferLengths re-stamped, and
one key whose fragments straddle the walk's 64-fragment chunks, each in fused, split and
pipelined form.
"""
import os

import numpy as np
import pytest

import oracle_ffi as O
import reas_lengths as RL
from test_gpu_golden import STATS
from test_gpu_reference_order import _gpu as ro_gpu, _oracle as ro_oracle

pytestmark = pytest.mark.gpu

NOW = 100


def _expected(s):
    """The guarded oracle over the stream in launch order, then one GC."""
    if s.ref is None:
        r = O.Reassembler(True)
        r.set_time(NOW)
        for a, n in s.launches:
            r.push_batch(s.rows[a:a + n], s.lens[a:a + n])
        ev = {}
        for b, e, d, nf in r.pop_all_frags():
            assert (e, d) not in ev
            ev[(e, d)] = (b, nf)
        st = r.stats()
        r.set_time(NOW + 1000)
        r.gc(500)
        lost = sorted(r.lost_pop_all())
        st2 = r.stats()
        assert set(ev) == set(s.S) - s.never and all(len(ev[k][0]) == s.S[k] for k in ev)
        assert [(e, d) for e, d, _ in lost] == sorted(s.never) and st["dataErrCnt"] >= 9
        s.ref = (ev, {k: int(st[k]) for k in STATS}, lost, int(st2["reassemblyLoss"]), int(st2["inProgress"]))
    return s.ref


def _upload(ctx, s):
    import torch
    if s.dev is None or s.dev[0].device != ctx.torch_device:
        flat = np.concatenate([s.rows.reshape(-1), np.zeros(256, np.uint8)])
        s.dev = (torch.from_numpy(flat).to(ctx.torch_device),
                 torch.from_numpy(s.lens.view(np.int32).copy()).to(ctx.torch_device))
    return s.dev


def _run(ctx, s, form):
    """-> (records, stats, arena after the launches, lost records, stats after the GC)."""
    import torch
    from e2sar_amd import sar
    kind, _, load = form.partition("_")
    gs = int(kind[5:]) if kind.startswith("fused") else int(kind[3:]) if kind.startswith("dev") else 0
    R = sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=4096, arena_bytes=s.arena_bytes, group_size=gs)
    R.arena_tensor().fill_(RL.SENTINEL)
    if load:
        R.set_cold(load == "cold")
    dpk, dln = _upload(ctx, s)
    st = s.stride
    args = [(dpk[a * st:], dln[a:], n) for a, n in s.launches]
    if kind.startswith("fused"):
        for pk, ln, n in args:
            R.reassemble(pk, st, ln, n, now_ms=NOW)
    elif kind.startswith("dev"):
        for pk, ln, n in args:
            R.reassemble_dev(pk, st, ln, torch.tensor([n], dtype=torch.int32, device=ctx.torch_device), now_ms=NOW)
    elif kind == "split":
        for pk, ln, n in args:
            w = R.alloc_work(n)
            R.classify(pk, st, ln, n, w, now_ms=NOW)
            R.scatter(pk, st, n, w)
    else:
        works = [R.alloc_work(max(n for _, _, n in args)) for _ in range(2)]
        R.classify(args[0][0], st, args[0][1], args[0][2], works[0], now_ms=NOW)
        for k, (pk, ln, n) in enumerate(args):
            if k + 1 < len(args):
                cpk, cln, cn = args[k + 1]
                R.scatter_classify(st, pk, n, works[k % 2], cpk, cln, cn, works[(k + 1) % 2], now_ms=NOW)
            else:
                R.scatter(pk, st, n, works[k % 2])
    torch.cuda.synchronize()
    recs, stats = R.poll(), R.stats()
    arena = R.arena_tensor().cpu().numpy()
    R.gc(now_ms=NOW + 1000, timeout_ms=500)
    lost = sorted((r.eventNum, r.dataId, r.numFragments) for r in R.lost_poll())
    st2 = R.stats()
    R.close()
    return recs, stats, arena, lost, st2


def _image(s, recs, ev):
    """The arena as the host expects it: every completed event at its arenaOffset, the taken
    fragments of the item in progress in the gap the records leave, the pre-fill elsewhere."""
    img = np.full(s.arena_bytes, RL.SENTINEL, np.uint8)
    used = s.arena_bytes - RL.SLACK
    free = np.ones(used, bool)
    for rec in recs:
        key = (rec.eventNum, rec.dataId)
        assert rec.arenaOffset % 256 == 0 and rec.arenaOffset + RL._rounded(rec.bytes) <= used, key
        assert free[rec.arenaOffset:rec.arenaOffset + RL._rounded(rec.bytes)].all(), f"{key} overlaps another record"
        free[rec.arenaOffset:rec.arenaOffset + RL._rounded(rec.bytes)] = False
        img[rec.arenaOffset:rec.arenaOffset + rec.bytes] = np.frombuffer(ev[key][0], np.uint8)
    (never,) = s.never
    gap = np.nonzero(free)[0]
    assert gap.size == RL._rounded(s.S[never]) and gap[-1] - gap[0] + 1 == gap.size, "one gap: the item in progress"
    for p, t in enumerate(s.tags):
        if t.key == never and t.off + t.pl <= min(t.blen, s.S[never]):
            img[gap[0] + t.off:gap[0] + t.off + t.pl] = s.rows[p, 36:36 + t.pl]
    return img


@pytest.mark.parametrize("name,form", [(n, f) for n, s in RL.default_streams().items() for f in RL.forms_of(s)])
def test_mixed_lengths_default_path(hip, name, form):
    s = RL.default_streams()[name]
    ev, rst, rlost, rloss, rinp = _expected(s)
    recs, st, arena, lost, st2 = _run(hip, s, form)
    label = f"{name} {form}"
    got = {}
    for rec in recs:
        key = (rec.eventNum, rec.dataId)
        assert key not in got and key in ev, (label, key)
        assert rec.bytes == s.S[key] == len(ev[key][0]), (label, key, rec.bytes)
        assert rec.numFragments == ev[key][1], (label, key, rec.numFragments, ev[key][1])
        got[key] = rec
    assert set(got) == set(ev), (label, sorted(set(got) ^ set(ev))[:4])
    stats = {k: int(getattr(st, k)) for k in STATS}
    assert stats == rst, (label, stats, rst)
    assert st.errorFlags == 0, label
    img = _image(s, recs, ev)
    bad = np.nonzero(arena != img)[0]
    assert bad.size == 0, f"{label}: {bad.size} arena bytes differ from the host image, at {bad[:12]}"
    assert not (arena == RL.MARK).any(), f"{label}: a dropped fragment's bytes are in the arena"
    assert lost == rlost, (label, lost, rlost)                   # fragment count without the dropped ones
    assert int(st2.reassemblyLoss) == rloss and int(st2.inProgress) == rinp == 0, label


# ----------------------------------------------------------------------------------
# reference order


@pytest.mark.parametrize("seed", range(int(os.environ.get("E2SAR_RANDOM_SEEDS", "12"))))
def test_restamped_arrival_orders_match_the_reference(hip, seed):
    pk, ln, stride, rnd, _ = RL.restamped_stream(seed)
    ref, rst, rlost, rloss, rinp = ro_oracle(pk, ln)
    assert rst["dataErrCnt"] >= 1
    n = len(ln)
    nb = rnd.randint(1, 5)
    cuts = sorted({0, n, *[rnd.randint(0, n) for _ in range(nb - 1)]})
    for mode in ("fused", "split", "pipelined"):
        got, st, lost, loss, inp = ro_gpu(hip, pk, ln, stride, cuts, mode)
        assert st == rst, (mode, st, rst)
        assert sorted(got) == sorted(ref), mode
        for k in ref:
            assert sorted(got[k]) == sorted(ref[k]), (k, mode)   # bytes and numFragments
        assert lost == rlost and loss == rloss and inp == rinp == 0, mode


@pytest.mark.parametrize("mode", ["fused", "split", "pipelined"])
def test_one_key_across_the_walk_chunks(hip, mode):
    # 206 consecutive fragments of one key: four chunks of the walk, each with a fragment that
    # overruns its item, a completion and an offset 0 that starts an item of another length;
    # one batch (the chunks as test_reas_lengths_cpu.py counts them), then cut inside chunks
    pk, ln, stride, _ = RL.chunk_straddler()
    ref, rst, rlost, rloss, rinp = ro_oracle(pk, ln)
    assert rst["eventSuccess"] == 8 and rst["dataErrCnt"] == 12 and len(rlost) == 1
    n = len(ln)
    for cuts in ([0, n], [0, 70, 71, 150, n]):
        got, st, lost, loss, inp = ro_gpu(hip, pk, ln, stride, cuts, mode)
        assert st == rst, (mode, cuts, st, rst)
        assert sorted(got) == sorted(ref), (mode, cuts)
        for k in ref:
            assert sorted(got[k]) == sorted(ref[k]), (k, mode, cuts)     # bytes and numFragments
        assert lost == rlost and loss == rloss and inp == rinp == 0
