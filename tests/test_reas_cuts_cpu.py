"""The hand-cut fragment matrices of tests/reas_cuts.py on the CPU: the oracle reassembles
them to the source bytes, and the branch model shows that they reach every store form --
which is what keeps tests/test_gpu_store_forms.py from passing vacuously."""
import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC

CLEAN = ("badHeaderDiscards", "dataErrCnt", "enqueueLoss", "reassemblyLoss")


def _ids(cfg):
    return f"{cfg[0]}{'lb' if cfg[1] else 're'}"


def _push(r, group, n=None):
    rows, lens = group
    n = len(lens) if n is None else n
    if n:
        r.push_batch(rows[:n], lens[:n])


@pytest.mark.parametrize("matrix", ["small", "full"])
@pytest.mark.parametrize("cfg", RC.CONFIGS, ids=_ids)
def test_oracle_reassembles_the_matrices(cfg, matrix):
    stride, with_lb = cfg
    h, m, t, events, cuts = RC.triples(stride, with_lb, RC.phases_for(stride), RC.lengths_for(stride, with_lb, matrix))
    n = len(cuts)
    assert n == len(events) and n >= 64
    for order in ("hmt", "htm"):
        r = O.Reassembler(with_lb)
        for g in ((h, m, t) if order == "hmt" else (h, t, m)):
            _push(r, g)
        got = {(e, d): (b, nf) for b, e, d, nf in r.pop_all_frags()}
        st = r.stats()
        assert st["eventSuccess"] == n and st["totalPackets"] == 3 * n
        assert all(st[f] == 0 for f in CLEAN), st
        assert set(got) == set(events)
        for k, b in events.items():
            assert got[k][0] == b, (k, order)
        empties = n - RC.n_nonempty(cuts)
        if order == "hmt":
            assert st["inProgress"] == 0 and all(nf == 3 for _, nf in got.values())
        else:
            # a late empty fragment finds its event gone and opens an item of its own
            assert st["inProgress"] == empties
            assert sorted(nf for _, nf in got.values()) == [2] * empties + [3] * (n - empties)


def test_counts_of_the_matrices():
    def count(stride, with_lb, matrix):
        return len(RC.triples(stride, with_lb, RC.phases_for(stride), RC.lengths_for(stride, with_lb, matrix))[4])
    for stride, with_lb in [(64, False), (80, True), (1472, True), (4112, True)]:
        assert count(stride, with_lb, "small") == 304
    assert count(48, False, "small") == 208 == count(64, True, "small")
    for stride in (1472, 2048, 2064, 4096, 4112):
        assert count(stride, True, "full") == 144
    for stride in (8976, 12288, 12304, 65520):
        assert count(stride, True, "full") == 9 * len(RC.FEW_PHASES)
    # the reduced phase set keeps the dword phases and at least three odd ones
    assert {0, 4, 8, 12} <= set(RC.FEW_PHASES) and sum(a & 1 for a in RC.FEW_PHASES) >= 3


def test_late_empty_fragment_opens_a_new_item():
    h, m, t, events, cuts = RC.triples(80, True, [0, 4, 7, 12, 15], [0])
    r = O.Reassembler(True)
    for g in (h, t, m):
        _push(r, g)
    st = r.stats()
    assert st["eventSuccess"] == 5 and st["inProgress"] == 5 and len(r.pop_all()) == 5


def test_lone_header_is_an_empty_event():
    for with_lb in (True, False):
        row, n = RC.dgram(RC.EV0, 9, 0, 0, b"", 80, with_lb)
        assert n == RC.hdr_len(with_lb)
        r = O.Reassembler(with_lb)
        r.push(row[:n])
        assert r.pop_all_frags() == [(b"", RC.EV0, 9, 1)]
        st = r.stats()
        assert st["eventSuccess"] == 1 and st["inProgress"] == 0


@pytest.mark.parametrize("cfg", RC.CONFIGS, ids=_ids)
def test_matrices_reach_every_store_form(cfg):
    stride, with_lb = cfg
    hl = RC.hdr_len(with_lb)
    small, phases = RC.matrix_classes(stride, with_lb, "small")
    fits = [a for a in RC.phases_for(stride) if hl + 16 + a <= stride]
    assert sorted(phases) == fits
    if stride <= 4112:
        assert fits == [a for a in range(16) if hl + 16 + a <= stride]
    assert ("empty",) in small
    for form in ("da", "sa"):
        for n in (1, 2, 3):
            assert (form, "edge", n) in small, (form, n)
        for cls in ("whole", "tail", "bytes", "single"):
            # (a slot of hl + 28 bytes holds a whole source chunk only when it is full: the
            # other matrix)
            if (form, cls) != ("sa", "whole") or stride > hl + 28:
                assert (form, cls) in small, (form, cls)
    # first-block edges of 3, 2 and 1 dwords: phases 4, 8 and 12
    for n in (1, 2, 3):
        assert ("da", "first-edge", n) in small
    assert {hi for c in small if c[:2] == ("da", "hi") for hi in c[2:]} == set(range(1, 17))
    # payloads that end at or near the slot's end: every slide of the load window
    fullm, phases = RC.matrix_classes(stride, with_lb, "full")
    assert sorted(phases) == fits
    assert {c[2] for c in fullm if c[:2] == ("da", "sh")} == {0, 4, 8, 12}
    for form in ("da", "sa"):
        for cls in ("whole", "tail", "bytes"):
            assert (form, cls) in fullm, (form, cls)


def test_model_agrees_with_a_byte_map():
    """The model's destination-aligned edges against a plain byte map of the payload."""
    for a in range(16):
        for L in RC.SMALL[1:]:
            covered = np.zeros(64, bool)
            covered[a:a + L] = True
            last = (a + L - 1) // 16
            his = {c[2] for c in RC.classes(a, L, 36, 4112) if c[:2] == ("da", "hi")}
            assert his == {int(covered[16 * last:16 * last + 16].sum()) + (a if last == 0 else 0)}
