"""The reassembly store forms against the oracle, with hand-cut fragments and odd strides.

tests/reas_cuts.py cuts every event into head | middle | tail with the middle fragment at a
chosen destination phase and length (tests/test_reas_cuts_cpu.py shows that the matrices
reach every branch of reas_store.hpp at every stride used here).  Each matrix runs through
every launch form of the public DeviceReassembler API, in three launch orders, at slot
strides on both sides of every variant switch of the launchers.  For each run:

* events, bytes, numFragments and every counter equal the oracle's, errorFlags is 0;
* no arena byte outside [arenaOffset, arenaOffset + bytes) of a delivered record is written:
  the arena is prefilled with 0xA5 and holds only 4096 bytes more than the 256-rounded events.

In the order h | t | m the fragment under test is stored last, over neighbours already in
place, so a store that is too wide damages bytes that were right.

One launch holds no arrival order for the default mode: an empty fragment's
add may land after the add that completes its event, and is then not part of the delivered
record's numFragments; if its table lookup comes later still, it opens an item of its own
(seen once in some ten runs, at group size 7).  Only for those events (L = 0, one launch,
default mode) the count may be one less than the oracle's, and inProgress may exceed the
oracle's by at most the number of such events; each is still delivered exactly once, with
its bytes.  REFERENCE_ORDER is exact there too.
"""
import random

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC

pytestmark = pytest.mark.gpu

FORMS = ["fused1", "fused7", "fused64", "fused0", "split_hot", "split_cold", "pipelined_hot", "pipelined_cold",
         "reforder_hot", "reforder_cold"]
ORDERS = ["h|m|t", "h|t|m", "h,m,t"]
SENTINEL = 0xA5
SLACK = 4096
COUNTERS = ("eventSuccess", "totalPackets", "totalBytes", "badHeaderDiscards", "dataErrCnt", "enqueueLoss",
            "reassemblyLoss", "inProgress")


def _upload(ctx, rows, lens):
    """Datagram rows as one device buffer (256 spare bytes behind the last slot) and their lengths."""
    import torch
    flat = np.concatenate([np.ascontiguousarray(rows).reshape(-1), np.zeros(256, np.uint8)])
    assert flat.size < 64 << 20
    dpk = torch.from_numpy(flat).to(ctx.torch_device)
    dln = torch.from_numpy(np.ascontiguousarray(lens, np.uint32).view(np.int32).copy()).to(ctx.torch_device)
    return dpk, dln


def _arena_bytes(lengths, copies=1):
    return copies * sum(max(256, (n + 255) // 256 * 256) for n in lengths) + SLACK


def _oracle(with_lb, rows, lens, launches):
    """The oracle over the launches' rows in launch order: ({key: (bytes, frags)}, stats)."""
    r = O.Reassembler(with_lb)
    for a, n in launches:
        r.push_batch(rows[a:a + n], lens[a:a + n])
    ref = {}
    for b, e, d, nf in r.pop_all_frags():
        assert (e, d) not in ref
        ref[(e, d)] = (b, nf)
    return ref, r.stats()


def _run(ctx, form, with_lb, stride, dpk, dln, launches, arena_bytes):
    """The launches [(first row, rows)] through one launch form.  -> (records, stats, arena)."""
    import torch
    from e2sar_amd import _capi, sar
    kind, _, load = form.partition("_")
    R = sar.DeviceReassembler(ctx, with_lb_header=with_lb, table_slots=4096, arena_bytes=arena_bytes,
                              flags=_capi.REAS_REFERENCE_ORDER if kind == "reforder" else 0,
                              group_size=int(kind[5:]) if kind.startswith("fused") else 0)
    R.arena_tensor().fill_(SENTINEL)
    if load:
        R.set_cold(load == "cold")
    args = [(dpk[a * stride:], dln[a:], n) for a, n in launches]
    if kind.startswith("fused") or kind == "reforder":
        for pk, ln, n in args:
            R.reassemble(pk, stride, ln, n)
    elif kind == "split":
        # every classify before any scatter: the most decoupled order the split API allows
        works = [R.alloc_work(n) for _, _, n in args]
        for (pk, ln, n), w in zip(args, works):
            R.classify(pk, stride, ln, n, w)
        for (pk, ln, n), w in zip(args, works):
            R.scatter(pk, stride, n, w)
    else:
        works = [R.alloc_work(max(n for _, _, n in args)) for _ in range(2)]
        R.classify(args[0][0], stride, args[0][1], args[0][2], works[0])
        for k, (pk, ln, n) in enumerate(args):
            if k + 1 < len(args):
                cpk, cln, cn = args[k + 1]
                R.scatter_classify(stride, pk, n, works[k % 2], cpk, cln, cn, works[(k + 1) % 2])
            else:
                R.scatter(pk, stride, n, works[k % 2])
    torch.cuda.synchronize()
    recs, st = R.poll(), R.stats()
    arena = R.arena_tensor().cpu().numpy()
    R.close()
    return recs, st, arena


def _delivered(recs, arena, label):
    """{key: (bytes, frags)} of the records, none twice, and the arena bytes they do not cover."""
    got, outside = {}, np.ones(arena.size, bool)
    for rec in recs:
        key = (rec.eventNum, rec.dataId)
        assert key not in got, f"{label}: {key} delivered twice"
        assert rec.arenaOffset % 256 == 0 and rec.arenaOffset + rec.bytes <= arena.size, label
        got[key] = (arena[rec.arenaOffset:rec.arenaOffset + rec.bytes].tobytes(), rec.numFragments)
        outside[rec.arenaOffset:rec.arenaOffset + rec.bytes] = False
    return got, outside


def _check(recs, st, arena, ref, rst, label, unordered=(), names=None):
    """unordered: keys whose empty fragment shares a default-mode launch with the fragment
    that completes the event (see the module docstring).  If its add lands after that one
    it is not in the record's numFragments; if even its lookup does, it has opened an item
    of its own, which stays in progress."""
    got, outside = _delivered(recs, arena, label)
    assert set(got) == set(ref), (label, sorted(set(got) ^ set(ref))[:4])
    late = 0
    for k, (b, nf) in ref.items():
        if got[k][0] != b:
            d = np.nonzero(np.frombuffer(got[k][0], np.uint8) != np.frombuffer(b, np.uint8))[0]
            raise AssertionError(f"{label}: event {k} {names[k] if names else ''} of {len(b)} bytes differs at {d[:12]}")
        if k in unordered and got[k][1] == nf - 1:
            late += 1
        else:
            assert got[k][1] == nf, (label, k, got[k][1], nf)
    for f in COUNTERS[:-1]:
        assert getattr(st, f) == rst[f], (label, f, getattr(st, f), rst[f])
    assert 0 <= st.inProgress - rst["inProgress"] <= late, (label, "inProgress", st.inProgress, rst["inProgress"], late)
    assert st.errorFlags == 0, label
    stray = np.nonzero(outside & (arena != SENTINEL))[0]
    assert stray.size == 0, f"{label}: {stray.size} arena bytes outside the delivered events written, at {stray[:12]}"


# ----------------------------------------------------------------------------------
# the fragment matrices


class _Matrix:
    """One (stride, header form, matrix) on the device: heads, mids and tails as three
    contiguous segments of one buffer, uploaded once; the oracle's result per arrival order."""

    def __init__(self, ctx, cfg, matrix):
        self.stride, self.with_lb = cfg
        h, m, t, events, cuts = RC.triples(self.stride, self.with_lb, RC.phases_for(self.stride),
                                           RC.lengths_for(self.stride, self.with_lb, matrix))
        self.n, self.n1 = len(cuts), RC.n_nonempty(cuts)
        self.rows = np.concatenate([h[0], m[0], t[0]])
        self.lens = np.concatenate([h[1], m[1], t[1]])
        self.dpk, self.dln = _upload(ctx, self.rows, self.lens)
        self.events = events
        self.names = {k: f"(a, L) = {c}" for k, c in zip(events, cuts)}
        self.empty = {k for k, c in zip(events, cuts) if c[1] == 0}
        self.blens = [len(b) for b in events.values()]
        self._ref = {}

    def launches(self, order):
        n, n1 = self.n, self.n1
        if order == "h|m|t":
            return [(0, n), (n, n), (2 * n, n)]
        if order == "h|t|m":                       # without the events whose middle is empty (they come last)
            return [(0, n1), (2 * n, n1), (n, n1)]
        return [(0, 3 * n)]

    def ref(self, order):
        key = "htm" if order == "h|t|m" else "hmt"
        if key not in self._ref:
            ref, rst = _oracle(self.with_lb, self.rows, self.lens, self.launches(order))
            m = self.n1 if key == "htm" else self.n
            assert len(ref) == m and rst["eventSuccess"] == m and rst["inProgress"] == 0
            assert all(ref[k][0] == b for k, b in list(self.events.items())[:m])
            self._ref[key] = (ref, rst)
        return self._ref[key]


_cache = {}


def _matrix(ctx, cfg, matrix):
    if _cache.get("key") != (cfg, matrix):
        _cache.clear()
        _cache.update(key=(cfg, matrix), value=_Matrix(ctx, cfg, matrix))
    return _cache["value"]


def _cfg_id(cfg):
    return f"{cfg[0]}{'lb' if cfg[1] else 're'}"


@pytest.mark.parametrize("cfg,matrix,form", [(c, m, f) for c in RC.CONFIGS for m in ("small", "full") for f in FORMS],
                         ids=lambda v: _cfg_id(v) if isinstance(v, tuple) else v)
def test_store_forms(hip, cfg, matrix, form):
    M = _matrix(hip, cfg, matrix)
    for order in ORDERS:
        launches = M.launches(order)
        m = M.n1 if order == "h|t|m" else M.n
        ref, rst = M.ref(order)
        unordered = M.empty if order == "h,m,t" and not form.startswith("reforder") else ()
        # (256 bytes for each item that an empty fragment may open for itself)
        recs, st, arena = _run(hip, form, M.with_lb, M.stride, M.dpk, M.dln, launches,
                               _arena_bytes(M.blens[:m]) + 256 * len(unordered))
        _check(recs, st, arena, ref, rst, f"{_cfg_id(cfg)} {matrix} {form} {order}", unordered, M.names)


# ----------------------------------------------------------------------------------
# further cases

SOME_FORMS = ["fused0", "split_cold", "reforder_hot"]
SOME_STRIDES = [80, 2064, 12304]


@pytest.mark.parametrize("form", SOME_FORMS)
@pytest.mark.parametrize("stride", SOME_STRIDES)
def test_dropped_datagrams_write_nothing(hip, stride, form):
    # among the heads: a fragment one byte past its event's length (for a live key and for a
    # key that has no item), a bad RE version that carries a full payload, a datagram
    # shorter than its headers.  Counted as the oracle counts them; no byte of theirs stored.
    h, m, t, events, cuts = RC.triples(stride, True, [0, 4, 7], [5, 16, 33])
    rng = np.random.default_rng(stride)
    keys = list(events)
    blen0 = len(events[keys[0]])
    junk = [RC.dgram(keys[0][0], RC.DATA_ID, blen0 - 7, blen0, rng.integers(0, 256, 8, dtype=np.uint8), stride, True, rng),
            RC.dgram(RC.EV0 + 5000, RC.DATA_ID, 93, 100, rng.integers(0, 256, 8, dtype=np.uint8), stride, True, rng),
            RC.dgram(keys[1][0], RC.DATA_ID, 16, stride, rng.integers(0, 256, stride - 36, dtype=np.uint8), stride, True),
            RC.dgram(keys[2][0], RC.DATA_ID, 16, len(events[keys[2]]), b"", stride, True, rng)]
    junk[2][0][16] = 0x20                                   # RE version 2
    junk[3] = (junk[3][0], 35)                              # one byte short of LB + RE
    rows, lens = list(h[0]), list(h[1])
    for at, (row, n) in zip((7, 5, 3, 1), reversed(junk)):
        rows.insert(at, row)
        lens.insert(at, n)
    nh = len(lens)
    rows = np.concatenate([np.stack(rows), m[0], t[0]])
    lens = np.concatenate([np.array(lens, np.uint32), m[1], t[1]])
    launches = [(0, nh), (nh, len(cuts)), (nh + len(cuts), len(cuts))]
    ref, rst = _oracle(True, rows, lens, launches)
    assert rst["dataErrCnt"] == 2 and rst["badHeaderDiscards"] == 2 and rst["eventSuccess"] == len(cuts)
    assert all(ref[k][0] == b for k, b in events.items())
    dpk, dln = _upload(hip, rows, lens)
    recs, st, arena = _run(hip, form, True, stride, dpk, dln, launches, _arena_bytes([len(b) for b in events.values()]))
    _check(recs, st, arena, ref, rst, f"dropped {stride} {form}")


@pytest.mark.parametrize("form", SOME_FORMS)
@pytest.mark.parametrize("stride", SOME_STRIDES)
def test_zero_length_event(hip, stride, form):
    # a lone header with bufferLength 0 is an event of no bytes and one fragment
    row, n = RC.dgram(RC.EV0 + 77, 9, 0, 0, b"", stride, True, np.random.default_rng(1))
    rows, lens = row[None, :], np.array([n], np.uint32)
    ref, rst = _oracle(True, rows, lens, [(0, 1)])
    assert ref == {(RC.EV0 + 77, 9): (b"", 1)} and rst["eventSuccess"] == 1
    dpk, dln = _upload(hip, rows, lens)
    recs, st, arena = _run(hip, form, True, stride, dpk, dln, [(0, 1)], _arena_bytes([0]))
    assert len(recs) == 1 and recs[0].bytes == 0 and recs[0].numFragments == 1
    _check(recs, st, arena, ref, rst, f"empty event {stride} {form}")


_long = {}


def _long_events(ctx, mp):
    """Seven events of 1 byte to about 12 x maxPld, cut uniformly, offset 0 first and the rest shuffled."""
    if _long.get("key") != mp:
        stride = (36 + mp + 15) // 16 * 16
        sizes = [12 * mp - 5, 1, mp, mp + 1, 5 * mp + 3, 3 * mp, 7 * mp + mp // 2]
        rng = np.random.default_rng(mp)
        pks, lns, starts, events = [], [], [], {}
        for k, size in enumerate(sizes):
            data = rng.integers(0, 256, size, dtype=np.uint8)
            events[(RC.EV0 + k, 4321)] = data.tobytes()
            p, l = O.segment_event(data, RC.EV0 + k, 4321, 1 + k, 99, 2, mp, stride)
            starts.append(sum(len(x) for x in lns))
            pks.append(p)
            lns.append(l)
        rows, lens = np.concatenate(pks), np.concatenate(lns)
        rest = [i for i in range(len(lens)) if i not in starts]
        random.Random(mp).shuffle(rest)
        order = starts + rest
        rows, lens = rows[order], lens[order]
        n = len(lens)
        launches = [(0, n // 2), (n // 2, n - n // 2)]
        ref, rst = _oracle(True, rows, lens, launches)
        assert {k: v[0] for k, v in ref.items()} == events
        _long.clear()
        _long.update(key=mp, value=(stride, rows, lens, launches, ref, rst, sizes) + _upload(ctx, rows, lens))
    return _long["value"]


@pytest.mark.parametrize("mp,form", [(mp, f) for mp in (2028, 4076, 4075, 12268, 65471) for f in FORMS])
def test_long_events_at_boundary_strides(hip, mp, form):
    # uniform segmentation at the strides where the launchers change variant (2064, 4112,
    # 12304), at a maximal UDP datagram (65520: several copy rounds per datagram) and at a
    # maxPld that is no multiple of 4 (the byte path): runs of many datagrams, several rounds
    stride, rows, lens, launches, ref, rst, sizes, dpk, dln = _long_events(hip, mp)
    assert stride == {2028: 2064, 4076: 4112, 4075: 4112, 12268: 12304, 65471: 65520}[mp]
    recs, st, arena = _run(hip, form, True, stride, dpk, dln, launches, _arena_bytes(sizes))
    _check(recs, st, arena, ref, rst, f"long maxPld {mp} {form}")


@pytest.mark.parametrize("form", SOME_FORMS)
@pytest.mark.parametrize("stride", SOME_STRIDES)
def test_late_empty_fragment(hip, stride, form):
    """An empty fragment (len == header, offset > 0) that arrives after its event is whole.

    The reference (and REFERENCE_ORDER, and the default mode when the completing launch has
    ended) finds the event gone and opens a new item for the fragment: one success and one
    item in progress per event.  With every classify ahead of the scatters the event is not
    yet marked done when the fragment is classified; it joins the finished event, completes
    nothing and opens nothing: the event is delivered once, with the two fragments that
    made it whole.  (Until `completes()` asked that the add itself reach the
    length, this add completed the event a second time: two records, eventSuccess 2 per
    event, inProgress below zero.)"""
    h, m, t, events, cuts = RC.triples(stride, True, [0, 4, 7, 12, 15], [0])
    n = len(cuts)
    rows, lens = np.concatenate([h[0], m[0], t[0]]), np.concatenate([h[1], m[1], t[1]])
    launches = [(0, n), (2 * n, n), (n, n)]
    ref, rst = _oracle(True, rows, lens, launches)
    assert rst["eventSuccess"] == n and rst["inProgress"] == n
    assert ref == {k: (b, 2) for k, b in events.items()}
    dpk, dln = _upload(hip, rows, lens)
    recs, st, arena = _run(hip, form, True, stride, dpk, dln, launches,
                           _arena_bytes([len(b) for b in events.values()], copies=2))
    label = f"late empty fragment {stride} {form}"
    if form == "split_cold":
        got, _ = _delivered(recs, arena, label)                  # no key twice
        assert st.eventSuccess == n and len(recs) == n, (label, st.eventSuccess, len(recs))
        assert 0 <= st.inProgress <= n, (label, st.inProgress)
        rst = dict(rst, inProgress=0)                            # joined the finished event: no new item
    _check(recs, st, arena, ref, rst, label)
