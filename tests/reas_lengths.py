"""Streams whose fragments disagree on bufferLength under one key -- TEST INFRASTRUCTURE
(tests/test_reas_lengths_cpu.py, tests/test_gpu_reas_lengths.py).

An item's length is the bufferLength of the fragment that creates it.  A later fragment of
the key may announce another length: it joins when it lies inside the item, and is dropped
(dataErrCnt) when it ends past the item's length although it fits its own -- classify_wave's
second bounds test in the default path, `viol` in ro_walk_chunk in the reference order, the
oracle's third guard.  Expected values come from the guarded oracle; the tags kept with
every datagram say what it was built to be, for the conditions the CPU test asserts.

Default path (one launch holds no arrival order): the streams keep the
creator of every item deterministic and stay where the default path and the reference agree:
no offset 0 except the creator, no overlapping taken fragments, nothing after a completion.

    case (a)  launch 1: every key's offset-0 fragment; launch 2: everything else but each
              key's last taken fragment; launch 3: those; launch 4: one whole event (so the
              item the arena ends with has a completed neighbour too)
    case (b)  one launch; each key's fragments are consecutive inside one aligned block of
              `block` datagrams (one wave of one fused group / one classify wave), the block
              filled up with whole one-datagram events.  The own-length control is no part of
              a run, so the key's fragments behind it form a second run in the same wave; its
              head carries the creator's length, so whichever head's claim wins, the item has
              length S.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

import oracle_ffi as O
import reas_cuts as RC

MARK = 0xEE                 # payload byte of every fragment that must be dropped; nowhere else
SENTINEL = 0xA5             # arena pre-fill
SLACK = 4096                # arena bytes past the items
FAR = 2048                  # the far overrun starts this far past S: still inside the slack
DATA_ID = RC.DATA_ID
EV0 = 7 << 33

PAYS = {64: (16, 28, 20, 24), 1472: (64, 48, 16, 32), 8976: (8940,)}


def _data(rng, n):
    """n random bytes, none of them MARK."""
    v = rng.integers(0, 255, n, dtype=np.uint16)
    return (v + (v >= MARK)).astype(np.uint8)


@dataclass
class Tag:
    key: tuple
    off: int
    pl: int
    blen: int
    # creator | join (another length, inside S) | rest | viol (overruns its item) | own (overruns
    # its own length) | whole (a one-item event) | orphan (its item is replaced by an offset 0)
    kind: str


@dataclass
class Stream:
    name: str
    stride: int
    rows: np.ndarray
    lens: np.ndarray
    tags: list
    launches: list        # [(first row, rows)]
    block: int = 0        # case (b): the alignment of the keys' blocks
    S: dict = field(default_factory=dict)       # key -> item length
    never: set = field(default_factory=set)     # keys that stay in progress
    ref: tuple = None     # the oracle's result, kept by the GPU test
    dev: tuple = None     # the device copy of rows and lens, kept by the GPU test

    @property
    def arena_bytes(self):
        return sum(_rounded(s) for s in self.S.values()) + SLACK


def _rounded(n):
    """Arena bytes of an item of n bytes."""
    return max(256, (n + 255) // 256 * 256)


def key_fragments(key, S, stride, rng, never=False, few=False):
    """The datagrams of one key in an order that is valid sequentially: creator, a joined
    fragment of a smaller length, an overrun by one byte, a joined fragment of a larger
    length, an overrun by far, the own-length control, the rest (length S), the last taken
    fragment.  -> ([(row, n, Tag)], event bytes)."""
    pays = (64,) if few else PAYS[stride]
    data = _data(rng, S)
    chunks, off, i = [], 0, 0
    while off < S:
        pl = min(pays[i % len(pays)], S - off)
        rest = S - off - pl
        if 0 < rest < 16:                      # no payload under 16 bytes
            pl = pl - (16 - rest) if pl - (16 - rest) >= 16 else pl + rest
            assert 36 + pl <= stride
        chunks.append((off, pl))
        off += pl
        i += 1
    assert len(chunks) >= 4
    lo, hi = S - 128, S + 1000
    assert chunks[1][0] + chunks[1][1] <= lo

    def frag(off, pl, blen, kind, payload=None):
        pay = data[off:off + pl] if payload is None else payload
        row, n = RC.dgram(key[0], key[1], off, blen, pay, stride, True)
        return row, n, Tag(key, off, pl, blen, kind)

    vp = min(pays[0], 64)
    mark = np.full(vp, MARK, np.uint8)
    out = [frag(*chunks[0], S, "creator"),
           frag(*chunks[1], lo, "join"),
           frag(S - vp + 1, vp, hi, "viol", mark),
           frag(*chunks[2], hi, "join"),
           frag(S + FAR, vp, S + 8192, "viol", mark),
           frag(100, vp, 50, "own", mark)]
    mid = [frag(o, p, S, "rest") for o, p in chunks[3:-1]]
    rng_order = list(range(len(mid)))
    random.Random(S + stride).shuffle(rng_order)
    if mid:                                    # the fragment behind the control carries S (case b)
        out += [mid[0]] + [mid[i] for i in rng_order if i != 0]
    if not never:
        out.append(frag(*chunks[-1], S, "rest"))
    return out, data.tobytes()


def _whole(key, stride, rng, n=16):
    row, ln = RC.dgram(key[0], key[1], 0, n, _data(rng, n), stride, True)
    return row, ln, Tag(key, 0, n, n, "whole")


def _pack(name, stride, launches_of_frags, S, never, block=0):
    rows, lens, tags, launches = [], [], [], []
    for fr in launches_of_frags:
        launches.append((len(rows), len(fr)))
        for row, n, tag in fr:
            rows.append(row)
            lens.append(n)
            tags.append(tag)
    return Stream(name, stride, np.stack(rows), np.array(lens, np.uint32), tags, launches, block, S, never)


def case_a(stride, sizes, seed=0):
    rng = np.random.default_rng([stride, seed, 0xA])
    rnd = random.Random(stride * 31 + seed)
    keys, S, never = [], {}, set()
    for k, s in enumerate(list(sizes) + [768 if stride < 8976 else 256]):
        key = (EV0 + k, DATA_ID)
        last = k == len(sizes)
        fr, _ = key_fragments(key, s, stride, rng, never=last, few=stride == 8976 and s < 4096)
        keys.append(fr)
        S[key] = s
        if last:
            never.add(key)
    creators = [fr[0] for fr in keys]
    finals = [fr[-1] for fr, key in zip(keys, S) if key not in never]
    mids = [fr[1:] if key in never else fr[1:-1] for fr, key in zip(keys, S)]
    mid = []
    while any(mids):                            # interleaved, each key's own order kept
        m = rnd.choice([m for m in mids if m])
        mid.append(m.pop(0))
    cap = (EV0 + 1000, DATA_ID)
    S[cap] = 16
    return _pack(f"a{stride}", stride, [creators, mid, finals, [_whole(cap, stride, rng)]], S, never)


def case_b(stride, sizes, block, seed=0):
    rng = np.random.default_rng([stride, seed, 0xB, block])
    out, S, never = [], {}, set()
    nfill = 0
    for k, s in enumerate(list(sizes) + [sizes[0]]):
        key = (EV0 + 100 + k, DATA_ID)
        last = k == len(sizes)
        fr, _ = key_fragments(key, s, stride, rng, never=last, few=block < 64)
        assert len(fr) <= block
        S[key] = s
        if last:
            never.add(key)
        lead = (k * 3) % (block - len(fr) + 1)              # the run starts at different lanes
        for j in range(block):
            if lead <= j < lead + len(fr):
                out.append(fr[j - lead])
            else:
                fk = (EV0 + 5000 + nfill, DATA_ID)
                nfill += 1
                S[fk] = 16
                out.append(_whole(fk, stride, rng))
    return _pack(f"b{stride}x{block}", stride, [out], S, never, block)


_streams = {}


def default_streams():
    """Every default-path stream, by name (built once)."""
    if not _streams:
        for s in (case_a(64, [256, 768, 4096]), case_a(1472, [256, 768, 4096]), case_a(8976, [4 << 20, 256]),
                  case_b(1472, [256, 256], 7), case_b(64, [256, 768], 64), case_b(1472, [256, 768], 64)):
            _streams[s.name] = s
    return _streams


# forms a stream may run in: a case (b) stream needs its blocks to be the kernels' groups, so
# fused at group size 1 or automatic and reassemble_dev at automatic are left out for it: there
# the key's fragments share no wave, and the lookup that claims the slot first -- with whatever
# length it carries -- would create the item
A_FORMS = ["fused1", "fused7", "fused64", "fused0", "split_hot", "split_cold", "pipelined_hot", "pipelined_cold", "dev0"]
B_FORMS = {7: ["fused7", "dev7"], 64: ["fused64", "split_hot", "split_cold", "pipelined_hot", "pipelined_cold", "dev64"]}


def forms_of(s: Stream):
    return B_FORMS[s.block] if s.block else A_FORMS


def conditions(s: Stream):
    """What the default-path streams promise, from the tags alone.  -> per key
    {taken, joined, viol, own, complete}."""
    per = {}
    for a, n in s.launches:
        for p in range(a, a + n):
            t = s.tags[p]
            k = per.setdefault(t.key, dict(S=None, mask=None, taken=0, joined=0, viol=0, own=0, complete=False))
            assert not k["complete"], f"{s.name}: a fragment of {t.key} after its completion"
            if t.off + t.pl > t.blen:
                assert t.kind == "own"
                k["own"] += 1
                continue
            if k["S"] is None:
                assert t.off == 0 and t.kind in ("creator", "whole"), f"{s.name}: {t.key} not created at offset 0"
                k["S"], k["mask"] = t.blen, np.zeros(t.blen, bool)
            else:
                assert t.off != 0, f"{s.name}: a second offset-0 fragment of {t.key}"
            if t.off + t.pl > k["S"]:
                assert t.kind == "viol"
                k["viol"] += 1
                continue
            assert t.kind != "viol"
            assert not k["mask"][t.off:t.off + t.pl].any(), f"{s.name}: overlapping fragments of {t.key}"
            k["mask"][t.off:t.off + t.pl] = True
            k["taken"] += 1
            k["joined"] += t.blen != k["S"]
            k["complete"] = bool(k["mask"].all())
    return per


# ----------------------------------------------------------------------------------
# reference order: any arrival order


def model(pk, ln):
    """The guarded arrival rules (test_gpu_reference_order._completes_with_a_hole) with the
    counts the CPU test asserts: -> (hole, item-length drops, joined other-length fragments)."""
    items, hole, drops, joined = {}, False, 0, 0
    for p in range(len(ln)):
        if int(ln[p]) < 36:
            continue
        ok, d, off, blen, ev, _ = O.re_parse(pk[p, 16:36].tobytes())
        pl = int(ln[p]) - 36
        if not ok or off + pl > blen:
            continue
        it = items.get((ev, d))
        if off == 0 or it is None:
            it = items[(ev, d)] = [blen, 0, np.zeros(blen, bool)]
        if off + pl > it[0]:
            drops += 1
            continue
        joined += blen != it[0]
        it[1] += pl
        it[2][off:off + pl] = True
        if it[1] == it[0]:
            hole = hole or not it[2].all()
            items[(ev, d)] = None
    return hole, drops, joined


def _restamp(row, blen):
    row[24:28] = np.frombuffer(int(blen).to_bytes(4, "big"), np.uint8)


def restamped_draw(seed):
    """test_gpu_reference_order._draw's stream with the bufferLength of some fragments of a
    random subset of events re-stamped: larger, smaller but still holding the fragment, or
    too small for it; offset-0 fragments included (they start an item of the other length)."""
    from test_gpu_reference_order import _draw
    pk, ln, stride, rnd = _draw(seed)
    pk = pk.copy()
    r2 = random.Random(seed ^ 0x1E57)
    keys = {}
    for p in range(len(ln)):
        ok, d, off, blen, ev, _ = O.re_parse(pk[p, 16:36].tobytes())
        if ok and int(ln[p]) >= 36:
            keys.setdefault((ev, d), []).append((p, off, int(ln[p]) - 36, blen))
    # one event for certain: its offset 0 announces a length that one later fragment lies
    # inside (it joins an item of another length) and another ends past (it overruns the item)
    forced = None
    order = sorted(keys)
    r2.shuffle(order)
    for key in order:
        fr = keys[key]
        z = [i for i, f in enumerate(fr) if f[1] == 0]
        if not z:
            continue
        ends = sorted({f[1] + f[2] for f in fr[z[-1] + 1:] if f[1] > 0})
        if len(ends) >= 2 and max(fr[z[-1]][2], ends[0]) < ends[-1]:
            other = r2.randint(max(fr[z[-1]][2], ends[0]), ends[-1] - 1)
            for i in z:
                _restamp(pk[fr[i][0]], other)
            forced = key
            break
    for key in sorted(keys):
        if key == forced or r2.random() < 0.5:
            continue
        zeros = [f for f in keys[key] if f[1] == 0 and f[2] < f[3]]
        mode = r2.random()
        if mode < 0.6 and zeros:
            # every offset 0 of the event announces one other length: shorter (later fragments
            # overrun the item or join it) or longer (they all join an item of another length)
            p0, _, pl0, blen0 = zeros[0]
            other = r2.randint(pl0, blen0 - 1) if mode < 0.4 else blen0 + r2.choice([1, 7, 256, 5000])
            for p, _, _, _ in zeros:
                _restamp(pk[p], other)
            continue
        for p, off, pl, blen in keys[key]:
            r = r2.random()
            if r < 0.10:
                _restamp(pk[p], blen + r2.choice([1, 7, 256, 5000]))
            elif r < 0.20 and off + pl < blen:
                _restamp(pk[p], r2.randint(off + pl, blen - 1))
            elif r < 0.24 and off + pl > 0:
                _restamp(pk[p], r2.randint(0, off + pl - 1))
    return pk, ln, stride, rnd


MAX_SUB = 1000


def restamped_stream(seed):
    """-> (pk, ln, stride, rnd, sub-draws rejected): redrawn on the guarded hole model."""
    for sub in range(MAX_SUB):
        out = restamped_draw(seed * 1000 + sub)
        if not model(out[0], out[1])[0]:
            return out + (sub,)
    raise AssertionError("no hole-free stream drawn")


CHUNK_KEY = (EV0 + 9000, DATA_ID)


def chunk_straddler():
    """More than 64 consecutive fragments of one key, at stride 64 with 16-byte payloads: items of
    256, 512 and 768 bytes one after the other, each started by an offset-0 fragment of
    another length than the item before it, each with two fragments that overrun it (one
    early, one late) and one joined fragment of another length, each completing.  In front: a
    fragment at offset 16 whose item the first offset 0 replaces; at the end: an offset 0 of
    yet another length that stays in progress.  -> (pk, ln, stride, tags)."""
    stride, pl = 64, 16
    rng = np.random.default_rng(64064)
    out = []
    other = (EV0 + 9001, DATA_ID)

    def add(key, off, blen, pay, kind):
        row, n = RC.dgram(key[0], key[1], off, blen, pay, stride, True)
        out.append((row, n, Tag(key, off, len(pay), blen, kind)))

    w = _data(rng, 48)
    for o in (0, 16, 32):
        add(other, o, 48, w[o:o + 16], "whole")
    add(CHUNK_KEY, 16, 100, _data(rng, pl), "orphan")
    mark = np.full(pl, MARK, np.uint8)
    for S in (256, 512, 768, 256, 512, 768):
        data = _data(rng, S)
        nfr = S // pl
        for j in range(nfr):
            add(CHUNK_KEY, j * pl, S + 64 if j == 3 else S, data[j * pl:(j + 1) * pl], "creator" if j == 0 else
                "join" if j == 3 else "rest")
            if j in (1, nfr - 2):
                add(CHUNK_KEY, S - pl + 1 + (j == 1) * 300, 2000, mark, "viol")
    add(CHUNK_KEY, 0, 1000, _data(rng, pl), "creator")
    w = _data(rng, 48)
    for o in (0, 16, 32):
        add((EV0 + 9002, DATA_ID), o, 48, w[o:o + 16], "whole")
    return (np.stack([r for r, _, _ in out]), np.array([n for _, n, _ in out], np.uint32), stride,
            [t for _, _, t in out])
