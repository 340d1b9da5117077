"""The mixed-bufferLength streams (tests/reas_lengths.py) on the CPU: the conditions the GPU
tests rely on, and the oracle's receive body under AddressSanitizer.

The oracle is the reference of test_gpu_reas_lengths.py, so it must itself stay inside the
buffers it owns when a key's fragments disagree on bufferLength.  oracle/asan_stream.c is
compiled here with e2sar_oracle.c under -fsanitize=address,undefined (host code, a program of
its own) and run on every stream: exit status 0 and the numbers of the ctypes oracle.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC
import reas_lengths as RL

SEEDS = range(12)


# ----------------------------------------------------------------------------------
# the conditions of the default-path streams


@pytest.mark.parametrize("name", list(RL.default_streams()))
def test_default_streams_keep_their_conditions(name):
    s = RL.default_streams()[name]
    per = RL.conditions(s)                   # asserts: one offset 0 per key, no overlap, nothing after a completion
    assert set(per) == set(s.S)
    mixed = [k for k, v in per.items() if v["viol"]]
    assert len(mixed) >= 3
    for key in mixed:
        v = per[key]
        assert v["S"] == s.S[key] and v["S"] % 256 == 0
        assert v["viol"] == 2 and v["own"] == 1 and v["joined"] == 2
        assert v["complete"] == (key not in s.never)
        tags = [t for t in s.tags if t.key == key]
        lens = {t.blen for t in tags if t.kind == "join"}
        assert min(lens) < v["S"] < max(lens)                       # S smaller and larger than the others
        ends = sorted(t.off + t.pl - v["S"] for t in tags if t.kind == "viol")
        assert ends[0] == 1 and ends[1] > 1000                      # past S by one byte, and by far
        assert all(t.off + t.pl <= t.blen for t in tags if t.kind == "viol")
        assert all((t.kind in ("viol", "own")) == (t.pl > 0 and t.off + t.pl > v["S"] or t.kind == "own") for t in tags)
    assert sum(1 for k in per if k in s.never) == 1
    assert all(v["complete"] for k, v in per.items() if k not in s.never)
    # the dropped fragments' payload byte is in no other datagram and in no event
    for p, t in enumerate(s.tags):
        pay = s.rows[p, 36:int(s.lens[p])]
        assert (pay == RL.MARK).all() if t.kind in ("viol", "own") else not (pay == RL.MARK).any()
    # a far overrun stays inside the arena wherever its item lies
    assert all(t.off + t.pl <= s.S[t.key] + RL.SLACK for t in s.tags if t.kind == "viol")
    where = {}
    for li, (a, n) in enumerate(s.launches):
        for p in range(a, a + n):
            where.setdefault(s.tags[p].key, []).append((li, p))
    if s.block == 0:
        # case (a): the creator alone in a launch before every other fragment of its key, the
        # completing fragment alone in a launch after them
        for key in mixed:
            ls = [li for li, _ in where[key]]
            assert ls.count(0) == 1 and s.tags[where[key][0][1]].kind == "creator"
            if key not in s.never:
                assert ls.count(2) == 1 and max(ls) == 2 and s.tags[where[key][-1][1]].kind == "rest"
    else:
        # case (b): one launch, the key's fragments consecutive inside one aligned block; behind
        # the control, which ends the first run, the next fragment carries the creator's length
        assert len(s.launches) == 1
        for key in mixed:
            ps = [p for _, p in where[key]]
            assert ps == list(range(ps[0], ps[0] + len(ps))) and ps[0] // s.block == ps[-1] // s.block
            kinds = [s.tags[p].kind for p in ps]
            c = kinds.index("own")
            assert c > 0 and (c + 1 == len(ps) or s.tags[ps[c + 1]].blen == s.S[key])
    assert all(f.startswith(("fused", "split", "pipelined", "dev")) for f in RL.forms_of(s))


def test_stream_sizes():
    st = RL.default_streams()
    sizes = {(s.stride, S) for s in st.values() for k, S in s.S.items() if S > 16}
    assert {(64, 256), (64, 768), (64, 4096), (1472, 256), (1472, 768), (1472, 4096), (8976, 4 << 20)} <= sizes
    big = st["a8976"]
    assert sum(1 for t in big.tags if t.key == (RL.EV0, RL.DATA_ID) and t.kind in ("creator", "rest", "join")) == 470
    for s in st.values():
        pays = [t.pl for t in s.tags if t.kind != "whole" and s.S[t.key] <= 4096]
        assert 16 <= min(pays) and max(pays) <= 64


# ----------------------------------------------------------------------------------
# the reference-order streams


@pytest.mark.parametrize("seed", SEEDS)
def test_restamped_streams_hold_drops_and_joins(seed):
    pk, ln, stride, _, sub = RL.restamped_stream(seed)
    assert sub < RL.MAX_SUB
    hole, drops, joined = RL.model(pk, ln)
    assert not hole and drops >= 1 and joined >= 1, (drops, joined)
    # some key's fragments announce more than one length
    lens = {}
    for p in range(len(ln)):
        ok, d, off, blen, ev, _ = O.re_parse(pk[p, 16:36].tobytes())
        if ok and int(ln[p]) >= 36:
            lens.setdefault((ev, d), set()).add(blen)
    assert any(len(v) > 1 for v in lens.values())


def test_restamped_offset_zero_fragments_over_the_seeds():
    # offset-0 fragments are among the re-stamped ones: they start items of the other length
    n = 0
    from test_gpu_reference_order import _draw
    for seed in SEEDS:
        pk, ln, _, _, sub = RL.restamped_stream(seed)
        base = _draw(seed * 1000 + sub)[0]
        for p in np.nonzero((pk != base).any(axis=1))[0]:
            n += O.re_parse(pk[p, 16:36].tobytes())[2] == 0
    assert n >= 3


def test_the_model_agrees_with_the_oracle_on_data_errors():
    # model's drops + own-length drops == the oracle's dataErrCnt, seed by seed
    for seed in SEEDS:
        pk, ln, _, _, _ = RL.restamped_stream(seed)
        own = 0
        for p in range(len(ln)):
            ok, d, off, blen, ev, _ = O.re_parse(pk[p, 16:36].tobytes())
            own += ok and int(ln[p]) >= 36 and off + int(ln[p]) - 36 > blen
        r = O.Reassembler(True)
        r.push_batch(pk, ln)
        assert r.stats()["dataErrCnt"] == own + RL.model(pk, ln)[1]


def test_chunk_straddler_has_every_feature_in_every_chunk():
    pk, ln, stride, tags = RL.chunk_straddler()
    mine = [p for p, t in enumerate(tags) if t.key == RL.CHUNK_KEY]
    assert mine == list(range(mine[0], mine[0] + len(mine))) and len(mine) > 3 * 64
    assert not RL.model(pk, ln)[0]
    # replay the key's fragments: per 64-chunk of the walk, which events happen
    feats = [set() for _ in range((len(mine) + 63) // 64)]
    S, cur = None, 0
    for i, p in enumerate(mine):
        t = tags[p]
        f = feats[i // 64]
        if t.off == 0 or S is None:
            if t.off == 0 and i > 0:
                assert t.blen != prev_S
                f.add("restart")
            S, cur = t.blen, 0
        if t.off + t.pl > S:
            assert t.kind == "viol"
            f.add("viol")
            continue
        cur += t.pl
        prev_S = S
        if cur == S:
            f.add("completion")
            S = None
    assert all(f == {"restart", "viol", "completion"} for f in feats), feats


# ----------------------------------------------------------------------------------
# the oracle under AddressSanitizer


def _two_datagrams():
    """Key 42: offset 0, length 256, payload 64; then offset 1024, length 4096, payload 64."""
    a = RC.dgram(42, 1, 0, 256, bytes(range(64)), 128, True)
    b = RC.dgram(42, 1, 1024, 4096, bytes(range(64, 128)), 128, True)
    return np.stack([a[0], b[0]]), np.array([a[1], b[1]], np.uint32), 128


def _checksum(b):
    a = np.frombuffer(b, np.uint8).astype(np.uint64)
    return int((a * np.arange(1, a.size + 1, dtype=np.uint64)).sum(dtype=np.uint64)) if a.size else 0


def _expected_text(pk, ln):
    r = O.Reassembler(True)
    r.set_time(100)
    r.push_batch(pk, ln)
    st = r.stats()
    lines = ["stats " + " ".join(str(st[k]) for k in ("enqueueLoss", "reassemblyLoss", "eventSuccess", "totalBytes",
                                                        "totalPackets", "badHeaderDiscards", "dataErrCnt", "inProgress"))]
    for b, e, d, nf in r.pop_all_frags():
        lines.append(f"event {e} {d} {len(b)} {nf} {_checksum(b):016x}")
    r.set_time(1100)
    r.gc(500)
    lines += [f"lost {e} {d} {nf}" for e, d, nf in r.lost_pop_all()]
    st = r.stats()
    lines.append(f"after {st['reassemblyLoss']} {st['inProgress']}")
    return lines


@pytest.fixture(scope="module")
def asan_prog(tmp_path_factory):
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    d = tmp_path_factory.mktemp("streams")
    flags = ["-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the skip is decided on a program that holds none of the project's code: whether this cc
    # can build and run anything with the sanitizers.  After that every failure is a failure.
    probe = d / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run([cc] + flags + ["-o", str(d / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("cc cannot build a program with the sanitizers")
    exe = str(d / "stream_prog")
    src = [os.path.join(O.ORACLE_DIR, f) for f in ("asan_stream.c", "e2sar_oracle.c")]
    r = subprocess.run([cc] + flags + ["-o", exe] + src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, d


@pytest.mark.parametrize("name", ["two"] + list(RL.default_streams()) + [f"restamped{s}" for s in SEEDS] + ["straddler"])
def test_oracle_stays_in_bounds_under_the_sanitizers(asan_prog, name):
    exe, d = asan_prog
    if name == "two":
        pk, ln, stride = _two_datagrams()
    elif name == "straddler":
        pk, ln, stride = RL.chunk_straddler()[:3]
    elif name.startswith("restamped"):
        pk, ln, stride = RL.restamped_stream(int(name[9:]))[:3]
    else:
        s = RL.default_streams()[name]
        pk, ln, stride = s.rows, s.lens, s.stride
    path = d / f"{name}.stream"
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", stride, len(ln)))
        f.write(np.ascontiguousarray(ln, "<u4").tobytes())
        f.write(np.ascontiguousarray(pk, np.uint8).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    os.unlink(path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == _expected_text(pk, ln)
    if name == "two":
        assert r.stdout.startswith("stats 0 0 0 200 2 0 1 1\n") and "lost 42 1 1\n" in r.stdout
