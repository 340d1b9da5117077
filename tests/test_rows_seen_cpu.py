"""The seen calls without a GPU: the model tests/rows_seen_ref.py against rows_ref on streams that
repeat nothing, the hole that a duplicate and a loss leave in a plain window, a random family of
drops, duplicates and shuffles, the division bufferOffset / fragBytes as the host and the kernel
compute it (e2sar_amd/csrc/rows_div.hpp, compiled for the host), the layout of
e2sar_hip_rows_seen, and RowWindow's argument checks."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_ffi as O
import reas_cuts as RC
import rows_ref as RR
import rows_seen_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stride(max_pld):
    return (36 + max_pld + 15) // 16 * 16


def _segment(rng, ev, d, size, max_pld, stride):
    data = rng.integers(0, 256, size, dtype=np.uint8)
    pk, ln = O.segment_event(data, ev & RR.M64, d, ev & 0xFFFF, ev & RR.M64, 2, max_pld, stride)
    return data, [(pk[i], int(ln[i])) for i in range(len(ln))]


def _feed(w, dgrams, stride):
    for slot, n in dgrams:
        w.push(slot.tobytes(), n, stride)


# ----------------------------------------------------------------------------------
# (a) nothing twice, everything on the grid: rows_ref


@pytest.mark.parametrize("order", [0, 1, "in order"])
@pytest.mark.parametrize("mtu", [100, 1500])
def test_equals_rows_ref_without_duplicates(mtu, order):
    max_pld = O.max_pld_len(mtu)
    stride = _stride(max_pld)
    rng = np.random.default_rng([mtu, 1])
    ids, pitch = [7, 9], 4096
    sizes = [1, max_pld - 1, max_pld, max_pld + 1, 3 * max_pld + 5, 4096, 5000, 2 * max_pld]
    dgrams = []
    for e, s in enumerate(sizes):
        for d in ids:
            dgrams += _segment(rng, 100 + e, d, s, max_pld, stride)[1]
    dgrams.append(RC.dgram(105, 7, 5, sizes[5], b"", stride, True))     # no bytes: accepted off the grid, no bit
    dgrams.append(RC.dgram(99, 7, 0, 16, b"x" * 16, stride, True))      # late
    dgrams.append(RC.dgram(103, 8, 0, 16, b"x" * 16, stride, True))     # foreign
    if order != "in order":
        random.Random(order).shuffle(dgrams)
    plain = RR.Window(ids, 8, pitch, 100)
    seen = SR.SeenWindow(ids, 8, pitch, max_pld, 256, 100)             # 5000 bytes are 139 fragments at MTU 100
    _feed(plain, dgrams[:40], stride)
    _feed(seen, dgrams[:40], stride)
    for w in (plain, seen):
        w.advance(2)
    _feed(plain, dgrams[40:], stride)
    _feed(seen, dgrams[40:], stride)
    assert seen.counts == plain.counts and seen.counts[SR.C_DUPLICATE] == 0
    assert seen.cells() == plain.cells() and seen.base == plain.base == 102
    assert (seen.out == plain.out).all()
    assert plain.counts[RR.C_COMPLETE] > 0 and plain.counts[RR.C_LATE] > 0
    # the bits: one per accepted fragment of more than 0 bytes
    bits = sum(bin(s).count("1") for s in seen.seen)
    assert 0 < bits < seen.counts[RR.C_ACCEPTED]


# ----------------------------------------------------------------------------------
# (b) the hole


def hole_example():
    """A 48-byte event in three 16-byte fragments: -> (fragment 0, fragment 0 again, fragment 2), fragment 1."""
    frag = [RC.dgram(3, 7, 16 * j, 48, bytes([0x10 + j]) * 16, 64, True) for j in range(3)]
    return [frag[0], frag[0], frag[2]], frag[1]


def test_hole_example():
    sent, missing = hole_example()
    plain = RR.Window([7], 8, 256)
    _feed(plain, sent, 64)
    c = plain.cell_index(3, 7)
    # the plain window: COMPLETE with the fill still in the row
    assert plain.cells()[c] == ((3 << RR.ACC_SHIFT) | 48, 48, RR.COMPLETE) and plain.counts[RR.C_COMPLETE] == 1
    assert (plain.out.reshape(-1, 256)[c][16:32] == RR.FILL).all()
    seen = SR.SeenWindow([7], 8, 256, 16, 128)
    _feed(seen, sent, 64)
    assert seen.cells()[c] == ((2 << RR.ACC_SHIFT) | 32, 48, 0)
    assert seen.counts[SR.C_DUPLICATE] == 1 and seen.counts[RR.C_COMPLETE] == 0 and seen.counts[RR.C_ACCEPTED] == 2
    assert seen.seen_words()[c] == [0b101, 0, 0, 0]
    _feed(seen, [missing], 64)
    assert seen.cells()[c] == ((3 << RR.ACC_SHIFT) | 48, 48, RR.COMPLETE) and seen.counts[RR.C_COMPLETE] == 1
    row = seen.out.reshape(-1, 256)[c]
    assert row[:48].tobytes() == bytes([0x10]) * 16 + bytes([0x11]) * 16 + bytes([0x12]) * 16 and (row[48:] == RR.FILL).all()


def test_grid_rules_and_empty_fragment():
    """Rule 4b's three refusals open nothing and set no bit; a fragment of no bytes is accepted
    off the grid, twice, and sets no bit."""
    w = SR.SeenWindow([7], 8, 256, 16, 128)
    bad = [RC.dgram(1, 7, 8, 4000, b"a" * 8, 64, True),             # off the grid
           RC.dgram(1, 7, 16, 4000, b"a" * 17, 64, True),           # longer than fragBytes
           RC.dgram(1, 7, 128 * 16, 4000, b"a" * 16, 64, True)]     # f == maxFrags
    _feed(w, bad, 64)
    assert w.counts[RR.C_DATA_ERR] == 3 and all(c == (0, 0, 0) for c in w.cells()) and not any(w.seen)
    empty = RC.dgram(1, 7, 5, 4000, b"", 64, True)
    _feed(w, [empty, empty, RC.dgram(1, 7, 127 * 16, 4000, b"a" * 16, 64, True)], 64)
    c = w.cell_index(1, 7)
    assert w.cells()[c] == ((3 << RR.ACC_SHIFT) | 16, 4000, RR.TRUNCATED) and w.seen[c] == 1 << 127
    assert w.counts[SR.C_DUPLICATE] == 0 and w.counts[RR.C_ACCEPTED] == 3


# ----------------------------------------------------------------------------------
# (c) drops, duplicates, shuffles


def random_family(seed, n_events=64, ids=(7, 9), max_pld=28, p_drop=0.16, p_dup=0.3):
    """-> (stride, datagrams, {(ev, id): (source bytes, every fragment arrived)})."""
    rng = np.random.default_rng(seed)
    stride = _stride(max_pld)
    dgrams, cells = [], {}
    for e in range(n_events):
        for d in ids:
            size = int(rng.integers(2 * max_pld + 1, 6 * max_pld))
            data, frags = _segment(rng, e, d, size, max_pld, stride)
            kept = [fr for fr in frags if rng.random() >= p_drop]
            cells[(e, d)] = (data, len(kept) == len(frags), bool(kept))
            for fr in kept:
                dgrams += [fr] * (1 + int(rng.random() < p_dup) + int(rng.random() < p_dup / 4))
    random.Random(seed).shuffle(dgrams)
    return stride, dgrams, cells


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_family(seed):
    pitch = 256
    stride, dgrams, cells = random_family(seed)
    w = SR.SeenWindow([7, 9], 64, pitch, 28, 128)
    cut = len(dgrams) // 3
    _feed(w, dgrams[:cut], stride)
    _feed(w, dgrams[cut:], stride)
    state = w.cells()
    opened = whole = holed = 0
    for (e, d), (data, all_arrived, any_arrived) in cells.items():
        c = w.cell_index(e, d)
        _, S, flags = state[c]
        assert (S != 0) == any_arrived
        if not S:
            continue
        opened += 1
        assert S == len(data)
        if flags & RR.COMPLETE:                                   # a COMPLETE cell is its source
            n = min(S, pitch)
            assert w.out.reshape(-1, pitch)[c][:n].tobytes() == data[:n].tobytes()
        assert bool(flags & RR.COMPLETE) == all_arrived           # and every whole cell is COMPLETE
        whole += all_arrived
        holed += not all_arrived
    assert whole * 4 >= opened and holed * 4 >= opened, (whole, holed, opened)
    assert w.counts[SR.C_DUPLICATE] * 8 >= w.counts[RR.C_ACCEPTED] > 0
    # the same stream through the plain model: some cell is COMPLETE with a hole, the fault the bits close
    plain = RR.Window([7, 9], 64, pitch)
    _feed(plain, dgrams, stride)
    wrong = sum(1 for (e, d), (_, all_arrived, _a) in cells.items()
                if plain.cells()[plain.cell_index(e, d)][2] & RR.COMPLETE and not all_arrived)
    assert wrong > 0


# ----------------------------------------------------------------------------------
# (d) the division

DIV_N = sorted({n & 0xFFFFFFFF for b in (0, 1436, 8936, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 8936, 2 ** 32 - 1436, 2 ** 32)
                for n in range(b - 3, b + 4) if 0 <= n < 2 ** 32} | {1436 * 731, 8936 * 118, 1436 * 2990865, 8936 * 480636})
DIV_D = [1, 2, 3, 16, 28, 1435, 1436, 1437, 8936, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1]

DIV_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "rows_div.hpp"
int main(int argc, char **argv)
{
    for (int k = 1; k + 1 < argc; k += 2) {
        const uint32_t n = (uint32_t)strtoull(argv[k], nullptr, 10), d = (uint32_t)strtoull(argv[k + 1], nullptr, 10);
        const e2sar_amd::RowsQuot v = e2sar_amd::rows_div(n, d, e2sar_amd::rows_div_magic(d));
        printf("%u %u %llu\n", v.q, v.r, (unsigned long long)e2sar_amd::rows_div_magic(d));
    }
    return 0;
}
"""


def test_division_edge_values(tmp_path):
    pairs = [(n, d) for n in DIV_N for d in DIV_D]
    assert {1, 1436, 8936, 2 ** 31 + 1} <= set(DIV_D) and max(DIV_N) == 2 ** 32 - 1
    for n, d in pairs:                                            # the model's form
        assert SR.div(n, d) == (n // d, n % d)
    src = tmp_path / "div.cpp"
    src.write_text(DIV_MAIN)
    exe = tmp_path / "div"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "e2sar_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [str(v) for p in pairs for v in p]
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True, check=True).stdout.split("\n")
    for (n, d), line in zip(pairs, out):                          # the library's form, compiled for the host
        assert [int(v) for v in line.split()] == [n // d, n % d, SR.magic(d)], (n, d)
    assert len(out) == len(pairs) + 1


# ----------------------------------------------------------------------------------
# (e) the struct

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "e2sar_hip.h"
_Static_assert(sizeof(e2sar_hip_rows) == 64, "e2sar_hip_rows is 64 bytes");
_Static_assert(sizeof(e2sar_hip_rows_seen) == 16, "e2sar_hip_rows_seen is 16 bytes");
_Static_assert(offsetof(e2sar_hip_rows_seen, d_seen) == 0, "d_seen comes first");
_Static_assert(offsetof(e2sar_hip_rows_seen, fragBytes) == 8, "fragBytes follows the pointer");
_Static_assert(offsetof(e2sar_hip_rows_seen, maxFrags) == 12, "maxFrags is the last word");
int main(void)
{
    int (*r)(e2sar_hip_ctx *, const e2sar_hip_rows *, const e2sar_hip_rows_seen *, const uint8_t *, uint32_t, const uint32_t *,
             const uint32_t *, uint32_t, void *) = e2sar_hip_rows_reassemble_seen;
    int (*a)(e2sar_hip_ctx *, const e2sar_hip_rows *, const e2sar_hip_rows_seen *, const uint32_t *, uint32_t, void *) =
        e2sar_hip_rows_advance_seen;
    int (*c)(e2sar_hip_ctx *, const e2sar_hip_rows *, const e2sar_hip_rows_seen *, uint64_t, void *) = e2sar_hip_rows_clear_seen;
    size_t (*b)(uint32_t, uint32_t, uint32_t) = e2sar_hip_rows_seen_bytes;
    printf("%zu %zu %zu %d\n", sizeof(e2sar_hip_rows_seen), offsetof(e2sar_hip_rows_seen, fragBytes),
           offsetof(e2sar_hip_rows_seen, maxFrags), r && a && c && b);
    return 0;
}
"""


def test_struct_layout(tmp_path):
    from e2sar_amd import _capi
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT)
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    S = _capi.RowsSeen
    assert [C.sizeof(S), S.d_seen.offset, S.fragBytes.offset, S.maxFrags.offset] == [16, 0, 8, 12]
    assert C.sizeof(_capi.Rows) == 64
    L = _capi.lib()
    assert L.e2sar_hip_rows_seen_bytes(8, 3, 128) == 8 * 3 * 16
    assert L.e2sar_hip_rows_seen_bytes(1 << 20, 64, 1 << 20) == (1 << 20) * 64 * (1 << 17)


# ----------------------------------------------------------------------------------
# (f) RowWindow's arguments


def test_row_window_arguments():
    from e2sar_amd.sar import RowWindow
    assert RowWindow.seen_frags(256, None) == 0
    assert RowWindow.seen_frags(256, 16) == 128 and RowWindow.seen_frags(65792, 28) == 2432
    assert RowWindow.seen_frags(1 << 20, 1436) == 768 and RowWindow.seen_frags(128 * 1436, 1436) == 128
    assert RowWindow.seen_frags(128 * 1436 + 256, 1436) == 256 and RowWindow.seen_frags(256, 16, 1024) == 1024
    for kw in (dict(max_frags=128), dict(frag_bytes=0), dict(frag_bytes=-5), dict(frag_bytes=1 << 32),
               dict(frag_bytes=16, max_frags=0), dict(frag_bytes=16, max_frags=64), dict(frag_bytes=16, max_frags=129),
               dict(frag_bytes=16, max_frags=1 << 32)):
        with pytest.raises(ValueError):                           # refused before the context is touched
            RowWindow(None, [7], 8, 256, **kw)
        with pytest.raises(ValueError):
            RowWindow.for_rank(None, [7], 8, 256, 2, 1, **kw)
