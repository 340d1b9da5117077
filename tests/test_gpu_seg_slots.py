"""seg_kernel byte for byte over whole slots: every launch form of the segmentation C ABI
against the host model of tests/seg_ref.py.

Each case segments into canary-filled packet and lens buffers with a guard at both ends and
compares the buffers whole: the datagram bytes, the zeros up to the end of each datagram's
last 16-byte chunk, and the canary everywhere the contract leaves alone.  The source arena
holds random non-zero bytes with the events packed back to back at every address residue
mod 16, so a missing tail mask shows as a neighbour's bytes in a slot.  The calls go through
the C ABI itself because the stride and maxPacketsPerEvent must be settable.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import oracle_ffi as O
import seg_ref as M

pytestmark = pytest.mark.gpu

MATRIX_PLD = [1, 3, 4, 5, 8, 11, 12, 13, 16, 20, 24, 28, 44, 1435, 1436, 8936]
VERSIONS = [2, 3]
SEG_EVENT = np.dtype([("data", "<u8"), ("eventNum", "<u8"), ("lbTick", "<u8"), ("bytes", "<u4"), ("pktBase", "<u4"),
                      ("dataId", "<u2"), ("entropy", "<u2"), ("reserved", "<u4")])
assert SEG_EVENT.itemsize == 40


def _subset_lengths(max_pld):
    return [1, 5, 12, 13, 17, max_pld - 1, max_pld, max_pld + 1, 3 * max_pld - 1, 3 * max_pld + 1]


@functools.lru_cache(maxsize=None)
def _batch(max_pld, kind):
    """-> (arena, event table) of the alignment x tail matrix ("matrix") or its subset, built once."""
    cases = M.matrix_cases(max_pld, None if kind == "matrix" else _subset_lengths(max_pld))
    offs, lens, need = M.pack_events(cases)
    return M.random_arena(need, 1000 + max_pld), M.make_events(offs, lens, max_pld, seed=max_pld)


@functools.lru_cache(maxsize=None)
def _expected(max_pld, kind, stride, ver, count=None):
    arena, ev = _batch(max_pld, kind)
    pk0, ln0 = M.canary_buffers(M.total_packets(ev, max_pld), stride)
    pk, ln = M.expected(arena, ev, max_pld, stride, ver, pk0, ln0, count)
    pk.setflags(write=False)
    ln.setflags(write=False)
    return pk, ln


def _table(ev, base):
    t = np.zeros(len(ev), SEG_EVENT)
    t["data"] = np.uint64(base) + ev["off"]
    for f in ("eventNum", "lbTick", "bytes", "pktBase", "dataId", "entropy"):
        t[f] = ev[f]
    return t


class _Launch:
    """One segmentation launch of `ev` over fresh canary buffers, and what it left."""

    def __init__(self, hip, arena, ev, max_pld, stride, ver, mpe=None, form="batch", count=None, reas=None):
        import torch
        from e2sar_amd._capi import check, lib
        dev = hip.torch_device
        n = M.total_packets(ev, max_pld)
        pk0, ln0 = M.canary_buffers(n, stride)
        self.arena = torch.from_numpy(arena).to(dev)
        assert self.arena.data_ptr() % 16 == 0
        self.table = torch.from_numpy(_table(ev, self.arena.data_ptr()).view(np.uint8)).to(dev)
        self.pkts = torch.from_numpy(pk0).to(dev)
        self.lens = torch.from_numpy(ln0.view(np.int32)).to(dev)
        self.n, self.stride = n, stride
        mpe = M.max_packets(ev, max_pld) if mpe is None else mpe
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        stream = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
        out = (p(self.pkts, M.GUARD), stride, p(self.lens, 4 * M.GUARD_LENS))
        if form == "batch":
            check(lib().e2sar_hip_segment_batch(hip.handle, p(self.table), len(ev), mpe, ver, max_pld, 0, *out, stream))
        elif form == "dev":
            self.counts = torch.tensor([count, 0x5A5A5A5A], dtype=torch.int32, device=dev)
            check(lib().e2sar_hip_segment_batch_dev(hip.handle, p(self.table), p(self.counts), len(ev), mpe, ver,
                                                    max_pld, *out, stream))
        else:
            check(lib().e2sar_hip_segment_batch_recycle(hip.handle, p(self.table), len(ev), mpe, ver, max_pld, 0, *out,
                                                        reas.handle, 1, stream))
        torch.cuda.synchronize()

    def check(self, want_pk, want_ln, what):
        got_ln = self.lens.cpu().numpy().view(np.uint32)
        bad = np.nonzero(got_ln != want_ln)[0]
        assert bad.size == 0, (f"{what}: {bad.size} lens entries differ, first at slot {int(bad[0]) - M.GUARD_LENS}: "
                               f"got {int(got_ln[bad[0]]):#x}, want {int(want_ln[bad[0]]):#x}")
        diff = M.first_difference(self.pkts.cpu().numpy(), want_pk, self.stride)
        assert diff is None, f"{what}: {diff}"


# ----------------------------------------------------------------------------------
# (a) alignment x tail matrix


@pytest.mark.parametrize("ver", VERSIONS)
@pytest.mark.parametrize("max_pld", MATRIX_PLD)
def test_matrix(hip, max_pld, ver):
    arena, ev = _batch(max_pld, "matrix")
    stride = M.min_stride(max_pld)
    _Launch(hip, arena, ev, max_pld, stride, ver).check(*_expected(max_pld, "matrix", stride, ver), f"maxPld {max_pld} v{ver}")


# ----------------------------------------------------------------------------------
# (b) wider strides: chunks wholly past a full datagram's end


@pytest.mark.parametrize("ver", VERSIONS)
@pytest.mark.parametrize("max_pld,mult", [(p, s) for p in (12, 1436) for s in ("min", "min+16", "2min", 4096)])
def test_strides(hip, max_pld, mult, ver):
    lo = M.min_stride(max_pld)
    stride = {"min": lo, "min+16": lo + 16, "2min": 2 * lo}.get(mult, mult)
    arena, ev = _batch(max_pld, "subset")
    _Launch(hip, arena, ev, max_pld, stride, ver).check(*_expected(max_pld, "subset", stride, ver),
                                                        f"maxPld {max_pld} stride {stride} v{ver}")


# ----------------------------------------------------------------------------------
# (c) unit boundaries, both instantiations


@functools.lru_cache(maxsize=None)
def _unit_batch(max_pld, stride, U):
    """Events whose chunk count npk * spc is 256 * U * m - 1, that, and + 1 for m = 1, 2 (the
    nearest reachable counts where spc does not divide it), each ending in a 1-byte and in a
    full last datagram; for U = 4 one more event of just over 2^18 chunks, which is what
    selects seg_kernel<4> under an exact maxPacketsPerEvent."""
    spc = stride // 16
    npks = sorted({n for m in (1, 2) for t in (-1, 0, 1) for n in M.npk_near(256 * U * m + t, spc)})
    cases = [((4 * k + (3 if k % 5 == 4 else 0)) % 16, (n - 1) * max_pld + tail)
             for k, (n, tail) in enumerate((n, tail) for n in npks for tail in (1, max_pld))]
    if U == 4:
        cases.insert(len(cases) // 2, (8, ((1 << 18) // spc + 1) * max_pld - 1))
    offs, lens, need = M.pack_events(cases)
    ev = M.make_events(offs, lens, max_pld, seed=U)
    assert (M.max_packets(ev, max_pld) * spc > 1 << 18) == (U == 4)
    return M.random_arena(need, 77 + U), ev


@pytest.mark.parametrize("ver", VERSIONS)
@pytest.mark.parametrize("U", [2, 4])
@pytest.mark.parametrize("max_pld,stride", [(12, 48), (28, 64), (1436, 1472)])
def test_unit_boundaries(hip, max_pld, stride, U, ver):
    arena, ev = _unit_batch(max_pld, stride, U)
    pk0, ln0 = M.canary_buffers(M.total_packets(ev, max_pld), stride)
    _Launch(hip, arena, ev, max_pld, stride, ver).check(*M.expected(arena, ev, max_pld, stride, ver, pk0, ln0),
                                                        f"maxPld {max_pld} U {U} v{ver}")


@pytest.mark.parametrize("ver", VERSIONS)
@pytest.mark.parametrize("max_pld", [12, 1436])
def test_matrix_inflated_bound(hip, max_pld, ver):
    """maxPacketsPerEvent is an upper bound: one past 2^18 chunks runs seg_kernel<4> over the
    same events, and the buffers must be those of the exact bound."""
    arena, ev = _batch(max_pld, "matrix")
    stride = M.min_stride(max_pld)
    mpe = (1 << 18) // (stride // 16) + 1
    assert mpe > M.max_packets(ev, max_pld)
    _Launch(hip, arena, ev, max_pld, stride, ver, mpe=mpe).check(*_expected(max_pld, "matrix", stride, ver),
                                                                 f"maxPld {max_pld} v{ver} bound {mpe}")


# ----------------------------------------------------------------------------------
# (d) event count read on the device


@pytest.mark.parametrize("count", ["0", "1", "n-1", "n"])
@pytest.mark.parametrize("max_pld,ver", [(12, 3), (1436, 2)])
def test_device_count(hip, max_pld, ver, count):
    arena, ev = _batch(max_pld, "subset")
    assert ev["bytes"][-1] > 0 and ev["bytes"][0] > 0
    count = {"0": 0, "1": 1, "n-1": len(ev) - 1, "n": len(ev)}[count]
    stride = M.min_stride(max_pld)
    call = _Launch(hip, arena, ev, max_pld, stride, ver, form="dev", count=count)
    call.check(*_expected(max_pld, "subset", stride, ver, count), f"maxPld {max_pld} count {count}")
    assert call.counts.cpu().tolist() == [count, 0x5A5A5A5A]


# ----------------------------------------------------------------------------------
# (e) recycle blocks behind the segmentation blocks


def test_recycle_form(hip):
    from e2sar_amd import sar
    max_pld, ver = 1436, 2
    arena, ev = _batch(max_pld, "matrix")
    stride = M.min_stride(max_pld)
    want = _expected(max_pld, "matrix", stride, ver)
    first = _Launch(hip, arena, ev, max_pld, stride, ver)
    first.check(*want, "plain form")
    # a reassembler with completed events and one in progress (the last datagram held back)
    R = sar.DeviceReassembler(hip, with_lb_header=True, arena_bytes=1 << 22)
    R.reassemble(first.pkts[M.GUARD:], stride, first.lens[M.GUARD_LENS:], first.n - 1)
    before = R.stats()
    assert before.inProgress == 1 and before.arenaUsed > 0 and before.tableUsed > 0 and before.errorFlags == 0
    _Launch(hip, arena, ev, max_pld, stride, ver, form="recycle", reas=R).check(*want, "recycle form")
    after = R.stats()
    assert (after.arenaUsed, after.tableUsed, after.inProgress) == (0, 0, 0)
    R.close()


# ----------------------------------------------------------------------------------
# (f) large indices, verified on the device


def _all(ok, flags, what):
    flags.append((what, ok.all()))


def _large(hip, max_pld, stride, nbytes, ver):
    """One event of nbytes at a 256-byte aligned address; every check is a torch op over
    [npk, stride] views, at most 1 GiB of slots at a time.  -> seconds spent in the launch."""
    import torch
    from e2sar_amd._capi import check, lib
    dev = hip.torch_device
    npk = -(-nbytes // max_pld)
    nfull, rem = divmod(nbytes, max_pld)
    gen = torch.Generator(device=dev)
    gen.manual_seed(nbytes % 1000003 + ver)
    src = torch.randint(-2**63, 2**63 - 1, ((nbytes + 64 + 7) // 8,), dtype=torch.int64, device=dev,
                        generator=gen).view(torch.uint8)
    buf = torch.full((2 * M.GUARD + npk * stride,), M.CANARY, dtype=torch.uint8, device=dev)
    lens = torch.full((2 * M.GUARD_LENS + npk,), M.CANARY_LEN - 2**32, dtype=torch.int32, device=dev)
    ev = M.make_events([0], [nbytes], max_pld, seed=ver)
    assert int(ev["bytes"][0]) == nbytes and npk * (stride // 16) < 2**32
    table = torch.from_numpy(_table(ev, src.data_ptr()).view(np.uint8)).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    check(lib().e2sar_hip_segment_batch(hip.handle, C.c_void_p(table.data_ptr()), 1, npk, ver, max_pld, 1,
                                        C.c_void_p(buf.data_ptr() + M.GUARD), stride,
                                        C.c_void_p(lens.data_ptr() + 4 * M.GUARD_LENS),
                                        C.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
    torch.cuda.synchronize()
    t_launch = time.perf_counter() - t0

    flags = []
    _all(buf[:M.GUARD] == M.CANARY, flags, "front guard")
    _all(buf[M.GUARD + npk * stride:] == M.CANARY, flags, "back guard")
    _all(lens[:M.GUARD_LENS] == M.CANARY_LEN - 2**32, flags, "lens front guard")
    _all(lens[M.GUARD_LENS + npk:] == M.CANARY_LEN - 2**32, flags, "lens back guard")
    _all(lens[M.GUARD_LENS:M.GUARD_LENS + nfull] == M.HDR + max_pld, flags, "lens of the full datagrams")
    if rem:
        _all(lens[M.GUARD_LENS + nfull] == M.HDR + rem, flags, "lens of the last datagram")
    e = ev[0]
    hdr = torch.from_numpy(np.frombuffer(O.lbre_hdr(ver, int(e["entropy"]), int(e["lbTick"]), int(e["dataId"]), 0, nbytes,
                                                    int(e["eventNum"])), np.uint8).copy()).to(dev)
    slots = buf[M.GUARD:M.GUARD + npk * stride].view(npk, stride)
    pad = M.min_stride(max_pld)                         # where a full datagram's last chunk ends
    step = max(1, (1 << 30) // stride)
    for a in range(0, npk, step):
        b = min(a + step, npk)
        s = slots[a:b]
        _all(s[:, :20] == hdr[:20], flags, f"header bytes 0..19, datagrams {a}..{b}")
        _all(s[:, 24:36] == hdr[24:], flags, f"header bytes 24..35, datagrams {a}..{b}")
        off = torch.arange(a, b, dtype=torch.int64, device=dev) * max_pld
        want = torch.stack([(off >> 24) & 255, (off >> 16) & 255, (off >> 8) & 255, off & 255], 1).to(torch.uint8)
        _all(s[:, 20:24] == want, flags, f"bufferOffset, datagrams {a}..{b}")
        f = min(b, nfull)                               # full datagrams of this piece: [a, f)
        if f > a:
            _all(s[:f - a, 36:36 + max_pld] == src[a * max_pld:f * max_pld].view(f - a, max_pld), flags,
                 f"payload, datagrams {a}..{f}")
            _all(s[:f - a, 36 + max_pld:pad] == 0, flags, f"zero padding, datagrams {a}..{f}")
            _all(s[:f - a, pad:] == M.CANARY, flags, f"canary behind the last chunk, datagrams {a}..{f}")
    if rem:
        last, end = slots[nfull], (M.HDR + rem + 15) // 16 * 16
        _all(last[36:36 + rem] == src[nfull * max_pld:nbytes], flags, "payload of the last datagram")
        _all(last[36 + rem:end] == 0, flags, "zero padding of the last datagram")
        _all(last[end:] == M.CANARY, flags, "canary behind the last datagram")
    ok = torch.stack([f for _, f in flags]).cpu().tolist()
    failed = [w for (w, _), o in zip(flags, ok) if not o]
    if failed:
        written = (slots[:, 0] != M.CANARY).sum().item()
        ln_written = (lens[M.GUARD_LENS:M.GUARD_LENS + npk] != M.CANARY_LEN - 2**32).sum().item()
        raise AssertionError(f"{npk} datagrams expected; {written} slots and {ln_written} lens entries written; "
                             f"{len(failed)} checks failed, first: {failed[:6]}")
    return t_launch


@pytest.mark.parametrize("ver", VERSIONS)
def test_large_float_path_limit(hip, ver):
    """npk = 2^22 - 1, the last count that divides by the float reciprocal; stride 256: the
    chunk index runs to 2^26, a 1-GiB buffer of which 48 bytes per slot are written."""
    t0 = time.perf_counter()
    dt = _large(hip, 4, 256, ((1 << 22) - 1) * 4, ver)
    print(f"float path limit v{ver}: launch {dt:.3f} s, case {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("ver", VERSIONS)
def test_large_integer_path(hip, ver):
    """npk = 3 * 2^22 at stride 48: the integer division; the float form is wrong for some of
    these chunk indices (test_seg_ref_cpu.py asserts that), so the case fails without the guard."""
    t0 = time.perf_counter()
    dt = _large(hip, 4, 48, 3 * (1 << 22) * 4, ver)
    print(f"integer path v{ver}: launch {dt:.3f} s, case {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("ver", VERSIONS)
def test_large_event_just_under_4_gib(hip, ver):
    """One event of 2^32 - 1 bytes at maxPld 8936: bytes + maxPld - 1 wraps in 32 bits, and so
    does 16 * (chunk index) from chunk 2^28 on (the event has 480637 * 561 = 269 637 357)."""
    t0 = time.perf_counter()
    dt = _large(hip, 8936, 8976, 2**32 - 1, ver)
    print(f"4 GiB event v{ver}: launch {dt:.3f} s, case {time.perf_counter() - t0:.3f} s")
