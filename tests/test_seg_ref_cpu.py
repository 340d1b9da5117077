"""The host model of a segmented batch (tests/seg_ref.py) against the oracle and by hand,
the float32 restatement of div_recip at the edges of its guard, and the host-side packet
count of an event just under 4 GiB."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
import seg_ref as M

# the integer-path shape of test_gpu_seg_slots.py: maxPld 4, stride 48, npk = 3 * 2^22
INT_SPC, INT_NPK = 3, 3 << 22


@pytest.mark.parametrize("max_pld,stride,ver", [(1436, 1472, 2), (12, 48, 3), (3, 48, 2), (20, 4096, 3), (8936, 8976, 2)])
def test_model_matches_oracle_datagrams(max_pld, stride, ver):
    offs, lens, need = M.pack_events([(r, n) for r, n in zip((0, 4, 7, 13, 5), (1, max_pld, max_pld + 1, 0, 3 * max_pld - 1))])
    arena = M.random_arena(need, 1)
    ev = M.make_events(offs, lens, max_pld, seed=3)
    n = M.total_packets(ev, max_pld)
    assert n == sum(O.num_packets(int(b), max_pld) for b in lens)
    pk0, ln0 = M.canary_buffers(n, stride)
    pk, ln = M.expected(arena, ev, max_pld, stride, ver, pk0, ln0)
    slots = pk[M.GUARD:-M.GUARD].reshape(n, stride)
    for e in ev:
        data = arena[int(e["off"]):int(e["off"]) + int(e["bytes"])]
        op, ol = O.segment_event(data, int(e["eventNum"]), int(e["dataId"]), int(e["entropy"]), int(e["lbTick"]),
                                 ver, max_pld, stride)
        for k in range(len(ol)):
            s, L = int(e["pktBase"]) + k, int(ol[k])
            assert ln[M.GUARD_LENS + s] == L
            assert np.array_equal(slots[s, :L], op[k, :L])
            pad = (L + 15) // 16 * 16
            assert (slots[s, L:pad] == 0).all() and (slots[s, pad:] == M.CANARY).all()
    assert (pk[:M.GUARD] == M.CANARY).all() and (pk[-M.GUARD:] == M.CANARY).all()
    assert (ln[:M.GUARD_LENS] == M.CANARY_LEN).all() and (ln[-M.GUARD_LENS:] == M.CANARY_LEN).all()
    assert (pk0 == M.CANARY).all() and (ln0 == M.CANARY_LEN).all()          # the inputs are left alone


def test_padding_and_canary_by_hand():
    """One 25-byte event at maxPld 20, stride 64, two slots behind it kept for a second event
    past the device-side count: datagram 0 is 56 bytes (zeros to 64 = the slot's end),
    datagram 1 is 41 bytes (zeros to 48, canary from 48 to 64)."""
    arena = np.arange(1, 101, dtype=np.uint8)
    ev = M.make_events([10, 40], [25, 40], 20)
    assert list(ev["pktBase"]) == [0, 2] and M.total_packets(ev, 20) == 4 and M.max_packets(ev, 20) == 2
    pk0, ln0 = M.canary_buffers(4, 64)
    pk, ln = M.expected(arena, ev, 20, 64, 2, pk0, ln0, count=1)
    slots = pk[M.GUARD:-M.GUARD].reshape(4, 64)
    hdr0 = O.lbre_hdr(2, int(ev["entropy"][0]), int(ev["lbTick"][0]), int(ev["dataId"][0]), 0, 25, int(ev["eventNum"][0]))
    hdr1 = O.lbre_hdr(2, int(ev["entropy"][0]), int(ev["lbTick"][0]), int(ev["dataId"][0]), 20, 25, int(ev["eventNum"][0]))
    want0 = np.concatenate([np.frombuffer(hdr0, np.uint8), np.arange(11, 31, dtype=np.uint8), np.zeros(8, np.uint8)])
    want1 = np.concatenate([np.frombuffer(hdr1, np.uint8), np.arange(31, 36, dtype=np.uint8), np.zeros(7, np.uint8),
                            np.full(16, M.CANARY, np.uint8)])
    assert np.array_equal(slots[0], want0)
    assert np.array_equal(slots[1], want1)
    assert (slots[2:] == M.CANARY).all()
    assert list(ln[M.GUARD_LENS:M.GUARD_LENS + 4]) == [56, 41, M.CANARY_LEN, M.CANARY_LEN]
    full, _ = M.expected(arena, ev, 20, 64, 2, pk0, ln0)
    assert (full[M.GUARD + 128:M.GUARD + 128 + 56] != M.CANARY).any()
    assert M.first_difference(pk, pk, 64) is None
    msg = M.first_difference(full, pk, 64)
    assert "slot 2, chunk 0, byte 0" in msg, msg


def test_pack_events_back_to_back():
    cases = M.matrix_cases(12)
    offs, lens, need = M.pack_events(cases)
    assert len(cases) == 16 * len(M.matrix_lengths(12)) + 1 and (lens == 0).sum() == 1
    assert all(int(o) % 16 == r for o, (r, _) in zip(offs, cases))
    ends = offs + lens
    assert (offs[1:] >= ends[:-1]).all() and (offs[1:] - ends[:-1] < 16).all()
    assert need >= int(ends[-1]) + 4
    assert M.matrix_lengths(4) == list(range(1, 18)) + [3, 4, 5, 7, 8, 9, 11, 12, 13]
    assert M.matrix_lengths(1)[17:] == [1, 2, 1, 2, 3, 2, 3, 4]
    assert (M.random_arena(1 << 16, 0) != 0).all()


def test_div_recip_exact_below_the_guard():
    """Exact for every divisor the kernel can see (stride / 16 of a slot up to 64 KiB) at the
    three indices around each multiple, for quotients sampled up to the guard q < 2^22 with
    its top 500 included.

    The quotients are those a launch can ask for: seg_geom refuses an event of 2^32 chunks or
    more, so every index is below npk * d <= 2^32 - 1, i.e. (q + 1) * d < 2^32.  That excludes
    q = 2^22 - 1 for d = 1024, 2048 and 4096 only (index 2^32 - 1), where the correction's own
    q * d wraps and the float form is wrong; test_div_recip_wraps_at_the_top pins that."""
    rng = np.random.default_rng(5)
    sample = np.concatenate([np.arange(0, 64), rng.integers(0, 1 << 22, 1500)])
    for d in range(3, 4097):
        top = min(1 << 22, ((1 << 32) - 1) // d)
        q = np.unique(np.concatenate([sample[sample < top], np.arange(top - 500, top)])).astype(np.uint64)
        i = np.concatenate([q * d + (d - 1), q * d, (q * d)[1:] - 1])
        assert i.max() < 1 << 32
        got = M.div_recip_f32(i.astype(np.uint32), d)
        bad = np.nonzero(got != (i // d).astype(np.uint32))[0]
        assert bad.size == 0, f"d = {d}: i = {int(i[bad[0]])} gives {int(got[bad[0]])}"


def test_div_recip_wraps_at_the_top():
    """Why seg_geom's bound on an event's chunk count matters to div_recip: at index 2^32 - 1
    the estimate 2^22 times 1024 wraps to 0 and the correction goes the wrong way."""
    assert int(M.div_recip_f32(np.array([2**32 - 1], np.uint32), 1024)[0]) != (2**32 - 1) // 1024
    assert int(M.div_recip_f32(np.array([2**32 - 1025], np.uint32), 1024)[0]) == (1 << 22) - 2


def test_div_recip_wrong_on_the_integer_path_shape():
    """The chunk indices of one event of 3 * 2^22 datagrams at stride 48: the float form is
    wrong for some of them, so that shape fails on the GPU if the npk < 2^22 guard goes."""
    assert INT_NPK >= 1 << 22
    bad = 0
    for j0 in range(0, INT_NPK * INT_SPC, 1 << 22):
        j = np.arange(j0, min(j0 + (1 << 22), INT_NPK * INT_SPC), dtype=np.uint32)
        bad += int((M.div_recip_f32(j, INT_SPC) != j // np.uint32(INT_SPC)).sum())
    assert bad > 0
    # ... and not for any chunk of the float path's largest shape (maxPld 4, stride 256)
    top = (1 << 22) - 1
    j = np.arange((top - 4096) * 16, top * 16, dtype=np.uint32)
    assert np.array_equal(M.div_recip_f32(j, 16), j // np.uint32(16))


def test_seg_plan_counts_an_event_just_under_4_gib():
    from e2sar_amd import _capi
    want = -(-(2**32 - 1) // 8936)
    assert want == 480637 and want * 8936 >= 2**32 - 1 > (want - 1) * 8936
    arr = (_capi.SegEvent * 2)()
    arr[0].bytes = 2**32 - 1
    arr[1].bytes = 1
    tot, mx = C.c_uint32(), C.c_uint32()
    _capi.check(_capi.lib().e2sar_hip_seg_plan(arr, 2, 8936, C.byref(tot), C.byref(mx)))
    assert (tot.value, mx.value, arr[0].pktBase, arr[1].pktBase) == (want + 1, want, 0, want)
    assert _capi.lib().e2sar_hip_num_packets(2**32 - 1, 8936) == want
    assert int(M.num_packets(2**32 - 1, 8936)) == want


def test_model_plan_matches_seg_plan():
    from e2sar_amd import _capi
    offs, lens, _ = M.pack_events(M.matrix_cases(12))
    ev = M.make_events(offs, lens, 12)
    arr = (_capi.SegEvent * len(ev))()
    for k, e in enumerate(ev):
        arr[k].bytes = int(e["bytes"])
    tot, mx = C.c_uint32(), C.c_uint32()
    _capi.check(_capi.lib().e2sar_hip_seg_plan(arr, len(ev), 12, C.byref(tot), C.byref(mx)))
    assert [arr[k].pktBase for k in range(len(ev))] == [int(b) for b in ev["pktBase"]]
    assert (tot.value, mx.value) == (M.total_packets(ev, 12), M.max_packets(ev, 12))
