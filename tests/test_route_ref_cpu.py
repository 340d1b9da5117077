"""The host model of routing (route_ref.py) against independent witnesses: the oracle's RE
parse for the owner rule, test_dist_gloo.stable_route for the packing, a per-datagram loop
for the append runs.  No GPU."""
import numpy as np
import pytest

import oracle_ffi as O
import route_ref as RR
from test_dist_gloo import stable_route


def _mixed_batch(n, stride, with_lb, seed):
    """Valid datagrams with every edge event number, and among them each way a datagram can
    fail to parse; lens anywhere from 0 to one past the slot."""
    rng = np.random.default_rng(seed)
    ev = RR.edge_event_nums(n)
    ev[n // 2:] = RR.uniform_event_nums(n - n // 2, seed + 1)
    pk, ln = RR.make_datagrams(n, stride, ev, with_lb, seed)
    o = 16 if with_lb else 0
    hl = o + 20
    ln = rng.integers(hl, stride + 1, n).astype(np.uint32)
    kind = rng.integers(0, 12, n)
    pk[kind == 0, o] = 0x20                          # version nibble
    pk[kind == 1, o] = 0x11                          # reserved nibble of byte 0
    pk[kind == 2, o + 1] = 0x01                      # reserved byte
    ln[kind == 3] = hl - 1
    ln[kind == 4] = 0
    ln[kind == 5] = stride + 1
    ln[kind == 6] = hl                               # the shortest datagram that parses
    return pk, ln, ev


def _oracle_dests(pk, ln, stride, world, self_rank, with_lb):
    o = 16 if with_lb else 0
    out = []
    for k in range(len(ln)):
        ok, _, _, _, ev, _ = O.re_parse(pk[k, o:o + 20].tobytes())
        stays = int(ln[k]) < o + 20 or int(ln[k]) > stride or not ok
        out.append(self_rank if stays else int(ev) % world)          # Python ints: exact
    return out


def test_make_datagrams_headers_and_stamps():
    for with_lb in (True, False):
        ev = RR.edge_event_nums(300)
        pk, ln = RR.make_datagrams(300, 48, ev, with_lb, seed=3)
        assert pk.shape == (300, 48) and ln.tolist() == [48] * 300
        assert RR.stamp_of(pk).tolist() == list(range(300))
        o = 16 if with_lb else 0
        for k in range(300):
            ok, d, off, length, e, ver = O.re_parse(pk[k, o:o + 20].tobytes())
            assert ok and ver == 1 and (d, off, length) == (0x1234, k, 300)
            assert e == int(ev[k])
        assert RR.event_nums_of(pk, with_lb).tolist() == [int(x) for x in ev]
    got = set(int(x) for x in RR.edge_event_nums(10))
    assert {0, 2**32 - 1, 2**32, 2**40 + 3, 2**40 + 8, 2**64 - 1} == got


@pytest.mark.parametrize("with_lb", [True, False])
@pytest.mark.parametrize("world,self_rank", [(2, 1), (3, 0), (5, 3), (7, 6), (64, 31)])
def test_route_dests_matches_oracle_parse(world, self_rank, with_lb):
    n, stride = 400, 64
    pk, ln, ev = _mixed_batch(n, stride, with_lb, seed=world)
    want = _oracle_dests(pk, ln, stride, world, self_rank, with_lb)
    got = RR.route_dests(pk, ln, stride, world, self_rank, with_lb)
    assert got.tolist() == want
    # every way of staying home, and every edge event number, is in the batch
    o = 16 if with_lb else 0
    valid = [k for k in range(n) if o + 20 <= ln[k] <= stride and pk[k, o] == 0x10 and pk[k, o + 1] == 0]
    assert 0 < len(valid) < n
    assert {0, 2**32 - 1, 2**32, 2**64 - 1} <= {int(ev[k]) for k in valid}
    assert any(2**40 <= int(ev[k]) < 2**40 + n for k in valid)
    assert all(want[k] == int(ev[k]) % world for k in valid)
    assert all(want[k] == self_rank for k in range(n) if k not in set(valid))


def test_route_dests_needs_64_bit_modulo():
    # 2^64 - 1 and 2^32 have owners a 32-bit truncation gets wrong at an odd world
    ev = np.array([2**64 - 1, 2**32, 2**40 + 5], np.uint64)
    pk, ln = RR.make_datagrams(3, 48, ev)
    assert RR.route_dests(pk, ln, 48, 7, 0).tolist() == [(2**64 - 1) % 7, 2**32 % 7, (2**40 + 5) % 7]
    assert (2**64 - 1) % 7 != (2**32 - 1) % 7 and 2**32 % 7 != 0


@pytest.mark.parametrize("with_lb", [True, False])
@pytest.mark.parametrize("world,self_rank", [(2, 0), (3, 2), (8, 5)])
def test_stable_pack_matches_stable_route(world, self_rank, with_lb):
    n, stride = 300, 64
    pk, ln, _ = _mixed_batch(n, stride, with_lb, seed=10 + world)
    ln[ln > stride] = stride                         # stable_route has no rule for ln > stride
    dests = RR.route_dests(pk, ln, stride, world, self_rank, with_lb)
    rpk, rln, rcounts = stable_route(pk, ln, world, self_rank, with_lb)
    gpk, gln, gcounts = RR.stable_pack(pk, ln, dests, world, self_rank, False)
    assert gcounts == rcounts and sum(gcounts) == n
    np.testing.assert_array_equal(gln, rln)
    np.testing.assert_array_equal(gpk, rpk)
    # foreign only: the same packing with this rank's span cut out
    fpk, fln, fcounts = RR.stable_pack(pk, ln, dests, world, self_rank, True)
    a, m = sum(rcounts[:self_rank]), rcounts[self_rank]
    assert m > 0
    assert fcounts == rcounts[:self_rank] + [0] + rcounts[self_rank + 1:]
    np.testing.assert_array_equal(fpk, np.concatenate([rpk[:a], rpk[a + m:]]))
    np.testing.assert_array_equal(fln, np.concatenate([rln[:a], rln[a + m:]]))


@pytest.mark.parametrize("foreign_only", [False, True])
def test_append_model_matches_a_plain_loop(foreign_only):
    world, self_rank, n = 5, 2, 700
    dests = np.random.default_rng(4).integers(0, world, n)
    dests[256:512][dests[256:512] == 4] = 0          # block 1 has nothing for rank 4
    want = [dict() for _ in range(world)]
    for k in range(n):
        d = int(dests[k])
        if not (foreign_only and d == self_rank):
            want[d].setdefault(k // 256, []).append(k)
    got = RR.append_model(dests, world, self_rank, foreign_only)
    for d in range(world):
        assert [g.tolist() for g in got[d]] == [want[d][b] for b in sorted(want[d])]
    assert len(got[4]) == 2 and (got[self_rank] == []) == foreign_only
