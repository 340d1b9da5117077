"""Host model of multi-GPU routing (e2sar_amd/csrc/route.hpp) -- TEST INFRASTRUCTURE.

Plain vectorised numpy: a batch of 130 000 datagrams is built and routed in well under a
second.  The model restates the contract, not the kernels:

* ``route_dests``: a datagram goes to ``eventNum % world``; one that cannot be parsed
  (shorter than its headers, longer than its slot, version/reserved bytes other than
  ``0x10 0x00``) stays on the rank it landed on;
* ``stable_pack``: route_batch / route_foreign pack whole slots into per-destination spans,
  destinations ascending, landing order kept inside a span;
* ``append_model``: route_append adds, per destination, one contiguous run per block of
  256 datagrams, the run in landing order; the order of the runs of one batch is not fixed.
"""
from __future__ import annotations

import numpy as np

BLOCK = 256                 # datagrams per workgroup (kBlock)
LB_HDR_LEN = 16
RE_HDR_LEN = 20

# event numbers at which a 32-bit (or signed) owner computation goes wrong
EDGE_EVENTS = (0, 2**32 - 1, 2**32, 2**64 - 1)


def edge_event_nums(n: int) -> np.ndarray:
    """0, 2^32 - 1, 2^32, 2^40 + k and 2^64 - 1, cycling over the datagram index k."""
    k = np.arange(n, dtype=np.uint64)
    table = np.array(EDGE_EVENTS[:3] + (0,) + EDGE_EVENTS[3:], dtype=np.uint64)
    ev = table[(k % np.uint64(5)).astype(np.int64)]
    pick = (k % np.uint64(5)) == np.uint64(3)
    ev[pick] = np.uint64(2**40) + k[pick]
    return ev


def uniform_event_nums(n: int, seed: int) -> np.ndarray:
    """Uniform random 64-bit event numbers."""
    return np.random.default_rng(seed).integers(0, 2**64, n, dtype=np.uint64, endpoint=False)


def stamp_of(pk: np.ndarray) -> np.ndarray:
    """The datagram index make_datagrams stamped into each slot (its last 4 bytes)."""
    return np.ascontiguousarray(pk[:, -4:]).view("<u4")[:, 0].astype(np.int64)


def make_datagrams(n, stride, event_nums, with_lb=True, seed=0, ln=None, data_id=0x1234):
    """-> (pk[n, stride] uint8, ln[n] uint32).  Every byte random, then the RE header (at 16
    behind the LB header, at 0 without it): 0x10 0x00, dataId, bufferOffset = k, length = n,
    big-endian eventNum; the index k little-endian in the slot's last 4 bytes (past both
    header forms for every stride >= 48)."""
    if stride < 48 or stride % 16:
        raise ValueError("stride must be a multiple of 16, >= 48")
    rng = np.random.default_rng(seed)
    pk = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    ev = np.broadcast_to(np.asarray(event_nums, dtype=np.uint64), (n,))
    k = np.arange(n, dtype=np.uint32)
    o = LB_HDR_LEN if with_lb else 0
    pk[:, o] = 0x10
    pk[:, o + 1] = 0x00
    pk[:, o + 2:o + 4] = np.full(n, data_id, ">u2").view(np.uint8).reshape(n, 2)
    pk[:, o + 4:o + 8] = k.astype(">u4").view(np.uint8).reshape(n, 4)
    pk[:, o + 8:o + 12] = np.full(n, n, ">u4").view(np.uint8).reshape(n, 4)
    pk[:, o + 12:o + 20] = ev.astype(">u8").view(np.uint8).reshape(n, 8)
    pk[:, stride - 4:] = k.astype("<u4").view(np.uint8).reshape(n, 4)
    if ln is None:
        ln = np.full(n, stride, np.uint32)
    ln = np.ascontiguousarray(ln, np.uint32)
    if ln.shape != (n,):
        raise ValueError("ln must have one entry per datagram")
    return pk, ln


def event_nums_of(pk: np.ndarray, with_lb: bool = True) -> np.ndarray:
    o = (LB_HDR_LEN if with_lb else 0) + 12
    return np.ascontiguousarray(pk[:, o:o + 8]).view(">u8")[:, 0].astype(np.uint64)


def route_dests(pk, ln, stride, world, self_rank, with_lb=True) -> np.ndarray:
    """route_dest of the header contract, per datagram (int64)."""
    o = LB_HDR_LEN if with_lb else 0
    hl = o + RE_HDR_LEN
    ln = np.asarray(ln).astype(np.int64)
    ok = (ln >= hl) & (ln <= stride) & (pk[:, o] == 0x10) & (pk[:, o + 1] == 0x00)
    owner = (event_nums_of(pk, with_lb) % np.uint64(world)).astype(np.int64)     # exact in uint64
    return np.where(ok, owner, np.int64(self_rank))


def stable_pack(pk, ln, dests, world, self_rank, foreign_only):
    """-> (pk_out, ln_out, counts): stable per-destination spans, destinations ascending;
    foreign_only drops self_rank's span (counts[self_rank] = 0)."""
    dests = np.asarray(dests, dtype=np.int64)
    order = np.argsort(dests, kind="stable")
    if foreign_only:
        order = order[dests[order] != self_rank]
    counts = np.bincount(dests[order], minlength=world).astype(np.int64)
    return pk[order], np.asarray(ln)[order], [int(c) for c in counts]


def append_model(dests, world, self_rank, foreign_only, block=BLOCK):
    """What one batch contributes to each destination's region under route_append:
    out[d] = list of index arrays, one per block of `block` datagrams that has any datagram
    for d, each ascending.  A region receives every array as one contiguous run; the order
    of a batch's runs is the order its workgroups reserved in."""
    dests = np.asarray(dests, dtype=np.int64)
    out = [[] for _ in range(world)]
    for b0 in range(0, len(dests), block):
        blk = dests[b0:b0 + block]
        for d in np.unique(blk):
            if foreign_only and d == self_rank:
                continue
            out[int(d)].append(b0 + np.nonzero(blk == d)[0])
    return out
