"""Multi-GPU SAR: events are owned by rank ``eventNum % world``.

Normal operation needs no communication: each GPU segments and reassembles the events it
owns.  When datagrams *land* on a rank that does not own their event (a modelled NIC /
RSS spread), each rank

1. reassembles the datagrams it owns where they landed (``DeviceReassembler.set_owner``:
   the reassembler skips other ranks' events, so nothing of its own is copied twice);
2. packs the foreign ones into per-owner spans on the GPU (``PacketRouter.route`` with
   ``foreign_only=True``: gfx950 route kernels behind e2sar_hip_route_foreign);
3. ``exchange`` moves the spans with one all-to-all-v (the split sizes come from one
   all-gather of the per-rank count vectors: one host read per exchange);
4. reassembles what it received.

With the ``nccl`` backend (RCCL on ROCm) the transfer runs over xGMI, peer to peer, not as
a ring.  The reference never needs this step -- its load balancer steers every fragment of
an event to one receiver (e2sarDPSegmenter.hpp:231-235), and the receiver keys its
threads by the same eventNum (e2sarDPReassembler.hpp:224-229) -- so there is no reference
call pattern to mirror.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.distributed as dist

from ._capi import lib
from .sar import _call, _s


def owner(event_num: int, world: int) -> int:
    return int(event_num) % int(world)


def _via_host(group) -> bool:
    """gloo's collectives take host tensors (device tensors are staged through host memory)
    and have no list all-to-all: with gloo every exchange goes through all_to_all_single on
    host tensors."""
    return dist.get_backend(group) == "gloo"


# ---- the pieces of an exchange, stated once: exchange, exchange_regions and SpreadPipeline use them ----

def _splits(m: List[List[int]], rank: int) -> Tuple[List[int], List[int]]:
    """(send, recv) split sizes of `rank`: its row and its column of the count matrix."""
    return m[rank], [row[rank] for row in m]


def _any_sent(m: List[List[int]]) -> bool:
    """False when no rank sends anything: every rank then skips the collective."""
    return any(any(row) for row in m)


def _check_cap(m: List[List[int]], cap: int) -> None:
    if any(c > cap for row in m for c in row):
        raise RuntimeError(f"route regions overflowed (cap {cap} datagrams per rank): {m}")


def _recv_buffers(out, n_recv: int, stride: int, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """`out` when it is on `dev` and holds n_recv datagrams, else new receive buffers."""
    if out is not None and out[0].numel() >= n_recv * stride and out[1].numel() >= n_recv and out[0].device == dev:
        return out
    return (torch.empty(max(n_recv, 1) * stride, dtype=torch.uint8, device=dev),
            torch.empty(max(n_recv, 1), dtype=torch.int32, device=dev))


def _a2a_spans(rpk, rln, spk, sln, sc: List[int], rc: List[int], stride: int, group) -> None:
    """The all_to_all_single pair (slots, lengths) over contiguous spans in rank order; with
    gloo through host staging copies."""
    def pair(rp, rl, sp, sl):
        dist.all_to_all_single(rp, sp, [c * stride for c in rc], [c * stride for c in sc], group=group)
        dist.all_to_all_single(rl, sl, rc, sc, group=group)

    if not _via_host(group):
        return pair(rpk, rln, spk, sln)
    hpk, hln = torch.empty(rpk.numel(), dtype=torch.uint8), torch.empty(rln.numel(), dtype=torch.int32)
    pair(hpk, hln, spk.cpu(), sln.cpu())
    rpk.copy_(hpk)
    rln.copy_(hln)


def _a2a_regions(send_pk, send_ln, recv_pk, recv_ln, sc: List[int], rc: List[int], cap: int, stride: int, group):
    """All-to-all of region views: the first sc[d] slots of region d (cap slots each) of the
    send buffers go to rank d; what rank s sends lands at slot sum(rc[:s]) of the receive
    buffers.  nccl: all_to_all over the views, no packing copy; gloo: the views are
    gathered on the host and go through _a2a_spans."""
    W = len(sc)
    spk = [send_pk[d * cap * stride:(d * cap + sc[d]) * stride] for d in range(W)]
    sln = [send_ln[d * cap:d * cap + sc[d]] for d in range(W)]
    if _via_host(group):
        return _a2a_spans(recv_pk[: sum(rc) * stride], recv_ln[: sum(rc)], torch.cat([v.cpu() for v in spk]),
                          torch.cat([v.cpu() for v in sln]), sc, rc, stride, group)
    roff = [sum(rc[:s]) for s in range(W)]
    dist.all_to_all([recv_pk[roff[s] * stride:(roff[s] + rc[s]) * stride] for s in range(W)], spk, group=group)
    dist.all_to_all([recv_ln[roff[s]:roff[s] + rc[s]] for s in range(W)], sln, group=group)


def count_matrix(counts: torch.Tensor, group: Optional[dist.ProcessGroup] = None) -> List[List[int]]:
    """m[s][d] = datagrams rank s sends rank d, from every rank's count vector (on the
    device): one all-gather of the world x world matrix, then ONE host read."""
    world = dist.get_world_size(group)
    if counts.numel() != world:
        raise ValueError("counts must have one entry per rank")
    c = counts.to(torch.int64)
    if _via_host(group):
        c = c.cpu()
    rows = [torch.empty_like(c) for _ in range(world)]
    dist.all_gather(rows, c, group=group)
    return [[int(x) for x in row] for row in torch.stack(rows).tolist()]    # the one host read


def exchange_counts(counts: torch.Tensor, group: Optional[dist.ProcessGroup] = None) -> Tuple[List[int], List[int]]:
    """(send, recv) split sizes of this rank (count_matrix's row and column)."""
    return _splits(count_matrix(counts, group), dist.get_rank(group))


def exchange(send_pk: torch.Tensor, send_ln: torch.Tensor, counts: Union[Sequence[int], torch.Tensor], stride: int,
             group: Optional[dist.ProcessGroup] = None,
             out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """All-to-all-v of datagram slots.

    send_pk: uint8, sum(counts)*stride bytes, the span for rank d at offset
    sum(counts[:d])*stride; send_ln: int32 lengths in the same order; counts: datagrams per
    destination rank, either the route kernels' device vector (split sizes by
    ``exchange_counts``: one host read) or host ints (receive sizes by an all-to-all of
    the counts).  out: optional preallocated (recv_pk, recv_ln) used when large enough, so
    a steady stream of batches does not allocate per call.  Returns (recv_pk, recv_ln,
    n_recv), spans ordered by source rank.  Backends: nccl (RCCL) on device tensors; gloo,
    whose all-to-all takes host tensors, through host staging copies (the CPU rehearsal path).
    """
    world = dist.get_world_size(group)
    dev = send_pk.device
    anything = True
    if isinstance(counts, torch.Tensor):
        m = count_matrix(counts, group)
        sc, rc = _splits(m, dist.get_rank(group))
        anything = _any_sent(m)
    else:
        sc = [int(x) for x in counts]
        if len(sc) != world:
            raise ValueError("counts must have one entry per rank")
        cnt = torch.tensor(sc, dtype=torch.int64, device=torch.device("cpu") if _via_host(group) else dev)
        rcnt = torch.empty_like(cnt)
        dist.all_to_all_single(rcnt, cnt, group=group)
        rc = [int(x) for x in rcnt.tolist()]
    n_send, n_recv = sum(sc), sum(rc)
    recv_pk, recv_ln = _recv_buffers(out, n_recv, stride, dev)
    if not anything:
        return recv_pk, recv_ln, 0
    _a2a_spans(recv_pk[: n_recv * stride], recv_ln[:n_recv], send_pk[: n_send * stride], send_ln[:n_send], sc, rc,
               stride, group)
    return recv_pk, recv_ln, n_recv


def exchange_regions(send_pk: torch.Tensor, send_ln: torch.Tensor, running: torch.Tensor, cap: int, stride: int,
                     group: Optional[dist.ProcessGroup] = None,
                     out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                     m: Optional[List[List[int]]] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """All-to-all-v of per-rank regions filled by ``RegionRouter``: rank d's datagrams are
    the first running[d] slots of region d (slots [d*cap, d*cap + running[d]) of send_pk /
    send_ln).  Split sizes from one all-gather of the running counters (one host read).
    nccl: one all_to_all over the region views (RCCL send/recv per peer, no packing copy);
    gloo: the regions are gathered on the host and sent with all_to_all_single.  Returns
    (recv_pk, recv_ln, n_recv), received spans contiguous in source-rank order.  m: the
    count matrix when the caller already gathered it."""
    if m is None:
        m = count_matrix(running, group)
    _check_cap(m, cap)
    sc, rc = _splits(m, dist.get_rank(group))
    n_recv = sum(rc)
    recv_pk, recv_ln = _recv_buffers(out, n_recv, stride, send_pk.device)
    if not _any_sent(m):
        return recv_pk, recv_ln, 0
    _a2a_regions(send_pk, send_ln, recv_pk, recv_ln, sc, rc, cap, stride, group)
    return recv_pk, recv_ln, n_recv


class _Router:
    """What both routers share: the send buffers of `slots` datagram slots, the per-rank
    count vector, and the leading arguments of every e2sar_hip_route_* call."""

    def __init__(self, ctx, stride: int, slots: int, max_batch: int, world: int, rank: int, with_lb_header: bool):
        self.ctx, self.stride, self.world, self.rank = ctx, stride, world, rank
        self.with_lb, self.max_batch = with_lb_header, max_batch
        self.send_pk = torch.empty(slots * stride, dtype=torch.uint8, device=ctx.torch_device)
        self.send_ln = torch.empty(slots, dtype=torch.int32, device=ctx.torch_device)

    def _rank_counts(self) -> torch.Tensor:
        return torch.zeros(self.world, dtype=torch.int32, device=self.ctx.torch_device)

    def _checked_args(self, pk: torch.Tensor, ln: torch.Tensor, n: int) -> tuple:
        """The arguments every e2sar_hip_route_* call begins with, for a batch the router was sized for."""
        if n > self.max_batch:
            raise ValueError("batch larger than the router was sized for")
        return (self.ctx.handle, pk.data_ptr(), self.stride, ln.data_ptr(), n, 1 if self.with_lb else 0,
                self.world, self.rank)


class RegionRouter(_Router):
    """Routes a stream of landed batches, one launch per batch, into per-rank regions of
    cap datagram slots (e2sar_hip_route_append); ``exchange_regions`` sends them once per
    step.  Routing a batch right after it landed reads it from the Infinity Cache."""

    def __init__(self, ctx, stride: int, cap: int, max_batch: int, world: int, rank: int,
                 with_lb_header: bool = True, foreign_only: bool = True):
        super().__init__(ctx, stride, world * cap, max_batch, world, rank, with_lb_header)
        self.cap, self.foreign_only = cap, foreign_only
        self.running = self._rank_counts()    # datagrams appended to each region since reset()

    def reset(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Empty the regions (a fill kernel on the stream, default the current one: capture-safe)."""
        _call("e2sar_hip_memset_async", self.ctx.handle, self.running.data_ptr(), 0, self.running.numel() * 4,
              _s(stream))

    def route(self, pk: torch.Tensor, ln: torch.Tensor, n: int, stream: Optional[torch.cuda.Stream] = None):
        # the workspace pair is unused by e2sar_hip_route_append (e2sar_hip.h): NULL / 0
        _call("e2sar_hip_route_append", *self._checked_args(pk, ln, n), 1 if self.foreign_only else 0,
              self.send_pk.data_ptr(), self.send_ln.data_ptr(), self.cap, self.running.data_ptr(), None, 0,
              _s(stream))

    def exchange(self, group: Optional[dist.ProcessGroup] = None,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        return exchange_regions(self.send_pk, self.send_ln, self.running, self.cap, self.stride, group, out)


class PacketRouter(_Router):
    """Packs a landed datagram batch into per-owner spans on the GPU."""

    def __init__(self, ctx, stride: int, max_packets: int, world: int, rank: int, with_lb_header: bool = True):
        super().__init__(ctx, stride, max(max_packets, 1), max_packets, world, rank, with_lb_header)
        self.max_packets = max_packets        # the name this router's size has always had: max_batch
        self.counts = self._rank_counts()
        ws = int(lib().e2sar_hip_route_workspace_bytes(max_packets, world))
        self.workspace = torch.empty(max(ws, 16), dtype=torch.uint8, device=ctx.torch_device)

    def route(self, pk: torch.Tensor, ln: torch.Tensor, n: int, stream: Optional[torch.cuda.Stream] = None,
              foreign_only: bool = False):
        """Returns (send_pk, send_ln, counts) with counts still on the device.  foreign_only:
        pack only datagrams other ranks own (e2sar_hip_route_foreign); the rest stay for a
        reassembler set to this rank's ownership."""
        _call("e2sar_hip_route_foreign" if foreign_only else "e2sar_hip_route_batch", *self._checked_args(pk, ln, n),
              self.send_pk.data_ptr(), self.send_ln.data_ptr(), self.counts.data_ptr(), self.workspace.data_ptr(),
              self.workspace.numel(), _s(stream))
        return self.send_pk, self.send_ln, self.counts


class SpreadPipeline:
    """BASELINE config 4 per landed batch, with the exchange overlapped.

    For each batch that lands on this rank (``land``), on the caller's stream:

    1. the datagrams this rank owns are reassembled where they landed (``R`` must be set to
       this rank's ownership, ``DeviceReassembler.set_owner``), while the batch is still in
       the Infinity Cache;
    2. the foreign ones are appended to per-owner regions (``RegionRouter``, one launch);

    then, on the communication stream, the per-owner counts are all-gathered (RCCL) and
    copied to pinned host memory.  The host reads batch b's counts only after it has queued
    batch b + depth - 1's landing work, then issues batch b's ``all_to_all`` of the regions
    (RCCL, peer to peer over xGMI) on the same stream and the reassembly of what arrived
    (classify + scatter with streaming loads) on a second stream.  So batch b's exchange and
    the reassembly of what it brought run while later batches land and are reassembled in
    place, and the step costs max(landing, exchange) instead of their sum.  ``depth``
    region / receive buffer sets rotate; a set is reused only after the exchange and
    reassembly that read it have finished (stream events, no host wait).

    Every collective -- count all-gathers and exchanges alike -- goes through ONE
    communicator on ONE stream, in one order that every rank issues identically (each
    land(): the exchange of batch b - depth + 1, then the count gather of batch b).  RCCL,
    like NCCL, does not promise progress for collectives of two communicators in flight at
    once, so nothing here depends on it: the stream serialises the collectives in the order
    every rank enqueued them.  The cost is that batch b's count gather queues behind batch
    b - depth + 1's exchange, so the host, reading b's counts depth - 1 landings later,
    waits only when the exchange has fallen depth - 1 batches behind the landing.

    With gloo (the CPU / one-GPU rehearsal) every exchange is synchronous through host
    memory and the received datagrams are reassembled on the caller's stream.

    The reference needs no exchange: its load balancer steers every fragment of an event to
    one receiver (e2sarDPSegmenter.hpp:231-233, e2sarDPReassembler.hpp:223-229).
    """

    def __init__(self, ctx, R, stride: int, max_batch: int, world: int, rank: int,
                 group: Optional[dist.ProcessGroup] = None, depth: int = 3, with_lb_header: bool = True,
                 in_place: bool = True):
        """in_place=False routes every landed datagram, this rank's own included, through the
        exchange (no in-place reassembly): the route-all form, which also drives the whole
        RCCL data path at world 1."""
        if depth < 2:
            # a region set is reused only after the exchange that reads it was issued, which
            # happens one land() later: with one set, land() would reset and refill it under
            # the previous batch's pending all_to_all
            raise ValueError("SpreadPipeline needs depth >= 2 (region / receive sets in rotation)")
        self.ctx, self.R, self.stride, self.max_batch = ctx, R, stride, max_batch
        self.world, self.rank, self.group, self.depth = world, rank, group, depth
        self.in_place = in_place
        dev = ctx.torch_device
        self.active = world > 1 or not in_place
        self.nccl = self.active and dist.get_backend(group) == "nccl"
        self.routers = [RegionRouter(ctx, stride, max_batch, max_batch, world, rank, with_lb_header,
                                     foreign_only=in_place) for _ in range(depth)] if self.active else []
        # a batch can bring at most every peer's whole batch (and its own, routing all)
        rcap = max(1, (world - (1 if in_place else 0)) * max_batch)
        self.recv = [(torch.empty(rcap * stride, dtype=torch.uint8, device=dev),
                      torch.empty(rcap, dtype=torch.int32, device=dev)) for _ in range(depth)] if self.active else []
        self.work = [R.alloc_work(rcap) for _ in range(depth)] if self.active else []
        self.comm = torch.cuda.Stream(dev) if self.nccl else None
        self.rx = torch.cuda.Stream(dev) if self.nccl else None
        self.lag = depth - 1                  # batches whose exchange is still to be issued
        self.mat_dev = [torch.zeros(world * world, dtype=torch.int32, device=dev) for _ in range(depth)]
        self.mat_host = [torch.zeros(world * world, dtype=torch.int32).pin_memory() for _ in range(depth)] \
            if self.nccl else []
        mk = (lambda: torch.cuda.Event()) if self.nccl else (lambda: None)
        self.ev_routed = [mk() for _ in range(depth)]
        self.ev_cnt = [mk() for _ in range(depth)]
        self.ev_a2a = [mk() for _ in range(depth)]       # region set free again
        self.ev_rx = [mk() for _ in range(depth)]        # receive set free again
        self.used = [False] * depth
        self.now_ms = 0
        self.pending: List[int] = []
        self.nb = 0
        self.sent = 0            # foreign datagrams sent / received since begin_step
        self.received = 0
        self.matrices: List[List[List[int]]] = []
        self.recv_log: List[Tuple[int, int]] = []        # (receive set, datagrams) per batch
        # timing hook: timed(name, stream, fn, *a, **kw) -> fn(*a, stream=stream, **kw)
        self.timed = lambda name, stream, fn, *a, **kw: fn(*a, stream=stream, **kw)

    def begin_step(self) -> None:
        self.sent = self.received = 0
        self.matrices = []
        self.recv_log = []

    def land(self, pk: torch.Tensor, ln: torch.Tensor, n: int, now_ms: int = 0) -> None:
        """One landed batch (on the current stream): in-place reassembly of the owned
        datagrams, routing of the foreign ones, and the exchange pipeline's next stage."""
        main = torch.cuda.current_stream() if torch.cuda.is_available() else None
        self.now_ms = now_ms
        if self.in_place:
            self.timed("reas_kernel", main, self.R.reassemble, pk, self.stride, ln, n, now_ms=now_ms)
        if not self.active:
            return
        slot = self.nb % self.depth
        self.nb += 1
        router = self.routers[slot]
        if self.nccl and self.used[slot]:
            main.wait_event(self.ev_a2a[slot])          # the region set's last exchange has read it
        router.reset(stream=main)
        self.timed("route_kernels", main, router.route, pk, ln, n)
        self.used[slot] = True
        if not self.nccl:
            self._exchange_sync(slot, main)
            return
        self.ev_routed[slot].record(main)
        # exchange the batch landed depth - 1 batches ago, then gather this batch's counts:
        # both on the one communication stream and communicator, in this order on every rank
        while len(self.pending) >= self.lag:
            self._finish(self.pending.pop(0))
        with torch.cuda.stream(self.comm):
            self.comm.wait_event(self.ev_routed[slot])
            dist.all_gather_into_tensor(self.mat_dev[slot], router.running, group=self.group)
            self.mat_host[slot].copy_(self.mat_dev[slot], non_blocking=True)
            self.ev_cnt[slot].record(self.comm)
        self.pending.append(slot)

    def _counts(self, m: List[List[int]]):
        _check_cap(m, self.max_batch)
        sc, rc = _splits(m, self.rank)
        self.sent += sum(c for d, c in enumerate(sc) if d != self.rank)
        self.received += sum(c for s, c in enumerate(rc) if s != self.rank)
        self.matrices.append(m)
        return sc, rc

    def _finish(self, slot: int) -> None:
        """Batch of region set `slot`: read its counts (host), exchange, reassemble arrivals.
        Called depth - 1 batches after the batch landed; its count gather was queued behind
        the exchange issued depth - 1 batches before it, so the wait below blocks only while
        the exchanges run more than depth - 1 batches behind the landing."""
        self.ev_cnt[slot].synchronize()
        flat = self.mat_host[slot].tolist()
        W = self.world
        m = [flat[s * W:(s + 1) * W] for s in range(W)]
        sc, rc = self._counts(m)
        router = self.routers[slot]
        rpk, rln = self.recv[slot]
        n_recv = sum(rc)
        with torch.cuda.stream(self.comm):
            self.comm.wait_event(self.ev_rx[slot])       # the receive set's last reassembly has read it
            if _any_sent(m):
                self.timed("exchange", self.comm, lambda stream=None: _a2a_regions(
                    router.send_pk, router.send_ln, rpk, rln, sc, rc, self.max_batch, self.stride, self.group))
            self.ev_a2a[slot].record(self.comm)
        self.recv_log.append((slot, n_recv))
        if n_recv:
            self.rx.wait_event(self.ev_a2a[slot])
            self._reassemble_received(rpk, rln, n_recv, self.work[slot], self.rx)
        self.ev_rx[slot].record(self.rx)

    def _reassemble_received(self, rpk, rln, n, work, stream) -> None:
        self.timed("reas_classify_kernel", stream, self.R.classify, rpk, self.stride, rln, n, work,
                   now_ms=self.now_ms)
        self.timed("reas_scatter_kernel", stream, self.R.scatter, rpk, self.stride, n, work)

    def _exchange_sync(self, slot: int, main) -> None:
        router = self.routers[slot]
        m = count_matrix(router.running, self.group)
        self._counts(m)
        res = []                # collected here: the timed hook need not return what fn returns
        self.timed("exchange", main, lambda stream=None: res.append(exchange_regions(
            router.send_pk, router.send_ln, router.running, self.max_batch, self.stride, self.group,
            out=self.recv[slot], m=m)))
        rpk, rln, n = res[0]
        self.recv_log.append((slot, n))
        if n:
            self._reassemble_received(rpk, rln, n, self.work[slot], main)

    def flush(self) -> None:
        """Finish every batch's exchange and reassembly; the current stream waits for them."""
        while self.pending:
            self._finish(self.pending.pop(0))
        if self.nccl:
            main = torch.cuda.current_stream()
            main.wait_stream(self.comm)
            main.wait_stream(self.rx)
