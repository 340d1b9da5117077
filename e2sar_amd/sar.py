"""Device-level SAR API over the C ABI (``include/e2sar_hip.h``).

``DeviceSegmenter`` and ``DeviceReassembler`` are thin, allocation-aware wrappers: event
bytes, datagrams and reassembled events stay in HBM; torch is used only as the device
memory / stream plumbing.  The reference-shaped ``Segmenter``/``Reassembler`` classes live in
the pybind module ``e2sar_amd.e2sar_py``, over the C++ facade on the same C ABI.

Every status-returning C-ABI call goes through ``_call``; its arguments are plain values
(``_capi.SIGNATURES`` declares the argtypes): ``t.data_ptr()``, ``_p(t)`` where a tensor may
be omitted, ``_s(stream)`` for the stream.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _capi
from ._capi import check, lib


def _stream_handle(stream: Optional[torch.cuda.Stream]) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream)


_s = _stream_handle        # the short form the call sites use


def _p(t: Optional[torch.Tensor]) -> int:
    """Device address of an optional tensor: NULL when it is omitted."""
    return t.data_ptr() if t is not None else 0


def _call(name: str, *args) -> int:
    """One C-ABI call by name; a negative status raises E2SARHipError."""
    return check(getattr(lib(), name)(*args))


class _Handle:
    """Owner of one C-ABI object: ``_h`` (a c_void_p) is destroyed once, by close() or
    when the owner is collected."""
    _destroy: str

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# e2sar_hip_seg_event, as DeviceSegmenter.emit and DeviceReassembler.relay_plan write it
SEG_EVENT = np.dtype(_capi.SegEvent)
SEG_EVENT_BYTES = SEG_EVENT.itemsize
# e2sar_hip_collect_rec: one event DeviceReassembler.collect delivered, and where in `out`
COLLECT_REC = np.dtype(_capi.CollectRec)
COLLECT_REC_BYTES = COLLECT_REC.itemsize
# e2sar_hip_built_rec: one built event of DeviceReassembler.build, and which members it has
BUILT_REC = np.dtype(_capi.BuiltRec)
BUILT_REC_BYTES = BUILT_REC.itemsize


def _parse(table: torch.Tensor, counts: torch.Tensor, rec: np.dtype) -> np.ndarray:
    torch.cuda.synchronize(table.device)
    n = int(counts[0].item())
    raw = table[: n * rec.itemsize].cpu().numpy().tobytes()
    return np.frombuffer(raw, rec).copy()


def parse_emit(events: torch.Tensor, counts: torch.Tensor) -> np.ndarray:
    """The descriptors DeviceSegmenter.emit wrote, on the host: waits for the device, copies
    the table and the counts, and returns a SEG_EVENT array of the n taken events."""
    return _parse(events, counts, SEG_EVENT)


def parse_collect(index: torch.Tensor, counts: torch.Tensor) -> np.ndarray:
    """The rows DeviceReassembler.collect wrote, on the host: waits for the device, copies
    the index and the counts, and returns a COLLECT_REC array of the n taken events."""
    return _parse(index, counts, COLLECT_REC)


def parse_build(members: torch.Tensor, groups: torch.Tensor, counts: torch.Tensor):
    """What DeviceReassembler.build wrote, on the host: waits for the device, copies the two
    tables and the counts, and returns (a COLLECT_REC array of the counts[1] members taken, a
    BUILT_REC array of the counts[0] groups taken)."""
    return _parse(members, counts[1:], COLLECT_REC), _parse(groups, counts, BUILT_REC)


def total_hdr_len(use_ipv6: bool = False) -> int:
    """IP + UDP + LB + RE header bytes (e2sarHeaders.hpp:419-421): 64 / 84."""
    return int(lib().e2sar_hip_total_hdr_len(1 if use_ipv6 else 0))


def max_pld_len(mtu: int, use_ipv6: bool = False) -> int:
    """Segmenter maxPldLen = mtu - total header (e2sarDPSegmenter.hpp:241)."""
    return int(lib().e2sar_hip_max_pld_len(mtu, 1 if use_ipv6 else 0))


def num_packets(nbytes: int, max_pld: int) -> int:
    """ceil(bytes / maxPldLen) (e2sarDPSegmenter.cpp:670)."""
    return int(lib().e2sar_hip_num_packets(nbytes, max_pld))


def packet_stride(max_pld: int) -> int:
    return int(lib().e2sar_hip_packet_stride(max_pld))


class Context(_Handle):
    """A device + stream binding (e2sar_hip_ctx)."""
    _destroy = "e2sar_hip_ctx_destroy"

    def __init__(self, device: int = 0, stream: Optional[torch.cuda.Stream] = None):
        torch.cuda.set_device(device)
        self.device = device
        self.torch_device = torch.device("cuda", device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(device)
        h = C.c_void_p()
        _call("e2sar_hip_ctx_create", device, _s(self.stream), C.byref(h))
        self._h = h

    def sync(self) -> None:
        _call("e2sar_hip_ctx_sync", self._h)

    def copy_spans(self, spans: Sequence[tuple], stream: Optional[torch.cuda.Stream] = None) -> None:
        """(src_ptr, dst_ptr, nbytes) spans, device or pinned host memory, copied by
        e2sar_hip_copy_spans (one launch per 64 spans)."""
        arr = (_capi.CopySpan * max(1, len(spans)))()
        for k, (a, b, n) in enumerate(spans):
            arr[k] = _capi.CopySpan(int(a), int(b), int(n))
        _call("e2sar_hip_copy_spans", self._h, arr, len(spans), _s(stream))


@dataclass
class SegPlan:
    """Host event table + its device copy for one segment batch."""
    host: "C.Array"
    device: torch.Tensor          # uint8 tensor holding the e2sar_hip_seg_event table
    n_events: int
    total_packets: int
    max_packets_per_event: int
    aligned4: bool


class DeviceSegmenter:
    """Segments batches of device-resident events into device-resident datagrams.

    Replaces SendThreadState::_send's fragment loop (e2sarDPSegmenter.cpp:660-871):
    every datagram is [LB header][RE header][payload slice] exactly as the reference
    emits it; the socket send is the caller's business (or the datagrams stay in HBM).
    """

    def __init__(self, ctx: Context, mtu: int = 1500, use_ipv6: bool = False, lb_hdr_version: int = 2):
        self.ctx = ctx
        self.mtu = mtu
        self.max_pld = max_pld_len(mtu, use_ipv6)
        if mtu > 9000:
            raise ValueError("MTU set too long, limit 9000")       # hpp:310-311
        if self.max_pld == 0:
            raise ValueError("Insufficient MTU length to accommodate headers")  # hpp:315-316
        self.stride = packet_stride(self.max_pld)
        self.lb_hdr_version = lb_hdr_version

    def _need_slots(self, n: int, packets: torch.Tensor, *lens: torch.Tensor) -> None:
        if packets.numel() < n * self.stride or any(ln.numel() < n for ln in lens):
            raise ValueError("packet buffer too small")

    def plan(self, events: Sequence[tuple]) -> SegPlan:
        """events: (data_ptr, nbytes, eventNum, dataId, entropy, lbTick) tuples, data on device."""
        n = len(events)
        arr = (_capi.SegEvent * max(n, 1))()
        aligned4 = True
        for k, (ptr, nbytes, evn, did, ent, tick) in enumerate(events):
            if nbytes >= 1 << 32:
                raise ValueError("event larger than 4 GiB (REHdr bufferLength is u32)")
            e = arr[k]
            e.data = int(ptr)
            e.bytes = int(nbytes)
            e.eventNum = int(evn) & (2**64 - 1)
            e.dataId = int(did) & 0xFFFF
            e.entropy = int(ent) & 0xFFFF
            e.lbTick = int(tick) & (2**64 - 1)
            aligned4 = aligned4 and (int(ptr) % 4 == 0)
        tot = C.c_uint32()
        mx = C.c_uint32()
        _call("e2sar_hip_seg_plan", arr, n, self.max_pld, C.byref(tot), C.byref(mx))
        raw = np.frombuffer(bytes(arr)[: n * C.sizeof(_capi.SegEvent)], dtype=np.uint8).copy()
        dev = torch.from_numpy(raw).to(self.ctx.torch_device, non_blocking=False)
        return SegPlan(arr, dev, n, int(tot.value), int(mx.value), aligned4)

    def groups(self, plan: SegPlan):
        """The reassembly groups that match this segmenter's XCD stripes for `plan`
        (e2sar_hip_seg_groups): (device uint32 tensor of starts, nGroups), or (None, 0)
        when the batch has no stripes.  For DeviceReassembler.reassemble_groups."""
        spc = self.stride // 16
        units = plan.n_events * max(1, (plan.max_packets_per_event * spc + 511) // 512)
        cap = units + 2
        starts = (C.c_uint32 * cap)()
        ng = C.c_uint32()
        _capi.need_experimental("DeviceSegmenter.groups")
        _call("e2sar_hip_seg_groups", plan.host, plan.n_events, plan.max_packets_per_event, self.max_pld,
              self.stride, starts, cap, C.byref(ng))
        if ng.value == 0:
            return None, 0
        host = np.frombuffer(bytes(starts), dtype=np.uint32)[: ng.value + 1].copy()
        return torch.from_numpy(host.view(np.int32)).to(self.ctx.torch_device), int(ng.value)

    def alloc_packets(self, n_packets: int):
        pk = torch.empty(max(n_packets, 1) * self.stride, dtype=torch.uint8, device=self.ctx.torch_device)
        ln = torch.empty(max(n_packets, 1), dtype=torch.int32, device=self.ctx.torch_device)
        return pk, ln

    def segment(self, plan: SegPlan, packets: torch.Tensor, lens: Optional[torch.Tensor],
                stream: Optional[torch.cuda.Stream] = None, recycle: Optional["DeviceReassembler"] = None,
                force: bool = False) -> int:
        """recycle: also recycle that reassembler (as DeviceReassembler.recycle(force)) in the
        same launch (e2sar_hip_segment_batch_recycle)."""
        self._need_slots(plan.total_packets, packets)
        batch = (self.ctx.handle, plan.device.data_ptr(), plan.n_events, plan.max_packets_per_event,
                 self.lb_hdr_version, self.max_pld, 1 if plan.aligned4 else 0, packets.data_ptr(), self.stride,
                 _p(lens))
        if recycle is not None:
            _call("e2sar_hip_segment_batch_recycle", *batch, recycle.handle, 1 if force else 0, _s(stream))
        else:
            _call("e2sar_hip_segment_batch", *batch, _s(stream))
        return plan.total_packets

    def segment_reassemble(self, plan: SegPlan, packets: torch.Tensor, lens: torch.Tensor,
                           reas: "DeviceReassembler", now_ms: int = 0,
                           stream: Optional[torch.cuda.Stream] = None) -> int:
        """Chained form: segment the batch and reassemble the same datagrams into `reas`
        in one launch (e2sar_hip_segment_reassemble_batch)."""
        self._need_slots(plan.total_packets, packets, lens)
        _capi.need_experimental("DeviceSegmenter.segment_reassemble")
        _call("e2sar_hip_segment_reassemble_batch", self.ctx.handle, plan.device.data_ptr(), plan.n_events,
              plan.max_packets_per_event, plan.total_packets, self.lb_hdr_version, self.max_pld, packets.data_ptr(),
              self.stride, lens.data_ptr(), reas._h, int(now_ms), _s(stream))
        return plan.total_packets

    def segment_reassemble_batches(self, plans: Sequence[SegPlan], bufs: Sequence[tuple],
                                   reas: "DeviceReassembler", now_ms: int = 0,
                                   stream: Optional[torch.cuda.Stream] = None) -> int:
        """Chained form over several batches in one launch (at most 8;
        e2sar_hip_segment_reassemble_batches); bufs[k] = (packets, lens) of plans[k], all distinct."""
        arr = (_capi.SegReasBatch * max(1, len(plans)))()
        for k, (p, (pk, ln)) in enumerate(zip(plans, bufs)):
            self._need_slots(p.total_packets, pk, ln)
            arr[k] = _capi.SegReasBatch(p.device.data_ptr(), pk.data_ptr(), ln.data_ptr(), p.n_events,
                                        p.max_packets_per_event, p.total_packets, 0)
        _capi.need_experimental("DeviceSegmenter.segment_reassemble_batches")
        _call("e2sar_hip_segment_reassemble_batches", self.ctx.handle, arr, len(plans), self.lb_hdr_version,
              self.max_pld, self.stride, reas._h, int(now_ms), _s(stream))
        return sum(p.total_packets for p in plans)

    def segment_device(self, events: torch.Tensor, counts: torch.Tensor, max_events: int,
                       max_packets_per_event: int, packets: torch.Tensor, lens: Optional[torch.Tensor],
                       stream: Optional[torch.cuda.Stream] = None) -> None:
        """Segment a descriptor table built on the device (DeviceReassembler.relay_plan):
        the event count is counts[0], read by the kernel; max_events bounds it."""
        if packets.numel() < max_events * max_packets_per_event * self.stride:
            raise ValueError("packet buffer too small for the bound")
        _call("e2sar_hip_segment_batch_dev", self.ctx.handle, events.data_ptr(), counts.data_ptr(), max_events,
              max_packets_per_event, self.lb_hdr_version, self.max_pld, packets.data_ptr(), self.stride, _p(lens),
              _s(stream))

    def emit(self, data: torch.Tensor, lengths: torch.Tensor, packets: torch.Tensor, lens: Optional[torch.Tensor],
             events: torch.Tensor, counts: torch.Tensor, *, offsets: Optional[torch.Tensor] = None, pitch: int = 0,
             count: Optional[torch.Tensor] = None, event_nums: Optional[torch.Tensor] = None,
             event_num_base: int = 0, lb_tick_base: int = 0, lb_tick_step: int = 0, data_id: int = 0,
             entropy_base: int = 0, ticks_as_event_num: bool = False, max_events: Optional[int] = None,
             max_event_bytes: int = 0, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Plan and segment events whose count, lengths and offsets live on the device
        (e2sar_hip_seg_emit): two launches, no allocation, no wait, capturable.

        `data`: uint8 device tensor the events lie in; event i has lengths[i] bytes (int32
        device tensor, read as uint32) at i * pitch (rows) or at offsets[i] (int64 device
        tensor, ragged) -- give one of the two.  `count`: a one-element int32 device tensor
        (None: every entry of `lengths`).  Numbering of event i: RE eventNum event_nums[i]
        (int64 device tensor) or event_num_base + i, lbTick lb_tick_base + i * lb_tick_step,
        entropy entropy_base + i; ticks_as_event_num puts the lbTick into the RE eventNum.
        `packets` / `lens` bound the datagrams (packets.numel() // stride slots); `events`:
        uint8 device tensor of max_events * SEG_EVENT_BYTES; `counts`: int32 device tensor of
        at least 8 entries: taken, datagrams, events left, why the prefix ended (0 all taken,
        1 packet capacity, 2 event outside `data`).  parse_emit reads the result back."""
        if data.dtype != torch.uint8 or packets.dtype != torch.uint8 or events.dtype != torch.uint8:
            raise ValueError("data, packets and events are uint8 tensors")
        if lengths.dtype != torch.int32 or counts.dtype != torch.int32 or (count is not None and count.dtype != torch.int32):
            raise ValueError("lengths, counts and count are int32 tensors")
        if (offsets is not None and offsets.dtype != torch.int64) or (event_nums is not None and event_nums.dtype != torch.int64):
            raise ValueError("offsets and event_nums are int64 tensors")
        if max_events is None:
            max_events = lengths.numel()
        max_packets = packets.numel() // self.stride
        if lens is not None:
            max_packets = min(max_packets, lens.numel())
        if (lengths.numel() < max_events or events.numel() < max_events * SEG_EVENT_BYTES or counts.numel() < 8
                or (offsets is not None and offsets.numel() < max_events)
                or (event_nums is not None and event_nums.numel() < max_events)):
            raise ValueError("emit buffers too small for max_events")
        src = _capi.SegSource(_p(data), data.numel(), _p(lengths), _p(count), _p(offsets), int(pitch),
                              min(int(max_event_bytes), 0xFFFFFFFF))
        num = _capi.SegNumbering(_p(event_nums), int(event_num_base) & (2**64 - 1), int(lb_tick_base) & (2**64 - 1),
                                 int(lb_tick_step) & (2**64 - 1), int(data_id) & 0xFFFF, int(entropy_base) & 0xFFFF,
                                 _capi.SEG_TICKS_AS_EVENTNUM if ticks_as_event_num else 0)
        _call("e2sar_hip_seg_emit", self.ctx.handle, C.byref(src), C.byref(num), max_events, self.lb_hdr_version,
              self.max_pld, packets.data_ptr(), self.stride, max_packets, _p(lens), events.data_ptr(),
              counts.data_ptr(), _s(stream))

    def emit_rows(self, rows: torch.Tensor, lengths: torch.Tensor, count: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None, **numbering):
        """emit() of the rows of a contiguous [n, pitch] uint8 tensor into new tensors sized
        for the bound (every row full): -> (packets, lens, events, counts).  Row i < counts[0]
        is event i with lengths[i] bytes; no host synchronisation happens here."""
        if rows.dim() != 2 or rows.dtype != torch.uint8 or not rows.is_contiguous():
            raise ValueError("emit_rows needs a contiguous [n, pitch] uint8 tensor")
        n, pitch = rows.shape
        if n == 0 or pitch == 0:
            raise ValueError("emit_rows needs at least one row of at least one byte")
        dev = self.ctx.torch_device
        packets, lens = self.alloc_packets(n * num_packets(pitch, self.max_pld))
        events = torch.empty(n * SEG_EVENT_BYTES, dtype=torch.uint8, device=dev)
        counts = torch.empty(8, dtype=torch.int32, device=dev)
        self.emit(rows.view(-1), lengths, packets, lens, events, counts, pitch=pitch, count=count, max_events=n,
                  stream=stream, **numbering)
        return packets, lens, events, counts


def _need_batch(what: str, n: int, stride: int, packets: torch.Tensor, *lens: torch.Tensor) -> None:
    if any(ln.numel() < n for ln in lens) or packets.numel() < n * stride:
        raise ValueError(what)


class DeviceReassembler(_Handle):
    """Reassembles device-resident datagram batches into a device event arena.

    Replaces the per-packet body of RecvThreadState::_threadBody
    (e2sarDPReassembler.cpp:310-428), the eventsInProgress map and the event queue.
    """
    _destroy = "e2sar_hip_reas_destroy"

    def __init__(self, ctx: Context, with_lb_header: bool = False, table_slots: int = 4096,
                 queue_capacity: int = 4096, lost_capacity: int = 4096, arena_bytes: int = 1 << 30,
                 compactable: bool = False, flags: int = 0, group_size: int = 0):
        """group_size: datagrams per fused-kernel workgroup (1..64), 0 = automatic."""
        self.ctx = ctx
        flags |= _capi.REAS_COMPACTABLE if compactable else 0
        cfg = _capi.ReasConfig(1 if with_lb_header else 0, table_slots, queue_capacity,
                               lost_capacity, arena_bytes, flags, group_size)
        h = C.c_void_p()
        _call("e2sar_hip_reas_create", ctx.handle, C.byref(cfg), C.byref(h))
        self._h = h
        self.with_lb_header = with_lb_header
        self.arena_bytes = arena_bytes
        self.arena_ptr = int(lib().e2sar_hip_reas_arena(h) or 0)
        self._evbuf = (_capi.EventRec * queue_capacity)()
        self._lostbuf = (_capi.LostRec * lost_capacity)()

    def set_owner(self, world: int, rank: int) -> None:
        """Take only events with eventNum % world == rank (e2sar_hip_reas_set_owner)."""
        _call("e2sar_hip_reas_set_owner", self._h, int(world), int(rank))

    def set_cold(self, cold: bool) -> None:
        """Streaming datagram loads for the following launches (e2sar_hip_reas_set_cold)."""
        _call("e2sar_hip_reas_set_cold", self._h, 1 if cold else 0)

    def reassemble(self, packets: torch.Tensor, stride: int, lens: torch.Tensor, n: int,
                   now_ms: int = 0, stream: Optional[torch.cuda.Stream] = None) -> None:
        if n == 0:
            return
        _need_batch("packet batch buffers too small", n, stride, packets, lens)
        _call("e2sar_hip_reassemble_batch", self._h, packets.data_ptr(), stride, lens.data_ptr(), n, int(now_ms),
              _s(stream))

    def reassemble_dev(self, packets: torch.Tensor, stride: int, lens: torch.Tensor, count: torch.Tensor,
                       max_packets: Optional[int] = None, now_ms: int = 0,
                       stream: Optional[torch.cuda.Stream] = None) -> None:
        """reassemble() of the first min(count[0], max_packets) datagrams, the count read by
        the kernels (e2sar_hip_reassemble_batch_dev): no host read, capturable.  `count`: an
        int32 device tensor (read as uint32) whose first element is the count -- a view such
        as counts[1:2] of DeviceSegmenter.emit or of relay_plan.  max_packets bounds it and
        sizes the launch; it defaults to what `packets` and `lens` hold."""
        if count.dtype != torch.int32 or lens.dtype != torch.int32 or packets.dtype != torch.uint8:
            raise ValueError("packets is a uint8 tensor, lens and count are int32 tensors")
        if count.device != packets.device or lens.device != packets.device:
            raise ValueError("packets, lens and count lie on one device")
        if count.numel() < 1:
            raise ValueError("count is empty")
        if max_packets is None:
            max_packets = min(lens.numel(), packets.numel() // stride)
        _need_batch("packet batch buffers too small for max_packets", max_packets, stride, packets, lens)
        _call("e2sar_hip_reassemble_batch_dev", self._h, packets.data_ptr(), stride, lens.data_ptr(), count.data_ptr(),
              max_packets, int(now_ms), _s(stream))

    def reassemble_groups(self, packets: torch.Tensor, stride: int, lens: torch.Tensor, n: int,
                          starts: Optional[torch.Tensor], n_groups: int, now_ms: int = 0,
                          stream: Optional[torch.cuda.Stream] = None) -> None:
        """reassemble() over a group table (DeviceSegmenter.groups: the XCD stripes the batch
        was segmented in), e2sar_hip_reassemble_groups."""
        if n == 0:
            return
        _need_batch("packet batch buffers too small", n, stride, packets, lens)
        if starts is not None and starts.numel() < n_groups + 1:
            raise ValueError("group table too small")
        _capi.need_experimental("DeviceReassembler.reassemble_groups")
        _call("e2sar_hip_reassemble_groups", self._h, packets.data_ptr(), stride, lens.data_ptr(), n, _p(starts),
              n_groups if starts is not None else 0, int(now_ms), _s(stream))

    def relay_plan(self, events: torch.Tensor, counts: torch.Tensor, first_record: int, max_events: int,
                   max_pld: int, lb_tick: int, entropy_base: int,
                   stream: Optional[torch.cuda.Stream] = None) -> None:
        """Completed records [first_record, +n) -> seg descriptors in `events` (uint8 device
        tensor of max_events * SEG_EVENT_BYTES) and counts[0:2] = (n, datagrams) (int32/uint32
        device tensor), without a host round trip (e2sar_hip_relay_plan)."""
        if events.numel() < max_events * SEG_EVENT_BYTES or counts.numel() < 2:
            raise ValueError("relay buffers too small")
        _call("e2sar_hip_relay_plan", self._h, first_record, max_events, max_pld, int(lb_tick),
              entropy_base & 0xFFFF, events.data_ptr(), counts.data_ptr(), _s(stream))

    def collect(self, out: torch.Tensor, index: torch.Tensor, counts: torch.Tensor, first_record: int = 0,
                max_events: Optional[int] = None, pitch: int = 0, align: int = 256,
                stream: Optional[torch.cuda.Stream] = None) -> None:
        """Completed records [first_record, ...) packed into `out` (uint8 device tensor) on
        the device, no host round trip (e2sar_hip_reas_collect): ragged at `align` when pitch
        is 0, else rows of `pitch` bytes, zero-filled, so that out[: n * pitch] is an
        [n, pitch] tensor.  `index`: uint8 device tensor of max_events * COLLECT_REC_BYTES
        (max_events defaults to what it holds); `counts`: int64 device tensor, at least 4
        entries: n, bytes of `out` spanned, records left, event bytes copied.  The records
        stay queued; parse_collect reads the result back."""
        if out.dtype != torch.uint8 or index.dtype != torch.uint8 or counts.dtype != torch.int64:
            raise ValueError("out and index are uint8 tensors, counts is int64")
        if max_events is None:
            max_events = index.numel() // COLLECT_REC_BYTES
        if index.numel() < max_events * COLLECT_REC_BYTES or counts.numel() < 4:
            raise ValueError("collect buffers too small")
        _call("e2sar_hip_reas_collect", self._h, first_record, max_events, out.data_ptr(), out.numel(), pitch, align,
              index.data_ptr(), counts.data_ptr(), _s(stream))

    def collect_rows(self, max_events: int, pitch: int, first_record: int = 0,
                     stream: Optional[torch.cuda.Stream] = None):
        """collect() in row mode into new tensors: -> (rows [max_events, pitch] uint8, index,
        counts).  Row i < counts[0] is event i, cut or zero-filled to `pitch`; no host
        synchronisation happens here."""
        if pitch <= 0 or max_events <= 0:
            raise ValueError("collect_rows needs a pitch and a row count")
        dev = self.ctx.torch_device
        rows = torch.empty((max_events, pitch), dtype=torch.uint8, device=dev)
        index = torch.empty(max_events * COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        self.collect(rows.view(-1), index, counts, first_record, max_events, pitch, stream=stream)
        return rows, index, counts

    def new_cursor(self) -> torch.Tensor:
        """A zeroed int32[1] on the device: the cursor of collect_next and turn."""
        return torch.zeros(1, dtype=torch.int32, device=self.ctx.torch_device)

    def collect_next(self, out: torch.Tensor, index: torch.Tensor, counts: torch.Tensor, cursor: torch.Tensor,
                     max_events: Optional[int] = None, pitch: int = 0, align: int = 0,
                     stream: Optional[torch.cuda.Stream] = None) -> None:
        """collect() from the record `cursor[0]` names, read on the device when the launch
        runs and left grown by the events taken (e2sar_hip_reas_collect_next): no host read,
        capturable, each event delivered once.  `cursor`: new_cursor().  A reassembler
        consumed this way is not polled."""
        if out.dtype != torch.uint8 or index.dtype != torch.uint8 or counts.dtype != torch.int64:
            raise ValueError("out and index are uint8 tensors, counts is int64")
        if cursor.dtype != torch.int32 or cursor.numel() < 1 or cursor.device != out.device:
            raise ValueError("cursor is an int32[1] tensor on the device of out")
        if max_events is None:
            max_events = index.numel() // COLLECT_REC_BYTES
        if index.numel() < max_events * COLLECT_REC_BYTES or counts.numel() < 4:
            raise ValueError("collect buffers too small")
        _call("e2sar_hip_reas_collect_next", self._h, cursor.data_ptr(), max_events, out.data_ptr(), out.numel(), pitch,
              align, index.data_ptr(), counts.data_ptr(), _s(stream))

    def turn(self, cursor: torch.Tensor, status: torch.Tensor, arena_mark: int = 0, record_mark: int = 0,
             table_mark: int = 0, max_carries: int = _capi.TURN_NEVER_LOST,
             stream: Optional[torch.cuda.Stream] = None) -> None:
        """Upkeep decided on the device (e2sar_hip_reas_turn): once every record is collected
        (cursor) and a mark is reached -- arena bytes in use, completed records, table slots
        claimed; 0 is always reached -- the arena, the table and the completed list are
        emptied except for the events in progress, which stay and complete later; one carried
        max_carries times already is lost instead.  `status`: int64 device tensor, at least 4
        entries: verdict (_capi.TURN_*), survivors, aged out, arena bytes in use.  No host
        read, capturable; needs compactable=True."""
        if cursor.dtype != torch.int32 or cursor.numel() < 1 or status.dtype != torch.int64 or status.numel() < 4:
            raise ValueError("cursor is an int32[1] tensor, status an int64 tensor of at least 4")
        marks = _capi.TurnMarks(int(arena_mark), int(record_mark), int(table_mark), int(max_carries), 0)
        _call("e2sar_hip_reas_turn", self._h, cursor.data_ptr(), C.byref(marks), status.data_ptr(), _s(stream))

    @staticmethod
    def build_work_bytes(n: int) -> int:
        """Bytes of device scratch a build over a window of up to n records needs."""
        return int(lib().e2sar_hip_reas_build_work_bytes(int(n)))

    def alloc_build_work(self, n: int) -> torch.Tensor:
        return torch.empty(self.build_work_bytes(n), dtype=torch.uint8, device=self.ctx.torch_device)

    def build(self, out: torch.Tensor, members: torch.Tensor, groups: torch.Tensor, counts: torch.Tensor,
              work: torch.Tensor, *, ids: Optional[Sequence[int]] = None, first_record: int = 0,
              max_records: Optional[int] = None, max_groups: Optional[int] = None, pitch: int = 0, align: int = 256,
              stream: Optional[torch.cuda.Stream] = None) -> None:
        """The window of completed records [first_record, +max_records) sorted by (eventNum,
        dataId), grouped into built events and packed into `out` (uint8 device tensor) on the
        device, no host round trip (e2sar_hip_reas_build).  `ids`: the dataIds of the sources,
        in cell order; records of other ids are skipped, a group that lacks one is flagged
        INCOMPLETE; None takes every dataId.  Ragged at `align` when pitch is 0; else cells of
        `pitch` bytes, zero-filled, so that out[: n * len(ids) * pitch] is an
        [n, len(ids), pitch] tensor.  `members`: uint8 device tensor of max_records *
        COLLECT_REC_BYTES, `groups`: of max_groups * BUILT_REC_BYTES (both default to what the
        tensors hold, max_records to at most 4096); `counts`: int64 device tensor, at least 8
        entries (groups, members, bytes spanned, bytes copied, window, duplicates, foreign,
        groups left); `work`: alloc_build_work(max_records).  The records stay queued;
        parse_build reads the result back."""
        if any(t.dtype != torch.uint8 for t in (out, members, groups, work)) or counts.dtype != torch.int64:
            raise ValueError("out, members, groups and work are uint8 tensors, counts is int64")
        if max_records is None:
            max_records = min(members.numel() // COLLECT_REC_BYTES, _capi.BUILD_MAX_RECORDS)
        if max_groups is None:
            max_groups = groups.numel() // BUILT_REC_BYTES
        if members.numel() < max_records * COLLECT_REC_BYTES or groups.numel() < max_groups * BUILT_REC_BYTES \
                or counts.numel() < 8:
            raise ValueError("build buffers too small")
        ids = list(ids or ())
        arr = (C.c_uint16 * max(1, len(ids)))(*ids)
        _call("e2sar_hip_reas_build", self._h, first_record, max_records, arr if ids else None, len(ids),
              out.data_ptr(), out.numel(), pitch, align, members.data_ptr(), groups.data_ptr(), max_groups,
              counts.data_ptr(), work.data_ptr(), work.numel(), _s(stream))

    def build_cells(self, ids: Sequence[int], max_groups: int, pitch: int, first_record: int = 0,
                    max_records: int = 4096, stream: Optional[torch.cuda.Stream] = None):
        """build() in cell mode into new tensors: -> (cells [max_groups, len(ids), pitch] uint8,
        members, groups, counts).  cells[g, j] of group g < counts[0] is source ids[j] of that
        eventNum, cut or zero-filled to `pitch`, all zeros when groups[g].presentMask lacks bit
        j; no host synchronisation happens here."""
        if pitch <= 0 or max_groups <= 0 or not len(ids):
            raise ValueError("build_cells needs ids, a pitch and a group count")
        dev = self.ctx.torch_device
        cells = torch.empty((max_groups, len(ids), pitch), dtype=torch.uint8, device=dev)
        members = torch.empty(max_records * COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
        groups = torch.empty(max_groups * BUILT_REC_BYTES, dtype=torch.uint8, device=dev)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        work = self.alloc_build_work(max_records)
        if stream is not None:
            work.record_stream(stream)        # freed on return: not reused before the build has run
        self.build(cells.view(-1), members, groups, counts, work, ids=ids, first_record=first_record,
                   max_records=max_records, max_groups=max_groups, pitch=pitch, stream=stream)
        return cells, members, groups, counts

    # ---- split form: classify (headers, table) then scatter (bytes), for pipelining ----
    @staticmethod
    def work_bytes(n: int) -> int:
        return int(lib().e2sar_hip_reas_work_bytes(int(n)))

    def alloc_work(self, n: int) -> torch.Tensor:
        """Device work buffer for one classified batch of up to n datagrams."""
        return torch.empty(self.work_bytes(n), dtype=torch.uint8, device=self.ctx.torch_device)

    def classify(self, packets: torch.Tensor, stride: int, lens: torch.Tensor, n: int, work: torch.Tensor,
                 now_ms: int = 0, stream: Optional[torch.cuda.Stream] = None) -> None:
        if n == 0:
            return
        _need_batch("packet batch buffers too small", n, stride, packets, lens)
        _call("e2sar_hip_reas_classify", self._h, packets.data_ptr(), stride, lens.data_ptr(), n, int(now_ms),
              work.data_ptr(), work.numel(), _s(stream))

    def scatter(self, packets: torch.Tensor, stride: int, n: int, work: torch.Tensor,
                stream: Optional[torch.cuda.Stream] = None) -> None:
        if n == 0:
            return
        _need_batch("packet batch buffer too small", n, stride, packets)
        _call("e2sar_hip_reas_scatter", self._h, packets.data_ptr(), stride, n, work.data_ptr(), work.numel(),
              _s(stream))

    def scatter_classify(self, stride: int, s_packets: torch.Tensor, s_n: int, s_work: torch.Tensor,
                         c_packets: torch.Tensor, c_lens: torch.Tensor, c_n: int, c_work: torch.Tensor,
                         now_ms: int = 0, stream: Optional[torch.cuda.Stream] = None) -> None:
        """One launch: scatter classified batch b while classifying batch b+1."""
        _need_batch("scatter batch buffer too small", s_n, stride, s_packets)
        _need_batch("classify batch buffers too small", c_n, stride, c_packets, c_lens)
        _call("e2sar_hip_reas_scatter_classify", self._h, stride, s_packets.data_ptr(), s_n, s_work.data_ptr(),
              s_work.numel(), c_packets.data_ptr(), c_lens.data_ptr(), c_n, int(now_ms), c_work.data_ptr(),
              c_work.numel(), _s(stream))

    def forget_stream(self, stream: torch.cuda.Stream) -> None:
        """Before the caller destroys `stream`, on which it launched through this reassembler:
        wait for it, stop tracking it and free its internal buffers
        (e2sar_hip_reas_forget_stream).  The stream must still be alive."""
        _call("e2sar_hip_reas_forget_stream", self._h, _s(stream))

    def gc(self, now_ms: int, timeout_ms: int, stream: Optional[torch.cuda.Stream] = None) -> None:
        _call("e2sar_hip_reas_gc", self._h, int(now_ms), int(timeout_ms), _s(stream))

    def _drain(self, name: str, buf: "C.Array") -> list:
        """One poll call into `buf`; the records it returned, each copied out of the buffer."""
        n = C.c_uint32()
        _call(name, self._h, buf, len(buf), C.byref(n))
        out = []
        for k in range(n.value):
            r = buf._type_()
            C.memmove(C.byref(r), C.byref(buf[k]), C.sizeof(r))
            out.append(r)
        return out

    def poll(self) -> List[_capi.EventRec]:
        return self._drain("e2sar_hip_reas_poll", self._evbuf)

    def lost_poll(self) -> List[_capi.LostRec]:
        return self._drain("e2sar_hip_reas_lost_poll", self._lostbuf)

    def stats(self) -> _capi.ReasStats:
        s = _capi.ReasStats()
        _call("e2sar_hip_reas_get_stats", self._h, C.byref(s))
        return s

    def recycle(self, force: bool = False, stream: Optional[torch.cuda.Stream] = None) -> None:
        _call("e2sar_hip_reas_recycle", self._h, 1 if force else 0, _s(stream))

    def compact(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Move in-progress events to the alternate arena (see e2sar_hip_reas_compact)."""
        _call("e2sar_hip_reas_compact", self._h, _s(stream))
        self.arena_ptr = int(lib().e2sar_hip_reas_arena(self._h) or 0)

    def reset_stats(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        _call("e2sar_hip_reas_reset_stats", self._h, _s(stream))

    def event_bytes(self, rec: _capi.EventRec) -> bytes:
        """Copy one reassembled event to host memory."""
        buf = (C.c_uint8 * max(rec.bytes, 1))()
        if rec.bytes:
            _call("e2sar_hip_memcpy_d2h", self.ctx.handle, buf, self.arena_ptr + rec.arenaOffset, rec.bytes)
        return bytes(buf)[: rec.bytes]

    def arena_tensor(self) -> torch.Tensor:
        """Zero-copy uint8 view of the whole device arena."""
        return _device_view(self.arena_ptr, self.arena_bytes, self.ctx.torch_device)


# e2sar_hip_rows_cell: the state of one (event, source) of a RowWindow
ROWS_CELL = np.dtype(_capi.RowsCell)
ROWS_CELL_BYTES = ROWS_CELL.itemsize
# e2sar_hip_rows_event: one ready event of RowWindow.ready
ROWS_EVENT = np.dtype(_capi.RowsEvent)
ROWS_EVENT_BYTES = ROWS_EVENT.itemsize


class RowWindow:
    """Reassembles device-resident datagram batches straight into a dense
    [n_events, n_ids, pitch] uint8 tensor (the e2sar_hip_rows_* family): the cell of a
    fragment follows from its header alone -- row eventNum mod n_events, column j where
    ids[j] == dataId, byte bufferOffset -- so there is no event table, no arena and no second
    copy.  The window holds the events [base, base + n_events) and is a ring: advance() lets
    the oldest go.  It owns `out`, `cells` (uint8, n_events * n_ids * ROWS_CELL_BYTES), `base`
    (int64[1], read as uint64) and `counts` (int64[16]); nothing else is kept, here or in the
    library.  Row bytes are never zeroed by these: a cell's `bytes` and flags say what of its row
    holds.  alloc_ready() and ready() add the delivery half: which of the oldest events are whole or
    given up is decided on the device, their rows are zero-filled on request, and the count goes
    to advance() as a device word.

    With step = S > 1 and phase = P the window is one rank's share of a stream sharded by
    eventNum % S (dist.owner): position i holds event base + i * S, base % S == P, the row of an
    event is (eventNum // S) mod n_events, and a datagram of another rank's event is passed over
    at the price of its header and counted in counts[10].  advance(), ready()'s slack and k_max
    then count positions, that is owned events.  Event numbers do not wrap on such a window.

    With frag_bytes (the sender's payload per datagram, the Segmenter's maxPld) the window survives
    duplicates: it also owns `seen` (int32, max_frags bits per cell), reassemble(), advance() and
    clear() go to the e2sar_hip_rows_*_seen calls, a fragment that arrives twice is taken once and
    counted in counts[11], and a COMPLETE cell has had every byte of its row's event written.
    max_frags (a multiple of 128) defaults to the fragments of `pitch` bytes, rounded up; an event
    longer than the pitch needs more to complete.
    """

    @staticmethod
    def seen_frags(pitch: int, frag_bytes: Optional[int], max_frags: Optional[int] = None) -> int:
        """The max_frags of a window: the argument checks of frag_bytes= and max_frags=, and the
        default -- cdiv(pitch, frag_bytes) rounded up to a multiple of 128.  0 without frag_bytes."""
        unit = _capi.ROWS_SEEN_FRAGS_UNIT
        if frag_bytes is None:
            if max_frags is not None:
                raise ValueError("max_frags needs frag_bytes")
            return 0
        if not 0 < int(frag_bytes) < 1 << 32:
            raise ValueError("frag_bytes must be in [1, 2^32)")
        if max_frags is None:
            return -(-(-(-int(pitch) // int(frag_bytes))) // unit) * unit
        if not 0 < int(max_frags) < 1 << 32 or int(max_frags) % unit:
            raise ValueError("max_frags must be a multiple of 128 in (0, 2^32)")
        return int(max_frags)

    def __init__(self, ctx: Context, ids: Sequence[int], n_events: int, pitch: int, event_base: int = 0,
                 with_lb_header: bool = True, step: int = 1, phase: int = 0, frag_bytes: Optional[int] = None,
                 max_frags: Optional[int] = None):
        ids = [int(d) for d in ids]
        if not ids or len(ids) > _capi.ROWS_MAX_IDS:
            raise ValueError("a RowWindow names 1..64 dataIds")
        self.step, self.phase = int(step), int(phase)
        if self.step > 1 and (int(event_base) & 0xFFFFFFFFFFFFFFFF) % self.step != self.phase:
            raise ValueError("event_base % step must be phase")
        self.max_frags = self.seen_frags(pitch, frag_bytes, max_frags)
        self.frag_bytes = None if frag_bytes is None else int(frag_bytes)
        self.ctx = ctx
        self.ids = ids
        self.n_events = int(n_events)
        self.pitch = int(pitch)
        self.with_lb_header = with_lb_header
        dev = ctx.torch_device
        self.out = torch.empty((self.n_events, len(ids), self.pitch), dtype=torch.uint8, device=dev)
        self.cells = torch.empty(self.n_events * len(ids) * ROWS_CELL_BYTES, dtype=torch.uint8, device=dev)
        self.base = torch.empty(1, dtype=torch.int64, device=dev)
        self.counts = torch.empty(16, dtype=torch.int64, device=dev)
        self._ids = (C.c_uint16 * len(ids))(*ids)
        self._w = _capi.Rows(self.out.data_ptr(), self.cells.data_ptr(), self.base.data_ptr(), self.counts.data_ptr(),
                             self._ids, len(ids), self.n_events, self.pitch, 1 if with_lb_header else 0, self.step, self.phase)
        self.seen, self._seen = None, None
        if self.frag_bytes is not None:
            self.seen = torch.empty(self.n_events * len(ids) * (self.max_frags // 32), dtype=torch.int32, device=dev)
            self._seen = _capi.RowsSeen(self.seen.data_ptr(), self.frag_bytes, self.max_frags)
        self.clear(event_base)

    def _rows_call(self, name: str, *args) -> None:
        """e2sar_hip_rows_<name>(ctx, w, ...), or with frag_bytes e2sar_hip_rows_<name>_seen(ctx, w, seen, ...)."""
        if self._seen is None:
            _call("e2sar_hip_rows_" + name, self.ctx.handle, C.byref(self._w), *args)
        else:
            _call("e2sar_hip_rows_" + name + "_seen", self.ctx.handle, C.byref(self._w), C.byref(self._seen), *args)

    @staticmethod
    def first_owned(first_event: int, world: int, rank: int) -> int:
        """The smallest event number >= first_event that rank `rank` of `world` owns
        (eventNum % world == rank)."""
        first_event, world, rank = int(first_event), int(world), int(rank)
        if world < 1 or not 0 <= rank < world:
            raise ValueError("rank must be in [0, world)")
        return first_event + (rank - first_event) % world

    @classmethod
    def for_rank(cls, ctx: Context, ids: Sequence[int], n_events: int, pitch: int, world: int, rank: int,
                 first_event: int = 0, with_lb_header: bool = True, frag_bytes: Optional[int] = None,
                 max_frags: Optional[int] = None) -> "RowWindow":
        """The window of rank `rank` of `world` on a stream that starts at first_event: step world,
        phase rank, its base the rank's first event (first_owned)."""
        return cls(ctx, ids, n_events, pitch, cls.first_owned(first_event, world, rank), with_lb_header,
                   step=world, phase=rank, frag_bytes=frag_bytes, max_frags=max_frags)

    def reassemble(self, packets: torch.Tensor, stride: int, lens: torch.Tensor, max_packets: int,
                   count: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None) -> None:
        """The first min(count[0], max_packets) datagrams of the batch -- max_packets when
        `count` (an int32 device tensor, read as uint32 by the kernel) is omitted -- into the
        window (e2sar_hip_rows_reassemble): one launch, no host read, capturable."""
        if lens.dtype != torch.int32 or packets.dtype != torch.uint8 or (count is not None and count.dtype != torch.int32):
            raise ValueError("packets is a uint8 tensor, lens and count are int32 tensors")
        if count is not None and count.numel() < 1:
            raise ValueError("count is empty")
        _need_batch("packet batch buffers too small for max_packets", max_packets, stride, packets, lens)
        self._rows_call("reassemble", packets.data_ptr(), stride, lens.data_ptr(), _p(count), max_packets, _s(stream))

    def advance(self, k: int, count: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Let go of the min(count[0], k, n_events) oldest events (positions of the window) -- min(k, n_events) when
        `count` (int32 device tensor) is omitted: their cells are counted (counts[8] released
        incomplete, counts[9] complete) and zeroed, and the base moves on
        (e2sar_hip_rows_advance).  No host read, capturable."""
        if count is not None and (count.dtype != torch.int32 or count.numel() < 1):
            raise ValueError("count is an int32 tensor of at least 1")
        self._rows_call("advance", _p(count), int(k), _s(stream))

    def clear(self, event_base: int = 0, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Every cell and count zeroed, the window at [event_base, event_base + n_events)
        (e2sar_hip_rows_clear; on a lattice event_base % step must be phase); row bytes stay."""
        self._rows_call("clear", int(event_base) & 0xFFFFFFFFFFFFFFFF, _s(stream))

    def alloc_ready(self, k_max: int) -> None:
        """Give the window what ready() writes: `ready` (int32[8], read as uint32), `events`
        (uint8, k_max * ROWS_EVENT_BYTES) and the call's work buffer."""
        dev = self.out.device
        self.k_max = int(k_max)
        self.ready_words = torch.zeros(8, dtype=torch.int32, device=dev)
        self.events = torch.zeros(self.k_max * ROWS_EVENT_BYTES, dtype=torch.uint8, device=dev)
        self.ready_work = torch.empty(int(lib().e2sar_hip_rows_ready_work_bytes(self.n_events)), dtype=torch.uint8, device=dev)

    def ready(self, slack: int, k_max: Optional[int] = None, required: Optional[Sequence[int]] = None, zero: bool = False,
              stream: Optional[torch.cuda.Stream] = None) -> None:
        """Decide on the device which of the oldest events are ready (e2sar_hip_rows_ready): an
        event whose `required` dataIds (default: all) are complete, or one that an event
        `slack` or more newer has overtaken (_capi.ROWS_NEVER_GIVEN_UP: none), up to the first
        that is neither and at most k_max (default: alloc_ready's).  Writes `ready_words` --
        k, complete, given up, horizon, complete cells, open incomplete cells -- and the k
        records of `events`; with `zero`, the k rows hold zeros wherever they do not hold a
        whole event.  advance(k_max, count=ready_words[0:1]) lets the k events go.  No host
        read, capturable; parse_ready reads the result back."""
        if not hasattr(self, "ready_words"):
            raise ValueError("alloc_ready(k_max) comes first")
        k_max = self.k_max if k_max is None else int(k_max)
        if min(k_max, self.n_events) > self.k_max:
            raise ValueError("more events than alloc_ready made room for")
        mask = 0
        for d in required or ():
            mask |= 1 << self.ids.index(int(d))
        rule = _capi.RowsReadyRule(mask, int(slack), k_max, _capi.ROWS_READY_ZERO if zero else 0, 0)
        _call("e2sar_hip_rows_ready", self.ctx.handle, C.byref(self._w), C.byref(rule), self.ready_words.data_ptr(),
              self.events.data_ptr() if self.events.numel() else 0, self.ready_work.data_ptr(), self.ready_work.numel(), _s(stream))

    def parse_ready(self):
        """-> (the 8 words ready() wrote, a ROWS_EVENT array of its k records): waits for the
        device and copies."""
        torch.cuda.synchronize(self.ready_words.device)
        words = [int(v) & 0xFFFFFFFF for v in self.ready_words.cpu().tolist()]
        raw = self.events[: words[0] * ROWS_EVENT_BYTES].cpu().numpy().tobytes()
        return words, np.frombuffer(raw, ROWS_EVENT).copy()

    def parse_cells(self) -> np.ndarray:
        """The cells on the host, a ROWS_CELL array of shape [n_events, n_ids]: waits for the
        device and copies."""
        torch.cuda.synchronize(self.cells.device)
        raw = self.cells.cpu().numpy().tobytes()
        return np.frombuffer(raw, ROWS_CELL).reshape(self.n_events, len(self.ids)).copy()

    def parse_seen(self) -> np.ndarray:
        """The fragment bits of a window with frag_bytes on the host, uint32 of shape
        [n_events, n_ids, max_frags // 32] -- bit f of a cell in word f // 32 at 1 << (f % 32):
        waits for the device and copies."""
        if self.seen is None:
            raise ValueError("a window without frag_bytes keeps no bits")
        torch.cuda.synchronize(self.seen.device)
        return self.seen.cpu().numpy().view(np.uint32).reshape(self.n_events, len(self.ids), self.max_frags // 32).copy()

    def parse_counts(self):
        """-> (the 16 counts, the base), as Python integers: waits for the device and copies."""
        torch.cuda.synchronize(self.counts.device)
        counts = [int(v) & 0xFFFFFFFFFFFFFFFF for v in self.counts.cpu().tolist()]
        return counts, int(self.base.cpu().item()) & 0xFFFFFFFFFFFFFFFF


class _CudaArray:
    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {
            "shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None,
        }


def _device_view(ptr: int, nbytes: int, device: torch.device) -> torch.Tensor:
    return torch.as_tensor(_CudaArray(ptr, nbytes), device=device)
