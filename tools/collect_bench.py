#!/usr/bin/env python3
"""Device-side delivery against the host-planned gather.

E events of B bytes are segmented and reassembled on the device; then three ways of moving
the completed events out of the arena into one device buffer are timed with HIP events,
alternating in one process after a warm-up:

  ragged  e2sar_hip_reas_collect, pitch 0, align 256 (plan launch + copy launch)
  rows    e2sar_hip_reas_collect, pitch = B rounded up to 16
  spans   e2sar_hip_copy_spans over the same source and destination spans, which the host
          can only know after a round trip (here: relay_plan's descriptors read back, the
          span table built before the clock starts, so the round trip is not in its time)

in two cache states: `steady` repeats the three over one reassembled batch; `fresh` recycles
and reassembles the batch before every timed call, so the arena was just written.  Every
form's output is compared with the events' source bytes once.

  python tools/collect_bench.py [--events 205] [--event-bytes 1048576] [--mtu 1500]
                                [--reps 40] [--warmup 5] [--out FILE]
Prints one JSON line (and writes it to --out).  Rates count read + write bytes.
"""
import ctypes as C
import os

import numpy as np

import ab_method


def main():
    args = ab_method.parser().parse_args()

    import torch
    from e2sar_amd import sar, _capi

    ab_method.need_gpu("collect_bench")
    dev = torch.device("cuda:0")
    ctx = sar.Context(0)
    E, B = args.events, args.event_bytes
    seg = sar.DeviceSegmenter(ctx, mtu=args.mtu, lb_hdr_version=2)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    ev_stride = (B + 255) // 256 * 256
    src = torch.randint(0, 256, (E, ev_stride), dtype=torch.uint8, device=dev, generator=g)
    plan = seg.plan([(src[i].data_ptr(), B, i, 4321, 1 + i, (1 << 48) + i) for i in range(E)])
    n = plan.total_packets
    pk, ln = seg.alloc_packets(n)
    seg.segment(plan, pk, ln)
    table = 1
    while table < 8 * E:
        table <<= 1
    R = sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=table, queue_capacity=E + 64,
                              lost_capacity=64, arena_bytes=E * ev_stride + 4096)
    pitch = (B + 15) // 16 * 16
    out = torch.zeros(E * max(ev_stride, pitch), dtype=torch.uint8, device=dev)
    index = torch.zeros(E * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    desc = torch.zeros(E * sar.SEG_EVENT_BYTES, dtype=torch.uint8, device=dev)
    rcnt = torch.zeros(2, dtype=torch.int32, device=dev)
    seg_event = np.dtype([("data", "<u8"), ("eventNum", "<u8"), ("lbTick", "<u8"), ("bytes", "<u4"),
                          ("pktBase", "<u4"), ("dataId", "<u2"), ("entropy", "<u2"), ("reserved", "<u4")])

    def reassemble():
        R.recycle(force=True)
        R.reassemble(pk, seg.stride, ln, n)

    def spans():
        """(src, dst, bytes) of every completed record in record order, destinations as the ragged form lays them out."""
        R.relay_plan(desc, rcnt, 0, E, seg.max_pld, 0, 0)
        torch.cuda.synchronize()
        t = np.frombuffer(desc.cpu().numpy().tobytes(), seg_event)[: int(rcnt[0].item())]
        arr = (_capi.CopySpan * len(t))()
        for k, r in enumerate(t):
            arr[k] = _capi.CopySpan(int(r["data"]), out.data_ptr() + k * ev_stride, int(r["bytes"]))
        return arr, t

    sp, t = None, None                          # the span table of the batch in the arena, and its records

    def fresh():
        nonlocal sp, t
        reassemble()
        sp, t = spans()

    forms = {
        "ragged": lambda: R.collect(out, index, counts, 0, E, 0, 256),
        "rows": lambda: R.collect(out, index, counts, 0, E, pitch),
        "spans": lambda: _capi.check(_capi.lib().e2sar_hip_copy_spans(
            ctx.handle, sp, len(sp), C.c_void_p(int(torch.cuda.current_stream().cuda_stream)))),
    }

    # every form delivers every event's bytes
    fresh()
    assert len(sp) == E, len(sp)
    host = src[:, :B].cpu().numpy()
    for name, fn in forms.items():
        out.zero_()
        fn()
        torch.cuda.synchronize()
        step = pitch if name == "rows" else ev_stride
        got = out[: E * step].view(E, step)[:, :B].cpu().numpy()
        for k, r in enumerate(t):
            assert np.array_equal(got[k], host[int(r["eventNum"])]), (name, k)

    result = {"tool": "collect_bench", "events": E, "event_bytes": B, "mtu": args.mtu, "reps": args.reps,
              "lib": os.path.basename(_capi.LIB_PATH), "device": torch.cuda.get_device_name(0), "states": {}}
    moved = {name: 2 * E * B for name in forms}
    for state in ("steady", "fresh"):
        us = ab_method.measure(forms, args, prepare=fresh if state == "fresh" else None)
        result["states"][state] = ab_method.summary(us, moved)
    ab_method.write_line(result, args.out)
    R.close()


if __name__ == "__main__":
    main()
