#!/usr/bin/env python3
"""Reassembly with the datagram count on the device against the host-count call.

One batch of E rows of B bytes (the bench's batch: 205 x 1 MiB, MTU 1500) is segmented just
before every timed reassembly, so its datagrams are as warm as a device-side chain leaves
them.  Each form is timed with HIP events, the forms alternating in one process after a
warm-up, while the device spins so the host side of a call is not in its time.  The
reassembler is recycled (force) in the untimed segmentation launch in front of each call.

  host         e2sar_hip_reassemble_batch with the host's n
  dev_full     e2sar_hip_reassemble_batch_dev, *d_count = maxPackets = n
  host_sparse  e2sar_hip_reassemble_batch with n / 64
  dev_sparse   e2sar_hip_reassemble_batch_dev, *d_count = n / 64 under the bound n: 63 of 64
               workgroups read the count and exit

and the whole chain recycle -> emit -> reassemble -> collect (rows), timed from its first
launch to its last kernel's end:

  chain_graph  with reassemble_dev on emit's counts[1:2], captured once into a HIP graph and replayed
  chain_host   the same calls launched one by one, the host reading counts[1] between emit
               and e2sar_hip_reassemble_batch (its wait is in the time)

dev_full's events are compared with the source rows once.

  python tools/reas_dev_bench.py [--events 205] [--event-bytes 1048576] [--mtu 1500] [--reps 40] [--warmup 5] [--out FILE]
Prints one JSON line (and writes it to --out).  Rates count datagram bytes read + event bytes written.
"""
import os

import ab_method


def main():
    args = ab_method.parser().parse_args()

    import torch
    from e2sar_amd import sar, _capi

    ab_method.need_gpu("reas_dev_bench")
    dev = torch.device("cuda:0")
    ctx = sar.Context(0)
    E, B = args.events, args.event_bytes
    seg = sar.DeviceSegmenter(ctx, mtu=args.mtu, lb_hdr_version=2)
    per_row = sar.num_packets(B, seg.max_pld)
    numbering = dict(event_num_base=1000, lb_tick_base=1 << 48, lb_tick_step=1, data_id=4321, entropy_base=1)
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + E)
    rows = torch.randint(0, 256, (E, B), dtype=torch.uint8, device=dev, generator=g)
    plan = seg.plan([(rows[i].data_ptr(), B, 1000 + i, 4321, 1 + i, (1 << 48) + i) for i in range(E)])
    n = plan.total_packets
    assert n == E * per_row
    pk, ln = seg.alloc_packets(n)
    R = sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=4096, queue_capacity=4096,
                              arena_bytes=E * ((B + 255) // 256 * 256) + (1 << 20))
    sparse = max(1, n // 64)
    d_n = torch.tensor([n, sparse], dtype=torch.int32, device=dev)
    # the chain's buffers
    d_len = torch.full((E,), B, dtype=torch.int32, device=dev)
    d_count = torch.tensor([E], dtype=torch.int32, device=dev)
    events = torch.zeros(E * sar.SEG_EVENT_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int32, device=dev)
    out = torch.empty((E, B), dtype=torch.uint8, device=dev)
    index = torch.empty(E * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
    ccounts = torch.zeros(4, dtype=torch.int64, device=dev)

    def fresh():
        seg.segment(plan, pk, ln, recycle=R, force=True)      # untimed: warm datagrams, an empty reassembler

    def emit(stream=None):
        seg.emit(rows.view(-1), d_len, pk, ln, events, counts, pitch=B, count=d_count, max_events=E, stream=stream,
                 **numbering)

    def chain_dev(stream=None):
        R.recycle(force=True, stream=stream)
        emit(stream)
        R.reassemble_dev(pk, seg.stride, ln, counts[1:2], max_packets=n, stream=stream)
        R.collect(out.view(-1), index, ccounts, 0, E, B, stream=stream)

    def chain_host():
        R.recycle(force=True)
        emit()
        R.reassemble(pk, seg.stride, ln, int(counts[1].item()))       # the host waits for emit and reads the count
        R.collect(out.view(-1), index, ccounts, 0, E, B)

    def delivered(label, want):
        torch.cuda.synchronize()
        got = sar.parse_collect(index, ccounts)
        st = R.stats()
        assert len(got) == want == st.eventSuccess and st.errorFlags == 0, (label, len(got), st.eventSuccess, st.errorFlags)
        for r, rec in enumerate(got):
            assert torch.equal(out[r], rows[int(rec["eventNum"]) - 1000]), f"{label}: event {int(rec['eventNum'])} differs"

    # once: dev_full delivers the source rows; so do both chains
    fresh()
    R.reassemble_dev(pk, seg.stride, ln, d_n[0:1], max_packets=n)
    R.collect(out.view(-1), index, ccounts, 0, E, B)
    delivered("dev_full", E)
    R.reset_stats()
    chain_host()
    delivered("chain_host", E)
    R.reset_stats()
    chain_dev()                                                   # also: internal state exists before the capture
    delivered("chain_dev", E)
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        chain_dev(cap)
    R.reset_stats()
    out.zero_()
    torch.cuda.synchronize()
    graph.replay()
    delivered("chain_graph", E)

    # (fn, before): `before` is the untimed segmentation, enqueued inside the spin
    forms = {
        "host": (lambda: R.reassemble(pk, seg.stride, ln, n), fresh),
        "dev_full": (lambda: R.reassemble_dev(pk, seg.stride, ln, d_n[0:1], max_packets=n), fresh),
        "host_sparse": (lambda: R.reassemble(pk, seg.stride, ln, sparse), fresh),
        "dev_sparse": (lambda: R.reassemble_dev(pk, seg.stride, ln, d_n[1:2], max_packets=n), fresh),
        "chain_graph": (graph.replay, None),
        "chain_host": (chain_host, None),
    }
    dgram = 36 + seg.max_pld
    tail = B - (per_row - 1) * seg.max_pld
    full_bytes = E * ((per_row - 1) * dgram + 36 + tail) + E * B
    moved = {"host": full_bytes, "dev_full": full_bytes}
    us = ab_method.measure(forms, args)
    result = {"tool": "reas_dev_bench", "events": E, "event_bytes": B, "mtu": args.mtu, "reps": args.reps,
              "datagrams": n, "sparse_datagrams": sparse, "lib": os.path.basename(_capi.LIB_PATH),
              "device": torch.cuda.get_device_name(0), "forms": ab_method.summary(us, moved)}
    ab_method.write_line(result, args.out)


if __name__ == "__main__":
    main()
