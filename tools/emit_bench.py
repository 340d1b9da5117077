#!/usr/bin/env python3
"""Device-side production against the host-planned segmentation.

Two batches of rows in one device tensor are segmented, each form timed with HIP events,
alternating in one process after a warm-up, while the device spins so the host side of a
call is not in its time:

headline  E rows of B bytes, every row full (the bench's batch: 205 x 1 MiB, MTU 1500)
  emit    e2sar_hip_seg_emit: emit_plan_kernel + seg_flat_kernel
  batch   e2sar_hip_segment_batch over a table the host planned and uploaded beforehand
  plan    e2sar_hip_seg_emit of the same rows with every length 0 and one packet slot: the
          plan's whole scan and all its descriptor stores, plus a copy launch of E + 1
          workgroups that exit -- the nearest the ABI comes to the plan launch on its own
  idle    e2sar_hip_seg_emit with every length 0 and all packet slots: the plan plus the
          whole bound grid of workgroups that read the unit total and exit

skewed    --skew-rows rows of B bytes pitch, lengths uniform in [--skew-min, --skew-max] (4 KiB .. B)
  emit        e2sar_hip_seg_emit, packet slots for the bound (every row full)
  emit_tight  the same with exactly the slots the batch needs (a caller that knows a byte budget)
  dev         e2sar_hip_segment_batch_dev over a device-side table (the one emit wrote) with
              the bound grid: rows x ceil(maxPacketsPerEvent * spc / (256 U)) workgroups

Every form's datagrams are compared with `batch`'s (headline) or `dev`'s (skewed) once.

  python tools/emit_bench.py [--events 205] [--event-bytes 1048576] [--skew-rows 1024] [--skew-min 4096]
                             [--skew-max B] [--mtu 1500] [--reps 40] [--warmup 5] [--out FILE]
Prints one JSON line (and writes it to --out).  Rates count event bytes read + datagram bytes written.
"""
import os

import numpy as np

import ab_method


def main():
    ap = ab_method.parser()
    ap.add_argument("--skew-rows", type=int, default=1024)
    ap.add_argument("--skew-min", type=int, default=4096)
    ap.add_argument("--skew-max", type=int, default=None)
    args = ap.parse_args()

    import torch
    from e2sar_amd import sar, _capi

    ab_method.need_gpu("emit_bench")
    dev = torch.device("cuda:0")
    ctx = sar.Context(0)
    B = args.event_bytes
    seg = sar.DeviceSegmenter(ctx, mtu=args.mtu, lb_hdr_version=2)
    per_row = sar.num_packets(B, seg.max_pld)
    numbering = dict(event_num_base=1000, lb_tick_base=1 << 48, lb_tick_step=1, data_id=4321, entropy_base=1)

    def measure(forms, moved):
        return ab_method.summary(ab_method.measure(forms, args), moved)

    def batch(rows_n, lengths):
        """-> the buffers of one batch of rows_n rows with the given host lengths."""
        g = torch.Generator(device=dev)
        g.manual_seed(1234 + rows_n)
        rows = torch.randint(0, 256, (rows_n, B), dtype=torch.uint8, device=dev, generator=g)
        d_len = torch.from_numpy(lengths.astype(np.int32)).to(dev)
        pk, ln = seg.alloc_packets(rows_n * per_row)
        pk.zero_()                              # the forms' buffers are compared whole
        events = torch.zeros(rows_n * sar.SEG_EVENT_BYTES, dtype=torch.uint8, device=dev)
        counts = torch.zeros(8, dtype=torch.int32, device=dev)
        return rows, d_len, pk, ln, events, counts

    def emit(rows, d_len, pk, ln, events, counts, slots=None):
        slots = pk.numel() // seg.stride if slots is None else slots
        seg.emit(rows.view(-1), d_len, pk[: slots * seg.stride], ln[:slots], events, counts, pitch=B, **numbering)

    result = {"tool": "emit_bench", "event_bytes": B, "mtu": args.mtu, "reps": args.reps,
              "lib": os.path.basename(_capi.LIB_PATH), "device": torch.cuda.get_device_name(0), "batches": {}}

    # ---- headline: every row full ----
    E = args.events
    lengths = np.full(E, B, np.int64)
    rows, d_len, pk, ln, events, counts = batch(E, lengths)
    zero_len = torch.zeros_like(d_len)
    plan = seg.plan([(rows[i].data_ptr(), B, 1000 + i, 4321, 1 + i, (1 << 48) + i) for i in range(E)])
    n = plan.total_packets
    pk2, ln2 = seg.alloc_packets(n)
    pk2.zero_()
    seg.segment(plan, pk2, ln2)
    emit(rows, d_len, pk, ln, events, counts)
    torch.cuda.synchronize()
    assert counts[:4].tolist() == [E, n, 0, 0], counts.tolist()
    assert torch.equal(ln[:n], ln2[:n]), "headline: emit's lens differ from segment_batch's"
    a, b = pk[: n * seg.stride].view(n, seg.stride), pk2[: n * seg.stride].view(n, seg.stride)
    assert torch.equal(a, b), "headline: emit's datagrams differ"
    forms = {
        "emit": lambda: emit(rows, d_len, pk, ln, events, counts),
        "batch": lambda: seg.segment(plan, pk2, ln2),
        "plan": lambda: emit(rows, zero_len, pk, ln, events, counts, slots=1),
        "idle": lambda: emit(rows, zero_len, pk, ln, events, counts),
    }
    moved = {k: E * B + n * (36 + seg.max_pld) for k in ("emit", "batch")}
    result["batches"]["headline"] = {"events": E, "datagrams": n, "forms": measure(forms, moved)}
    del rows, pk, ln, pk2, ln2, a, b

    # ---- skewed: lengths uniform in [skew-min, skew-max] ----
    S = args.skew_rows
    hi = B if args.skew_max is None else min(args.skew_max, B)
    lengths = np.random.default_rng(77).integers(min(args.skew_min, hi), hi + 1, S)
    rows, d_len, pk, ln, events, counts = batch(S, lengths)
    n = int(sum(sar.num_packets(int(x), seg.max_pld) for x in lengths))
    pk2, ln2 = seg.alloc_packets(S * per_row)
    pk2.zero_()
    ev2, cnt2 = events.clone(), counts.clone()
    emit(rows, d_len, pk, ln, events, counts)
    emit(rows, d_len, pk2, ln2, ev2, cnt2)
    seg.segment_device(ev2, cnt2, S, per_row, pk2, ln2)      # over emit's own table: the relay form's launch
    torch.cuda.synchronize()
    assert counts[:4].tolist() == [S, n, 0, 0], counts.tolist()
    assert torch.equal(ln[:n], ln2[:n]) and torch.equal(pk[: n * seg.stride], pk2[: n * seg.stride]), "skewed: forms differ"
    forms = {
        "emit": lambda: emit(rows, d_len, pk, ln, events, counts),
        "emit_tight": lambda: emit(rows, d_len, pk, ln, events, counts, slots=n),
        "dev": lambda: seg.segment_device(ev2, cnt2, S, per_row, pk2, ln2),
    }
    moved = {k: int(lengths.sum()) + n * (36 + seg.max_pld) for k in forms}
    spc, unit = seg.stride // 16, 256 * (2 if per_row * (seg.stride // 16) <= 1 << 18 else 4)
    result["batches"]["skewed"] = {
        "rows": S, "min_bytes": int(lengths.min()), "max_bytes": int(lengths.max()), "datagrams": n, "event_bytes_total": int(lengths.sum()),
        "workgroups": {"emit": -(-S * per_row * spc // unit) + S, "emit_tight": -(-n * spc // unit) + S,
                       "dev": S * -(-per_row * spc // unit),
                       "units_of_work": int(sum(-(-sar.num_packets(int(x), seg.max_pld) * spc // unit) for x in lengths))},
        "forms": measure(forms, moved)}

    ab_method.write_line(result, args.out)


if __name__ == "__main__":
    main()
