#!/usr/bin/env python3
"""The turn against the host round trip it replaces.

A reassembler of the headline shape (1 MiB events at MTU 1500, a 4096-slot table, COMPACTABLE)
is brought into a state -- P events of 1 MiB in progress, each lacking its last datagram, and
C completed records, all consumed through the cursor -- and one upkeep step is timed on it:

  host   the path before the turn: wait for the device, e2sar_hip_reas_poll, then
         e2sar_hip_reas_compact (P > 0) or e2sar_hip_reas_recycle(force = 0) (P = 0); and
         `host_wait_poll`, the wait and the read-back alone
  turn   e2sar_hip_reas_turn with all-zero marks; `turn_skipped`: marks out of reach

for P in 0, 8, 64 and C in 0, 1024.  Every form is timed by the host's clock around the call
and a device wait, the state rebuilt untimed before every call, the forms alternating in one
process after a warm-up; the turn also with HIP events while the device spins (ab_method), the
time of its five launches alone.  One turn per state is checked against what it must report.

  python tools/turn_bench.py [--event-bytes 1048576] [--mtu 1500] [--reps 40] [--warmup 5] [--out FILE]
Prints one JSON line (and writes it to --out).
"""
import os
import time

import ab_method

IN_PROGRESS = (0, 8, 64)
CONSUMED = (0, 1024)
FAR = dict(arena_mark=1 << 62, record_mark=0xFFFFFFFF, table_mark=0xFFFFFFFF)


def main():
    args = ab_method.parser(events=None).parse_args()

    import torch
    from e2sar_amd import sar

    ab_method.need_gpu("turn_bench")
    dev = torch.device("cuda:0")
    ctx = sar.Context(0)
    B, P, C = args.event_bytes, max(IN_PROGRESS), max(CONSUMED)
    seg = sar.DeviceSegmenter(ctx, mtu=args.mtu, lb_hdr_version=2)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    ev_stride = (B + 255) // 256 * 256
    big = torch.randint(0, 256, (P, ev_stride), dtype=torch.uint8, device=dev, generator=g)
    small = torch.randint(0, 256, (C, 256), dtype=torch.uint8, device=dev, generator=g)
    per = sar.num_packets(B, seg.max_pld)
    # the P partial events: every datagram but each event's last; the C small ones: one datagram each
    plan_big = seg.plan([(big[i].data_ptr(), B, 10_000 + i, 4321, 1 + i, (1 << 48) + i) for i in range(P)])
    pk_all, ln_all = seg.alloc_packets(plan_big.total_packets)
    seg.segment(plan_big, pk_all, ln_all)
    keep = torch.tensor([i * per + j for i in range(P) for j in range(per - 1)], device=dev)
    pk_big = pk_all.view(-1, seg.stride)[keep].contiguous().view(-1)
    ln_big = ln_all[keep].contiguous()
    plan_small = seg.plan([(small[i].data_ptr(), 64, i, 4321, 1, (1 << 48) + i) for i in range(C)])
    pk_small, ln_small = seg.alloc_packets(plan_small.total_packets)
    seg.segment(plan_small, pk_small, ln_small)
    R = sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=4096, queue_capacity=4096, lost_capacity=64,
                              arena_bytes=P * ev_stride + C * 256 + 4096, compactable=True)
    out = torch.zeros(C * 256 + 4096, dtype=torch.uint8, device=dev)
    index = torch.zeros(4096 * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    cursor = R.new_cursor()

    def state(p, c):
        """p events in progress, c records completed and consumed; nothing pending on the host's side."""
        def prepare():
            R.recycle(force=True)
            cursor.zero_()
            if c:
                R.reassemble(pk_small, seg.stride, ln_small, c)
            if p:
                R.reassemble(pk_big, seg.stride, ln_big, p * (per - 1))
            R.collect_next(out, index, counts, cursor, 4096)
        return prepare

    def host_wait_poll():
        torch.cuda.synchronize()
        R.poll()

    def host_path(p):
        def fn():
            host_wait_poll()
            if p:
                R.compact()
            else:
                R.recycle(force=False)
        return fn

    turn = lambda: R.turn(cursor, status)
    skipped = lambda: R.turn(cursor, status, **FAR)

    # one turn per state reports what it must
    for p in IN_PROGRESS:
        for c in CONSUMED:
            state(p, c)()
            turn()
            torch.cuda.synchronize()
            assert status.cpu().tolist() == [1, p, 0, p * ev_stride], (p, c, status.cpu().tolist())
            st = R.stats()
            assert st.inProgress == p and st.tableUsed == p and st.completedPending == 0 and st.errorFlags == 0
    state(8, 0)()
    skipped()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0, 8 * ev_stride]

    def host_clock(forms):
        """name -> (prepare, fn): microseconds of fn plus a device wait, by the host's clock."""
        us = {name: [] for name in forms}
        for rep in range(args.warmup + args.reps):
            for name, (prepare, fn) in forms.items():
                prepare()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if rep >= args.warmup:
                    us[name].append((t1 - t0) * 1e6)
        return us

    hforms, dforms = {}, {}
    for p in IN_PROGRESS:
        for c in CONSUMED:
            tag = f"p{p}_c{c}"
            hforms[f"host_{tag}"] = (state(p, c), host_path(p))
            hforms[f"host_wait_poll_{tag}"] = (state(p, c), host_wait_poll)
            hforms[f"turn_{tag}"] = (state(p, c), turn)
            dforms[f"turn_{tag}"] = (state(p, c), turn)
    hforms["turn_skipped_p8_c0"] = (state(8, 0), skipped)
    dforms["turn_skipped_p8_c0"] = (state(8, 0), skipped)

    result = {"tool": "turn_bench", "event_bytes": B, "mtu": args.mtu, "reps": args.reps, "table_slots": 4096,
              "in_progress": list(IN_PROGRESS), "consumed": list(CONSUMED),
              "lib": os.path.basename(sar._capi.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    result["host_clock"] = ab_method.summary(host_clock(hforms))
    dev_us = {name: [] for name in dforms}
    for rep in range(args.warmup + args.reps):
        for name, (prepare, fn) in dforms.items():
            prepare()
            t_us = ab_method.timed(fn)
            if rep >= args.warmup:
                dev_us[name].append(t_us)
    result["device_events"] = ab_method.summary(dev_us)
    hc = result["host_clock"]
    result["turn_below_wait_and_readback"] = {
        f"p{p}_c{c}": hc[f"turn_p{p}_c{c}"]["median_us"] < hc[f"host_wait_poll_p{p}_c{c}"]["median_us"]
        for p in IN_PROGRESS for c in CONSUMED}
    result["host_over_turn_median"] = {
        f"p{p}_c{c}": round(hc[f"host_p{p}_c{c}"]["median_us"] / hc[f"turn_p{p}_c{c}"]["median_us"], 2)
        for p in IN_PROGRESS for c in CONSUMED}
    ab_method.write_line(result, args.out)
    R.close()


if __name__ == "__main__":
    main()
