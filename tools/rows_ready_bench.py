#!/usr/bin/env python3
"""Deciding on the device which events of a rows window are ready, against deciding on the host
(DESIGN.md 4.14).

E events of B bytes are segmented on the device and reassembled into an [E, 1, pitch] window,
pitch = B rounded up to 256; the clear and the reassembly are outside every clock.  Then, per
case, two ways of letting the ready events go, alternating in one process after a warm-up
(the method of tools/ab_method.py):

  device   e2sar_hip_rows_ready, then e2sar_hip_rows_advance with d_k = d_ready: no host read
  host     synchronise, copy the cells and the base to the host, decide in numpy by the same
           rule, e2sar_hip_rows_advance(k)

  (a) every event whole, no zero fill       (b) the same with E2SAR_HIP_ROWS_READY_ZERO: nothing to zero
  (c) a batch that lost one fragment of every event, slack 0, zero fill: every row is zeroed;
      beside it Tensor.zero_() over the same number of bytes, and the device way without the flag

The host way waits for the device, so both ways are timed by the host's clock from an idle device
to an idle device (wall_us); the device way also with HIP events while the device spins (gpu_us),
which is what a captured chain pays.

  python tools/rows_ready_bench.py [--events 64] [--event-bytes 1048576] [--mtu 9000]
                                   [--reps 40] [--warmup 5] [--out FILE]
Prints one JSON line (and writes it to --out).
"""
import os
import statistics
import time

import numpy as np

import ab_method


def host_decide(cells, base, n_events, n_ids, slack, k_max):
    """k by the rule of e2sar_hip_rows_ready, all ids required, from the cells as the host sees them."""
    order = (base + np.arange(n_events, dtype=np.uint64)) & np.uint64(n_events - 1)
    c = cells.reshape(n_events, n_ids)[order.astype(np.int64)]
    complete = ((c["flags"] & 1) != 0).all(axis=1)
    opened = (c["bytes"] != 0).any(axis=1)
    H = int(np.flatnonzero(opened)[-1]) + 1 if opened.any() else 0
    i = np.arange(n_events)
    given_up = ~complete & (i < H) & (H - 1 - i >= slack)
    stop = np.flatnonzero(~(complete | given_up)[: min(k_max, n_events)])
    return int(stop[0]) if stop.size else min(k_max, n_events)


def wall(fn, before, torch):
    before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = ab_method.parser(events=64)
    ap.set_defaults(mtu=9000)
    args = ap.parse_args()

    import torch
    from e2sar_amd import sar, _capi

    ab_method.need_gpu("rows_ready_bench")
    dev = torch.device("cuda:0")
    ctx = sar.Context(0)
    E, B = args.events, args.event_bytes
    base = 1 << 48
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    pitch = (B + 255) // 256 * 256
    src = torch.randint(1, 256, (E, pitch), dtype=torch.uint8, device=dev, generator=g)
    seg = sar.DeviceSegmenter(ctx, mtu=args.mtu, lb_hdr_version=2)
    plan = seg.plan([(src[i].data_ptr(), B, base + i, 4321, 1 + i, base + i) for i in range(E)])
    n = plan.total_packets
    pk, ln = seg.alloc_packets(n)
    seg.segment(plan, pk, ln)
    # the same batch without the second datagram of every event
    per = n // E
    assert per * E == n and per >= 3, (n, E)
    keep = torch.tensor([p for p in range(n) if p % per != 1], device=dev)
    pk_lossy = pk[: n * seg.stride].view(n, seg.stride)[keep].contiguous().view(-1)
    ln_lossy = ln[:n][keep].contiguous()
    n_lossy = n - E

    n_events = 1
    while n_events < E:
        n_events <<= 1
    win = sar.RowWindow(ctx, [4321], n_events, pitch, base, with_lb_header=True)
    win.alloc_ready(n_events)
    other = torch.empty(E * pitch, dtype=torch.uint8, device=dev)

    def fill_whole():
        win.clear(base)
        win.reassemble(pk, seg.stride, ln, n)

    def fill_lossy():
        win.clear(base)
        win.reassemble(pk_lossy, seg.stride, ln_lossy, n_lossy)

    def device_way(slack, zero):
        def fn():
            win.ready(slack, n_events, zero=zero)
            win.advance(n_events, count=win.ready_words[0:1])
        return fn

    def host_way(slack):
        def fn():
            torch.cuda.synchronize()
            cells = np.frombuffer(win.cells.cpu().numpy().tobytes(), sar.ROWS_CELL)
            b = int(win.base.cpu().item()) & 0xFFFFFFFFFFFFFFFF
            win.advance(host_decide(cells, b, n_events, 1, slack, n_events))
        return fn

    never = _capi.ROWS_NEVER_GIVEN_UP
    # what each case decides, once
    fill_whole()
    win.ready(never, n_events, zero=True)
    words, events = win.parse_ready()
    assert words[:6] == [E, E, 0, E, E, 0], words
    assert np.array_equal(win.out[:, 0, :B].cpu().numpy()[events["row"][:E]], src[:, :B].cpu().numpy())
    cells = np.frombuffer(win.cells.cpu().numpy().tobytes(), sar.ROWS_CELL)
    assert host_decide(cells, base, n_events, 1, never, n_events) == E
    fill_lossy()
    win.ready(0, n_events, zero=True)
    words, _ = win.parse_ready()
    assert words[:6] == [E, 0, E, E, 0, E], words
    assert not win.out[:E].any().item()
    cells = np.frombuffer(win.cells.cpu().numpy().tobytes(), sar.ROWS_CELL)
    assert host_decide(cells, base, n_events, 1, 0, n_events) == E

    cases = {
        "a": (fill_whole, {"device": device_way(never, False), "host": host_way(never)}),
        "b": (fill_whole, {"device": device_way(never, True), "host": host_way(never)}),
        "c": (fill_lossy, {"device": device_way(0, True), "device_flag_off": device_way(0, False),
                           "zero_": lambda: other.zero_()}),
    }
    result = {"tool": "rows_ready_bench", "events": E, "event_bytes": B, "mtu": args.mtu, "reps": args.reps,
              "zeroed_bytes_c": E * pitch, "lib": os.path.basename(_capi.LIB_PATH),
              "device": torch.cuda.get_device_name(0), "case": {}}
    for name, (before, forms) in cases.items():
        gpu = ab_method.measure({k: (fn, before) for k, fn in forms.items() if k != "host"}, args)
        walls = {k: [] for k in forms}
        for rep in range(args.warmup + args.reps):
            for k, fn in forms.items():
                t = wall(fn, before, torch)
                if rep >= args.warmup:
                    walls[k].append(t)
        out = {"gpu_us": ab_method.summary(gpu), "wall_us": ab_method.summary(walls)}
        if "host" in forms:
            out["device_over_host_wall"] = round(statistics.median(walls["device"]) / statistics.median(walls["host"]), 3)
        else:
            out["device_over_zero_gpu"] = round(statistics.median(gpu["device"]) / statistics.median(gpu["zero_"]), 3)
            out["flag_cost_over_zero_gpu"] = round((statistics.median(gpu["device"]) - statistics.median(gpu["device_flag_off"]))
                                                   / statistics.median(gpu["zero_"]), 3)
        result["case"][name] = out
    ab_method.write_line(result, args.out)


if __name__ == "__main__":
    main()
