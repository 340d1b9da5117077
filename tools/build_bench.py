#!/usr/bin/env python3
"""Device-side event building against device-side delivery.

Workload 1: E eventNums x S dataIds events of B bytes (default 41 x 5 x 1 MiB = 205 events)
are segmented and reassembled on the device; then the forms below are timed with HIP events,
alternating in one process after a warm-up, over the one reassembled batch:

  collect_ragged   e2sar_hip_reas_collect, pitch 0, align 256
  collect_rows     e2sar_hip_reas_collect, pitch = B rounded up to 16
  build_ragged     e2sar_hip_reas_build, no id list, pitch 0, align 256
  build_cells      e2sar_hip_reas_build, the S ids, pitch = B rounded up to 16
  *_plan           the same four calls with outBytes = 0: the plan launch alone

The copy half of a form is its median minus its plan's median; build's is set against
collect's: ragged with ragged, cells with rows.  Every full form's output is compared with
the events' source bytes once.

Workload 2: 4096 events of 64 bytes (1024 eventNums x 4 dataIds); the plan-only and the full
ragged calls of both functions over windows of 1024 and 4096 records, to show how the
one-workgroup plans grow with the window.

  python tools/build_bench.py [--event-nums 41] [--sources 5] [--event-bytes 1048576]
                              [--mtu 1500] [--reps 40] [--warmup 5] [--out FILE]
Prints one JSON line (and writes it to --out).
"""
import ctypes as C
import os

import numpy as np

import ab_method


def main():
    ap = ab_method.parser(events=None)          # the events are event numbers x sources here
    ap.add_argument("--event-nums", type=int, default=41)
    ap.add_argument("--sources", type=int, default=5)
    args = ap.parse_args()

    import torch
    from e2sar_amd import sar, _capi

    ab_method.need_gpu("build_bench")
    dev = torch.device("cuda:0")
    ctx = sar.Context(0)
    seg = sar.DeviceSegmenter(ctx, mtu=args.mtu, lb_hdr_version=2)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    vp = C.c_void_p

    def stream():
        return vp(int(torch.cuda.current_stream().cuda_stream))

    def batch(n_nums, n_src, nbytes):
        """n_nums x n_src events of nbytes, segmented and reassembled: -> (R, src rows, event count)."""
        n_ev = n_nums * n_src
        ev_stride = (nbytes + 255) // 256 * 256
        src = torch.randint(0, 256, (n_ev, ev_stride), dtype=torch.uint8, device=dev, generator=g)
        # event i: eventNum i // n_src, dataId 100 + i % n_src, sent in an order that is not the built one
        order = np.random.default_rng(5).permutation(n_ev)
        plan = seg.plan([(src[i].data_ptr(), nbytes, 1000 + i // n_src, 100 + i % n_src, 1 + i, (1 << 48) + i)
                         for i in order])
        pk, ln = seg.alloc_packets(plan.total_packets)
        seg.segment(plan, pk, ln)
        table = 1
        while table < 8 * n_ev:
            table <<= 1
        R = sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=table, queue_capacity=max(n_ev, 64),
                                  lost_capacity=64, arena_bytes=n_ev * ev_stride + 4096)
        R.reassemble(pk, seg.stride, ln, plan.total_packets)
        torch.cuda.synchronize()
        return R, src, n_ev

    def measure(forms):
        return ab_method.summary(ab_method.measure(forms, args))

    def calls(R, out, n_max, ids, pitch):
        """The collect and build calls over R's records as closures of (out_bytes) -> callable."""
        index = torch.zeros(n_max * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
        members = torch.zeros(n_max * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
        groups = torch.zeros(n_max * sar.BUILT_REC_BYTES, dtype=torch.uint8, device=dev)
        c4 = torch.zeros(4, dtype=torch.int64, device=dev)
        c8 = torch.zeros(8, dtype=torch.int64, device=dev)
        work = R.alloc_build_work(n_max)
        arr = (C.c_uint16 * max(1, len(ids)))(*ids)
        L = _capi.lib()

        def collect(window, out_bytes, p):
            return lambda: _capi.check(L.e2sar_hip_reas_collect(R.handle, 0, window, vp(out.data_ptr()), out_bytes, p, 256,
                                                                vp(index.data_ptr()), vp(c4.data_ptr()), stream()))

        def build(window, out_bytes, p):
            return lambda: _capi.check(L.e2sar_hip_reas_build(
                R.handle, 0, window, arr if p else None, len(ids) if p else 0, vp(out.data_ptr()), out_bytes, p, 256,
                vp(members.data_ptr()), vp(groups.data_ptr()), n_max, vp(c8.data_ptr()), vp(work.data_ptr()),
                work.numel(), stream()))

        return collect, build, (index, c4, members, groups, c8)

    result = {"tool": "build_bench", "mtu": args.mtu, "reps": args.reps, "warmup": args.warmup,
              "lib": os.path.basename(_capi.LIB_PATH), "device": torch.cuda.get_device_name(0)}

    # ---- workload 1: the flagship batch as event numbers x sources ----
    S, B = args.sources, args.event_bytes
    R, src, E = batch(args.event_nums, S, B)
    ids = [100 + j for j in range(S)]
    pitch = (B + 15) // 16 * 16
    ev_stride = (B + 255) // 256 * 256
    room = E * max(ev_stride, pitch)
    out = torch.zeros(room, dtype=torch.uint8, device=dev)
    collect, build, (index, c4, members, groups, c8) = calls(R, out, E, ids, pitch)
    forms = {
        "collect_ragged": collect(E, room, 0), "collect_rows": collect(E, room, pitch),
        "build_ragged": build(E, room, 0), "build_cells": build(E, room, pitch),
        "collect_ragged_plan": collect(E, 0, 0), "collect_rows_plan": collect(E, 0, pitch),
        "build_ragged_plan": build(E, 0, 0), "build_cells_plan": build(E, 0, pitch),
    }
    # every full form delivers every event's bytes, build in (eventNum, dataId) order
    host = src[:, :B].cpu().numpy()
    for name in ("collect_ragged", "collect_rows", "build_ragged", "build_cells"):
        out.zero_()
        forms[name]()
        torch.cuda.synchronize()
        if name.startswith("collect"):
            rows = sar.parse_collect(index, c4)
        else:
            rows, grp = sar.parse_build(members, groups, c8)
            assert len(grp) == args.event_nums and all(int(x) == S for x in grp["nMembers"]), name
            keys = [(int(r["eventNum"]), int(r["dataId"])) for r in rows]
            assert keys == sorted(keys), name
        assert len(rows) == E, (name, len(rows))
        got = out.cpu().numpy()
        for r in rows:
            i = (int(r["eventNum"]) - 1000) * S + int(r["dataId"]) - 100
            o = int(r["outOffset"])
            assert np.array_equal(got[o:o + B], host[i]), (name, i)
    t = measure(forms)
    halves = {}
    for name in ("collect_ragged", "collect_rows", "build_ragged", "build_cells"):
        halves[name] = round(t[name]["median_us"] - t[name + "_plan"]["median_us"], 2)
    result["batch"] = {
        "events": E, "event_nums": args.event_nums, "sources": S, "event_bytes": B, "forms": t,
        "copy_half_us": halves,
        "copy_half_build_over_collect": {"ragged": round(halves["build_ragged"] / halves["collect_ragged"], 4),
                                         "cells_over_rows": round(halves["build_cells"] / halves["collect_rows"], 4)},
        "TBps_copy_half": {k: round(2 * E * B / v / 1e6, 3) for k, v in halves.items()},
    }
    R.close()
    del out, src

    # ---- workload 2: how the plans grow with the window ----
    R, src, E = batch(1024, 4, 64)
    room = E * 256
    out = torch.zeros(room, dtype=torch.uint8, device=dev)
    collect, build, _keep = calls(R, out, E, [100, 101, 102, 103], 64)
    result["windows"] = {}
    for window in (1024, 4096):
        result["windows"][str(window)] = measure({
            "collect_ragged": collect(window, room, 0), "build_ragged": build(window, room, 0),
            "collect_ragged_plan": collect(window, 0, 0), "build_ragged_plan": build(window, 0, 0),
            "build_cells_plan": build(window, 0, 64),
        })
    R.close()

    ab_method.write_line(result, args.out)


if __name__ == "__main__":
    main()
