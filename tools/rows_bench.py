#!/usr/bin/env python3
"""Reassembly straight into a tensor against reassembly plus delivery.

E events of B bytes are segmented on the device; then three ways of getting them out of the
datagrams are timed with HIP events, alternating in one process after a warm-up
(tools/ab_method.py), for a batch at each MTU of --mtus:

  rows               e2sar_hip_rows_clear outside the clock, then one e2sar_hip_rows_reassemble
                     into an [nEvents, 1, pitch] window, pitch = B rounded up to 256
  reas+collect_rows  forced recycle outside the clock, then e2sar_hip_reassemble_batch and
                     e2sar_hip_reas_collect in row mode at the same pitch: the same tensor, by
                     way of the arena
  reas               forced recycle outside the clock, then e2sar_hip_reassemble_batch alone

With --step W[,W...] the window of rank 0 of W (eventStep W, eventPhase 0) is
timed beside `rows` instead of the two arena forms, one form per W:

  --landing own      rows_stepW: the batch holds only this rank's events, the same bytes numbered
                     base + k W; the window takes all of them
  --landing spread   rows_spreadW: the batch is the one `rows` takes, all W ranks' events numbered
                     consecutively; the window takes every W-th event and passes the rest over.
                     Reported with the time of `rows` and that time divided by W beside it.

With --seen [pair|dup16|all] a window that survives duplicates (frag_bytes = the segmenter's payload
per datagram) is timed beside the plain one instead of the two arena forms -- pair
(the default): rows and rows_seen; dup16: rows_dup16 and rows_seen_dup16; all: the four in one
process, where a form's time follows its place among them:

  rows_seen          e2sar_hip_rows_clear_seen outside the clock, then one
                     e2sar_hip_rows_reassemble_seen of the batch `rows` takes
  rows_dup16,        the same two calls on that batch with every 16th datagram sent twice, the copy
  rows_seen_dup16    straight behind the original; the plain window's result is then not the events
                     (its curBytes pass the events' lengths), only its time is used

Every form's output is compared with the events' source bytes once.

  python tools/rows_bench.py [--events 205] [--event-bytes 1048576] [--mtus 1500,9000]
                             [--step W[,W...]] [--landing own|spread] [--seen [MODE]]
                             [--reps 40] [--warmup 5] [--out FILE]
Prints one JSON line (and writes it to --out).  Rates count payload bytes read + written once.
"""
import os

import numpy as np

import ab_method


def batch(ctx, args, mtu, src, torch, sar):
    dev = ctx.torch_device
    E, B = args.events, args.event_bytes
    base = 1 << 48
    seg = sar.DeviceSegmenter(ctx, mtu=mtu, lb_hdr_version=2)
    plan = seg.plan([(src[i].data_ptr(), B, base + i, 4321, 1 + i, base + i) for i in range(E)])
    n = plan.total_packets
    pk, ln = seg.alloc_packets(n)
    seg.segment(plan, pk, ln)
    n_events = 1
    while n_events < E:
        n_events <<= 1
    pitch = (B + 255) // 256 * 256
    win = sar.RowWindow(ctx, [4321], n_events, pitch, base, with_lb_header=True)
    table = 1
    while table < 8 * E:
        table <<= 1
    R = sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=table, queue_capacity=E + 64, lost_capacity=64,
                              arena_bytes=E * pitch + 4096)
    rows = torch.zeros(E * pitch, dtype=torch.uint8, device=dev)
    index = torch.zeros(E * sar.COLLECT_REC_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)

    def reas_collect():
        R.reassemble(pk, seg.stride, ln, n)
        R.collect(rows, index, counts, 0, E, pitch)

    def recycle():
        R.recycle(force=True)

    forms = {
        "rows": (lambda: win.reassemble(pk, seg.stride, ln, n), lambda: win.clear(base)),
        "reas+collect_rows": (reas_collect, recycle),
        "reas": (lambda: R.reassemble(pk, seg.stride, ln, n), recycle),
    }

    # every form's output against the source events
    host = src[:, :B].cpu().numpy()
    win.out.zero_()
    win.clear(base)
    forms["rows"][0]()
    cells = win.parse_cells()[:, 0]
    c, _ = win.parse_counts()
    assert c[0] == E and c[1] == n and c[2] == E * B and not any(c[3:]), c
    got = win.out[:, 0, :B].cpu().numpy()
    for i in range(E):
        r = (base + i) & (n_events - 1)
        assert cells[r]["flags"] == 1 and cells[r]["bytes"] == B, (i, cells[r])
        assert np.array_equal(got[r], host[i]), ("rows", i)
    rows.zero_()
    recycle()
    reas_collect()
    recs = sar.parse_collect(index, counts)
    assert len(recs) == E, len(recs)
    got = rows.view(E, pitch)[:, :B].cpu().numpy()
    for k, r in enumerate(recs):
        assert np.array_equal(got[k], host[int(r["eventNum"]) - base]), ("reas+collect_rows", k)
    recycle()
    forms["reas"][0]()
    done = R.poll()
    assert len(done) == E, len(done)
    arena = R.arena_tensor()
    for r in done[:: max(1, E // 8)]:
        ev = arena[r.arenaOffset: r.arenaOffset + B].cpu().numpy()
        assert r.bytes == B and np.array_equal(ev, host[r.eventNum - base]), ("reas", r.eventNum)

    moved = {name: 2 * E * B for name in forms}
    moved["reas+collect_rows"] = 4 * E * B
    if args.step:
        forms = {"rows": forms["rows"]}
        for W in args.step:
            name, form, owned = lattice(ctx, args, W, seg, src, host, (pk, ln, n), base, pitch, sar)
            forms[name] = form
            moved[name] = 2 * owned * B
    if args.seen:
        more, n_dup = seen_forms(ctx, args, seg, host, (pk, ln, n), base, pitch, n_events, win, torch, sar)
        more["rows"] = forms["rows"]
        forms = {name: more[name] for name in SEEN_FORMS[args.seen]}
        moved.update({name: 2 * E * B for name in forms})
    us = ab_method.measure(forms, args)
    out = ab_method.summary(us, moved)
    out["datagrams"] = n
    if args.seen:
        out["datagrams_dup16"] = n_dup
        for name, against in (("rows_seen", "rows"), ("rows_seen_dup16", "rows_dup16")):
            if name not in out:
                continue
            out[name]["of_plain_median"] = round(out[name]["median_us"] / out[against]["median_us"], 3)
    if args.step and args.landing == "spread":
        for W in args.step:
            out[f"rows_spread{W}"]["rows_median_over_W_us"] = round(out["rows"]["median_us"] / W, 2)
            out[f"rows_spread{W}"]["of_rows_median"] = round(out[f"rows_spread{W}"]["median_us"] / out["rows"]["median_us"], 3)
    R.close()
    return out


# --seen MODE: the forms of one process.  Two forms on one batch follow each other alike; with all four in one
# process a form's time follows its place among them -- whose batch went through the caches before it
SEEN_FORMS = {"pair": ("rows", "rows_seen"), "dup16": ("rows_dup16", "rows_seen_dup16"),
              "all": ("rows", "rows_seen", "rows_dup16", "rows_seen_dup16")}


def seen_forms(ctx, args, seg, host, whole, base, pitch, n_events, plain, torch, sar):
    """The window with bits beside `plain`, and both on the batch with every 16th datagram twice:
    -> ({form name: (fn, before)}, the datagrams of that batch)."""
    E, B = args.events, args.event_bytes
    pk, ln, n = whole
    win = sar.RowWindow(ctx, [4321], n_events, pitch, base, with_lb_header=True, frag_bytes=seg.max_pld)
    idx = torch.tensor([k for i in range(n) for k in ((i, i) if i % 16 == 0 else (i,))], dtype=torch.int64, device=pk.device)
    n2 = idx.numel()
    pk2 = pk.view(-1, seg.stride)[:n].index_select(0, idx).reshape(-1).contiguous()
    ln2 = ln[:n].index_select(0, idx).contiguous()
    forms = {
        "rows_seen": (lambda: win.reassemble(pk, seg.stride, ln, n), lambda: win.clear(base)),
        "rows_dup16": (lambda: plain.reassemble(pk2, seg.stride, ln2, n2), lambda: plain.clear(base)),
        "rows_seen_dup16": (lambda: win.reassemble(pk2, seg.stride, ln2, n2), lambda: win.clear(base)),
    }
    for name, dup in (("rows_seen", 0), ("rows_seen_dup16", n2 - n)):
        win.out.zero_()
        win.clear(base)
        forms[name][0]()
        cells = win.parse_cells()[:, 0]
        c, _ = win.parse_counts()
        assert c[0] == E and c[1] == n and c[2] == E * B and c[11] == dup and not any(c[3:11]), (name, c)
        got = win.out[:, 0, :B].cpu().numpy()
        for i in range(E):
            r = (base + i) & (n_events - 1)
            assert cells[r]["flags"] == 1 and cells[r]["bytes"] == B, (name, i, cells[r])
            assert np.array_equal(got[r], host[i]), (name, i)
        assert int(np.unpackbits(win.parse_seen().view(np.uint8)).sum()) == n, name
    return forms, n2


def lattice(ctx, args, W, seg, src, host, whole, base, pitch, sar):
    """The window of rank 0 of W and the batch it is fed: -> (form name, (fn, before), owned events)."""
    E, B = args.events, args.event_bytes
    first = sar.RowWindow.first_owned(base, W, 0)
    if args.landing == "own":                                      # the same bytes, numbered first + k W
        nums = [first + i * W for i in range(E)]
        plan = seg.plan([(src[i].data_ptr(), B, nums[i], 4321, 1 + i, nums[i]) for i in range(E)])
        n = plan.total_packets
        pk, ln = seg.alloc_packets(n)
        seg.segment(plan, pk, ln)
        owned = list(range(E))
    else:                                                          # the whole batch: events base + i of every rank
        pk, ln, n = whole
        nums = [base + i for i in range(E)]
        owned = [i for i in range(E) if nums[i] % W == 0]
    n_events = 1
    while n_events < len(owned):
        n_events <<= 1
    win = sar.RowWindow(ctx, [4321], n_events, pitch, first, with_lb_header=True, step=W, phase=0)
    form = (lambda: win.reassemble(pk, seg.stride, ln, n), lambda: win.clear(first))

    win.out.zero_()
    form[0]()
    c, b = win.parse_counts()
    cells = win.parse_cells()[:, 0]
    assert b == first and c[0] == len(owned) and c[2] == len(owned) * B and c[1] + c[10] == n and not any(c[3:10]), c
    got = win.out[:, 0, :B].cpu().numpy()
    for i in owned:
        r = (nums[i] // W) & (n_events - 1)
        assert cells[r]["flags"] == 1 and cells[r]["bytes"] == B, (W, i, cells[r])
        assert np.array_equal(got[r], host[i]), (f"step {W}", i)
    return ("rows_step%d" if args.landing == "own" else "rows_spread%d") % W, form, len(owned)


def main():
    ap = ab_method.parser()
    ap.add_argument("--mtus", default="1500,9000")
    ap.add_argument("--step", default="", help="W[,W...]: time the window of rank 0 of W beside `rows`")
    ap.add_argument("--landing", choices=["own", "spread"], default="own")
    ap.add_argument("--seen", nargs="?", const="pair", default=None, choices=sorted(SEEN_FORMS),
                    help="time the window that survives duplicates beside `rows`: pair (default), dup16 or all")
    args = ap.parse_args()
    args.step = [int(w) for w in args.step.split(",") if w]
    if any(w < 2 for w in args.step):
        ap.error("--step takes values of at least 2")
    if args.seen and args.step:
        ap.error("--seen and --step are separate runs")

    import torch
    from e2sar_amd import sar, _capi

    ab_method.need_gpu("rows_bench")
    dev = torch.device("cuda:0")
    ctx = sar.Context(0)
    E, B = args.events, args.event_bytes
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    src = torch.randint(0, 256, (E, (B + 255) // 256 * 256), dtype=torch.uint8, device=dev, generator=g)
    result = {"tool": "rows_bench", "events": E, "event_bytes": B, "reps": args.reps,
              "step": args.step, "landing": args.landing if args.step else None, "seen": args.seen,
              "lib": os.path.basename(_capi.LIB_PATH), "device": torch.cuda.get_device_name(0), "mtu": {}}
    for mtu in (int(m) for m in args.mtus.split(",")):
        result["mtu"][str(mtu)] = batch(ctx, args, mtu, src, torch, sar)
    ab_method.write_line(result, args.out)


if __name__ == "__main__":
    main()
