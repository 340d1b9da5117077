"""The A/B method of DESIGN.md 4.8, once, for collect_bench, emit_bench, build_bench and reas_dev_bench.

Forms are timed with HIP events, alternating in one process after a warm-up, while the device
spins so that the host side of a call is not in its time; each form is summarised by its
median, minimum and 90th percentile, and the result leaves as one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPIN = 300_000                                  # clocks; covers the host side of a call


def parser(events=205):
    """The arguments every tool takes; events=None for a tool that counts its events otherwise."""
    ap = argparse.ArgumentParser()
    if events is not None:
        ap.add_argument("--events", type=int, default=events)
    ap.add_argument("--event-bytes", type=int, default=1 << 20)
    ap.add_argument("--mtu", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    return ap


def need_gpu(tool):
    import torch
    if not torch.cuda.is_available():
        sys.exit(f"{tool} needs a GPU: nothing is measured without one")


def timed(fn, before=None):
    """-> microseconds of fn's launches; `before` is enqueued in front of the clock, inside the spin."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(SPIN)                     # the host enqueues the timed calls while the device spins
    if before:
        before()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def measure(forms, args, prepare=None):
    """forms: name -> fn or (fn, before).  -> name -> the times of args.reps alternating rounds
    after args.warmup; `prepare` runs untimed, and ahead of the spin, before every call."""
    us = {name: [] for name in forms}
    for rep in range(args.warmup + args.reps):
        for name, form in forms.items():
            fn, before = form if isinstance(form, tuple) else (form, None)
            if prepare:
                prepare()
            t_us = timed(fn, before)
            if rep >= args.warmup:
                us[name].append(t_us)
    return us


def summary(us, moved=None):
    """-> name -> median / min / p90; with moved (name -> bytes, 0 for a name it lacks) also TB/s at the median."""
    out = {}
    for name, v in us.items():
        out[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                     "p90_us": round(sorted(v)[int(0.9 * (len(v) - 1))], 2)}
        if moved is not None:
            out[name]["TBps_median"] = round(moved.get(name, 0) / statistics.median(v) / 1e6, 3)
    return out


def write_line(result, out):
    line = json.dumps(result)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
