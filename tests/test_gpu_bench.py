"""bench.py's workload on the GPU at a small size: a plain run times the steps and nothing
else, --dump-outputs writes what the last timed step computed (checked against the source
events and the oracle's datagrams), the same arguments give the same files, and --full adds
the verification, the roofline pass and the cold leg without changing the outputs."""
import numpy as np
import pytest

import bench
import oracle_ffi as O

pytestmark = pytest.mark.gpu

E, B, BATCH, STEPS = 7, 100_000, 3, 4
SMALL = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--events", str(E), "--event-bytes", str(B),
         "--batch-events", str(BATCH), "--quiet"]


def _run(hip, argv, headline=False):
    import torch
    import torch.distributed as dist

    from e2sar_amd import sar

    dev = hip.torch_device
    env = bench.Env(torch=torch, dist=dist, sar=sar, ctx=hip, dev=dev, world=1, rank=0, backend="nccl", coll_dev=dev)
    return bench.run_workload(bench.parse(argv), env, headline=headline)


def _load(res):
    return {n: np.load(f"{res['dir']}/{n}.npy") for n in res["files"]}


@pytest.fixture(scope="module")
def plain(hip, tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    line = _run(hip, SMALL + ["--dump-outputs", str(d)])
    return line, _load(line["outputs"])


def test_plain_run_times_the_steps_and_nothing_else(plain):
    line, _ = plain
    assert line["steps"] == STEPS and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: payload of the timed steps / their time
    # (ms_per_step is rounded to 1e-4 ms: half a percent of a step of 0.01 ms, and a step is longer)
    assert line["value"] == pytest.approx(E * B / (line["ms_per_step"] * 1e-3) / 2**30, rel=1e-2)
    assert line["config"]["verified_roundtrip"] is None and line["config"]["verified_at"] is None
    assert line["reas_cold"] is None and "kernel" not in line["roofline"] and "cpu_baseline" not in line
    assert f"hipGraph of {STEPS} step(s), replayed 1 times" == line["config"]["launch"]


@pytest.fixture(scope="module")
def src(hip):
    """bench.py's inputs: rank 0's events from its seed."""
    import torch

    g = torch.Generator(device=hip.torch_device)
    g.manual_seed(0xE25A2)
    stride = (B + 255) // 256 * 256
    s = torch.randint(0, 256, (E, stride), dtype=torch.uint8, device=hip.torch_device, generator=g)
    return s.cpu().numpy()[:, :B].copy()


def test_dumped_events_are_the_source_events(plain, src):
    line, got = plain
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert line["outputs"]["bytes"] == sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT
    npk = O.num_packets(B, O.max_pld_len(1500))
    assert got["records"].tolist() == [[i, B, 4321, npk] for i in range(E)]
    w = np.arange(B, dtype=np.int64) % 65521 + 1
    assert got["event_sums"].tolist() == [[int(e.sum()), int((e.astype(np.int64) * w).sum())] for e in src]
    pos = got["events_sample_pos"].astype(np.int64)
    assert pos[0] == 0 and pos[-1] == B - 1
    assert np.array_equal(got["events_sample"], src[:, pos].astype(np.float32))
    assert np.array_equal(got["events_head"], src[got["events_head_idx"].astype(np.int64)].astype(np.float32))


def test_dumped_datagrams_are_the_oracles(plain, src):
    _, got = plain
    # the step's last batch is event 6 alone (batches of 3): its datagrams as the oracle cuts them
    stride = got["datagrams_sample"].shape[1]
    op, ol = O.segment_event(src[6], 6, 4321, 1 + (6 * 0x9E37) % 65535, (1 << 48) + 6, 2, O.max_pld_len(1500), stride)
    assert got["datagram_lengths"].tolist() == [int(x) for x in ol]
    which = got["datagrams_sample_idx"].astype(np.int64)
    want = op[which] * (np.arange(stride)[None, :] < ol[which][:, None])
    assert np.array_equal(got["datagrams_sample"], want.astype(np.float32))


def test_same_arguments_same_outputs(hip, plain, tmp_path):
    _, got = plain
    again = _load(_run(hip, SMALL + ["--dump-outputs", str(tmp_path)])["outputs"])
    assert sorted(again) == sorted(got)
    assert all(np.array_equal(got[n], again[n]) for n in got)


def test_full_adds_its_legs_and_leaves_the_outputs_alone(hip, plain, tmp_path):
    _, got = plain
    line = _run(hip, SMALL + ["--full", "--cold-steps", "2", "--roofline-steps", "1", "--dump-outputs", str(tmp_path)])
    assert line["full"] is True and line["steps"] == STEPS and line["ms_per_step"] > 0
    assert line["config"]["verified_roundtrip"] is True and len(line["config"]["verified_at"]) == 3
    assert line["roofline"]["kernel"] in line["roofline"]["avg_launch_ms"] and line["roofline"]["achieved"] > 0
    assert line["reas_cold"]["verified"] is True and line["reas_cold"]["value"] > 0
    full = _load(line["outputs"])
    assert all(np.array_equal(got[n], full[n]) for n in got)
