"""bench.py's output contract: one JSON line with the driver's keys plus `roofline` and
`cpu_baseline` (run as a child process so that it owns its own GPU context)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_contract_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--pairs", "16",
                          "--cpu-pairs", "1", "--warmup-seconds", "0.2", "--repeats", "4"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "frames/s"
    assert j["higher_is_better"] is True and j["scaling"] == "weak" and j["vs_baseline"] is None
    assert j["dtype"] == "f32" and j["data"] == "synthetic" and "workload" in j["config"] and "model" not in j["config"]
    assert j["value"] > 1000 and abs(j["value"] - 16 * 3 / (j["ms_per_step"] * 3e-3)) / j["value"] < 0.01
    r = j["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["avg_us"] > 0
    # a roofline fraction is physical: compulsory bytes of the launch as built / time / 8 TB/s
    assert 0.0 < r["frac"] < 1.0 and r["peak_measured"]["read"] > 1000
    assert abs(r["achieved"] - r["alg_bytes_per_launch"] / (r["avg_us"] * 1e-6) / 1e9) / r["achieved"] < 0.01
    assert "traffic_source" in r and (r["traffic"] is None or r["traffic_source"])
    # the issue-rate evidence next to the byte roofline: present only for the launch shape the counters were taken on
    # (32 pairs per launch), then with a duration-derived figure of this run
    if "valu_issue" in r:
        assert r["valu_issue"]["vector_insts_per_launch"] > 0 and r["valu_issue"]["ns_per_inst_per_simd_this_run"] > 0
    assert 0.0 < j["pipeline"]["frac"] < 1.0 and all(0.0 < k["frac"] < 1.0 for k in j["kernels"])
    assert j["warmup_steps_run"] >= 1
    # the headline is the median of `repeats` timed windows of exactly `steps` steps each
    assert j["repeats"] == 4 and j["value_min"] <= j["value"] <= j["value_max"] and j["timed_seconds_total"] > 0
    # device evidence: one rank, one device, with something that identifies it
    assert j["ranks"] == 1 and j["distinct_devices"] == 1 and len(j["devices"]) == 1
    assert j["devices"][0]["rank"] == 0 and ("uuid" in j["devices"][0] or "pci" in j["devices"][0])
    c = j["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0


@pytest.mark.parametrize("config, pairs, runs", [("c2", 5, 2), ("c1", 4, 1)])
def test_bench_dump_outputs(tmp_path, config, pairs, runs):
    """--dump-outputs DIR leaves what the last timed step computed as DIR/<name>.npy: float32 / float64 only, under 64 MB,
    the same from run to run, and equal to the library's own answer for that step computed here -- the step's flow fields
    (the seeded pixel sample of them when the batch is beyond 48 MB: 5 fields of 1080p; the whole batch at 640x480) and
    the histogram counters and thresholds of those fields."""
    import numpy as np
    import bench
    from ripcurrents_amd import synth
    from ripcurrents_amd.api import Context

    def run(d):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--steps", "3", "--warmup", "1",
                              "--pairs", str(pairs), "--warmup-seconds", "0.2", "--repeats", "2", "--no-roof", "--no-cpu-baseline",
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        j = json.loads(lines[0])
        got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
        assert sorted(got) == ["flow", "hist_words", "prop_above_upper", "upper", "upper2d"]
        assert j["dumped_outputs"]["arrays"] == {k: list(a.shape) for k, a in got.items()}
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
        return j, got

    j, got = run(tmp_path / "a")
    for r in range(1, runs):
        _, again = run(tmp_path / ("b%d" % r))
        assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got)
    # the step the dump is of: the clip forwards on even steps, backwards on odd ones (warm-up steps included)
    w, h = (640, 480) if config == "c1" else (1920, 1080)
    clip = (synth.translating_clip if config == "c1" else synth.surf_clip)(w, h, pairs + 1, seed=1234, device="cuda")
    last = j["warmup_steps_run"] + j["repeats"] * j["steps"] - 1
    with Context(w, h) as c:
        want = c.farneback_clip(clip if last % 2 == 0 else clip.flip(0).contiguous(), **bench.PARAMS)
        c.analysis_reset(w, h)
        c.histogram_accumulate_clip(want)
        c.thresholds()
        st = c.histogram_read()
        words = c.histogram_words().cpu().numpy()
    want = want.cpu().numpy()
    if want.nbytes > bench.DUMP_FLOW_BYTES:
        want = want.reshape(-1, 2)[bench.dump_sample_index(pairs * h * w, bench.DUMP_FLOW_BYTES // 8)]
    assert got["flow"].dtype == np.float32 and np.array_equal(got["flow"], want)
    assert words.any() and np.array_equal(got["hist_words"], words)
    assert got["upper"][0] == np.float32(st.UPPER) and np.array_equal(got["upper2d"], st.UPPER2d)
    assert np.array_equal(got["prop_above_upper"], st.prop_above_upper, equal_nan=True)


@pytest.mark.parametrize("how", ["launcher", "plain"])
def test_bench_two_ranks_rehearsal(how):
    """The N>1 path of bench.py end to end on the one GPU of the test box, both ways the driver may start it: under
    torch.distributed.run, and as a plain `python bench.py --gpus 2` (no WORLD_SIZE: the script then starts the launcher
    itself, as a child, before it touches the GPU).  Both ranks on cuda:0 with gloo as the transport (RC_REHEARSE_GLOO=1;
    RCCL refuses two ranks on one device).  Segments per rank, the asynchronous histogram all-reduce consumed one step
    later, max-over-ranks timing, one JSON line from rank 0 that names every rank's device."""
    env = dict(os.environ, RC_REHEARSE_GLOO="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    port = 29600 + os.getpid() % 300
    args = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--pairs", "4", "--no-roof",
            "--warmup-seconds", "0.2", "--repeats", "3"]
    if how == "launcher":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port)] + args
    else:
        cmd = [sys.executable] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["scaling"] == "weak" and j["config"]["segments"] == 2
    assert "all_reduce int32[1887]" in j["config"]["collective"]
    assert abs(j["value"] - 2 * 4 * 3 / (j["ms_per_step"] * 3e-3)) / j["value"] < 0.01
    assert "cpu_baseline" not in j          # rank 0 at N = 1 only
    assert j["ranks"] == 2 and sorted(d["rank"] for d in j["devices"]) == [0, 1]
    assert j["distinct_devices"] == 1       # the rehearsal puts both ranks on the box's one GPU; a real run reports N


@pytest.mark.parametrize("collective", ["torch", "rccl"])
def test_bench_rccl_backend_rehearsal_with_one_rank(collective):
    """The N>1 code path of bench.py over the REAL backend, as far as one GPU allows: one rank under
    torch.distributed.run with RC_FORCE_DIST=1 initialises the `nccl` (= RCCL) process group and runs every collective of
    the multi-rank run -- the asynchronous int32[1887] histogram all-reduce consumed one step later (torch.distributed, or
    the library's own rcflow_allreduce_hist over a one-rank RCCL communicator whose id travels by broadcast), the
    warm-up broadcast, the barriers and the max-over-ranks reduction of the timing."""
    env = dict(os.environ, RC_FORCE_DIST="1")
    port = 29900 + os.getpid() % 90 + (0 if collective == "torch" else 1)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--pairs", "8", "--no-roof", "--no-cpu-baseline", "--warmup-seconds", "0.2", "--collective", collective]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 1 and j["value"] > 1000
    assert ("librccl" if collective == "rccl" else "torch.distributed") in j["config"]["collective"]
