"""bench.py's contract with the driver: one JSON line with the fields the task statement names (GPU tier), and a
loud refusal -- not a CPU fallback -- when there is no GPU (CPU tier)."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="this machine has a GPU")
def test_bench_and_smoke_refuse_to_run_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode != 0 and "needs a GPU" in (r.stderr + r.stdout)
    assert "metric" not in r.stdout                                   # no line, no number
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode != 0 and "__SMOKE_OK__" not in r.stdout


GUARD_SCRIPT = r"""
import argparse, json, sys, time
sys.path.insert(0, %r)
import bench
mode = sys.argv[1]
def leg(args, rank, world, dist, torch, stage, flat=None):
    flat["gather_backend"] = "nccl"                  # a stage that finished before the trouble
    stage[0] = "broad sweep, resident regime"
    if mode == "raise":
        raise SystemExit("bench broad: the gathered tiles of rank(s) [1] differ")
    if mode == "hang":
        time.sleep(60)
    flat["rccl_world"] = 1
    return flat, {}
bench.multi_gpu_leg = leg
args = argparse.Namespace(multi_gpu_timeout=1.0)
line = {"metric": "fft_frames_per_sec_n8192", "value": 123.0}
flat, lines = bench.guarded_multi_gpu_leg(args, 0, 1, None, None, line)
line["extra"] = flat
bench.emit_line(line, 0)
bench.emit_line(line, 0)          # a second call prints nothing
"""


@pytest.mark.parametrize("mode", ["ok", "raise", "hang"])
def test_the_multi_gpu_leg_can_fail_or_hang_without_costing_the_line(mode):
    """`value` is measured before the multi-GPU leg and nothing in the leg may cost the driver its line: an exception lands in
    extra.multi_gpu_error, a hang ends at the watchdog, which prints the line as it stands -- one line, exit code 0."""
    r = subprocess.run([sys.executable, "-c", GUARD_SCRIPT % ROOT, mode], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["value"] == 123.0
    err = d["extra"]["multi_gpu_error"]
    assert d["extra"]["gather_backend"] == "nccl"     # what the leg had finished is in the line either way
    if mode == "ok":
        assert err is None and d["extra"]["rccl_world"] == 1
    elif mode == "raise":
        assert "stage broad sweep, resident regime" in err and "differ" in err
    else:
        assert "did not finish within 1 s" in err and "broad sweep, resident regime" in err


GUARDIAN_TEST = r"""
import os, signal, sys
sys.path.insert(0, %r)
import bench
mode = sys.argv[1]
line = {"metric": "fft_frames_per_sec_n8192", "value": 123.0}
bench.start_guardian(line, 0)
assert bench._GUARDIAN[0] is not None
if mode == "killed":
    os.kill(os.getpid(), signal.SIGKILL)           # what an RCCL watchdog's abort() or the launcher's SIGKILL looks like
if mode == "aborted":
    os.abort()
line["extra"] = {"multi_gpu_error": None, "rccl_world": 8}
bench.emit_line(line, 0)
bench.emit_line(line, 0)
"""


@pytest.mark.parametrize("mode", ["ok", "killed", "aborted"])
def test_a_hard_failure_behind_the_headline_still_leaves_the_line(mode):
    """SIGKILL / abort() inside the multi-GPU leg cannot be caught by Python; the guardian child (the one
    printer) prints the provisional headline with extra.multi_gpu_error when its stdin closes without a final line."""
    r = subprocess.run([sys.executable, "-c", GUARDIAN_TEST % ROOT, mode], capture_output=True, text=True, cwd=ROOT, timeout=120)
    if mode == "ok":
        assert r.returncode == 0, r.stderr[-2000:]
    else:
        assert r.returncode != 0
    import time
    time.sleep(0.5)                                    # the guardian outlives a killed parent by a few milliseconds
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["value"] == 123.0
    if mode == "ok":
        assert d["extra"] == {"multi_gpu_error": None, "rccl_world": 8}
    else:
        assert "ended without printing its line" in d["extra"]["multi_gpu_error"]


MULTI_GPU_KEYS = ("broad_sweep_ms_resident", "broad_sweep_ms_ingest", "stft_stream_ms", "regime", "gather_chunks",
                  "gather_backend", "rccl_world", "broad_sweep_resident_gathered_checksum_ok",
                  "broad_sweep_ingest_gathered_checksum_ok", "stft_stream_gathered_checksum_ok", "gather_gbps_per_link",
                  "multi_gpu_error", "distinct_gpus", "rank_devices", "broad_sweep_resident_gathered_checksum_matches_pinned",
                  "broad_sweep_ingest_gathered_checksum_matches_pinned", "stft_stream_gathered_checksum_matches_pinned")


@pytest.mark.gpu
def test_bench_with_two_ranks_runs_the_sharded_sweep_and_stream_with_a_gather():
    """The driver's own N > 1 command line (`python -m torch.distributed.run ... bench.py --gpus 2 ...`), two ranks sharing
    this box's one GPU over gloo (RCCL refuses two ranks on one device): after the headline's steps the line must carry
    the sharded config-4 sweep in both regimes and the config-5 stream, gathered to rank 0, with the checksums of what
    arrived against what the members computed."""
    env = dict(os.environ, FSEA_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29731", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
                        "--warmup", "5", "--stream-frames", "4095", "--full"],
                       capture_output=True, text=True, cwd=ROOT, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["metric"] == "fft_frames_per_sec_n8192"
    ex = d["extra"]
    for key in MULTI_GPU_KEYS:
        assert key in ex, key
    assert ex["multi_gpu_error"] is None
    assert ex["gather_backend"] == "gloo" and ex["rccl_world"] == 2 and ex["gather_chunks"] == 8
    assert ex["broad_sweep_resident_gathered_checksum_ok"] is True and ex["broad_sweep_ingest_gathered_checksum_ok"] is True
    assert ex["stft_stream_gathered_checksum_ok"] is True
    assert ex["broad_sweep_ms_resident"] > 0 and ex["broad_sweep_ms_ingest"] > 0 and ex["stft_stream_ms"] > 0
    assert ex["gather_gbps_per_link"] > 0 and ex["gather_bytes_per_peer"] == 256 * 256 * 4096
    assert "resident" in ex["regime"]["broad_sweep_ms_resident"] and "ingest" in ex["regime"]["broad_sweep_ms_ingest"]
    assert ex["broad_sweep_resident_gathered_checksum"] == ex["broad_sweep_ingest_gathered_checksum"]
    # what arrived on rank 0 is the image tests/test_gpu_bench_jobs.py compared with the oracle (tests/golden/bench_job_checksums.json)
    assert ex["broad_sweep_resident_gathered_checksum_matches_pinned"] is True
    assert ex["broad_sweep_ingest_gathered_checksum_matches_pinned"] is True
    assert ex["stft_stream_gathered_checksum_matches_pinned"] is None      # --stream-frames 4095: no constant for that length
    _same_image_at_every_world_size(2, ex["broad_sweep_resident_gathered_checksum"])


_IMAGE_CHECKSUMS = {}


def _same_image_at_every_world_size(world, checksum):
    """The sweep's captures are seeded per centre frequency, so the stitched image -- and its checksum in the line -- must not
    depend on how many ranks made it (whichever of the two bench tests runs second compares)."""
    _IMAGE_CHECKSUMS[world] = checksum
    assert len(set(_IMAGE_CHECKSUMS.values())) == 1, _IMAGE_CHECKSUMS


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--cpu-budget", "1.0", "--full"], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["metric"] == "fft_frames_per_sec_n8192" and d["unit"] == "frames/s" and d["n_gpus"] == 1
    assert d["steps"] == 5 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    roof = d["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12 and 0.2 < roof["frac"] < 1.0
    assert roof["kernel"] == "fsea_fft8192_u8_mag"
    assert roof["traffic"] is None or 0.9 < roof["traffic"] / roof["algorithmic_bytes_per_launch"] < 1.2
    # value = frames of all ranks / HOST WALL CLOCK of the K timed steps (the bench contract); the device's own
    # time for the same steps (two HIP events on the launch stream) is reported beside it and can only be shorter, and the
    # roofline figures are priced with it (the kernel's average launch duration)
    assert abs(d["value"] - 4096 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-6
    assert d["ms_per_step_events"] <= d["ms_per_step"] * 1.02 and d["value_events"] >= d["value"] * 0.98
    assert abs(d["value_events"] - 4096 * 1e3 / d["ms_per_step_events"]) / d["value_events"] < 1e-6
    assert abs(roof["avg_launch_ms"] - d["ms_per_step_events"]) < 1e-9
    assert abs(roof["frac_by_step_time"] - roof["algorithmic_bytes_per_launch"] / (d["ms_per_step"] * 1e-3) / 1e9 / 8000.0) < 1e-9
    assert roof["frac_by_step_time"] <= roof["frac"] * 1.02
    # the clock-settle loop in front of the warm-up: bounded, at least the old fixed 0.25 s, its seconds on the line
    assert 0.25 <= d["config"]["clock_prewarm_s"] <= d["config"]["clock_prewarm_limit_s"] + 0.5 and d["config"]["clock_prewarm_limit_s"] == 2.0
    assert d["config"]["clock_prewarm_blocks_of_64_launches"] >= 4
    # `value` is the FIRST K-step region; nine identical regions behind it say how representative that sample was
    for key in ("headline_regions_ms", "headline_regions_events_ms"):
        rg = d[key]
        assert set(rg) >= {"official", "min", "median", "max"} and rg["regions_behind_official"] == 9
        assert 0 < rg["min"] <= rg["median"] <= rg["max"]
    assert abs(d["headline_regions_ms"]["official"] - d["ms_per_step"]) < 1e-9
    assert abs(d["headline_regions_events_ms"]["official"] - d["ms_per_step_events"]) < 1e-9
    assert abs(d["official_over_median"] - d["ms_per_step"] / d["headline_regions_ms"]["median"]) < 1e-9
    assert 0.6 < d["official_over_median"] < 1.6         # (5-step regions of 0.25 ms here: loose; the driver's 20-step form is recorded in profiles/)
    # the secondary ceilings SURVEY 8(d) names, in the line itself: how busy the vector pipes and the LDS are (committed PMC
    # constants under the same kernel / grid / LDS guard as `traffic`, priced with this run's launch time), and the package
    # power in the timed steps' own launch shape beside the long launches' (which limit binds where)
    if roof["traffic"] is not None:
        assert 0.3 < roof["valu_issue_frac"] < 1.0 and 0.05 < roof["lds_active_frac"] < 1.0
    if roof.get("package_power_w_in_bench_shape") is not None:
        assert 300 < roof["package_power_w_in_bench_shape"] <= roof["package_power_w_long_launches"] * 1.05 < 1600
        assert roof["frac"] * 0.95 < roof["frac_long_launches"] < roof["io_skeleton_frac"] * 1.05 if "io_skeleton_frac" in roof else True
    # the ceilings measured in the same run: the kernel cannot beat its own I/O skeleton, nor that a plain stream
    if "io_skeleton_frac" in roof:
        assert roof["frac"] < roof["io_skeleton_frac"] * 1.05 < roof["copy_frac"] * 1.3 and roof["copy_frac"] < 1.0
        assert 0.5 < roof["kernel_over_io_skeleton"] < 1.0 and 0.5 < roof["kernel_over_copy"] < 1.0
    ex = d["extra"]
    assert ex["host_path_frames_per_sec_n8192"] > 0
    # the multi-GPU leg's keys at N = 1: the first point of the driver's scaling curve
    for key in MULTI_GPU_KEYS:
        assert key in ex, key
    assert ex["multi_gpu_error"] is None and ex["rccl_world"] == 1 and ex["gather_gbps_per_link"] is None
    assert ex["broad_sweep_resident_gathered_checksum_ok"] is True and ex["stft_stream_gathered_checksum_ok"] is True
    assert abs(ex["broad_sweep_ms_resident"] - ex["broad_sweep_1gpu_ms"]) < 1e-12 and ex["broad_sweep_ms_ingest"] > ex["broad_sweep_ms_resident"]
    assert ex["broad_sweep_resident_gathered_checksum_matches_pinned"] is True and ex["stft_stream_gathered_checksum_matches_pinned"] is True
    _same_image_at_every_world_size(1, ex["broad_sweep_resident_gathered_checksum"])
    # independent batches on two streams: one launch's drain under the next one's ramp; beside `value`, never in it
    assert 0.9 * d["value"] < ex["two_stream_frames_per_sec_n8192"] < 1.3 * d["value_events"]
    assert 0.1 < ex["stft16384_roofline_frac"] < 1.0 and 0.1 < ex["broad_sweep_roofline_frac"] < 1.0
    # the taper window, fused: Hann beside rectangular, same run, same method; both kernels named
    assert ex["hann_n8192_kernel"] == "fsea_fft8192_u8_mag_win" and ex["stft16384_hann_kernel"] == "fsea_fft16384_u8_mag_half_win"
    assert 0.85 < ex["hann_n8192_over_rect"] < 1.1 and 0.85 < ex["stft16384_hann_over_rect"] < 1.1
    assert 0.1 < ex["stft16384_hann_roofline_frac"] < 1.0
    # the sweep: step time by the wall clock, kernel time by events, both fractions, and the two-stream form beside them
    assert ex["broad_sweep_1gpu_kernel_ms"] <= ex["broad_sweep_1gpu_ms"] * 1.02
    assert ex["broad_sweep_roofline_frac_by_step_time"] <= ex["broad_sweep_roofline_frac"] * 1.02
    assert 0 < ex["broad_sweep_1gpu_ms_two_streams"] < ex["broad_sweep_1gpu_ms"] * 1.1
    assert ex["timed_regions_per_figure"] >= 5
    # BASELINE config 2, the nrf_* API per rendered frame, with the oracle's restatement of the reference's loop beside it
    assert 0 < ex["nrf_fft_1024x1024_process_us"] < ex["nrf_fft_1024x1024_process_get_buffer_us"] < 5000
    cb = d["cpu_baseline"]
    assert cb["unit"] == "frames/s" and cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0
    assert isinstance(cb["sample"], str) and cb["sample"]
    assert cb["host_cpus_visible"] >= cb["cores"] and cb["nrf_stream"]["process_get_buffer_us"] > 0


@pytest.mark.gpu
def test_a_plain_bench_run_is_the_headline_alone_and_dumps_what_its_last_step_computed(tmp_path):
    """Without --full the run is set-up, warm-up, exactly K timed steps and the line; --dump-outputs writes the rows the last
    timed step computed (a seeded sample of them), float32, within 64 MB, and they are the numpy transform of that step's
    input (seeded: the same in every run)."""
    import numpy as np
    import bench
    steps, warmup, n, frames = 7, 3, 8192, 4096
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(dump)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "fft_frames_per_sec_n8192" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == steps and d["warmup"] == warmup
    assert abs(d["value"] - frames * 1e3 / d["ms_per_step"]) / d["value"] < 1e-6
    for key in ("extra", "cpu_baseline", "headline_regions_ms", "parity_rel_l2_first_rows"):
        assert key not in d, key                          # measured and checked with --full only
    assert sorted(os.listdir(dump)) == ["mag_rows.npy"]
    rows = np.load(dump / "mag_rows.npy")
    idx = bench.dump_rows(frames, 4 * n)
    assert rows.dtype == np.float32 and rows.shape == (len(idx), n) and rows.nbytes <= 64e6
    # the last timed step is step warmup + steps - 1: buffer set (warmup + steps - 1) % 6, whose input is the seeded batch
    # rolled by 16 bytes per set (bench.run_gpu)
    host = np.roll(bench.synth_batch(3, 2 * n * frames), 2 * 8 * ((warmup + steps - 1) % 6))
    for j in (0, len(idx) // 2, len(idx) - 1):
        f = int(idx[j])
        want = bench.numpy_rows(host[2 * n * f: 2 * n * (f + 1)], 1, n, n)[0]
        rel = float(np.linalg.norm(rows[j] - want) / np.linalg.norm(want))
        assert rel <= 1e-6, (f, rel)
