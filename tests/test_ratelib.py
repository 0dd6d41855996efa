"""scripts/ratelib.py, the measurement module of the scripts/*_rate.py: the kernel-trace reader on a trace of the test's own
making (a stub in rocprofv3's place), the part runner on a stub script, the seeded recording, and that every script that
moved onto the module still imports and kept no copy of what it replaced.  GPU tier, at the bottom: the three timing
functions on the smallest launch of a real kernel -- how often they call and what they return, no timing thresholds."""
import importlib.util
import math
import os
import stat
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
MOVED = ["cfar_rate", "demod_rate", "detect_rate", "events_rate", "extract_rate", "interp_rate", "iq_chain_rate",
         "iq_draw_rate", "persist_rate", "pfb_rate", "trace_rate", "zoom_rate", "fir_roofline", "measure_rate", "audio_rate"]
CUTOUT_SCRIPTS = ["extract_rate", "measure_rate", "audio_rate"]     # they measure on ratelib.cutouts


def load(name, monkeypatch):
    """scripts/<name>.py as a module, with its directory first on sys.path as when it is started, and sys.path put back."""
    monkeypatch.setattr(sys, "path", [SCRIPTS] + sys.path)
    if name != "ratelib":
        monkeypatch.delitem(sys.modules, "ratelib", raising=False)
    spec = importlib.util.spec_from_file_location("_scripts_" + name, os.path.join(SCRIPTS, name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture
def ratelib(monkeypatch):
    return load("ratelib", monkeypatch)


def executable(path, text):
    with open(path, "w") as f:
        f.write(text)
    os.chmod(path, os.stat(path).st_mode | stat.S_IXUSR)
    return path


# ---- the trace reader

# (kernel name, start, end): two kernels interleaved, out of time order.  Of "mine_" there are six: two cases of three.
TRACE = [("mine_a(int)", 500, 530), ("other", 90, 95), ("mine_a(int)", 100, 110), ("mine_b(int)", 900, 960),
         ("other", 510, 515), ("mine_a(int)", 300, 320), ("mine_b(int)", 700, 740), ("other", 910, 915), ("mine_b(int)", 800, 850)]

STUB_ROCPROF = """#!%s
import os, sys
args = sys.argv[1:]
assert args[0] == "--kernel-trace" and "--pmc" not in args, args
out_dir, name, rest = args[args.index("-d") + 1], args[args.index("-o") + 1], args[args.index("--") + 1:]
assert rest == ["the-program", "launches"], rest
rows = %r
for k in range(%d):
    os.makedirs(os.path.join(out_dir, "host%%d" %% k))
    with open(os.path.join(out_dir, "host%%d" %% k, name + "_kernel_trace.csv"), "w") as f:
        f.write('"Kind","Kernel_Name","Start_Timestamp","End_Timestamp"\\n')
        for kernel, start, end in rows:
            f.write('"KERNEL_DISPATCH","%%s",%%d,%%d\\n' %% (kernel, start, end))
print("rocprofv3's own chatter")
"""


def stub_rocprofv3(tmp_path, monkeypatch, rows, n_files=1):
    bin_dir = tmp_path / "bin"
    bin_dir.mkdir()
    executable(str(bin_dir / "rocprofv3"), STUB_ROCPROF % (sys.executable, rows, n_files))
    monkeypatch.setenv("PATH", str(bin_dir) + os.pathsep + os.environ["PATH"])


def test_kernel_trace_gives_each_case_in_start_order(ratelib, tmp_path, monkeypatch, capfd):
    stub_rocprofv3(tmp_path, monkeypatch, TRACE)
    cases = ratelib.kernel_trace(["the-program", "launches"], "mine_", 3, 2)
    assert [name for name, _ in cases] == ["mine_a(int)", "mine_b(int)"]
    assert [[round(t * 1e9) for t in times] for _, times in cases] == [[10, 20, 30], [40, 50, 60]]
    assert "chatter" not in capfd.readouterr().out
    kept = tmp_path / "kept"
    assert ratelib.kernel_trace(["the-program", "launches"], "mine_", 3, 2, out_dir=str(kept)) == cases
    assert (kept / "host0" / "mine__kernel_trace.csv").exists()


def test_kernel_trace_refuses_a_wrong_dispatch_count(ratelib, tmp_path, monkeypatch):
    stub_rocprofv3(tmp_path, monkeypatch, TRACE[1:])
    with pytest.raises(SystemExit) as e:
        ratelib.kernel_trace(["the-program", "launches"], "mine_", 3, 2)
    assert str(e.value) == "expected 6 dispatches of mine_, found 5"


@pytest.mark.parametrize("n_files", [0, 2])
def test_kernel_trace_refuses_no_trace_and_two(ratelib, tmp_path, monkeypatch, n_files):
    stub_rocprofv3(tmp_path, monkeypatch, TRACE, n_files)
    out = str(tmp_path / "out")
    with pytest.raises(SystemExit) as e:
        ratelib.kernel_trace(["the-program", "launches"], "mine_", 3, 2, out_dir=out)
    assert str(e.value) == "expected one kernel trace under %s, found %d" % (out, n_files)


def test_kernel_trace_takes_several_prefixes(ratelib, tmp_path, monkeypatch):
    """a call whose kernels share no prefix (measure_rate.py: the job tables' upload and fsea_measure_*): one case of all
    that start with any of them, in start order; the first prefix names the trace"""
    stub_rocprofv3(tmp_path, monkeypatch, TRACE)
    kept = tmp_path / "kept"
    cases = ratelib.kernel_trace(["the-program", "launches"], ("oth", "mine_b"), 6, 1, out_dir=str(kept))
    assert [(name, [round(t * 1e9) for t in times]) for name, times in cases] == [("other", [5, 5, 40, 50, 60, 5])]
    assert (kept / "host0" / "oth_kernel_trace.csv").exists()
    with pytest.raises(SystemExit) as e:
        ratelib.kernel_trace(["the-program", "launches"], ("oth", "mine_b"), 5, 1)
    assert str(e.value) == "expected 5 dispatches of oth / mine_b, found 6"


# ---- the host time of a call that does not wait

def test_host_time_stops_the_clock_round_the_call_alone(ratelib, monkeypatch):
    """a stub clock that every look at it advances by 1, a call that advances it by 10 and an idle() that advances it by 100:
    each sample is the call's 10 and the one step of the first look, and idle() runs in front of every call and once behind
    the last, never inside the clock"""
    now, log = [0.0], []

    def clock():
        now[0] += 1.0
        log.append("clock")
        return now[0]

    def call():
        now[0] += 10.0
        log.append("call")

    def idle():
        now[0] += 100.0
        log.append("idle")

    monkeypatch.setattr(ratelib.time, "perf_counter", clock)
    assert ratelib.host_time(call, idle, 3) == [11.0, 11.0, 11.0]
    assert log == ["idle", "clock", "call", "clock"] * 3 + ["idle"]
    del log[:]
    assert ratelib.host_time(call, idle, 0) == [] and log == ["idle"]


# ---- the part runner

STUB_SCRIPT = """import sys, time
part = sys.argv[1]
if part == "a":
    print("a one")
    print("a two")
elif part == "b":
    sys.exit(3)
elif part == "c":
    open(%r, "w").close()
    print("c ran", " ".join(sys.argv[2:]))
elif part == "slow":
    print("slow started", flush=True)
    time.sleep(30)
"""


@pytest.fixture
def stub_script(tmp_path):
    marker = str(tmp_path / "marker")
    script = str(tmp_path / "stub_rate.py")
    with open(script, "w") as f:
        f.write(STUB_SCRIPT % marker)
    return script, marker


def test_run_parts_stops_at_the_first_failure(ratelib, stub_script, tmp_path, capfd):
    script, marker = stub_script
    to = str(tmp_path / "text.txt")
    with pytest.raises(SystemExit) as e:
        ratelib.run_parts(script, {"a": 20, "b": 20, "c": 20}, ["--to", to], header="# header\n")
    assert str(e.value) == "b failed (exit status 3): stopping"
    assert not os.path.exists(marker)
    assert not os.path.exists(to)
    assert capfd.readouterr().out == "a one\na two\n"


def test_run_parts_writes_header_and_outputs_after_the_last_part(ratelib, stub_script, tmp_path, capfd):
    script, marker = stub_script
    to, other = str(tmp_path / "text.txt"), str(tmp_path / "other.txt")
    assert ratelib.run_parts(script, {"a": 20, "c": 20}, ["--out", "DIR"], to=to, header="# header\n") is None
    assert os.path.exists(marker)
    with open(to) as f:
        assert f.read() == "# header\na one\na two\nc ran --out DIR\n"      # what is not --to goes on to the parts
    assert capfd.readouterr().out == "a one\na two\nc ran --out DIR\n"
    ratelib.run_parts(script, {"a": 20}, ["--to", other], to=to)             # --to FILE: there instead
    with open(other) as f:
        assert f.read() == "a one\na two\n"
    before = sorted(os.listdir(str(tmp_path)))
    ratelib.run_parts(script, {"a": 20}, [])                                 # no file named: none written
    assert sorted(os.listdir(str(tmp_path))) == before


def test_run_parts_reports_a_part_past_its_limit(ratelib, stub_script, tmp_path):
    script, marker = stub_script
    to = str(tmp_path / "text.txt")
    with pytest.raises(SystemExit) as e:
        ratelib.run_parts(script, {"a": 20, "slow": 1, "c": 20}, [], to=to)
    assert str(e.value) == "slow failed (exit status 124): stopping"
    assert not os.path.exists(marker) and not os.path.exists(to)


def test_run_parts_names_the_part_it_was_started_with(ratelib, stub_script):
    script, marker = stub_script
    parts = {"a": 20, "measure 16": 20, "c": 20}
    assert ratelib.run_parts(script, parts, ["c"]) == "c"
    assert ratelib.run_parts(script, parts, ["--out", "DIR", "a", "--to", "FILE"]) == "a"
    assert ratelib.run_parts(script, parts, ["measure", "16"]) == "measure 16"
    assert not os.path.exists(marker)


# ---- the recording, and the scripts

def test_recording_is_the_seeded_bytes(ratelib):
    want = np.random.default_rng(1).integers(0, 256, 8192, dtype=np.uint8)
    got = ratelib.recording(4096)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(ratelib.recording(4096, seed=2), np.random.default_rng(2).integers(0, 256, 8192, dtype=np.uint8))


def test_importing_ratelib_does_not_import_torch():
    import subprocess
    code = "import sys; sys.path.insert(0, %r); import ratelib; assert 'torch' not in sys.modules" % SCRIPTS
    subprocess.run([sys.executable, "-c", code], check=True)


@pytest.mark.parametrize("name", MOVED)
def test_a_moved_script_imports_and_kept_no_copy(name, monkeypatch):
    module = load(name, monkeypatch)
    assert callable(module.main)
    assert module.ratelib.__file__ == os.path.join(SCRIPTS, "ratelib.py")
    for gone in ("event_times", "timed", "rounds", "median_us", "step", "kernels", "release"):
        assert not hasattr(module, gone), "%s.py still has its own %s" % (name, gone)
    if name in CUTOUT_SCRIPTS:
        with open(os.path.join(SCRIPTS, name + ".py")) as f:
            text = f.read()
        for gone in ("ExtractJob(", "lowpass_taps(10e6", "torch"):
            assert gone not in text, "%s.py still builds its own cut-outs: %s" % (name, gone)


def test_cutout_jobs_are_the_scripts_jobs(ratelib):
    from frequensea_amd import fsea
    jobs = ratelib.cutout_jobs(fsea, 256, 65540)
    assert len(jobs) == 256
    for i, j in enumerate(jobs):
        first = 131072 * i + 3 + i % 5
        assert (j.first, j.n_samples, j.sample_offset, j.out_first) == (first, 65540, first, 0)
        assert (j.cycles_per_sample, j.phase0_cycles) == ((i - 128) / 1024, 0.0)


# ---- GPU tier: the plumbing of the three timing functions on the smallest launch of a real kernel

@pytest.fixture
def tiny_launch(ratelib):
    import torch  # noqa: F401  torch's HIP runtime first, then the library, as the scripts do
    from frequensea_amd import fsea
    n, frames = 1024, 64
    d_in = fsea.DeviceBuffer(2 * n * frames).upload(ratelib.recording(n * frames))
    d_out = fsea.DeviceBuffer(4 * n * frames)
    plan = fsea.Plan(n)
    calls = []

    def call():
        calls.append(1)
        plan.exec_device(d_in.ptr.value, frames, d_out.ptr.value)

    yield plan, call, calls
    plan.synchronize()
    plan.close()
    d_in.free()
    d_out.free()


def finite_positive(times):
    return all(isinstance(t, float) and math.isfinite(t) and t > 0 for t in times)


@pytest.mark.gpu
def test_gpu_per_call_and_per_round_call_as_often_as_they_say(ratelib, tiny_launch):
    plan, call, calls = tiny_launch
    times = ratelib.per_call(call, 2, 5)
    assert len(times) == 5 and finite_positive(times) and len(calls) == 7
    del calls[:]
    times = ratelib.per_round(call, 1, 3, 2)
    assert len(times) == 2 and finite_positive(times) and len(calls) == 7


@pytest.mark.gpu
def test_gpu_wall_of_a_waiting_call_is_no_shorter_than_the_launch(ratelib, tiny_launch):
    plan, call, calls = tiny_launch
    shortest = min(ratelib.per_call(call, 2, 5))
    del calls[:]

    def waiting_call():
        call()
        plan.synchronize()

    times = ratelib.wall(waiting_call, 1, 4)
    assert len(times) == 4 and len(calls) == 5
    assert all(t >= shortest for t in times), (times, shortest)
