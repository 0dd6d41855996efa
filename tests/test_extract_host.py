"""CPU tier: event cut-outs without a GPU -- the argument checks of fsea_extract_* (before any device work, against a fake
object where a check must not look into the object beyond its decimation), their order, the no-op cases; fsea_extract_jobs
and fsea_extract_layout against the restatement of tests/extract_ref.py, field for field; the shipped fsea_extract_u8
kernels' resource usage; the restatement's own end-to-end check on the CPU; fsea-cutouts' usage errors."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import extract_ref as R
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels
from tests.test_zoom_host import zoom_reference

FSEA_EINVAL = -1
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-cutouts")


def job(first=0, n=64, offset=0, cps=0.01, phase0=0.0, out_first=0):
    return fsea.ExtractJob(first, n, offset, cps, phase0, out_first)


def table(*jobs):
    return (fsea.ExtractJob * len(jobs))(*jobs)


def test_header_constants_and_the_job_record_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()
    assert int(re.search(r"#define FSEA_EXTRACT_MAX_JOBS (\d+)", text).group(1)) == fsea.EXTRACT_MAX_JOBS == 65536
    body = re.search(r"typedef struct \{([^}]*)\} fsea_extract_job;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(name.strip(), {"uint64_t": "<u8", "double": "<f8"}[ctype]) for ctype, name in re.findall(r"(uint64_t|double)\s+(\w+);", body)]
    assert np.dtype(fields) == R.JOB and R.JOB.itemsize == ctypes.sizeof(fsea.ExtractJob) == 48
    assert [n for n, _ in fields] == [n for n, _ in fsea.ExtractJob._fields_]
    assert len([n for n in fsea.EXPORTS if n.startswith("fsea_extract_")]) == 10


def test_extract_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    err = L.fsea_last_error_string
    h = ctypes.c_void_p()
    taps = np.ones(fsea.FIR_MAX_TAPS + 1)
    t = taps.ctypes.data
    for n in (0, -3, fsea.FIR_MAX_TAPS + 1):
        assert L.fsea_extract_create(ctypes.byref(h), t, n, 4, 0) == FSEA_EINVAL and not h.value and b"n_taps" in err()
    for d in (0, -1, fsea.ZOOM_MAX_DECIMATION + 1):
        assert L.fsea_extract_create(ctypes.byref(h), t, 21, d, 0) == FSEA_EINVAL and not h.value and b"decimation" in err()
    assert L.fsea_extract_create(ctypes.byref(h), None, 21, 4, 0) == FSEA_EINVAL and b"taps is NULL" in err()
    assert L.fsea_extract_create(None, t, 21, 4, 0) == FSEA_EINVAL and b"out-pointer" in err()
    bad = np.ones(21)
    bad[3] = np.nan
    assert L.fsea_extract_create(ctypes.byref(h), bad.ctypes.data, 21, 4, 0) == FSEA_EINVAL and b"not finite" in err()
    assert L.fsea_extract_destroy(None) == 0
    assert L.fsea_extract_decimation(None) == 0 and L.fsea_extract_n_taps(None) == 0 and L.fsea_extract_out_pairs(None, 64) == 0

    buf = np.full(8192, 0x5A, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    pairs = p + 4096
    one = table(job())
    j = ctypes.addressof(one)
    forms = ((L.fsea_extract_run_device, (None,)), (L.fsea_extract_run_host, ()))
    # a NULL object, before anything else
    for run, tail in forms:
        assert run(None, None, 0, 0, None, fsea.EXTRACT_MAX_JOBS + 1, None, 0, *tail) == FSEA_EINVAL and b"extract is NULL" in err()
    total = ctypes.c_size_t(77)
    assert L.fsea_extract_layout(None, j, 1, ctypes.byref(total)) == FSEA_EINVAL and b"extract is NULL" in err()

    # a fake object: the struct begins `int n_taps; int decimation; int device;`, and the checks read the decimation alone
    fake = ctypes.create_string_buffer(4096)
    struct.pack_into("<iii", fake, 0, 97, 4, 0)
    f = ctypes.cast(fake, ctypes.c_void_p)
    assert L.fsea_extract_decimation(f) == 4 and L.fsea_extract_n_taps(f) == 97 and L.fsea_extract_out_pairs(f, 67) == 16
    big = 1 << 40

    def refused(jobs, word, n_iq=512, capacity=512, iq=p, out=pairs, n_jobs=None):
        tab = table(*jobs)
        for run, tail in forms:
            rc = run(f, iq, n_iq, 0, ctypes.addressof(tab) if jobs else None, len(jobs) if n_jobs is None else n_jobs, out, capacity, *tail)
            assert rc == FSEA_EINVAL and word in err(), (run, word, err())

    for run, tail in forms:
        # the count comes before the table and the buffers; no jobs: a no-op whatever else is given
        assert run(f, None, 0, 0, None, fsea.EXTRACT_MAX_JOBS + 1, None, 0, *tail) == FSEA_EINVAL and b"n_jobs" in err()
        assert run(f, None, 0, 0, None, 0, None, 0, *tail) == 0
        assert run(f, p + 4, 7, 1, None, 0, pairs + 8, 0, *tail) == 0
        assert run(f, None, 512, 0, None, 1, None, 512, *tail) == FSEA_EINVAL and b"NULL job table" in err()
        assert run(f, None, 512, 0, j, 1, pairs, 512, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
        assert run(f, p, 512, 0, j, 1, None, 512, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
    refused([job(), job(first=500, n=13)], b"job 1: samples")                      # past the input
    refused([job(first=big)], b"job 0: samples")
    refused([job(n=(1 << 64) - 1, first=2)], b"job 0: samples")                    # first + n wraps
    refused([job(n=(1 << 31) + 1)], b"job 0: n_samples", n_iq=big)
    refused([job(n=(1 << 31) + 1, first=big)], b"samples", n_iq=big)               # past the input before too long
    for cps, ph in ((np.nan, 0.0), (np.inf, 0.0), (2.0 ** 21, 0.0)):
        refused([job(), job(cps=cps, phase0=ph)], b"job 1: cycles_per_sample")
    for ph in (np.nan, -np.inf):
        refused([job(phase0=ph)], b"job 0: phase0_cycles")
    refused([job(offset=(1 << 52) + 1)], b"job 0: sample_offset + n_samples")
    refused([job(offset=(1 << 52) - 63)], b"job 0: sample_offset + n_samples")
    refused([job(n=1 << 31, cps=np.nan), job(n=(1 << 31) + 1)], b"job 0: cycles_per_sample", n_iq=big)    # table order
    refused([job(n=1 << 31), job(n=1 << 31), job(n=1 << 31), job(n=1 << 31), job(n=4)], b"more than 2^31", n_iq=big, capacity=big)
    struct.pack_into("<iii", fake, 0, 97, 1, 0)
    refused([job(n=1 << 31), job(n=1, cps=np.inf)], b"job 1: cycles_per_sample", n_iq=big, capacity=big)   # jobs before the total
    refused([job(n=1 << 31, out_first=1 << 33), job(n=1)], b"more than 2^31", n_iq=big, capacity=4)       # the total before the ranges
    struct.pack_into("<iii", fake, 0, 97, 4, 0)
    refused([job(out_first=497)], b"job 0: outputs")                               # 16 outputs from 497: one past 512
    refused([job(out_first=big)], b"job 0: outputs")
    refused([job(), job(out_first=(1 << 64) - 1)], b"job 1: outputs")
    refused([job(out_first=40), job(n=3, out_first=44), job(out_first=30), job(out_first=45)], b"jobs 0 and 2 overlap")
    refused([job(out_first=8), job(out_first=8)], b"jobs 0 and 1 overlap")
    refused([job(out_first=600), job(out_first=0), job(out_first=15)], b"job 0: outputs")                 # capacity before overlap
    # jobs without output take no room: anywhere, also on top of another
    empty = table(job(out_first=0), job(n=3, out_first=5), job(n=0, out_first=1 << 50))
    assert L.fsea_extract_run_device(f, p + 4, 512, 0, ctypes.addressof(empty), 3, pairs, 512, None) == FSEA_EINVAL and b"aligned" in err()
    for d_iq, d_pairs in ((p + 4, pairs), (p, pairs + 8), (p + 1, pairs)):
        assert L.fsea_extract_run_device(f, d_iq, 512, 0, j, 1, d_pairs, 512, None) == FSEA_EINVAL and b"aligned" in err()
    over = table(job(out_first=8), job(out_first=8))
    assert L.fsea_extract_run_device(f, p + 4, 512, 0, ctypes.addressof(over), 2, pairs, 512, None) == FSEA_EINVAL and b"overlap" in err()
    assert np.all(buf == 0x5A)                                                     # a refused call writes nothing

    # the layout
    assert L.fsea_extract_layout(f, j, 1, None) == FSEA_EINVAL and b"total_pairs" in err()
    assert L.fsea_extract_layout(f, None, 1, ctypes.byref(total)) == FSEA_EINVAL and b"NULL job table" in err()
    assert L.fsea_extract_layout(f, j, fsea.EXTRACT_MAX_JOBS + 1, ctypes.byref(total)) == FSEA_EINVAL and b"n_jobs" in err()
    assert L.fsea_extract_layout(f, None, 0, ctypes.byref(total)) == 0 and total.value == 0

    # the jobs of events: host arithmetic
    ev = np.zeros(2, fsea.EVENTS_EVENT)
    out, fits = table(job(), job()), np.zeros(2, np.uint8)
    e, o, ft = ev.ctypes.data, ctypes.addressof(out), fits.ctypes.data
    assert L.fsea_extract_jobs(e, 2, 1024, 1024, 1 << 20, 97, 16, 0.8, o, ft) == 0
    for args in ((None, 2, 1024, 1024, 1 << 20, 97, 16, 0.8, o, ft), (e, 2, 1024, 1024, 1 << 20, 97, 16, 0.8, None, ft),
                 (e, 2, 1024, 1024, 1 << 20, 97, 16, 0.8, o, None)):
        assert L.fsea_extract_jobs(*args) == FSEA_EINVAL and b"NULL" in err()
    assert L.fsea_extract_jobs(None, 0, 1024, 1024, 1 << 20, 97, 16, 0.8, None, None) == 0
    for width, hop, word in ((0, 1024, b"width"), (-4, 1024, b"width"), (1024, 0, b"hop"), (1024, -1, b"hop")):
        assert L.fsea_extract_jobs(e, 2, width, hop, 1 << 20, 97, 16, 0.8, o, ft) == FSEA_EINVAL and word in err()
    for n_taps in (0, fsea.FIR_MAX_TAPS + 1):
        assert L.fsea_extract_jobs(e, 2, 1024, 1024, 1 << 20, n_taps, 16, 0.8, o, ft) == FSEA_EINVAL and b"n_taps" in err()
    for d in (0, fsea.ZOOM_MAX_DECIMATION + 1):
        assert L.fsea_extract_jobs(e, 2, 1024, 1024, 1 << 20, 97, d, 0.8, o, ft) == FSEA_EINVAL and b"decimation" in err()
    for fill in (0.0, -0.5, 1.0000001, np.nan, np.inf):
        assert L.fsea_extract_jobs(e, 2, 1024, 1024, 1 << 20, 97, 16, fill, o, ft) == FSEA_EINVAL and b"max_fill" in err()
    assert L.fsea_extract_jobs(e, 2, 1024, 1024, 1 << 20, 97, 16, 1.0, o, ft) == 0


def test_lead():
    L = fsea.hip_lib()
    for n_taps in (1, 2, 16, 17, 97, 512):
        for d in (1, 2, 3, 16, 25, 64):
            assert fsea.extract_lead(n_taps, d) == R.lead(n_taps, d)
            assert R.lead(n_taps, d) % d == 0 and 0 <= R.lead(n_taps, d) - (n_taps - 1) < d
    assert L.fsea_extract_lead(0, 4) == 0 and L.fsea_extract_lead(97, 0) == 0


def _events(rows_first, rows_last, cols_first, cols_last):
    ev = np.zeros(len(rows_first), fsea.EVENTS_EVENT)
    ev["row_first"], ev["row_last"], ev["col_first"], ev["col_last"] = rows_first, rows_last, cols_first, cols_last
    return ev


def _compare(ev, width, hop, n_samples, n_taps, d, fill):
    got, fits = fsea.extract_jobs(ev, width, hop, n_samples, n_taps, d, fill)
    want, want_fits = R.jobs(ev, width, hop, n_samples, n_taps, d, fill)
    got = np.frombuffer(got, dtype=R.JOB) if len(ev) else np.zeros(0, R.JOB)
    assert np.array_equal(fits, want_fits)
    for name in R.JOB.names:                    # field for field; the doubles as bits
        assert np.array_equal(got[name].view(np.uint64), want[name].view(np.uint64)), name
    return got, fits


@pytest.mark.parametrize("width,hop,n_taps,d,fill", [(1024, 1024, 97, 16, 0.8), (1000, 300, 41, 3, 0.5), (1, 1, 1, 1, 1.0),
                                                     (777, 1500, 512, 64, 0.8), (4096, 512, 97, 25, 0.33)])
def test_jobs_of_random_boxes_equal_the_restatement(width, hop, n_taps, d, fill):
    rng = np.random.default_rng(width + d)
    n = 3000
    rows = np.sort(rng.integers(0, 5000, (n, 2)), axis=1)
    cols = np.sort(rng.integers(0, width, (n, 2)), axis=1)
    narrow = rng.random(n) < 0.7                 # most boxes narrow enough to fit
    cols[narrow, 1] = np.minimum(cols[narrow, 0] + rng.integers(0, max(int(fill * width / d), 1) + 2, n)[narrow], width - 1)
    n_samples = 4000 * hop + width // 2          # some boxes end past the recording, some begin past it
    got, fits = _compare(_events(rows[:, 0], rows[:, 1], cols[:, 0], cols[:, 1]), width, hop, n_samples, n_taps, d, fill)
    assert 0 < fits.sum() < n or width == 1
    assert np.all(got["first"] == got["sample_offset"]) and np.all(got["out_first"] == 0) and np.all(got["phase0_cycles"] == 0)
    assert np.all(got["first"] + got["n_samples"] <= max(n_samples, int(got["first"].max())))


def test_jobs_at_the_edges():
    N, H, taps, d = 1024, 512, 97, 16
    ld = R.lead(taps, d)
    assert ld == 96
    limit = int(0.8 * N / d)                     # 51 columns fit, 52 do not
    ev = _events([0, 0, 1, 10, 10, 10, 10, 10, 4000, 4100],
                 [0, 3, 1, 12, 12, 12, 12, 9000, 4000, 4100],
                 [5, 512, 700, 100, 100, 512, 0, 30, 40, 50],
                 [5, 512, 700, 100 + limit - 1, 100 + limit, 512, N - 1, 31, 40, 50])
    n_samples = 4000 * H + 100                   # row 4000 begins inside the recording and ends past it; row 4100 lies past it
    got, fits = _compare(ev, N, H, n_samples, taps, d, 0.8)
    assert list(fits) == [1, 1, 1, 1, 0, 1, 0, 1, 1, 1]
    assert (got["first"][0], got["n_samples"][0]) == (0, N)                        # row_first = 0: no room for a lead
    assert got["first"][2] == 512 - ld                                             # begin >= lead
    assert got["n_samples"][4] == 0 and got["n_samples"][6] == 0                   # one column over the fill limit; the whole width
    assert got["n_samples"][3] == 12 * H + N - (10 * H - ld)
    assert got["cycles_per_sample"][1] == 0.0 and not np.signbit(got["cycles_per_sample"][1])     # the centre column: exactly +0
    assert got["cycles_per_sample"][5] == 0.0
    assert got["cycles_per_sample"][0] == (512 - 5) / 1024.0 and got["cycles_per_sample"][2] == -(700 - 512) / 1024.0
    assert got["cycles_per_sample"][7] == (1024 - 61) / 2048.0                     # a half-column centre
    assert got["first"][7] + got["n_samples"][7] == n_samples                      # a box ending past the recording is cut there
    assert got["n_samples"][8] == n_samples - (4000 * H - ld) and got["n_samples"][9] == 0        # and one that begins past it is empty
    # begin < lead, an odd width, a width of 1
    got, _ = _compare(_events([1, 0], [2, 5], [3, 0], [3, 0]), 7, 10, 1000, taps, 3, 1.0)      # 3 of 7 columns: fits
    assert got["first"][0] == 0 and got["n_samples"][0] == 2 * 10 + 7 and got["cycles_per_sample"][0] == 0.0     # column 3 of 7 is the centre
    assert got["cycles_per_sample"][1] == 6 / 14.0
    got, fits = _compare(_events([3], [3], [0], [0]), 1, 1, 50, 5, 1, 1.0)
    assert list(fits) == [1] and got["cycles_per_sample"][0] == 0.0 and (got["first"][0], got["n_samples"][0]) == (0, 4)
    _compare(_events([], [], [], []), N, H, 100, taps, d, 0.8)


def test_layout_puts_every_job_at_an_even_pair():
    L = fsea.hip_lib()
    for d in (1, 3, 16):
        fake = ctypes.create_string_buffer(4096)
        struct.pack_into("<iii", fake, 0, 97, d, 0)
        f = ctypes.cast(fake, ctypes.c_void_p)
        ns = [0, d - 1, d, 3 * d, 3 * d + 1, 0, 0, 7 * d + d - 1, 1000, 2 * d, 0]
        tab = table(*[job(n=n, out_first=12345) for n in ns])
        total = ctypes.c_size_t()
        assert L.fsea_extract_layout(f, ctypes.addressof(tab), len(ns), ctypes.byref(total)) == 0
        firsts, want_total = R.layout(ns, d)
        assert [t.out_first for t in tab] == firsts and total.value == want_total
        assert all(x % 2 == 0 for x in firsts)
        ends = [a + n // d for a, n in zip(firsts, ns)]
        assert all(b >= e for b, e in zip(firsts[1:], ends[:-1])) and total.value == ends[-1]
        assert [t.n_samples for t in tab] == ns                                    # nothing else is touched


def test_shipped_library_has_the_extract_kernels_within_their_budget():
    """The three LDS sizes of fsea_extract_u8: wave64, 256 lanes, no scratch, no spilled register, the zoom's LDS sizes and so
    its eight, four and two workgroups on a CU's 160 KiB; no more registers than the build it was written against."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    cu_lds = 160 * 1024
    for name, per_cu, zoom in (("fsea_extract_u8_s", 8, "fsea_shift_decim_u8_s"), ("fsea_extract_u8_m", 4, "fsea_shift_decim_u8_m"),
                               ("fsea_extract_u8", 2, "fsea_shift_decim_u8")):
        k = ks[name]
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= VGPRS and k[".sgpr_count"] <= SGPRS, (name, k[".vgpr_count"], k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == ks[zoom][".group_segment_fixed_size"]
        assert cu_lds // k[".group_segment_fixed_size"] == per_cu, (name, k[".group_segment_fixed_size"])


VGPRS, SGPRS = 38, 90      # read off the build: eight waves per SIMD need no more than 64 VGPRs


def test_the_restatement_alone_finds_each_burst_at_the_centre_of_its_cutout():
    """What tests/test_gpu_extract.py asks of the device's cut-outs, first asked of the restatement on the CPU: jobs from the
    boxes of the injection, zoom_reference on each job's slice, the run-in dropped, and the largest FFT bin over the outputs
    inside the burst is bin 0 or +-1 -- as they are, and with the 0.5 + 0.5j the shifter's samples rest on taken off
    (tests/extract_ref.py: only then does bin 0 say anything about the shift)."""
    raw = R.recording()
    c = fsea.lowpass_taps(1.0, 0.4 / R.D, R.TAPS)
    jobs, fits = R.jobs(R.ideal_events(), R.N, R.N, R.N * R.ROWS, R.TAPS, R.D)
    assert list(fits) == [1, 1, 1]
    for j, burst in zip(jobs, R.BURSTS):
        first, n = int(j["first"]), int(j["n_samples"])
        assert first == burst[0] * R.N - R.lead(R.TAPS, R.D) and first + n == burst[1] * R.N
        y, _ = zoom_reference(raw[2 * first:2 * (first + n)], 1, float(j["cycles_per_sample"]), 0.0, c, R.D, offset=first)
        k = R.peak_bin_inside_the_burst(y[R.lead(R.TAPS, R.D) // R.D:], first, burst)
        assert abs(k) <= 1, (burst, k)
        k = R.peak_bin_inside_the_burst(y[R.lead(R.TAPS, R.D) // R.D:], first, burst, rest=(0.5 + 0.5j) * c.sum())
        assert abs(k) <= 1, (burst, k, "without the shifter's 0.5 + 0.5j")
    # and it has teeth: a centre eight columns off (still inside the low-pass) puts the peak an eighth of the bins away
    j = jobs[0]
    first, n = int(j["first"]), int(j["n_samples"])
    y, _ = zoom_reference(raw[2 * first:2 * (first + n)], 1, float(j["cycles_per_sample"]) + 8.0 / R.N, 0.0, c, R.D, offset=first)
    assert abs(R.peak_bin_inside_the_burst(y[R.lead(R.TAPS, R.D) // R.D:], first, R.BURSTS[0], rest=(0.5 + 0.5j) * c.sum())) > 100


def test_tool_usage_errors():
    assert os.path.exists(TOOL), "fsea-cutouts not built"
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("usage: fsea-cutouts FILE --size N --decimation D --out DIR")
    x = ["x.raw", "--size", "1024", "--out", "y"]
    for args, word in ((x + ["--decimation", "4", "--image", "y.png"], "--image"), (x, "--decimation D is required"),
                       (x + ["--decimation", "65"], "--decimation must be in [1, 64]"), (x + ["--decimation", "-2"], "--decimation must be"),
                       (x + ["--decimation", "4", "--taps", "513"], "--taps"), (x + ["--decimation", "4", "--fill", "1.5"], "--fill"),
                       (x + ["--decimation", "4", "--max-events", "0"], "--max-events"),
                       (x + ["--decimation", "4", "--max-samples", "16777217"], "--max-samples"),
                       (["x.raw", "--size", "1024", "--decimation", "4"], "--out DIR is required"),
                       (x + ["--decimation", "4", "--bogus"], "usage: fsea-cutouts"),
                       (["--size", "1024", "--decimation", "4", "--out", "y"], "no recording")):
        r = subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr and r.stderr.startswith("fsea-cutouts: "), (args, r.stderr)
