"""CPU tier: event cut-outs without a GPU -- the argument checks of fsea_extract_* (before any device work, against a fake
object where a check must not look into the object beyond its decimation), their order, the no-op cases; fsea_extract_jobs
and fsea_extract_layout against the restatement of tests/extract_ref.py, field for field; the shipped fsea_extract_u8
kernels' resource usage; the restatement's own end-to-end check on the CPU; the job grid of tests/test_gpu_extract_domain.py
(domain_jobs: what it holds, asserted here) and the teeth of the reference that tier compares with; fsea-cutouts' usage
errors."""
import ctypes
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import extract_ref as R
from tests.conftest import ROOT
from tests.test_fir_host import fir_reference
from tests.test_gpu_fir import check
from tests.test_gpu_shift_domain import ABOVE, CPS, EVERYWHERE, PHASE0
from tests.test_gpu_zoom import lowpass_like_taps
from tests.test_iq_chain_host import shifted_samples as product_samples
from tests.test_shift_ref_host import GRID_CYCLES, GRID_PHASES, LIMIT, grid_positions
from tests.test_shipped_artifacts import LIB, _kernels
from tests.test_zoom_host import zoom_reference

FSEA_EINVAL = -1
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-cutouts")
ZT = fsea.ZOOM_TILE_OUTPUTS
DOMAIN_CASES = [(3, 21, 0), (25, 97, 1), (64, 512, 0)]          # (D, L, flip): one per LDS size, _s, _m, _l
RESIDUE_GROUPS = ("residues, high", "residues, low")


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


# ---- the job grid of tests/test_gpu_extract_domain.py: what it is for, and the teeth of its reference ------------------

def domain_lengths(D):
    """(n_long, n_tile, n_short): five outputs more than a tile and one sample over; one output more than a tile (two tiles)
    and two samples over; three outputs and seventeen samples over, so that a whole 16-byte group lies inside at any first."""
    return D * (ZT + 5) + 1, D * (ZT + 1) + 2, 3 * D + 17


def domain_jobs(D, L):
    """The jobs of one case over the argument domain check_shift admits per job -> ({group: [fsea.ExtractJob]}, n_iq).
      positions         n_long samples at every grid position with the three cycles and two phases of EVERYWHERE, and one job
                        with 2^32 in the middle of its second tile;
      grid across 2^31  n_tile samples, every GRID_CYCLES x GRID_PHASES;
      grid, last call   the same where sample_offset + n_samples == 2^52;
      residues, high    n_short samples, first = a + 8 k, sample_offset = 2^40 + r for all (a, r) in 0 .. 7 x 0 .. 7;
      residues, low     the same at sample_offset = r: the first group's base lies in front of stream position 0.
    Outside the residue groups `first` walks 0 .. 15, so the jobs overlap in a recording of n_long + 21 samples.  The grid does
    not depend on L; the argument is the case's."""
    n_long, n_tile, n_short = domain_lengths(D)
    walk = itertools.count()

    def job(n, offset, cps, phase0, first=None):
        return fsea.ExtractJob(next(walk) % 16 if first is None else first, n, offset, cps, phase0, 0)

    groups = {"positions": [job(n_long, p, c, ph) for p in grid_positions(n_long) for c, ph in EVERYWHERE]}
    groups["positions"].append(job(n_long, (1 << 32) - (ZT * D + (n_long - ZT * D) // 2), CPS, PHASE0))
    at = grid_positions(n_tile)
    for name, p in (("grid across 2^31", at[2]), ("grid, last call", at[5])):
        groups[name] = [job(n_tile, p, c, ph) for c in GRID_CYCLES for ph in GRID_PHASES]
    for name, base in zip(RESIDUE_GROUPS, (ABOVE, 0)):
        groups[name] = [job(n_short, base + r, CPS, PHASE0, first=a + 8 * ((a + r) & 1)) for a in range(8) for r in range(8)]
    return groups, n_long + 21


def domain_calls(groups):
    """The grid as three calls.  The call-wide relative bound of tests/test_gpu_fir.py rests on rms(y) >= ~0.3, which a call
    of residue jobs alone (three to eight outputs each on a fresh tail, most of them run-in) does not have: the residue groups
    share a call with long jobs."""
    return [groups["positions"] + groups["residues, high"], groups["grid across 2^31"] + groups["residues, low"],
            groups["grid, last call"]]


def phase_key(j):
    """what shift_ref.exact_turns is cached on"""
    return (j.cycles_per_sample, j.phase0_cycles, j.sample_offset, j.n_samples)


@pytest.mark.parametrize("D,L,flip", DOMAIN_CASES)
def test_the_domain_grid_holds_what_it_is_for(D, L, flip):
    groups, n_iq = domain_jobs(D, L)
    n_long, n_tile, n_short = domain_lengths(D)
    jobs = [j for g in groups.values() for j in g]
    assert all(j.first + j.n_samples <= n_iq and j.sample_offset + j.n_samples <= LIMIT and j.n_samples // D >= 3 for j in jobs)
    assert sorted(map(id, jobs)) == sorted(id(j) for call in domain_calls(groups) for j in call)      # every job is in one call
    assert {j.first for j in jobs if j.n_samples != n_short} == set(range(16))
    assert n_long // D == ZT + 5 and n_tile // D == ZT + 1 and n_long % D and n_tile % D
    # both residue groups: all 64 pairs; every job holds a whole group of eight of the buffer (one 16-byte load) and begins
    # inside a group, but for first = 0 and 8, which end inside one
    for name in RESIDUE_GROUPS:
        g = groups[name]
        assert {(j.first % 8, j.sample_offset % 8) for j in g} == set(itertools.product(range(8), range(8))) and len(g) == 64
        assert all(j.sample_offset < 8 for j in g) == (name == "residues, low") and all(j.first < 16 for j in g)
        for j in g:
            end = j.first + j.n_samples
            assert -(-j.first // 8) * 8 + 8 <= end, (name, j.first, "no whole group")
            assert j.first % 8 or end % 8, (name, j.first, "neither end is ragged")
    assert all(j.sample_offset >= (1 << 40) for j in groups["residues, high"])
    # 2^32 strictly inside a job, inside a tile of it: the added job has it in the middle of its second tile
    j = groups["positions"][-1]
    k = (1 << 32) - j.sample_offset
    assert ZT * D < k < j.n_samples == n_long and k % (ZT * D) == (n_long - ZT * D) // 2 != 0
    assert sum(1 for j in jobs if j.sample_offset < (1 << 32) < j.sample_offset + j.n_samples) >= 1
    assert sum(1 for j in jobs if j.sample_offset < (1 << 31) < j.sample_offset + j.n_samples) >= 60
    # the last admissible job, in both lengths
    assert {j.n_samples for j in jobs if j.sample_offset + j.n_samples == LIMIT} == {n_long, n_tile}
    for name in ("grid across 2^31", "grid, last call"):
        assert {(j.cycles_per_sample, j.phase0_cycles) for j in groups[name]} >= set(itertools.product(GRID_CYCLES, GRID_PHASES))
        assert len(groups[name]) == len(GRID_CYCLES) * len(GRID_PHASES) == 60
    assert {(j.cycles_per_sample, j.phase0_cycles) for j in groups["positions"]} == set(EVERYWHERE)
    assert {j.sample_offset for j in groups["positions"][:-1]} == set(grid_positions(n_long))
    # The exact phase is a Python loop per sample, cached on phase_key: no two jobs share a key but the eight firsts of a
    # residue, which must (the residue is the offset's), and then the second costs nothing
    long_keys = [phase_key(j) for name, g in groups.items() if name not in RESIDUE_GROUPS for j in g]
    assert len(set(long_keys)) == len(long_keys)
    for name in RESIDUE_GROUPS:
        assert len({phase_key(j) for j in groups[name]}) == 8
    steps = sum(k[3] for k in {phase_key(j) for j in jobs})
    print("D = %d: %d jobs, %d samples of exact phase" % (D, len(jobs), steps))
    assert steps == 37 * n_long + 120 * n_tile + 16 * n_short


def product_cutout(iq, job, taps, D, flip):
    """cutout_reference with the phase as ONE rounded double product (tests/test_iq_chain_host.py: shifted_samples): the
    error a kernel has whose phase reduction is a plain multiplication"""
    part = iq[2 * job.first:2 * (job.first + job.n_samples)]
    x = product_samples(part, flip, job.cycles_per_sample, job.phase0_cycles, job.sample_offset)
    y = fir_reference(x, taps)[0]
    return y[::D][:job.n_samples // D]


def test_the_cutout_reference_has_teeth_through_the_bounds_of_the_gpu_tier():
    """Reference against reference through tests/test_gpu_fir.py's check, the comparison of the GPU tier: a two-tile job at
    cycles -0.12 and position 2^44 against the same job one stream position on (a slip of o, of a group base or of the step
    table is at least that), and against the single rounded product (1.2e-4 cycles there,
    test_the_product_restatement_is_no_judge_at_2_to_the_44).  Both fail; if either passed, the comparison of
    tests/test_gpu_extract_domain.py would judge nothing."""
    D, L, flip = 3, 21, 0
    c = lowpass_like_taps(L, 5)
    n = domain_lengths(D)[1]
    iq = np.random.default_rng(44).integers(0, 256, 2 * (n + 5), dtype=np.uint8)
    j = fsea.ExtractJob(5, n, 1 << 44, CPS, PHASE0, 0)
    assert CPS == -0.12 and n // D == ZT + 1
    want = R.cutout_reference(iq, j, c, D, flip)
    assert want.size == ZT + 1 and want.dtype == np.complex128
    check(want.astype(np.complex64), want, "the reference rounded to f32 passes")
    check(product_cutout(iq, fsea.ExtractJob(5, n, 0, CPS, PHASE0, 0), c, D, flip),
          R.cutout_reference(iq, fsea.ExtractJob(5, n, 0, CPS, PHASE0, 0), c, D, flip), "at position 0 the product is good")
    one_on = fsea.ExtractJob(5, n, (1 << 44) + 1, CPS, PHASE0, 0)
    for name, other in (("sample_offset + 1", R.cutout_reference(iq, one_on, c, D, flip)), ("one rounded product", product_cutout(iq, j, c, D, flip))):
        print(name, "max |delta| %.3e, relative L2 %.3e" % (np.abs(other - want).max(), np.linalg.norm(other - want) / np.linalg.norm(want)))
        with pytest.raises(AssertionError):
            check(other, want, name)
    # the reference of a job is the job's own: an empty job, one shorter than D, a record of the restatement's dtype
    assert R.cutout_reference(iq, fsea.ExtractJob(3, 0, 7, CPS, 0.0, 0), c, D, flip).size == 0
    assert R.cutout_reference(iq, fsea.ExtractJob(3, D - 1, 7, CPS, 0.0, 0), c, D, flip).size == 0
    rec = np.zeros((), R.JOB)
    rec["first"], rec["n_samples"], rec["sample_offset"], rec["cycles_per_sample"], rec["phase0_cycles"] = 5, n, 1 << 44, CPS, PHASE0
    assert np.array_equal(R.cutout_reference(iq, rec[()], c, D, flip), want)


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
