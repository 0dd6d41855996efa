"""CPU tier: cut-out spectra without a GPU -- the header's constants and records against the binding; the restatement
tests/spectra_ref.py on signals whose spectra are known (a tone at an exact bin, Parseval, the nonlinear lines of PSK);
fsea_spectra_finish against the literal loop; fsea_spectra_jobs, _segments and _layout against their formulas; the
refusals of fsea_spectra_create and fsea_spectra_run_* in the header's order, against a fake object (the checks read
nothing of it but n and hop), and every text byte for byte against tests/golden/spectra_messages.json; the shipped kernels'
resource usage; fsea-cutouts' new usage errors."""
import ctypes
import json
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import measure_ref as M
from tests import spectra_ref as R
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-cutouts")
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectra_messages.json")
RESULT_FIELDS = ("total", "centroid_cycles", "obw_centre_cycles", "peak_power", "peak_cycles", "floor", "line_db", "obw_lo", "obw_hi",
                 "obw_bins", "peak_bin")
NAMES = ["fsea_spectra_create", "fsea_spectra_destroy", "fsea_spectra_finish", "fsea_spectra_hop", "fsea_spectra_jobs", "fsea_spectra_kind",
         "fsea_spectra_layout", "fsea_spectra_n", "fsea_spectra_run_device", "fsea_spectra_run_host", "fsea_spectra_segments"]


def test_header_constants_and_records_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()

    def define(name):
        return int(re.search(r"#define FSEA_SPECTRA_%s\s+(\d+)" % name, text).group(1))

    assert [define(k) for k in ("Z", "ENVELOPE", "SQUARE", "FOURTH")] == [fsea.SPECTRA_Z, fsea.SPECTRA_ENVELOPE, fsea.SPECTRA_SQUARE,
                                                                         fsea.SPECTRA_FOURTH] == list(R.KINDS) == [0, 1, 2, 3]
    assert sorted(fsea.SPECTRA_KINDS.items(), key=lambda kv: kv[1]) == [("z", 0), ("env", 1), ("sq", 2), ("fourth", 3)]
    assert (define("MIN_N"), define("MAX_N")) == (fsea.SPECTRA_MIN_N, fsea.SPECTRA_MAX_N) == (64, 4096)
    assert define("TILE_SEGMENTS") == fsea.SPECTRA_TILE_SEGMENTS == R.TILE_SEGMENTS
    assert define("MAX_JOBS") == fsea.SPECTRA_MAX_JOBS == fsea.EXTRACT_MAX_JOBS
    assert re.search(r"#define FSEA_SPECTRA_MAX_PAIRS\s+\(1u << 24\)", text) and fsea.SPECTRA_MAX_PAIRS == 1 << 24
    ctype = {"uint64_t": "<u8", "double": "<f8", "int32_t": "<i4"}
    for c_name, binding, dtype, size in (("fsea_spectra_job", fsea.SpectraJob, R.JOB, 24), ("fsea_spectra_result", fsea.SpectraResult, None, 72)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % c_name, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for kind, names in re.findall(r"(uint64_t|double|int32_t)\s+([\w\s,]+);", body):
            fields += [(n.strip(), ctype[kind]) for n in names.split(",")]
        assert [n for n, _ in fields] == [n for n, _ in binding._fields_], c_name
        assert np.dtype(fields).itemsize == ctypes.sizeof(binding) == size, c_name
        if dtype is not None:
            assert np.dtype(fields) == dtype, c_name
    assert tuple(n for n, _ in fsea.SpectraResult._fields_) == RESULT_FIELDS
    assert sorted(n for n in fsea.EXPORTS if n.startswith("fsea_spectra_")) == NAMES
    L = fsea.hip_lib()
    for name in NAMES:
        assert getattr(L, name).argtypes == fsea.API[name][1], name


# ---- the restatement's teeth -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k0", [(64, 0), (64, 32), (256, 200), (4096, 4095), (1024, 513)])
def test_a_tone_at_an_exact_bin_gives_n_squared_a_squared_there_and_rounding_noise_elsewhere(n, k0):
    """e^(2 pi i (k0 - n/2) j / n) with amplitude A = 0.75: the f32 pairs carry the tone within 2^-24, so bin k0 holds
    n^2 A^2 within a few 1e-7 of itself and every other bin what the pairs' rounding leaves, below n A^2 2^-46 n."""
    amp = 0.75
    j = np.arange(3 * n)
    z = (amp * np.exp(2j * np.pi * ((k0 - n // 2) / n) * j)).astype(np.complex64)
    for hop in (n, n // 2, 1):
        P, scale = R.spectrum(z[:n + 4 * hop], n, hop, R.Z)
        assert P.shape == (n,) and abs(P[k0] / (n * n * amp * amp) - 1.0) < 1e-6 and abs(scale - P[k0]) < 1e-6 * P[k0]
        rest = np.delete(P, k0)
        assert rest.max() <= (n * amp * 2.0 ** -22) ** 2             # every pair within 2^-24 A of the tone, at worst all in line
    # the envelope of a tone is constant: all of it in the centre bin, exactly where the squares are exact
    P, _ = R.spectrum(z[:2 * n], n, n, R.ENVELOPE)
    assert np.argmax(P) == n // 2 and np.delete(P, n // 2).max() <= (n * 2.0 ** -21) ** 2


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("window", [None, "hann"])
def test_parseval(kind, window):
    """sum_k P[k] = n mean_s sum_j |x_j|^2 on the f32 inputs themselves, to f64 rounding."""
    n, hop = 256, 100
    z = R.qpsk_cutout(n + 9 * hop + 13)
    w = None if window is None else R.hann(n)
    P, _ = R.spectrum(z, n, hop, kind, w, 0.5 + 0.5j)
    x = R.inputs(z, n, hop, kind, w, 0.5 + 0.5j).astype(np.complex128)
    assert x.shape == (10, n)
    energy = float(np.mean(np.sum(x.real ** 2 + x.imag ** 2, axis=1)))
    assert abs(P.sum() / (n * energy) - 1.0) < 1e-13
    # the terms: the pedestal goes in f64 before the one rounding to f32; the sign is (-1)^j; the taper multiplies (u, v)
    a, b = R.terms(z, 0.5 + 0.5j)
    assert a.dtype == np.float32 and np.array_equal(a, (z.real.astype(np.float64) - 0.5).astype(np.float32))
    u, v = R.kind_of(a, b, kind)
    want = (u[hop:hop + n].astype(np.float64) + 1j * v[hop:hop + n].astype(np.float64)) * np.where(np.arange(n) % 2, -1.0, 1.0)
    if w is not None:
        want = (w * u[hop:hop + n]).astype(np.float64) + 1j * (w * v[hop:hop + n]).astype(np.float64)
        want = want * np.where(np.arange(n) % 2, -1.0, 1.0)
    assert np.array_equal(x[1], want)


def test_the_kinds_are_the_headers_expressions():
    a = np.array([3.0, 1.0 + 2.0 ** -12, -0.5, 1e-20], np.float32)
    b = np.array([4.0, 1.0 - 2.0 ** -12, 0.25, 1e10], np.float32)
    f = np.float32
    with np.errstate(over="ignore"):
        u, v = R.kind_of(a, b, R.ENVELOPE)
        assert np.array_equal(u, [f(f(x * x) + f(y * y)) for x, y in zip(a, b)]) and np.all(v.view(np.uint32) == 0)
        u, v = R.kind_of(a, b, R.SQUARE)
        assert np.array_equal(u, [f(f(x * x) - f(y * y)) for x, y in zip(a, b)]) and np.array_equal(v, [f(f(2) * f(x * y)) for x, y in zip(a, b)])
        u4, v4 = R.kind_of(a, b, R.FOURTH)
        assert np.array_equal(u4, [f(f(x * x) - f(y * y)) for x, y in zip(u, v)]) and np.array_equal(v4, [f(f(2) * f(x * y)) for x, y in zip(u, v)])
    assert u[0] == -7.0 and v[0] == 24.0 and u4[0] == 49.0 - 576.0 and u[1] != np.float32(np.float64(a[1]) ** 2 - np.float64(b[1]) ** 2)


def line_of(pairs, n, kind, guard=2):
    P, _ = R.spectrum(pairs, n, n // 2, kind, R.hann(n))
    return R.finish(P.astype(np.float32), guard, 0.99)


def test_the_nonlinear_lines_of_psk_stand_where_the_theory_puts_them():
    """QPSK at 8 pairs a symbol, its carrier f off the centre: z^4 has its line at 4 f and |z|^2 at the symbol rate, 1 / 8
    cycles per pair (a real sequence: both signs, the lower bin is named); BPSK: z^2 at 2 f.  And not the other way round:
    the square of QPSK has no line: finish finds 10 dB less there."""
    n, f = 1024, 0.03125                                  # f n = 32: whole bins, so `within a bin` is exact here
    rng = np.random.default_rng(3)
    noise = 0.05 * (rng.normal(0, 1, 40 * n) + 1j * rng.normal(0, 1, 40 * n))
    qpsk = (R.psk(40 * n, 4, 8, f) + noise).astype(np.complex64)
    bpsk = (R.psk(40 * n, 2, 8, f) + noise).astype(np.complex64)
    fourth, envelope, square = line_of(qpsk, n, R.FOURTH), line_of(qpsk, n, R.ENVELOPE), line_of(bpsk, n, R.SQUARE)
    print(fourth, envelope, square)
    assert fourth["peak_cycles"] == 4 * f and fourth["line_db"] > 30
    assert abs(envelope["peak_cycles"]) == 1 / 8 and envelope["peak_bin"] == n // 2 - n // 8 and envelope["line_db"] > 30
    assert square["peak_cycles"] == 2 * f and square["line_db"] > 30
    # the square of QPSK is BPSK still and has none: what finish names there is the crest of a continuous spectrum over its median
    assert line_of(qpsk, n, R.SQUARE)["line_db"] < fourth["line_db"] - 10
    # the plain spectrum: its centroid is the carrier, its occupied band a few symbol rates round it
    plain = line_of(qpsk, n, R.Z, 0)
    assert abs(plain["centroid_cycles"] - f) < 0.01 and abs(plain["obw_centre_cycles"] - f) < 0.02 and 1 / 8 < plain["obw_bins"] / n < 0.6


@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
def test_the_closed_forms_the_gpu_tier_expects_are_the_restatements(n):
    """tests/test_gpu_spectra.py holds the device to constant_spectrum and impulse_spectrum bit for bit.  Here, without a GPU:
    the restatement gives the exact (float64) forms within 1e-12 of the peak in every bin, and the float32 forms are those
    rounded once -- for z^4, u u + v v = 17850625 / 65536 needs 25 bits, so its f32 form stands 2^-25 off the exact value."""
    offset, hop, S = 0.5 + 0.5j, 5, 4
    for kind in R.KINDS:
        got, scale = R.spectrum(R.constant_pairs(n + (S - 1) * hop, offset), n, hop, kind, None, offset)
        exact, want = R.constant_spectrum(n, kind, np.float64), R.constant_spectrum(n, kind)
        u, v = R.kind_of(np.float32([2.0]), np.float32([-0.25]), kind)
        assert want.dtype == np.float32 and want[n // 2] == np.float32(n) ** 2 * (u[0] * u[0] + v[0] * v[0])
        assert exact[n // 2] == float(n) ** 2 * (float(u[0]) ** 2 + float(v[0]) ** 2) and np.count_nonzero(exact) == np.count_nonzero(want) == 1
        assert got.shape == (n,) and np.max(np.abs(got - exact)) <= 1e-12 * exact[n // 2] and abs(scale / exact[n // 2] - 1.0) <= 1e-12
        assert np.array_equal(exact.astype(np.float32), want) and not np.any(np.signbit(want))
        assert (exact[n // 2] == want[n // 2]) == (kind != R.FOURTH)
    got, _ = R.spectrum(R.impulse_pairs(n, offset), n, hop, R.Z, None, offset)
    assert np.max(np.abs(got - 20.0)) <= 20.0 * 1e-12
    assert np.array_equal(R.impulse_spectrum(n), np.full(n, 20.0, np.float32)) and np.all(R.impulse_spectrum(n, np.float64) == 20.0)


# ---- fsea_spectra_finish -----------------------------------------------------------------------------------------------------

def same(a, b):
    return a == b or (a != a and b != b)


def check_finish(power, guard, fraction):
    got, want = fsea.spectra_finish(power, guard, fraction), R.finish(power, guard, fraction)
    for name in RESULT_FIELDS:
        assert same(getattr(got, name), want[name]), (name, getattr(got, name), want[name], guard, fraction)
    return want


def test_finish_is_the_literal_loop():
    n = 256
    rows = [R.spectrum(R.qpsk_cutout(6 * n), n, n // 2, kind, R.hann(n), 0.5 + 0.5j)[0].astype(np.float32) for kind in R.KINDS]
    rows.append(R.spectrum(R.noise_cutout(6 * n), n, n, R.Z)[0].astype(np.float32))
    one = np.zeros(n, np.float32)
    one[77] = 3.5
    for row in rows + [one, np.zeros(n, np.float32), np.ones(64, np.float32)]:
        for guard in (-1, 0, 2, row.size // 2 - 1):
            for fraction in (0.5, 0.99, 1.0):
                check_finish(row, guard, fraction)
    # one bin: the band is that bin, the centroid its frequency; the floor is 0 and the line infinitely high
    r = check_finish(one, 0, 0.99)
    assert (r["obw_lo"], r["obw_hi"], r["obw_bins"], r["peak_bin"]) == (77, 77, 1, 77) and r["centroid_cycles"] == (77 - 128) / n
    assert r["obw_centre_cycles"] == (77 - 128) / n and r["floor"] == 0.0 and r["line_db"] == math.inf and r["total"] == 3.5
    # silence: no band, NaN ratios, FSEA_OK
    r = check_finish(np.zeros(n, np.float32), 2, 0.99)
    assert math.isnan(r["centroid_cycles"]) and math.isnan(r["line_db"]) and math.isnan(r["obw_centre_cycles"])
    assert (r["obw_lo"], r["obw_hi"], r["obw_bins"], r["total"]) == (-1, -1, 0, 0.0)
    # the guard: the strongest bin in the centre is passed over; with the widest guard bin 0 alone is left
    row = np.arange(1, n + 1, dtype=np.float32)
    row[n // 2] = 1e6
    row[n // 2 + 2] = 5e5
    assert check_finish(row, -1, 0.99)["peak_bin"] == n // 2 and check_finish(row, 0, 0.99)["peak_bin"] == n // 2 + 2
    assert check_finish(row, 2, 0.99)["peak_bin"] == n - 1
    r = check_finish(row, n // 2 - 1, 0.99)
    assert r["peak_bin"] == 0 and r["floor"] == 1.0 and r["line_db"] == 0.0
    # equal maxima: the lowest bin; the lower median of an even count
    row = np.ones(64, np.float32)
    row[[5, 40]] = 9.0
    r = check_finish(row, -1, 1.0)
    assert r["peak_bin"] == 5 and r["floor"] == 1.0 and (r["obw_lo"], r["obw_hi"]) == (0, 63)
    assert check_finish(np.array([1.0, 2.0] * 32, np.float32), -1, 0.5)["floor"] == 1.0      # 32 ones, 32 twos: the lower median
    assert check_finish(np.array([1.0, 2.0] * 32, np.float32), 0, 0.5)["floor"] == 2.0       # without the centre's one: 31 and 32
    # a NaN among the powers: no band, no crash
    row = np.ones(64, np.float32)
    row[9] = np.nan
    r = check_finish(row, 0, 0.99)
    assert r["obw_bins"] == 0 and math.isnan(r["total"])


def test_finish_refuses_bad_arguments_in_order():
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    row = np.ones(64, np.float32)
    out = fsea.SpectraResult()
    p, r = row.ctypes.data, ctypes.byref(out)
    assert L_.fsea_spectra_finish(None, 63, 99, 0.0, r) == FSEA_EINVAL and b"NULL buffer" in err()
    assert L_.fsea_spectra_finish(p, 63, 99, 0.0, None) == FSEA_EINVAL and b"NULL buffer" in err()
    for n in (0, 32, 63, 96, 8192, -64):
        assert L_.fsea_spectra_finish(p, n, 99, 0.0, r) == FSEA_EINVAL and b"n must be a power of two in [64, 4096]" in err()
    for g in (-2, 32, 99):
        assert L_.fsea_spectra_finish(p, 64, g, 0.0, r) == FSEA_EINVAL and b"guard_bins must be in [-1, 31]" in err()
    for f in (0.0, -0.5, 1.0000001, np.nan, np.inf):
        assert L_.fsea_spectra_finish(p, 64, 31, f, r) == FSEA_EINVAL and b"fraction must be in (0, 1]" in err()
    assert L_.fsea_spectra_finish(p, 64, 31, 1.0, r) == 0 and out.total == 64.0


# ---- jobs, segments, layout ----------------------------------------------------------------------------------------------------

def fake_object(n=256, hop=128, kind=0):
    """the struct begins `int n; int hop; int kind; int device;` and the checks read n and hop alone"""
    fake = ctypes.create_string_buffer(4096)
    struct.pack_into("<iiii", fake, 0, n, hop, kind, 0)
    return fake


def table(*jobs):
    return (fsea.SpectraJob * len(jobs))(*[fsea.SpectraJob(*j) for j in jobs])


@pytest.mark.parametrize("n,hop", [(64, 1), (64, 64), (256, 100), (4096, 2048), (1024, 1023)])
def test_segments_and_layout_are_their_formulas(n, hop):
    L_ = fsea.hip_lib()
    fake = fake_object(n, hop, 3)
    f = ctypes.cast(fake, ctypes.c_void_p)
    assert (L_.fsea_spectra_n(f), L_.fsea_spectra_hop(f), L_.fsea_spectra_kind(f)) == (n, hop, 3)
    ns = [0, n - 1, n, n + hop - 1, n + hop, 0, 5 * n + 3, 1 << 24, n - 1, n]
    want = [0, 0, 1, 1, 2]
    assert [L_.fsea_spectra_segments(f, m) for m in ns[:5]] == want == [R.segments(m, n, hop) for m in ns[:5]]
    assert L_.fsea_spectra_segments(f, 1 << 24) == ((1 << 24) - n) // hop + 1 and L_.fsea_spectra_segments(None, 1 << 24) == 0
    tab = table(*[(5 * i, m, 12345) for i, m in enumerate(ns)])
    total = ctypes.c_size_t(99)
    assert L_.fsea_spectra_layout(f, ctypes.addressof(tab), len(tab), ctypes.byref(total)) == 0
    firsts, floats = R.layout(ns, n, hop)
    assert [j.out_first for j in tab] == firsts and total.value == floats == 6 * n
    assert firsts[:6] == [0, 0, 0, n, 2 * n, 3 * n]                 # a job without a segment: the running position and no room
    assert [(j.first_pair, j.n_pairs) for j in tab] == [(5 * i, m) for i, m in enumerate(ns)]
    assert L_.fsea_spectra_layout(f, None, 0, ctypes.byref(total)) == 0 and total.value == 0


def test_layout_refusals_and_the_getters_of_null():
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    fake = fake_object()
    f = ctypes.cast(fake, ctypes.c_void_p)
    tab, total = table((0, 300, 0)), ctypes.c_size_t()
    assert L_.fsea_spectra_layout(None, ctypes.addressof(tab), 1, ctypes.byref(total)) == FSEA_EINVAL and b"spectra is NULL" in err()
    assert L_.fsea_spectra_layout(f, ctypes.addressof(tab), 1, None) == FSEA_EINVAL and b"total_floats is NULL" in err()
    assert L_.fsea_spectra_layout(f, ctypes.addressof(tab), fsea.SPECTRA_MAX_JOBS + 1, ctypes.byref(total)) == FSEA_EINVAL and b"n_jobs" in err()
    assert L_.fsea_spectra_layout(f, None, 1, ctypes.byref(total)) == FSEA_EINVAL and b"NULL job table" in err()
    assert (L_.fsea_spectra_n(None), L_.fsea_spectra_hop(None), L_.fsea_spectra_kind(None)) == (0, 0, -1)


def test_jobs_are_the_twin_of_the_measures():
    ejobs = [fsea.ExtractJob(0, 4096, 0, 0.0, 0.0, 0), fsea.ExtractJob(0, 100, 0, 0.0, 0.0, 256), fsea.ExtractJob(0, 15, 0, 0.0, 0.0, 262),
             fsea.ExtractJob(0, 16 * 300 + 7, 0, 0.0, 0.0, 262)]
    for d, skip in ((16, 6), (16, 0), (1, 50), (3, 1 << 30)):
        got = fsea.spectra_jobs(ejobs, d, skip)
        want, twin = R.spectra_jobs(ejobs, d, skip), M.measure_jobs(ejobs, d, skip)
        assert [(j.first_pair, j.n_pairs, j.out_first) for j in got] == [tuple(int(v) for v in w) for w in want]
        assert [(j.first_pair, j.n_pairs) for j in got] == [tuple(int(v) for v in w) for w in twin] and all(j.out_first == 0 for j in got)
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    long = (fsea.ExtractJob * 1)(fsea.ExtractJob(0, (1 << 24) + 8, 0, 0.0, 0.0, 0))
    out = (fsea.SpectraJob * 1)()
    assert L_.fsea_spectra_jobs(ctypes.addressof(long), 1, 1, 7, ctypes.addressof(out)) == FSEA_EINVAL and b"job 0: 16777217 pairs" in err()
    assert L_.fsea_spectra_jobs(ctypes.addressof(long), 1, 1, 8, ctypes.addressof(out)) == 0 and out[0].n_pairs == 1 << 24
    assert L_.fsea_spectra_jobs(ctypes.addressof(long), 1, 0, 0, ctypes.addressof(out)) == FSEA_EINVAL and b"decimation" in err()
    assert L_.fsea_spectra_jobs(None, 1, 1, 0, ctypes.addressof(out)) == FSEA_EINVAL and b"NULL job table" in err()
    assert L_.fsea_spectra_jobs(None, fsea.SPECTRA_MAX_JOBS + 1, 0, 0, None) == FSEA_EINVAL and b"n_jobs" in err()
    assert L_.fsea_spectra_jobs(None, 0, 1, 0, None) == 0


# ---- the refusals, in the header's order ------------------------------------------------------------------------------------------

def test_create_refuses_bad_arguments_in_order_before_it_looks_for_a_device():
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    h = ctypes.c_void_p()
    w, bad = np.ones(4096, np.float32), np.ones(4096, np.float32)
    bad[3] = np.inf
    # every refusal with everything behind it in the order wrong as well: the earlier check speaks
    assert L_.fsea_spectra_create(None, 100, 0, 9, bad.ctypes.data, 99) == FSEA_EINVAL and b"out-pointer" in err()
    for n in (100, 32, 0, -64, 8192, 96):
        assert L_.fsea_spectra_create(ctypes.byref(h), n, 0, 9, bad.ctypes.data, 99) == FSEA_EINVAL and b"n must be a power of two in [64, 4096]" in err()
    for hop in (0, -1, 65):
        assert L_.fsea_spectra_create(ctypes.byref(h), 64, hop, 9, bad.ctypes.data, 99) == FSEA_EINVAL and b"hop must be in [1, 64]" in err()
    for kind in (-1, 4, 9):
        assert L_.fsea_spectra_create(ctypes.byref(h), 64, 64, kind, bad.ctypes.data, 99) == FSEA_EINVAL and b"kind must be" in err()
    assert L_.fsea_spectra_create(ctypes.byref(h), 64, 1, 3, bad.ctypes.data, 99) == FSEA_EINVAL and b"window weight 3 is not finite" in err()
    bad[3], bad[63] = 1.0, np.nan
    assert L_.fsea_spectra_create(ctypes.byref(h), 64, 1, 3, bad.ctypes.data, 99) == FSEA_EINVAL and b"window weight 63 is not finite" in err()
    assert not h.value and L_.fsea_spectra_destroy(None) == 0
    for window in (None, w.ctypes.data):
        rc = L_.fsea_spectra_create(ctypes.byref(h), 4096, 4096, 3, window, 0)
        if fsea.device_count() == 0:
            assert rc == -2 and not h.value                                                             # FSEA_ENODEVICE
        else:
            assert rc == 0 and L_.fsea_spectra_kind(h) == 3 and L_.fsea_spectra_destroy(h) == 0


P, P4, P1, S, S2, S1 = "P", "P+4", "P+1", "S", "S+2", "S+1"       # a 16-byte aligned host buffer and its second half, and off them
MAX, BIG = 65536, 1 << 40
NAN, INF = float("nan"), float("inf")
_ONE = ((0, 300, 0),)
_MANY = tuple((0, 1 << 24, 64 * i) for i in range(129))          # n = 64, hop = 64: 2^18 segments each, 2^24 points; 129 of them


def _run(obj=(256, 128), pairs=P, n_buffer=512, jobs=_ONE, n_jobs=None, off=(0.5, 0.5), power=S, n_power=1024):
    return (obj, pairs, n_buffer, jobs, (len(jobs) if jobs is not None else 0) if n_jobs is None else n_jobs, off[0], off[1], power, n_power)


# fsea_spectra_run_*(sp, pairs, n_buffer, jobs, n_jobs, offset_re, offset_im, power, n_power[, stream]); the fake object has
# n = 256 and hop = 128 where nothing else is said, the power 1024 floats
_RUN = [
    ("NULL object before the job count", _run(obj=None, n_jobs=MAX + 1, jobs=None, pairs=None, off=(NAN, 0.0))),
    ("n_jobs above the maximum", _run(n_jobs=MAX + 1, jobs=None, pairs=None, off=(NAN, 0.0))),
    ("no jobs", ((256, 128), None, 0, None, 0, NAN, 0.0, None, 0)),
    ("no jobs, whatever else", ((256, 128), P4, 7, None, 0, 0.0, 0.0, S1, 0)),
    ("NULL job table", _run(jobs=None, n_jobs=1, pairs=None, off=(NAN, 0.0))),
    ("NULL input before the offset", _run(pairs=None, off=(NAN, 0.0))),
    ("NULL output before the offset", _run(power=None, off=(NAN, 0.0))),
    ("offset nan before a span", _run(off=(NAN, 0.0), jobs=((600, 1, 0),))),
    ("offset inf before a span", _run(off=(0.0, INF), jobs=((600, 1, 0),))),
    ("offset -inf before a span", _run(off=(-INF, 0.0), jobs=((600, 1, 0),))),
    ("job 1 past the buffer", _run(jobs=((0, 300, 0), (500, 13, 256)))),
    ("first past the buffer", _run(jobs=((BIG, 1, 0),))),
    ("first + n wraps", _run(jobs=((2, (1 << 64) - 1, 0),))),
    ("n_pairs too large", _run(jobs=((0, (1 << 24) + 1, 0),), n_buffer=BIG)),
    ("powers one past n_power", _run(jobs=((0, 300, 769),))),
    ("out_first past n_power", _run(jobs=((0, 300, BIG),))),
    ("out_first + n wraps", _run(jobs=((0, 300, (1 << 64) - 3),))),
    ("more powers than n_power", _run(n_power=255)),
    ("a job without a segment has no place to check", _run(jobs=((0, 255, BIG), (600, 1, 0)))),
    ("a span before placement, one job", _run(jobs=((500, 300, 5000),))),
    ("a span before placement, table order", _run(jobs=((0, 300, 2000), (BIG, 1, 0)), n_power=2256)),
    ("placement before a later span", _run(jobs=((0, 300, 2000), (BIG, 1, 0)))),
    ("jobs 0 and 2 overlap", _run(jobs=((0, 300, 100), (0, 255, 100), (64, 256, 355), (0, 0, 101)))),
    ("jobs 1 and 2 overlap", _run(jobs=((0, 300, 600), (8, 256, 50), (64, 400, 50)))),
    ("n_power before overlap", _run(jobs=((0, 300, 1200), (0, 300, 0), (64, 300, 255)))),
    ("overlap before alignment", _run(jobs=((0, 300, 356), (64, 300, 101)), pairs=P4)),
    ("the total before alignment", _run(obj=(64, 64), jobs=_MANY, n_buffer=BIG, n_power=BIG, pairs=P4)),
    ("overlap before the total", _run(obj=(64, 64), jobs=_MANY + ((0, 64, 5),), n_buffer=BIG, n_power=BIG)),
]
_DEV, _HOST = ("_device", (None,)), ("_host", ())
_EMPTY = ((0, 300, 0), (0, 255, 5), (0, 0, 1 << 50))               # jobs without a segment take no room, anywhere
_W, _WB, H, N_ = "W", "WB", "H", "N"                                # 4096 weights of 1.0; the same with an inf as weight 3; a handle; a size_t
_EJ = ("E", ((0, 64, 0, 0.0, 0.0, 0), (0, (1 << 24) + 8, 0, 0.0, 0.0, 0)))
_SJ = ("J", ((0, 0, 0), (0, 0, 0)))

CASES = (
    [("fsea_spectra_run%s: %s" % (suffix, label), "fsea_spectra_run" + suffix, tuple(args) + tail) for suffix, tail in (_DEV, _HOST)
     for label, args in _RUN]
    + [("fsea_spectra_run_device: alignment behind the jobs' checks", "fsea_spectra_run_device", _run(jobs=_EMPTY, pairs=P4) + (None,)),
       ("fsea_spectra_run_device: input off 8 bytes", "fsea_spectra_run_device", _run(pairs=P4) + (None,)),
       ("fsea_spectra_run_device: output off 4 bytes by 2", "fsea_spectra_run_device", _run(power=S2) + (None,)),
       ("fsea_spectra_run_device: input off 1 byte", "fsea_spectra_run_device", _run(pairs=P1) + (None,)),
       ("fsea_spectra_run_device: output off 1 byte", "fsea_spectra_run_device", _run(power=S1) + (None,)),
       ("fsea_spectra_run_device: 2^31 points pass, the alignment speaks", "fsea_spectra_run_device",
        _run(obj=(64, 64), jobs=_MANY[:128], n_buffer=BIG, n_power=BIG, pairs=P4) + (None,)),
       ("fsea_spectra_layout: fine", "fsea_spectra_layout", ((256, 128), _EMPTY, 3, N_)),
       ("fsea_spectra_layout: NULL object", "fsea_spectra_layout", (None, _ONE, 1, N_)),
       ("fsea_spectra_layout: NULL total_floats", "fsea_spectra_layout", ((256, 128), _ONE, 1, None)),
       ("fsea_spectra_layout: NULL job table", "fsea_spectra_layout", ((256, 128), None, 1, N_)),
       ("fsea_spectra_layout: n_jobs above the maximum", "fsea_spectra_layout", ((256, 128), _ONE, MAX + 1, N_)),
       ("fsea_spectra_layout: total_floats before n_jobs", "fsea_spectra_layout", ((256, 128), None, MAX + 1, None)),
       ("fsea_spectra_layout: object before total_floats", "fsea_spectra_layout", (None, None, MAX + 1, None)),
       ("fsea_spectra_layout: no jobs", "fsea_spectra_layout", ((256, 128), None, 0, N_)),
       # fsea_spectra_create(out, n, hop, kind, window, device): every refusal with everything behind it wrong as well
       ("fsea_spectra_create: NULL out-pointer", "fsea_spectra_create", (None, 100, 0, 9, _WB, 99)),
       ("fsea_spectra_create: n 100", "fsea_spectra_create", (H, 100, 0, 9, _WB, 99)),
       ("fsea_spectra_create: n 32", "fsea_spectra_create", (H, 32, 0, 9, _WB, 99)),
       ("fsea_spectra_create: n 8192", "fsea_spectra_create", (H, 8192, 0, 9, _WB, 99)),
       ("fsea_spectra_create: n -64", "fsea_spectra_create", (H, -64, 0, 9, _WB, 99)),
       ("fsea_spectra_create: hop 0", "fsea_spectra_create", (H, 64, 0, 9, _WB, 99)),
       ("fsea_spectra_create: hop 65", "fsea_spectra_create", (H, 64, 65, 9, _WB, 99)),
       ("fsea_spectra_create: hop 4097", "fsea_spectra_create", (H, 4096, 4097, 9, _WB, 99)),
       ("fsea_spectra_create: kind 4", "fsea_spectra_create", (H, 64, 64, 4, _WB, 99)),
       ("fsea_spectra_create: kind -1", "fsea_spectra_create", (H, 64, 64, -1, _WB, 99)),
       ("fsea_spectra_create: weight 3 inf", "fsea_spectra_create", (H, 64, 64, 3, _WB, 99)),
       ("fsea_spectra_jobs: too many pairs", "fsea_spectra_jobs", (_EJ, 2, 1, 7, _SJ)),
       ("fsea_spectra_jobs: fine", "fsea_spectra_jobs", (_EJ, 2, 1, 8, _SJ)),
       ("fsea_spectra_jobs: decimation 0", "fsea_spectra_jobs", (_EJ, 2, 0, 0, _SJ)),
       ("fsea_spectra_jobs: NULL extract jobs", "fsea_spectra_jobs", (None, 2, 1, 0, _SJ)),
       ("fsea_spectra_jobs: NULL jobs", "fsea_spectra_jobs", (_EJ, 2, 1, 0, None)),
       ("fsea_spectra_jobs: n_jobs above the maximum", "fsea_spectra_jobs", (_EJ, MAX + 1, 1, 0, _SJ)),
       ("fsea_spectra_jobs: no jobs", "fsea_spectra_jobs", (None, 0, 1, 0, None)),
       # fsea_spectra_finish(power, n, guard_bins, fraction, result); R: a result to write to
       ("fsea_spectra_finish: NULL power", "fsea_spectra_finish", (None, 63, 99, 0.0, "R")),
       ("fsea_spectra_finish: NULL result", "fsea_spectra_finish", (_W, 63, 99, 0.0, None)),
       ("fsea_spectra_finish: n 63", "fsea_spectra_finish", (_W, 63, 99, 0.0, "R")),
       ("fsea_spectra_finish: guard 32 of 64", "fsea_spectra_finish", (_W, 64, 32, 0.0, "R")),
       ("fsea_spectra_finish: guard -2", "fsea_spectra_finish", (_W, 64, -2, 0.0, "R")),
       ("fsea_spectra_finish: fraction 0", "fsea_spectra_finish", (_W, 64, 31, 0.0, "R")),
       ("fsea_spectra_finish: fraction nan", "fsea_spectra_finish", (_W, 64, 31, NAN, "R")),
       ("fsea_spectra_finish: fine", "fsea_spectra_finish", (_W, 64, 31, 1.0, "R"))]
)
IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)


def call(case):
    """(code, text): what the case's call returns and, where that is an error, fsea_last_error_string() behind it"""
    _, name, args = case
    L = fsea.hip_lib()
    buf = np.full(8192 + 16, 0x5A, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    n = ctypes.c_size_t(77)
    handle, result = ctypes.c_void_p(), fsea.SpectraResult()
    w, bad = np.ones(4096, np.float32), np.ones(4096, np.float32)
    bad[3] = np.inf
    values = {P: p, P4: p + 4, P1: p + 1, S: p + 4096, S2: p + 4096 + 2, S1: p + 4096 + 1, N_: ctypes.byref(n), H: ctypes.byref(handle),
              _W: w.ctypes.data, _WB: bad.ctypes.data, "R": ctypes.byref(result)}
    alive = []

    def value(a, position):
        if isinstance(a, str):
            return values[a]
        if not isinstance(a, tuple):
            return a
        if position == 0 and len(a) == 2 and isinstance(a[0], int):          # a fake object (n, hop)
            alive.append(fake_object(*a))
            return ctypes.cast(alive[-1], ctypes.c_void_p)
        if a and a[0] in ("E", "J"):
            kind, rows = (fsea.ExtractJob, a[1]) if a[0] == "E" else (fsea.SpectraJob, a[1])
        else:
            kind, rows = fsea.SpectraJob, a
        alive.append((kind * len(rows))(*[kind(*j) for j in rows]))
        return ctypes.addressof(alive[-1])

    code = getattr(L, name)(*[value(a, i) for i, a in enumerate(args)])
    assert np.all(buf == 0x5A) and not handle.value      # a refused call writes nothing, nor does one without jobs
    return [code, L.fsea_last_error_string().decode() if code else None]


@pytest.fixture(scope="module")
def golden():
    with open(TABLE) as f:
        return json.load(f)


def test_the_golden_table_is_the_cases_and_says_what_the_header_says(golden):
    assert sorted(golden) == sorted(IDS)
    for form in ("_device", "_host"):
        texts = " | ".join(t for k, (_, t) in golden.items() if k.startswith("fsea_spectra_run" + form + ":") and t)
        for part in ("spectra is NULL", "n_jobs 65537 above 65536", "NULL job table", "NULL buffer", "the offset is not finite", "lie past the",
                     "of the buffer", "of the power", "too large", "overlap", "points in one call: more than 2^31"):
            assert part in texts, (form, part)
        for label in ("no jobs", "no jobs, whatever else"):
            assert golden["fsea_spectra_run%s: %s" % (form, label)] == [0, None]
        # the order of the checks, through the cases that break two rules at once
        assert "offset" in golden["fsea_spectra_run%s: offset nan before a span" % form][1]
        assert "job 1: pairs" in golden["fsea_spectra_run%s: a job without a segment has no place to check" % form][1]
        assert "job 0: pairs" in golden["fsea_spectra_run%s: a span before placement, one job" % form][1]
        assert "job 0: outputs" in golden["fsea_spectra_run%s: placement before a later span" % form][1]
        assert "job 0: outputs" in golden["fsea_spectra_run%s: n_power before overlap" % form][1]
        assert "jobs 0 and 1 overlap" in golden["fsea_spectra_run%s: overlap before alignment" % form][1]
        assert "2164260864 points" in golden["fsea_spectra_run%s: the total before alignment" % form][1]
        assert "jobs 0 and 129 overlap" in golden["fsea_spectra_run%s: overlap before the total" % form][1]
    assert "aligned" in golden["fsea_spectra_run_device: 2^31 points pass, the alignment speaks"][1]
    assert all(code == FSEA_EINVAL for k, (code, _) in golden.items() if k.startswith("fsea_spectra_create:"))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_code_and_text(case, golden):
    assert call(case) == golden[case[0]]


# ---- the shipped kernels ------------------------------------------------------------------------------------------------------

# DESIGN.md section 4, "Cut-out spectra": two images of max(n, 1024) pairs; VGPRs read off the build: 44, 49, 50, 55, 64, 113, 212
TILES = {64: (16384, 64), 128: (16384, 64), 256: (16384, 64), 512: (16384, 64), 1024: (16384, 64), 2048: (32768, 128), 4096: (65536, 256)}


def test_shipped_library_has_the_spectra_kernels_within_their_budget():
    """From the code object's metadata alone: wave64, 256 lanes, no private segment, no spilled register; the LDS DESIGN.md
    states, so ten, five and two workgroups fit a CU's 160 KiB; VGPRs within the step that gives 8, 4 and 2 waves a SIMD."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    kernels = _kernels(LIB)
    for n, (lds, vgprs) in TILES.items():
        k = kernels["fsea_spectra_tiles_%d" % n]
        print(n, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
        assert k[".group_segment_fixed_size"] == lds == 2 * 8 * max(n, 1024) and k[".vgpr_count"] <= vgprs
    k = kernels["fsea_spectra_fold"]
    assert k[".group_segment_fixed_size"] == 0 and k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0
    assert k[".vgpr_count"] <= 32 and k[".max_flat_workgroup_size"] == 256
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("Cut-out spectra"):]
    for n, (lds, _) in TILES.items():
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*\|" % (n, lds), section), (n, lds)


def test_tool_knows_spectra_and_refuses_what_it_cannot_do():
    assert os.path.exists(TOOL), "fsea-cutouts not built"
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--spectra N [--spectra-hop H] [--spectra-kind z|env|sq|fourth] [--spectra-window NAME]" in r.stdout
    assert r.stdout.startswith("usage: fsea-cutouts FILE --size N --decimation D --out DIR [--hop H] [--window NAME] [--flip] [--mode db5|db10|db]\n")
    assert "--audio fm|am" in r.stdout and "` spectra P`" in r.stdout
    x = ["x.raw", "--size", "1024", "--out", "y", "--decimation", "4"]
    for extra, word in ((["--spectra", "100"], "--spectra must be a power of two in [64, 4096]"),
                        (["--spectra", "32"], "--spectra must be a power of two in [64, 4096]"),
                        (["--spectra", "8192"], "--spectra must be a power of two in [64, 4096]"),
                        (["--spectra", "256", "--spectra-hop", "257"], "--spectra-hop must be in [1, N]"),
                        (["--spectra", "256", "--spectra-hop", "-3"], "--spectra-hop must be in [1, N]"),
                        (["--spectra", "256", "--spectra-kind", "cube"], "--spectra-kind must be z, env, sq or fourth"),
                        (["--spectra", "256", "--spectra-window", "kaiser"], "--spectra-window must be rect, hann, hamming"),
                        (["--spectra", "256", "--spectra-guard", "128"], "--spectra-guard must be in [-1, N / 2 - 1]"),
                        (["--spectra", "256", "--spectra-guard", "-2"], "--spectra-guard must be in [-1, N / 2 - 1]"),
                        (["--spectra", "256", "--spectra-fraction", "0"], "--spectra-fraction must be in (0, 1]"),
                        (["--spectra", "256", "--spectra-fraction", "1.5"], "--spectra-fraction must be in (0, 1]"),
                        (["--spectra-kind", "fourth"], "need --spectra N")):
        r = subprocess.run([TOOL] + x + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr and r.stderr.startswith("fsea-cutouts: "), (extra, r.stderr)
    # the last option without its value is the usage text, as for every other option
    r = subprocess.run([TOOL] + x + ["--spectra"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stderr.startswith("fsea-cutouts: usage: fsea-cutouts FILE")
