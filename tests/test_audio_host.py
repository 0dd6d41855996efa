"""CPU tier: cut-out audio without a GPU -- the restatement tests/audio_ref.py against the reference's discriminator as
tests/demod_ref.py restates it (bit for bit, random and branch-edge inputs), the arctangent expression's own error against
atan2 as a recorded property, the filter's order on hand-made values, a synthetic FM tone and an AM tone through extract's
restatement and this one; fsea_audio_layout; the refusals of fsea_audio_create and fsea_audio_run_* in the header's order,
against a fake object (the checks read nothing of it but its decimation); the shipped kernel's resource usage and its
instruction mix; the Python declarations; fsea-cutouts' new usage errors."""
import collections
import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import audio_ref as A
from tests import demod_ref as R
from tests import extract_ref as X
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _code_objects, _kernels

FSEA_EINVAL = -1
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-cutouts")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_header_constants_and_records_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()
    assert int(re.search(r"#define FSEA_AUDIO_FM (\d+)", text).group(1)) == fsea.AUDIO_FM == A.FM == 0
    assert int(re.search(r"#define FSEA_AUDIO_AM (\d+)", text).group(1)) == fsea.AUDIO_AM == A.AM == 1
    assert int(re.search(r"#define FSEA_AUDIO_MAX_DECIMATION (\d+)", text).group(1)) == fsea.AUDIO_MAX_DECIMATION == 64
    assert int(re.search(r"#define FSEA_AUDIO_MAX_JOBS\s+(\d+)", text).group(1)) == fsea.AUDIO_MAX_JOBS == fsea.EXTRACT_MAX_JOBS
    assert re.search(r"#define FSEA_AUDIO_MAX_PAIRS\s+\(1u << 24\)", text) and fsea.AUDIO_MAX_PAIRS == 1 << 24
    body = re.search(r"typedef struct \{([^}]*)\} fsea_audio_job;", text).group(1)
    names = [n.strip() for n in re.search(r"uint64_t\s+([\w\s,]+);", body).group(1).split(",")]
    assert names == [n for n, _ in fsea.AudioJob._fields_] == list(A.JOB.names)
    assert ctypes.sizeof(fsea.AudioJob) == A.JOB.itemsize == 24
    assert sorted(n for n in fsea.EXPORTS if n.startswith("fsea_audio_")) == [
        "fsea_audio_create", "fsea_audio_decimation", "fsea_audio_destroy", "fsea_audio_kind", "fsea_audio_layout", "fsea_audio_n_taps",
        "fsea_audio_run_device", "fsea_audio_run_host"]
    L = fsea.hip_lib()
    for name in fsea.EXPORTS:
        if name.startswith("fsea_audio_"):
            assert getattr(L, name).argtypes == fsea.API[name][1], name


# ---- the restatement -------------------------------------------------------------------------------------------------

def edge_inputs():
    """(li, lq, yi, yq) whose products meet every branch: real == imag, imag < 0, real < imag, real < 0, zeros, and the
    values either side of each edge."""
    cases = []
    for real, imag in ((1.0, 1.0), (1.0, -1.0), (2.0, 1.0), (1.0, 2.0), (-1.0, 2.0), (-1.0, -2.0), (-1.0, 0.5), (-1.0, -0.5), (0.0, 1.0),
                       (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (3.0, np.nextafter(3.0, 4.0)), (3.0, np.nextafter(3.0, 2.0)), (1e-300, 1e-300),
                       (1e300, 1.0), (1.0, 1e300), (2.0 ** -1074, 2.0 ** -1074), (-1.0, 2.0 ** -1074), (-1.0, -2.0 ** -1074)):
        cases.append((1.0, 0.0, real, imag))           # li yi + lq yq = real, li yq - yi lq = imag
        cases.append((0.0, 1.0, imag, -real))          # the same products from the other factor
    return np.array(cases).T


def test_the_fm_discriminator_is_the_references_bit_for_bit():
    rng = np.random.default_rng(5)
    li, lq, yi, yq = rng.normal(0.0, 1.0, (4, 200000))
    lq[:1000] = 0.0                                    # imag = li yq: a product alone
    yq[1000:2000] = yi[1000:2000]
    e = edge_inputs()
    li, lq, yi, yq = (np.concatenate([x, y]) for x, y in zip((li, lq, yi, yq), e))
    real, imag = li * yi + lq * yq, li * yq - yi * lq
    assert np.any(real == imag) and np.any(imag < 0) and np.any(real < np.abs(imag)) and np.any(real < 0)
    with np.errstate(over="ignore", invalid="ignore"):
        want = R.discriminate(li, lq, yi, yq, 1.0)
    got = A.arctangent(real, imag)
    # -1 / 2^-1074 overflows and the expression gives inf / inf: a NaN in both, at the edge inputs made for it
    nan = np.isnan(want)
    assert nan.sum() == 4 and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))
    # through the job's own path: pairs in, d out; d[0] is +0.0
    z = (rng.normal(0.0, 1.0, 5000) + 1j * rng.normal(0.0, 1.0, 5000)).astype(np.complex64)
    a, b = A.terms(z, 0.25 - 0.5j)
    assert np.array_equal(a, z.real.astype(np.float64) - 0.25) and np.array_equal(b, z.imag.astype(np.float64) + 0.5)
    d = A.discriminator(z, A.FM, 0.25 - 0.5j)
    assert bits(d[:1])[0] == 0 and np.array_equal(bits(d[1:]), bits(R.discriminate(a[:-1], b[:-1], a[1:], b[1:], 1.0)))


def test_a_silent_pair_gives_plus_zero_where_the_reference_gives_a_quarter_of_pi():
    """The one stated deviation: real == imag == 0 is the reference's `real == imag` branch, div = 1."""
    zeros = np.array([0.0, -0.0, 0.0, -0.0])
    other = np.array([0.0, 0.0, -0.0, -0.0])
    ref = R.discriminate(np.ones(4), np.zeros(4), zeros, other, 1.0)
    assert np.allclose(np.abs(ref), 1.0 / (A.C0 + A.C1 + A.C2)) and abs(abs(ref[0]) - math.pi / 4) < 1e-3
    assert np.all(bits(A.arctangent(zeros, other)) == 0)
    silent = np.zeros(40, np.complex64)
    for kind in (A.FM, A.AM):
        assert np.all(bits(A.discriminator(silent, kind)) == 0)
    assert np.all(A.audio(silent, A.FM, np.ones(5), 3, 0j, -2.0).view(np.uint32) == 0x80000000)    # gain * +0.0, not a sum: -0.0


ATAN_ERROR_QUARTER_TURN = 9.4e-4     # measured below: 9.301e-4 rad at 0.866 rad, the reference expression's own


def test_the_arctangent_expressions_own_error_is_recorded():
    """The reference's expression against math.atan2 on 4 million angles round the circle.  Recorded, not a tolerance of the
    code under test (which is held to the expression bit for bit): 9.3e-4 rad up to a quarter turn; behind it the third
    branch divides a negative real by imag and the polynomial was not made for that: 0.019 off at 0.6 pi, 0.135 at 0.75 pi,
    pi / 2 at half a turn.  include/fsea.h and DESIGN.md quote these."""
    th = np.linspace(-math.pi, math.pi, 4000001)
    err = np.abs(A.arctangent(np.cos(th), np.sin(th)) - th)
    found = [float(err[np.abs(th) <= lim * math.pi].max()) for lim in (0.25, 0.5, 0.6, 0.75, 1.0)]
    print("largest error up to 0.25, 0.5, 0.6, 0.75 and 1 pi:", found)
    assert 9.2e-4 < found[0] == found[1] < ATAN_ERROR_QUARTER_TURN
    assert 0.018 < found[2] < 0.020 and 0.13 < found[3] < 0.14 and abs(found[4] - math.pi / 2) < 1e-6
    assert err[np.abs(th) <= 1e-3].max() < 2e-5          # and it is an arctangent: the small steps of an FM signal


def test_the_filter_is_one_chain_per_output_over_the_taps_ascending():
    """Numbers whose sum depends on the order, D = 2, L = 3, AM so that d is |re| exactly."""
    d = np.array([1.0, 2.0 ** -30, 2.0 ** 53, 1.0, 1.0, 2.0 ** -24, 7.0])
    c = np.array([1.0, 1.0, -1.0])
    z = d.astype(np.float32).astype(np.complex64)
    assert np.array_equal(A.discriminator(z, A.AM), d)
    ext = [0.0, 0.0] + d.tolist()
    want = [((0.0 + c[0] * ext[2 * j]) + c[1] * ext[2 * j + 1]) + c[2] * ext[2 * j + 2] for j in range(3)]
    got = A.audio(z, A.AM, c, 2, 0j, 3.0)
    assert got.dtype == np.float32 and got.size == 3
    assert np.array_equal(got, (3.0 * np.array(want)).astype(np.float32))
    assert want[2] != (c[2] * ext[6] + c[1] * ext[5]) + c[0] * ext[4]                 # descending is another number
    for n, D in ((0, 1), (1, 2), (5, 6), (6, 6), (13, 6)):
        assert A.audio(np.ones(n, np.complex64), A.AM, c, D).size == n // D
    # an accumulator is never -0.0: -0.0 taps on the zero prefix and on zeros leave +0.0
    assert np.all(bits(np.zeros(3) + -1.0 * 0.0) == 0)
    got = A.audio(np.zeros(8, np.complex64), A.AM, -np.ones(4), 1)
    assert np.all(got.view(np.uint32) == 0)
    # the offset is taken off before anything else, in f64
    z = np.full(9, 0.5 + 0.25j, np.complex64)
    assert np.all(A.discriminator(z, A.AM, 0.5 + 0.25j) == 0.0) and np.all(A.discriminator(z, A.AM, 0.5 - 0.75j) == 1.0)


def test_which_outputs_a_nan_pair_reaches():
    """nan_outputs, the helper of the GPU tier's special-value test, against the restatement itself."""
    rng = np.random.default_rng(9)
    for kind in (A.FM, A.AM):
        for n, L, D in ((40, 5, 3), (64, 1, 1), (30, 41, 8), (100, 7, 2)):
            c = rng.uniform(0.5, 1.5, L)
            for at in (0, 1, n // 2, n - 2, n - 1):
                z = (rng.normal(0, 1, n) + 1j * rng.normal(0, 1, n)).astype(np.complex64)
                z[at] = np.nan
                got = np.flatnonzero(np.isnan(A.audio(z, kind, c, D))).tolist()
                assert got == A.nan_outputs(n, kind, L, D, at), (kind, n, L, D, at)


# ---- a tone through extract's restatement and this one --------------------------------------------------------------------

RATE, D, L = 1536000, 16, 97                    # the recording's rate, extract's decimation and taps: pairs at 96 kHz
D2, L2, AUDIO_CUTOFF = 2, 41, 8000.0            # audio at 48 kHz
TONE, DEVIATION, CARRIER_BIN = 1000.0, 5000.0, 200
# The amplitude of the demodulated tone against deviation / --deviation: the step of the phase over one pair is
# (deviation / tone) 2 sin(pi tone / pair rate) cos(..), so the discriminator gives deviation / --deviation times
# sinc(pi tone / pair rate) = 0.99982, the audio low-pass passes 1 kHz at 1.00005.  The arctangent expression is off by up to
# 9.4e-4 rad (recorded above) on a peak step of 2 pi 5000 / 96000 = 0.327 rad: 0.29 % of the amplitude at the very most; the
# 8-bit recording leaves a rest of 1.4e-3 rms beside the tone, which a fit over 3800 outputs averages to 3e-5.  Measured on
# the restatement: 0.99985.  Fixed at 0.5 %: the expression's 0.29 %, the two filters' 0.02 %, and as much again.
TONE_MARGIN = 0.005


def tone_recording(kind, n=2 * 61440):
    """8-bit IQ (int8, the tools' --flip) of one emission CARRIER_BIN / 1024 cycles per sample off the centre: FM by a cosine of
    TONE Hz at DEVIATION Hz, or AM at depth 0.5; its one job, the extract's taps, the pedestal of its cut-outs."""
    sig = A.fm_signal(n, RATE, TONE, DEVIATION, 100.0) if kind == A.FM else A.am_signal(n, RATE, TONE, 0.5, 60.0)
    sig = sig * np.exp(2j * np.pi * (CARRIER_BIN / 1024) * np.arange(n))
    x = np.empty(2 * n)
    x[0::2], x[1::2] = sig.real, sig.imag
    u8 = np.clip(np.rint(x), -128, 127).astype(np.int8).view(np.uint8)
    taps = fsea.lowpass_taps(RATE, 0.4 * RATE / D, L)
    pedestal = 0.5 * float(np.sum(taps.astype(np.float32).astype(np.float64)))
    return u8, fsea.ExtractJob(0, n, 0, -CARRIER_BIN / 1024, 0.0, 0), taps, complex(pedestal, pedestal)


def audio_taps():
    return fsea.lowpass_taps(RATE / D, AUDIO_CUTOFF, L2)


def tone_check(audio, kind, carrier_hz=0.0):
    """The CPU tier's check of a demodulated tone, the GPU tier's too: after the filter's run-in the audio is mean + A cos(2 pi
    TONE t + phi) and little else; FM: A within TONE_MARGIN of DEVIATION / --deviation (the gain was made with DEVIATION) and
    the mean where the carrier stands from the cut-out's centre, carrier_hz / DEVIATION (0 for a cut-out mixed to its carrier);
    AM: the envelope is carrier (1 + 0.5 cos), so A / mean is the depth 0.5 whatever the scale of the samples."""
    amp, mean, rest = A.tone_fit(np.asarray(audio, dtype=np.float64)[L2:], RATE / D / D2, TONE)
    print("kind", kind, "amplitude", amp, "mean", mean, "rest rms", rest)
    if kind == A.FM:
        assert abs(amp - 1.0) <= TONE_MARGIN and abs(mean - carrier_hz / DEVIATION) <= TONE_MARGIN and rest <= TONE_MARGIN
    else:
        assert abs(amp / mean - 0.5) <= TONE_MARGIN and rest <= TONE_MARGIN * mean
    return amp, mean


@pytest.fixture(scope="module")
def tone_cutouts():
    out = {}
    for kind in (A.FM, A.AM):
        u8, job, taps, pedestal = tone_recording(kind)
        z = X.cutout_reference(u8, job, taps, D, True)[X.lead(L, D) // D:].astype(np.complex64)
        out[kind] = (z, pedestal)
    return out


@pytest.mark.parametrize("kind", [A.FM, A.AM])
def test_a_synthetic_tone_comes_back_at_its_frequency_and_amplitude(tone_cutouts, kind):
    z, pedestal = tone_cutouts[kind]
    gain = RATE / D / (2 * math.pi * DEVIATION) if kind == A.FM else 1.0
    audio = A.audio(z, kind, audio_taps(), D2, pedestal, gain)
    assert audio.size == z.size // D2 > 3000
    amp, mean = tone_check(audio, kind)
    if kind == A.FM:
        assert abs(amp - 0.99985) < 2e-4                 # the measured figure the margin's comment quotes
        half = A.audio(z, kind, audio_taps(), D2, pedestal, gain / 2)      # --deviation twice the deviation: half the amplitude
        assert abs(A.tone_fit(half[L2:].astype(np.float64), RATE / D / D2, TONE)[0] - amp / 2) < 1e-6
        # the other frequency is not there
        assert A.tone_fit(audio[L2:].astype(np.float64), RATE / D / D2, 1.7 * TONE)[0] < 0.01


# ---- the C side without a device ----------------------------------------------------------------------------------------

def fake_object(kind=0, n_taps=41, decimation=4):
    """the struct begins `int kind; int n_taps; int decimation; int device;` and the checks read the decimation alone"""
    fake = ctypes.create_string_buffer(4096)
    struct.pack_into("<iiii", fake, 0, kind, n_taps, decimation, 0)
    return fake


def table(*jobs):
    return (fsea.AudioJob * len(jobs))(*[fsea.AudioJob(*j) for j in jobs])


def test_layout_is_back_to_back_in_table_order():
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    for d in (1, 3, 64):
        fake = fake_object(1, 7, d)
        f = ctypes.cast(fake, ctypes.c_void_p)
        assert (L_.fsea_audio_kind(f), L_.fsea_audio_n_taps(f), L_.fsea_audio_decimation(f)) == (1, 7, d)
        ns = [0, d - 1, d, 3 * d, 3 * d + 1, 0, 7 * d + d - 1, 1000, 2 * d, 0]
        tab = table(*[(5 * i, n, 12345) for i, n in enumerate(ns)])
        total = ctypes.c_size_t(99)
        assert L_.fsea_audio_layout(f, ctypes.addressof(tab), len(tab), ctypes.byref(total)) == 0
        firsts, want = A.layout(ns, d)
        assert [j.out_first for j in tab] == firsts and total.value == want
        assert [(j.first_pair, j.n_pairs) for j in tab] == [(5 * i, n) for i, n in enumerate(ns)]
        py, py_total = fsea.audio_layout([fsea.AudioJob(5 * i, n, 777) for i, n in enumerate(ns)], d)
        assert bytes(py) == bytes(tab) and py_total == want
        assert L_.fsea_audio_layout(f, None, 0, ctypes.byref(total)) == 0 and total.value == 0
    assert L_.fsea_audio_layout(None, ctypes.addressof(tab), 1, ctypes.byref(total)) == FSEA_EINVAL and b"audio is NULL" in err()
    assert L_.fsea_audio_layout(f, ctypes.addressof(tab), 1, None) == FSEA_EINVAL and b"total_outputs is NULL" in err()
    assert L_.fsea_audio_layout(f, ctypes.addressof(tab), fsea.AUDIO_MAX_JOBS + 1, ctypes.byref(total)) == FSEA_EINVAL and b"n_jobs" in err()
    assert L_.fsea_audio_layout(f, None, 1, ctypes.byref(total)) == FSEA_EINVAL and b"NULL job table" in err()
    assert (L_.fsea_audio_kind(None), L_.fsea_audio_n_taps(None), L_.fsea_audio_decimation(None)) == (-1, 0, 0)


def test_create_refuses_bad_arguments_in_order_before_it_looks_for_a_device():
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    h = ctypes.c_void_p()
    taps = np.ones(21)
    bad = np.ones(21)
    bad[3] = np.nan
    t, b = taps.ctypes.data, bad.ctypes.data
    # every refusal with everything behind it in the order wrong as well: the earlier check speaks
    assert L_.fsea_audio_create(None, 2, None, 0, 0, 99) == FSEA_EINVAL and b"out-pointer" in err()
    assert L_.fsea_audio_create(ctypes.byref(h), 2, None, 0, 0, 99) == FSEA_EINVAL and b"kind must be" in err()
    assert L_.fsea_audio_create(ctypes.byref(h), -1, None, 0, 0, 99) == FSEA_EINVAL and b"kind must be" in err()
    assert L_.fsea_audio_create(ctypes.byref(h), 0, None, 0, 0, 99) == FSEA_EINVAL and b"taps is NULL" in err()
    for n in (0, -1, fsea.FIR_MAX_TAPS + 1):
        assert L_.fsea_audio_create(ctypes.byref(h), 1, b, n, 0, 99) == FSEA_EINVAL and b"n_taps must be in [1, 512]" in err()
    assert L_.fsea_audio_create(ctypes.byref(h), 1, b, 21, 0, 99) == FSEA_EINVAL and b"tap 3 is not finite" in err()
    for d in (0, -1, 65):
        assert L_.fsea_audio_create(ctypes.byref(h), 1, t, 21, d, 99) == FSEA_EINVAL and b"decimation must be in [1, 64]" in err()
    assert not h.value and L_.fsea_audio_destroy(None) == 0
    rc = L_.fsea_audio_create(ctypes.byref(h), 1, t, 21, 64, 0)
    if fsea.device_count() == 0:
        assert rc == -2 and not h.value                                                             # FSEA_ENODEVICE
    else:
        assert rc == 0 and L_.fsea_audio_kind(h) == 1 and L_.fsea_audio_destroy(h) == 0


def test_run_refuses_bad_arguments_without_a_device_in_the_headers_order():
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    buf = np.full(8192, 0x5A, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    out = p + 4096
    fake = fake_object(0, 41, 4)
    f = ctypes.cast(fake, ctypes.c_void_p)
    big = 1 << 40
    one = table((0, 64, 0))
    forms = ((L_.fsea_audio_run_device, (None,)), (L_.fsea_audio_run_host, ()))

    def refused(word, obj=f, pairs=p, n_buffer=512, jobs=one, off=(0.5, 0.5), gain=1.0, audio=out, n_audio=1024, only=None, n_jobs=None):
        for run, tail in forms:
            if only is not None and run is not only:
                continue
            rc = run(obj, pairs, n_buffer, ctypes.addressof(jobs) if jobs is not None else None, len(jobs) if n_jobs is None else n_jobs,
                     off[0], off[1], gain, audio, n_audio, *tail)
            assert rc == FSEA_EINVAL and word in err(), (run, word, err())

    nan = np.nan
    refused(b"audio is NULL", obj=None, n_jobs=fsea.AUDIO_MAX_JOBS + 1, jobs=None, pairs=None, gain=nan)
    refused(b"n_jobs", n_jobs=fsea.AUDIO_MAX_JOBS + 1, jobs=None, pairs=None, gain=nan)
    for run, tail in forms:                                # no jobs: a no-op whatever else is given
        assert run(f, None, 0, None, 0, nan, 0.0, nan, None, 0, *tail) == 0
        assert run(f, p + 4, 7, None, 0, 0.0, 0.0, 1.0, out + 1, 0, *tail) == 0
    refused(b"NULL job table", jobs=None, n_jobs=1, pairs=None, gain=nan)
    refused(b"NULL buffer", pairs=None, gain=nan)
    refused(b"NULL buffer", audio=None, gain=nan)
    for off in ((nan, 0.0), (0.0, np.inf), (-np.inf, 0.0)):
        refused(b"offset is not finite", off=off, gain=nan, jobs=table((600, 1, 0)))
    for gain in (nan, np.inf, -np.inf):
        refused(b"gain is not finite", gain=gain, jobs=table((600, 1, 0)))
    refused(b"job 1: pairs", jobs=table((0, 64, 0), (500, 13, 16)))                         # past the buffer
    refused(b"job 0: pairs", jobs=table((big, 1, 0)))
    refused(b"job 0: pairs", jobs=table((2, (1 << 64) - 1, 0)))                            # first + n wraps
    refused(b"job 0: n_pairs", jobs=table((0, (1 << 24) + 1, 0)), n_buffer=big)
    refused(b"job 0: outputs", jobs=table((0, 64, 1009)))                                  # 16 outputs from 1009: one past 1024
    refused(b"job 0: outputs", jobs=table((0, 64, big)))
    refused(b"job 0: outputs", jobs=table((0, 64, (1 << 64) - 3)))                         # out_first + outputs wraps
    refused(b"job 0: outputs", jobs=table((0, 64, 0)), n_audio=15)
    refused(b"job 1: pairs", jobs=table((0, 64, 2000), (big, 1, 0)), n_jobs=2, n_audio=2016)          # table order: job 0 is fine
    refused(b"job 0: outputs", jobs=table((0, 64, 2000), (big, 1, 0)), n_jobs=2)                     # ... and here it is not
    refused(b"the outputs of jobs 0 and 2 overlap", jobs=table((0, 64, 100), (0, 3, 100), (64, 64, 115), (0, 0, 101)))
    refused(b"the outputs of jobs 1 and 2 overlap", jobs=table((0, 64, 100), (8, 64, 50), (64, 64, 50)))      # a job again in the same place
    refused(b"the outputs of jobs 0 and 1 overlap", jobs=table((0, 64, 116), (64, 64, 101)), pairs=p + 4)      # before the alignment
    fake1 = fake_object(0, 41, 1)
    f1 = ctypes.cast(fake1, ctypes.c_void_p)
    many = table(*[(0, 1 << 24, i << 24) for i in range(129)])
    refused(b"more than 2^31", obj=f1, jobs=many, n_buffer=big, n_audio=big, pairs=p + 4)          # the total before the alignment
    clash = table(*([(0, 1 << 24, i << 24) for i in range(129)] + [(0, 8, 5)]))
    refused(b"the outputs of jobs 0 and 129 overlap", obj=f1, jobs=clash, n_buffer=big, n_audio=big)   # the overlap before the total
    for d_pairs, d_audio in ((p + 4, out), (p, out + 2), (p + 1, out), (p, out + 1)):
        refused(b"aligned", pairs=d_pairs, audio=d_audio, only=L_.fsea_audio_run_device)
    assert np.all(buf == 0x5A)                                                                      # a refused call writes nothing


# ---- the shipped kernel -----------------------------------------------------------------------------------------------------

TILES_VGPRS, TILES_SGPRS, TILES_LDS = 64, 96, 8 * (4096 + 128)      # read off the build: 36 and 78; the image is a constant
FMA_PER_DIVISION, FMA_PER_SQRT = 5, 7                               # the compiler's own expansions of / and sqrt in f64


def test_shipped_library_has_the_audio_kernel_within_its_budget():
    """fsea_audio_tiles from the code object's metadata alone: wave64, 256 lanes, no scratch, no spilled register; 33 KiB of
    LDS and at most 64 VGPRs, so four workgroups share a CU ("Cut-out audio")."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    k = _kernels(LIB)["fsea_audio_tiles"]
    print(k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"], k[".vgpr_spill_count"],
          k[".sgpr_spill_count"])
    assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".vgpr_count"] <= TILES_VGPRS and k[".sgpr_count"] <= TILES_SGPRS
    assert k[".group_segment_fixed_size"] == TILES_LDS and 4 * TILES_LDS <= 160 * 1024


def test_the_audio_kernel_contracts_nothing_into_an_fma(tmp_path):
    """The contract rounds every product and every sum on its own.  A kernel that divides and takes a square root in f64
    cannot be free of v_fma_f64 as the measures' kernels are: the compiler expands a correctly rounded division into five
    fused steps round v_div_fmas_f64 and a square root into seven round v_rsq_f64.  So: every fused multiply-add in the
    shipped kernel is one of those -- as many as its divisions and square roots account for and not one more -- and the
    chain and the products are plain v_mul_f64 and v_add_f64."""
    assert os.path.exists(OBJDUMP) and os.path.exists(LIB)
    body = None
    for i, elf in enumerate(_code_objects(LIB)):
        path = tmp_path / ("audio%d.elf" % i)
        path.write_bytes(elf)
        text = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", str(path)], capture_output=True, text=True, check=True).stdout
        m = re.search(r"<fsea_audio_tiles>:\n(.*?)(?=\n\n[0-9a-f]+ <|\Z)", text, re.S)
        if m:
            body = m.group(1)
    assert body, "fsea_audio_tiles is not in the library"
    ops = collections.Counter(re.sub(r"_e(32|64)$", "", op) for op in re.findall(r"^\s*([a-z]\w+)", body, re.M))
    fused = sum(n for op, n in ops.items() if re.match(r"v_(pk_)?fma(c|ak|mk)?_", op))
    print({op: n for op, n in ops.items() if "fma" in op or op in ("v_div_fmas_f64", "v_rsq_f64", "v_mul_f64", "v_add_f64", "ds_read_b64")})
    assert ops["v_div_fmas_f64"] == 2 and ops["v_rsq_f64"] == 1          # imag / real or real / imag, div / (..); the envelope
    assert fused == FMA_PER_DIVISION * ops["v_div_fmas_f64"] + FMA_PER_SQRT * ops["v_rsq_f64"], ops
    assert not any("f32" in op or "f16" in op for op in ops if "fma" in op or "mac" in op)
    assert ops["v_mul_f64"] >= 16 and ops["v_add_f64"] >= 16 and ops["ds_read_b64"] >= 8          # the chain, eight taps at a time
    assert not any(op.startswith(("scratch_", "buffer_atomic", "global_atomic", "ds_add", "ds_cmpst")) for op in ops)
    assert ops["s_barrier"] == 1


def test_tool_knows_audio_and_refuses_what_it_cannot_do():
    assert os.path.exists(TOOL), "fsea-cutouts not built"
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--audio fm|am" in r.stdout and "--deviation HZ" in r.stdout
    x = ["x.raw", "--size", "1024", "--out", "y", "--decimation", "4"]
    for extra, word in ((["--audio", "ssb", "--rate", "1e6", "--freq", "100"], "--audio must be fm or am"),
                        (["--audio", "fm"], "--audio needs --rate"),
                        (["--audio", "fm", "--rate", "1e6", "--freq", "100", "--audio-rate", "1000"], "--audio-rate"),
                        (["--audio", "fm", "--rate", "1e6", "--freq", "100", "--audio-taps", "0"], "--audio-taps must be in [1, 512]"),
                        (["--audio", "fm", "--rate", "1e6", "--freq", "100", "--deviation", "0"], "--deviation must be positive")):
        r = subprocess.run([TOOL] + x + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr and r.stderr.startswith("fsea-cutouts: "), (extra, r.stderr)
