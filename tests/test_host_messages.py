"""CPU tier: the fatal-error convention of the C99 host layer (frequensea_amd/host) and of fsea-fft-batch, pinned byte for
byte: a failure prints one line to stderr and the process ends with status 1.  Every case runs in a child process.

Three groups:
  * argument checks that come before any device work: the whole line is pinned;
  * the create failure of each block with NRF_FFT_DEVICE=-1, which the library's device check refuses before any device
    work -- FSEA_ENODEVICE without a GPU, FSEA_EINVAL ("device -1 out of range") with one -- so the line is pinned up to
    and including " failed (" and the tail is not;
  * fsea-fft-batch: the usage line needs no device.  Its other three checks (an argument without '=', a capture that
    cannot be opened, a capture with too few transfers) come after the plan, the streams and the buffers are created:
    where that succeeds the whole line is pinned, and without a GPU the tool ends at its first device call, whose line
    is pinned up to the library's own error text.  A capture with too few transfers is reported and skipped: status 0.
Not here: NRF_FFT_WINDOW=bogus is read after nrf_fft_new has created its plan, so it cannot be reached without a device;
fsea-fft-batch --window bogus comes after the tool's plan as well (tests/test_gpu_tools.py has it).  nrf_fft_set_window
checks the name before it looks at the block, so its message is reached with a NULL block."""
import os
import subprocess
import sys

import pytest

from frequensea_amd import fsea
from tests.conftest import ROOT

BATCH = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-fft-batch")
PRELUDE = ("import sys; sys.path.insert(0, %r)\n"
           "import numpy as np\n"
           "from frequensea_amd import nrf\n"
           "L = nrf.nrf_lib()\n"
           "block = np.zeros(64, np.uint8)\n"
           "buf = L.nut_buffer_new_u8(32, 2, block.ctypes.data)\n") % ROOT


def run_child(body, env=None):
    child_env = dict(os.environ)
    child_env.pop("NRF_FFT_DEVICE", None)
    child_env.pop("NRF_FFT_WINDOW", None)
    child_env.update(env or {})
    r = subprocess.run([sys.executable, "-c", PRELUDE + body + "\nprint('returned')\n"], capture_output=True, text=True,
                       timeout=120, env=child_env)
    assert "returned" not in r.stdout
    return r


ARGUMENT_CHECKS = [
    ("L.nrf_iq_filter_new(5000000, 200000, 0)",
     "NRF IQ filter fatal error: kernel length 0 is outside [1, %d]\n" % fsea.FIR_MAX_TAPS),
    ("L.nrf_iq_filter_new(5000000, 200000, %d)" % (fsea.FIR_MAX_TAPS + 1),
     "NRF IQ filter fatal error: kernel length %d is outside [1, %d]\n" % (fsea.FIR_MAX_TAPS + 1, fsea.FIR_MAX_TAPS)),
    ("L.nrf_iq_chain_new(5000000, 200000, 0)",
     "NRF IQ chain fatal error: kernel length 0 is outside [1, %d]\n" % fsea.FIR_MAX_TAPS),
    ("L.nrf_iq_chain_new(5000000, 200000, %d)" % (fsea.FIR_MAX_TAPS + 1),
     "NRF IQ chain fatal error: kernel length %d is outside [1, %d]\n" % (fsea.FIR_MAX_TAPS + 1, fsea.FIR_MAX_TAPS)),
    ("L.nrf_fir_filter_new(5000000, 200000, 0)", "NRF FIR fatal error: filter length 0 is not >= 1\n"),
    ("L.nrf_buffer_to_iq_lines(buf, 0, 1.0)",
     "NRF IQ draw fatal error: size_multiplier 0 is outside [1, %d]\n" % fsea.IQ_MAX_MULTIPLIER),
    ("L.nrf_buffer_to_iq_lines(buf, 17, 1.0)",
     "NRF IQ draw fatal error: size_multiplier 17 is outside [1, %d]\n" % fsea.IQ_MAX_MULTIPLIER),
    # the multiplier is checked before the chain is looked at (and before its mutex is taken)
    ("L.nrf_iq_chain_get_iq_lines(None, 0, 1.0)",
     "NRF IQ draw fatal error: size_multiplier 0 is outside [1, %d]\n" % fsea.IQ_MAX_MULTIPLIER),
    ("L.nrf_iq_chain_get_iq_lines(None, 17, 1.0)",
     "NRF IQ draw fatal error: size_multiplier 17 is outside [1, %d]\n" % fsea.IQ_MAX_MULTIPLIER),
    ("L.nrf_fft_set_window(None, b'bogus')",
     "NRF FFT fatal error: nrf_fft_set_window: \"bogus\" is not one of hann, hamming, blackman, blackmanharris, flattop, "
     "rect\n"),
    ("L.nrf_interpolator_get_buffer(L.nrf_interpolator_new(0.1))",
     "NRF interpolator fatal error: nrf_interpolator_get_buffer before the first nrf_interpolator_process\n"),
]


@pytest.mark.parametrize("call,line", ARGUMENT_CHECKS, ids=[c for c, _ in ARGUMENT_CHECKS])
def test_an_argument_check_prints_its_line_and_exits_with_1(call, line):
    r = run_child(call)
    assert r.returncode == 1 and r.stderr == line, (r.returncode, r.stderr)


CREATE_FAILURES = [
    ("L.nrf_fft_new(1024, 4)", "NRF FFT fatal error: fsea_plan_create failed ("),
    ("L.nrf_iq_filter_new(5000000, 200000, 51)", "NRF IQ filter fatal error: fsea_fir_create failed ("),
    ("L.nrf_iq_chain_new(5000000, 200000, 51)", "NRF IQ chain fatal error: fsea_chain_create failed ("),
    ("L.nrf_buffer_to_iq_points(buf)", "NRF IQ draw fatal error: fsea_iq_draw_create failed ("),
    ("L.nrf_raw_demodulator_new(5000000, 48000)", "NRF decoder fatal error: fsea_demod_create failed ("),
    ("L.nrf_interpolator_process(L.nrf_interpolator_new(0.1), buf)",
     "NRF interpolator fatal error: fsea_interp_create failed ("),
]


@pytest.mark.parametrize("call,prefix", CREATE_FAILURES, ids=[c for c, _ in CREATE_FAILURES])
def test_a_create_failure_names_its_block_and_exits_with_1(call, prefix):
    r = run_child(call, env={"NRF_FFT_DEVICE": "-1"})
    assert r.returncode == 1, (r.returncode, r.stderr)
    # "<prefix><rc>): <the library's text>\n": one line, a negative FSEA_* code
    assert r.stderr.startswith(prefix + "-") and r.stderr.endswith("\n") and r.stderr.count("\n") == 1, r.stderr
    assert "): " in r.stderr[len(prefix):]


def run_batch(*args):
    return subprocess.run([BATCH] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_fft_batch_without_captures_prints_its_usage():
    r = run_batch("--rows", "4")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == ("usage: fsea-fft-batch [--broad] [--rows H] [--fft N] [--skip K] [--out DIR] [--device D] [--timing] "
                        "[--window NAME] FREQ_MHZ=capture.raw ...\n")


def check_batch(r, status, line):
    """The line of a check that follows the tool's device setup; without a GPU, the line of the first device call."""
    no_device = "fsea-fft-batch: fsea_plan_create: "
    if r.stderr.startswith(no_device):
        assert r.returncode == 1 and r.stderr.count("\n") == 1 and len(r.stderr) > len(no_device) + 1, r.stderr
    else:
        assert r.returncode == status and r.stderr == line, (r.returncode, r.stderr)


def test_fft_batch_with_an_argument_without_equals_sign():
    r = run_batch("--rows", "4", "capture.raw")
    check_batch(r, 1, "fsea-fft-batch: expected FREQ_MHZ=capture.raw, got capture.raw\n")


def test_fft_batch_with_a_capture_that_does_not_exist(tmp_path):
    path = tmp_path / "absent.raw"
    r = run_batch("--rows", "4", "--out", tmp_path, "100=%s" % path)
    check_batch(r, 1, "fsea-fft-batch: cannot open %s\n" % path)


def test_fft_batch_with_a_capture_of_too_few_transfers(tmp_path):
    path = tmp_path / "short.raw"
    path.write_bytes(bytes(16))
    r = run_batch("--rows", "4", "--out", tmp_path, "100=%s" % path)
    check_batch(r, 0, "fsea-fft-batch: %s holds 0 transfers, need more than 10\n" % path)
    assert not list(tmp_path.glob("*.png"))
