"""ctypes view of libfsea_nrf.so: the reference's nut_buffer / nrf_device / nrf_fft C API
(include/nut.h, include/nrf.h).  Mirrors how src/main.cpp's Lua wrappers call it."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

NUT_BUFFER_U8 = 1
NUT_BUFFER_F64 = 2
NRF_BUFFER_SIZE_BYTES = 16 * 16384
NRF_SAMPLES_LENGTH = 131072

NUT_EXPORTS = [
    "nut_sleep_milliseconds", "nut_buffer_new_u8", "nut_buffer_new_f64", "nut_buffer_copy",
    "nut_buffer_reduce", "nut_buffer_clip", "nut_buffer_set_data", "nut_buffer_append",
    "nut_buffer_get_u8", "nut_buffer_get_f64", "nut_buffer_set_u8", "nut_buffer_set_f64",
    "nut_buffer_convert", "nut_buffer_save", "nut_buffer_free",
]
# additions beside the reference's prototypes (include/nrf.h says so at each): the reference's nrf.h has no such function
NRF_ADDITIONS = ["nrf_fft_set_window", "nrf_fft_set_window_weights", "nrf_decoder_free", "nrf_player_pop_pcm",
                 "nrf_iq_chain_new", "nrf_iq_chain_set_shifter", "nrf_iq_chain_process", "nrf_iq_chain_get_iq_points",
                 "nrf_iq_chain_get_iq_lines", "nrf_iq_chain_get_buffer", "nrf_iq_chain_free"]
NRF_EXPORTS = [
    "nrf_block_init", "nrf_block_connect", "nrf_block_process", "nrf_device_new",
    "nrf_device_new_with_config", "nrf_device_set_frequency", "nrf_device_set_decode_handler",
    "nrf_device_set_paused", "nrf_device_step", "nrf_device_get_samples_buffer", "nrf_device_free",
    "nrf_fft_new", "nrf_fft_shift", "nrf_fft_process", "nrf_fft_get_buffer", "nrf_fft_free",
    "nrf_freq_shifter_new", "nrf_freq_shifter_process_samples", "nrf_freq_shifter_process",
    "nrf_freq_shifter_get_buffer", "nrf_freq_shifter_free",
    "nrf_fir_get_low_pass_coefficients", "nrf_fir_filter_new", "nrf_fir_filter_load", "nrf_fir_filter_get",
    "nrf_fir_filter_free", "nrf_iq_filter_new", "nrf_iq_filter_process", "nrf_iq_filter_get_buffer", "nrf_iq_filter_free",
    "nrf_device_get_iq_buffer", "nrf_device_get_iq_lines", "nrf_buffer_add_position_channel", "nrf_buffer_to_iq_points",
    "nrf_buffer_to_iq_lines", "nrf_signal_detector_new", "nrf_signal_detector_process", "nrf_signal_detector_free",
    "nrf_downsampler_new", "nrf_downsampler_process", "nrf_downsampler_free", "nrf_raw_demodulator_new",
    "nrf_raw_demodulator_process", "nrf_raw_demodulator_free", "nrf_fm_demodulator_new", "nrf_fm_demodulator_process",
    "nrf_fm_demodulator_free", "nrf_decoder_new", "nrf_decoder_process", "nrf_player_new", "nrf_player_set_freq_offset",
    "nrf_player_set_gain", "nrf_player_free",
    "nrf_interpolator_new", "nrf_interpolator_process", "nrf_interpolator_get_buffer", "nrf_interpolator_free",
]
NRF_DEMODULATE_RAW, NRF_DEMODULATE_WBFM = 0, 1


class NutData(ctypes.Union):
    _fields_ = [("u8", ctypes.POINTER(ctypes.c_uint8)), ("f64", ctypes.POINTER(ctypes.c_double))]


class NutBuffer(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("length", ctypes.c_int), ("channels", ctypes.c_int),
                ("size_bytes", ctypes.c_int), ("data", NutData)]


NutBufferP = ctypes.POINTER(NutBuffer)


def bind_nut(L):
    """Attach nut_buffer_* prototypes to a loaded library (ours or the reference build)."""
    L.nut_buffer_new_u8.restype = NutBufferP
    L.nut_buffer_new_u8.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.nut_buffer_new_f64.restype = NutBufferP
    L.nut_buffer_new_f64.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.nut_buffer_copy.restype = NutBufferP
    L.nut_buffer_copy.argtypes = [NutBufferP]
    L.nut_buffer_reduce.restype = NutBufferP
    L.nut_buffer_reduce.argtypes = [NutBufferP, ctypes.c_double]
    L.nut_buffer_clip.restype = NutBufferP
    L.nut_buffer_clip.argtypes = [NutBufferP, ctypes.c_int, ctypes.c_int]
    L.nut_buffer_set_data.restype = None
    L.nut_buffer_set_data.argtypes = [NutBufferP, NutBufferP]
    L.nut_buffer_append.restype = None
    L.nut_buffer_append.argtypes = [NutBufferP, NutBufferP]
    L.nut_buffer_get_u8.restype = ctypes.c_uint8
    L.nut_buffer_get_u8.argtypes = [NutBufferP, ctypes.c_int]
    L.nut_buffer_get_f64.restype = ctypes.c_double
    L.nut_buffer_get_f64.argtypes = [NutBufferP, ctypes.c_int]
    L.nut_buffer_set_u8.restype = None
    L.nut_buffer_set_u8.argtypes = [NutBufferP, ctypes.c_int, ctypes.c_uint8]
    L.nut_buffer_set_f64.restype = None
    L.nut_buffer_set_f64.argtypes = [NutBufferP, ctypes.c_int, ctypes.c_double]
    L.nut_buffer_convert.restype = NutBufferP
    L.nut_buffer_convert.argtypes = [NutBufferP, ctypes.c_int]
    L.nut_buffer_save.restype = None
    L.nut_buffer_save.argtypes = [NutBufferP, ctypes.c_char_p]
    L.nut_buffer_free.restype = None
    L.nut_buffer_free.argtypes = [NutBufferP]
    return L


class NrfFirFilter(ctypes.Structure):
    """nrf_fir_filter (include/nrf.h): the reference's layout."""
    _fields_ = [("length", ctypes.c_int), ("coefficients", ctypes.POINTER(ctypes.c_double)), ("offset", ctypes.c_int),
                ("center", ctypes.c_int), ("samples_length", ctypes.c_int), ("samples", ctypes.POINTER(ctypes.c_double))]


def bind_fir(L):
    """Attach the host FIR filter prototypes (nrf_fir_*) to a loaded library (ours or a build of the reference)."""
    fp = ctypes.POINTER(NrfFirFilter)
    L.nrf_fir_get_low_pass_coefficients.restype = ctypes.POINTER(ctypes.c_double)
    L.nrf_fir_get_low_pass_coefficients.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.nrf_fir_filter_new.restype = fp
    L.nrf_fir_filter_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.nrf_fir_filter_load.restype = None
    L.nrf_fir_filter_load.argtypes = [fp, ctypes.c_void_p, ctypes.c_int]
    L.nrf_fir_filter_get.restype = ctypes.c_double
    L.nrf_fir_filter_get.argtypes = [fp, ctypes.c_int]
    L.nrf_fir_filter_free.restype = None
    L.nrf_fir_filter_free.argtypes = [fp]
    return L


class NrfSignalDetector(ctypes.Structure):
    """nrf_signal_detector (include/nrf.h): the reference's layout."""
    _fields_ = [("mean", ctypes.c_double), ("standard_deviation", ctypes.c_double)]


def bind_iq_draw(L):
    """Attach the IQ drawing and signal detector prototypes to a loaded library (ours or a build of the reference)."""
    vp = ctypes.c_void_p
    dp = ctypes.POINTER(NrfSignalDetector)
    L.nrf_device_get_iq_buffer.restype = NutBufferP
    L.nrf_device_get_iq_buffer.argtypes = [vp]
    L.nrf_device_get_iq_lines.restype = NutBufferP
    L.nrf_device_get_iq_lines.argtypes = [vp, ctypes.c_int, ctypes.c_float]
    L.nrf_buffer_add_position_channel.restype = NutBufferP
    L.nrf_buffer_add_position_channel.argtypes = [NutBufferP]
    L.nrf_buffer_to_iq_points.restype = NutBufferP
    L.nrf_buffer_to_iq_points.argtypes = [NutBufferP]
    L.nrf_buffer_to_iq_lines.restype = NutBufferP
    L.nrf_buffer_to_iq_lines.argtypes = [NutBufferP, ctypes.c_int, ctypes.c_float]
    L.nrf_signal_detector_new.restype = dp
    L.nrf_signal_detector_new.argtypes = []
    L.nrf_signal_detector_process.restype = None
    L.nrf_signal_detector_process.argtypes = [dp, NutBufferP]
    L.nrf_signal_detector_free.restype = None
    L.nrf_signal_detector_free.argtypes = [dp]
    return L


class NrfBlock(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("process_fn", ctypes.c_void_p), ("result_fn", ctypes.c_void_p),
                ("n_outputs", ctypes.c_int), ("outputs", ctypes.c_void_p * 10)]


class NrfFreqShifter(ctypes.Structure):
    """nrf_freq_shifter (include/nrf.h): the reference's layout."""
    _fields_ = [("block", NrfBlock), ("freq_offset", ctypes.c_int), ("sample_rate", ctypes.c_int),
                ("cosine", ctypes.c_double), ("sine", ctypes.c_double), ("buffer", NutBufferP)]


_dp = ctypes.POINTER(ctypes.c_double)


class NrfDownsampler(ctypes.Structure):
    """nrf_downsampler (include/nrf.h): the reference's layout."""
    _fields_ = [("in_rate", ctypes.c_int), ("out_rate", ctypes.c_int), ("filter", ctypes.POINTER(NrfFirFilter)),
                ("rate_mul", ctypes.c_double), ("out_length", ctypes.c_int), ("out_samples", _dp)]


class NrfRawDemodulator(ctypes.Structure):
    """nrf_raw_demodulator: the reference's members (this build appends a backend handle)."""
    _fields_ = [("in_sample_rate", ctypes.c_int), ("out_sample_rate", ctypes.c_int),
                ("downsampler_audio", ctypes.POINTER(NrfDownsampler)), ("audio_samples", _dp),
                ("audio_samples_length", ctypes.c_int)]


class NrfFmDemodulator(ctypes.Structure):
    """nrf_fm_demodulator: the reference's members (this build appends a backend handle)."""
    _fields_ = [("in_sample_rate", ctypes.c_int), ("out_sample_rate", ctypes.c_int), ("ampl_conv", ctypes.c_double),
                ("l_i", ctypes.c_double), ("l_q", ctypes.c_double), ("deemphasis_val", ctypes.c_double),
                ("downsampler_i", ctypes.POINTER(NrfDownsampler)), ("downsampler_q", ctypes.POINTER(NrfDownsampler)),
                ("downsampler_audio", ctypes.POINTER(NrfDownsampler)), ("demodulated_samples", _dp),
                ("demodulated_length", ctypes.c_int), ("audio_samples", _dp), ("audio_samples_length", ctypes.c_int)]


class NrfDecoder(ctypes.Structure):
    """nrf_decoder: the reference's members (this build appends a backend handle)."""
    _fields_ = [("in_sample_rate", ctypes.c_int), ("out_sample_rate", ctypes.c_int), ("demodulate_type", ctypes.c_int),
                ("demodulator", ctypes.c_void_p), ("freq_shifter", ctypes.POINTER(NrfFreqShifter)),
                ("samples_i", _dp), ("samples_q", _dp), ("samples_length", ctypes.c_int), ("audio_samples", _dp),
                ("audio_samples_length", ctypes.c_int)]


class NrfInterpolator(ctypes.Structure):
    """nrf_interpolator: the reference's members (this build appends a backend handle)."""
    _fields_ = [("block", NrfBlock), ("interpolate_step", ctypes.c_double), ("t", ctypes.c_double),
                ("buffer_a", NutBufferP), ("buffer_b", NutBufferP)]


def bind_interpolator(L):
    """Attach the interpolator prototypes to a loaded library (ours or a build of the reference)."""
    ip = ctypes.POINTER(NrfInterpolator)
    L.nrf_interpolator_new.restype = ip
    L.nrf_interpolator_new.argtypes = [ctypes.c_double]
    L.nrf_interpolator_process.restype = None
    L.nrf_interpolator_process.argtypes = [ip, NutBufferP]
    L.nrf_interpolator_get_buffer.restype = NutBufferP
    L.nrf_interpolator_get_buffer.argtypes = [ip]
    L.nrf_interpolator_free.restype = None
    L.nrf_interpolator_free.argtypes = [ip]
    return L


def bind_demod(L):
    """Attach the downsampler, demodulator, decoder and (where the library has them) player prototypes to a loaded
    library (ours or a build of the reference)."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    dsp, rawp, fmp, decp = (ctypes.POINTER(NrfDownsampler), ctypes.POINTER(NrfRawDemodulator),
                            ctypes.POINTER(NrfFmDemodulator), ctypes.POINTER(NrfDecoder))
    L.nrf_downsampler_new.restype = dsp
    L.nrf_downsampler_new.argtypes = [ci, ci, ci, ci]
    L.nrf_downsampler_process.restype = None
    L.nrf_downsampler_process.argtypes = [dsp, vp, ci]
    L.nrf_downsampler_free.restype = None
    L.nrf_downsampler_free.argtypes = [dsp]
    L.nrf_raw_demodulator_new.restype = rawp
    L.nrf_raw_demodulator_new.argtypes = [ci, ci]
    L.nrf_raw_demodulator_process.restype = None
    L.nrf_raw_demodulator_process.argtypes = [rawp, vp, vp, ci]
    L.nrf_raw_demodulator_free.restype = None
    L.nrf_raw_demodulator_free.argtypes = [rawp]
    L.nrf_fm_demodulator_new.restype = fmp
    L.nrf_fm_demodulator_new.argtypes = [ci, ci]
    L.nrf_fm_demodulator_process.restype = None
    L.nrf_fm_demodulator_process.argtypes = [fmp, vp, vp, ci]
    L.nrf_fm_demodulator_free.restype = None
    L.nrf_fm_demodulator_free.argtypes = [fmp]
    L.nrf_decoder_new.restype = decp
    L.nrf_decoder_new.argtypes = [ci, ci, ci, ci]
    L.nrf_decoder_process.restype = None
    L.nrf_decoder_process.argtypes = [decp, vp, ctypes.c_size_t]
    L.nrf_decoder_free.restype = None
    L.nrf_decoder_free.argtypes = [decp]
    if hasattr(L, "nrf_player_pop_pcm"):       # this build's headless player (include/nrf.h)
        L.nrf_player_new.restype = vp
        L.nrf_player_new.argtypes = [vp, ci, ci]
        L.nrf_player_set_freq_offset.restype = None
        L.nrf_player_set_freq_offset.argtypes = [vp, ci]
        L.nrf_player_set_gain.restype = None
        L.nrf_player_set_gain.argtypes = [vp, ctypes.c_float]
        L.nrf_player_free.restype = None
        L.nrf_player_free.argtypes = [vp]
        L.nrf_player_pop_pcm.restype = ci
        L.nrf_player_pop_pcm.argtypes = [vp, vp, ci, ctypes.POINTER(ctypes.c_long)]
    return L


_LIB = None


def lib_path():
    return os.path.join(_HERE, "libfsea_nrf.so")


def nrf_lib():
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError("libfsea_nrf.so is missing: run frequensea_amd.build()")
        L = bind_nut(ctypes.CDLL(path))
        vp = ctypes.c_void_p
        L.nrf_device_new.restype = vp
        L.nrf_device_new.argtypes = [ctypes.c_double, ctypes.c_char_p]
        L.nrf_device_set_frequency.restype = ctypes.c_double
        L.nrf_device_set_frequency.argtypes = [vp, ctypes.c_double]
        L.nrf_device_set_paused.restype = None
        L.nrf_device_set_paused.argtypes = [vp, ctypes.c_int]
        L.nrf_device_step.restype = None
        L.nrf_device_step.argtypes = [vp]
        L.nrf_device_get_samples_buffer.restype = NutBufferP
        L.nrf_device_get_samples_buffer.argtypes = [vp]
        L.nrf_device_free.restype = None
        L.nrf_device_free.argtypes = [vp]
        L.nrf_block_connect.restype = None
        L.nrf_block_connect.argtypes = [vp, vp]
        L.nrf_block_process.restype = None
        L.nrf_block_process.argtypes = [vp, NutBufferP]
        L.nrf_fft_new.restype = vp
        L.nrf_fft_new.argtypes = [ctypes.c_int, ctypes.c_int]
        L.nrf_fft_shift.restype = None
        L.nrf_fft_shift.argtypes = [vp, ctypes.c_double]
        L.nrf_fft_process.restype = None
        L.nrf_fft_process.argtypes = [vp, NutBufferP]
        L.nrf_fft_get_buffer.restype = NutBufferP
        L.nrf_fft_get_buffer.argtypes = [vp]
        L.nrf_fft_free.restype = None
        L.nrf_fft_free.argtypes = [vp]
        L.nrf_fft_set_window.restype = None
        L.nrf_fft_set_window.argtypes = [vp, ctypes.c_char_p]
        L.nrf_fft_set_window_weights.restype = None
        L.nrf_fft_set_window_weights.argtypes = [vp, ctypes.c_void_p]
        L.nrf_freq_shifter_new.restype = vp
        L.nrf_freq_shifter_new.argtypes = [ctypes.c_int, ctypes.c_int]
        L.nrf_freq_shifter_process_samples.restype = None
        L.nrf_freq_shifter_process_samples.argtypes = [vp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.nrf_freq_shifter_process.restype = None
        L.nrf_freq_shifter_process.argtypes = [vp, NutBufferP]
        L.nrf_freq_shifter_get_buffer.restype = NutBufferP
        L.nrf_freq_shifter_get_buffer.argtypes = [vp]
        L.nrf_freq_shifter_free.restype = None
        L.nrf_freq_shifter_free.argtypes = [vp]
        bind_fir(L)
        L.nrf_iq_filter_new.restype = vp
        L.nrf_iq_filter_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.nrf_iq_filter_process.restype = None
        L.nrf_iq_filter_process.argtypes = [vp, NutBufferP]
        L.nrf_iq_filter_get_buffer.restype = NutBufferP
        L.nrf_iq_filter_get_buffer.argtypes = [vp]
        L.nrf_iq_filter_free.restype = None
        L.nrf_iq_filter_free.argtypes = [vp]
        L.nrf_iq_chain_new.restype = vp
        L.nrf_iq_chain_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.nrf_iq_chain_set_shifter.restype = None
        L.nrf_iq_chain_set_shifter.argtypes = [vp, ctypes.c_int]
        L.nrf_iq_chain_process.restype = None
        L.nrf_iq_chain_process.argtypes = [vp, NutBufferP]
        L.nrf_iq_chain_get_iq_points.restype = NutBufferP
        L.nrf_iq_chain_get_iq_points.argtypes = [vp]
        L.nrf_iq_chain_get_iq_lines.restype = NutBufferP
        L.nrf_iq_chain_get_iq_lines.argtypes = [vp, ctypes.c_int, ctypes.c_float]
        L.nrf_iq_chain_get_buffer.restype = NutBufferP
        L.nrf_iq_chain_get_buffer.argtypes = [vp]
        L.nrf_iq_chain_free.restype = None
        L.nrf_iq_chain_free.argtypes = [vp]
        bind_iq_draw(L)
        bind_demod(L)
        bind_interpolator(L)
        _LIB = L
    return _LIB


def buffer_to_numpy(L, buf):
    """Copy a nut_buffer's payload out (the buffer stays owned by the caller)."""
    b = buf.contents
    count = b.length * b.channels
    if b.type == NUT_BUFFER_U8:
        return np.ctypeslib.as_array(b.data.u8, shape=(count,)).copy()
    return np.ctypeslib.as_array(b.data.f64, shape=(count,)).copy()
