"""ctypes binding of libfsea_hip.so (include/fsea.h).  No compute happens here."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

UNITS_AUTO, UNITS_STATIC, UNITS_TICKETS = 0, 1, 2
MODE_MAG_F32 = 0
MODE_DB10_U8 = 1
MODE_DB5_U8_DCFIX = 2
MODE_COMPLEX_F32 = 3
MODE_MAG_NODC_F32 = 4
MODE_DB_F32 = 5
WINDOW_RECT, WINDOW_HANN, WINDOW_HAMMING, WINDOW_BLACKMAN, WINDOW_BLACKMANHARRIS, WINDOW_FLATTOP = range(6)
WINDOW_KINDS = {"rect": 0, "boxcar": 0, "hann": 1, "hamming": 2, "blackman": 3, "blackmanharris": 4, "flattop": 5}

_MODE_DTYPE = {
    MODE_MAG_F32: np.float32, MODE_DB10_U8: np.uint8, MODE_DB5_U8_DCFIX: np.uint8,
    MODE_COMPLEX_F32: np.complex64, MODE_MAG_NODC_F32: np.float32, MODE_DB_F32: np.float32,
}

FIR_MAX_TAPS = 512          # FSEA_FIR_MAX_TAPS (include/fsea.h)
ZOOM_MAX_DECIMATION = 64    # FSEA_ZOOM_MAX_DECIMATION
ZOOM_TILE_OUTPUTS = 128     # FSEA_ZOOM_TILE_OUTPUTS: outputs per workgroup of fsea_shift_decim_u8
PFB_MAX_CHANNELS = 16384    # FSEA_PFB_MAX_CHANNELS
PFB_MAX_BRANCH_TAPS = 16    # FSEA_PFB_MAX_BRANCH_TAPS
PERSIST_LEVELS = 256        # FSEA_PERSIST_LEVELS
PERSIST_MAX_WIDTH = 65536   # FSEA_PERSIST_MAX_WIDTH
PERSIST_RUN_ROWS = 1024     # FSEA_PERSIST_RUN_ROWS: rows per workgroup of fsea_persist_u8 / fsea_persist_f32
PERSIST_U8, PERSIST_F32 = 0, 1                                       # FSEA_PERSIST_*: element type of a row
PERSIST_MAP_SATURATE, PERSIST_MAP_LINEAR, PERSIST_MAP_LOG = 0, 1, 2  # FSEA_PERSIST_MAP_*
PERSIST_TRACE_MAX, PERSIST_TRACE_MIN, PERSIST_TRACE_QUANTILE = 0, 1, 2   # FSEA_PERSIST_TRACE_*
CFAR_MAX_WIDTH = 1 << 20     # FSEA_CFAR_MAX_WIDTH
CFAR_MAX_GUARD = 64         # FSEA_CFAR_MAX_GUARD
CFAR_MAX_TRAIN = 256        # FSEA_CFAR_MAX_TRAIN, per side
CFAR_MAX_OFFSET = 1 << 20   # FSEA_CFAR_MAX_OFFSET
CFAR_F32_SCALE = 64         # FSEA_CFAR_F32_SCALE: f32 dB rows are taken in 1/64 dB
CFAR_TILE_COLUMNS = 1024    # FSEA_CFAR_TILE_COLUMNS: columns per workgroup of fsea_cfar_u8 / fsea_cfar_f32
CFAR_RUN_ROWS = 64          # FSEA_CFAR_RUN_ROWS: rows per workgroup
CFAR_U8, CFAR_F32 = 0, 1                # FSEA_CFAR_*: element type of a row
CFAR_CA, CFAR_GO, CFAR_SO = 0, 1, 2     # FSEA_CFAR_*: method
OSCFAR_TILE_COLUMNS = 1024  # FSEA_OSCFAR_TILE_COLUMNS: columns per workgroup of fsea_oscfar_u8 / fsea_oscfar_f32
OSCFAR_RUN_ROWS = 64        # FSEA_OSCFAR_RUN_ROWS: rows per workgroup
TCFAR_TILE_COLUMNS = 1024   # FSEA_TCFAR_TILE_COLUMNS: columns per workgroup of fsea_tcfar_u8 / fsea_tcfar_f32
TCFAR_RUN_ROWS = 32         # FSEA_TCFAR_RUN_ROWS: rows a workgroup decides
TCFAR_MASK_SET, TCFAR_MASK_OR, TCFAR_MASK_AND = 0, 1, 2   # FSEA_TCFAR_MASK_*: what an add does with the mask already there
CFAR_BAND = np.dtype([("first", "<i4"), ("last", "<i4"), ("peak", "<i4"), ("peak_hits", "<u4"), ("hits_sum", "<u8")])   # fsea_cfar_band
EVENTS_MAX_WIDTH = 1 << 20      # FSEA_EVENTS_MAX_WIDTH
EVENTS_MAX_GAP_COLS = 64        # FSEA_EVENTS_MAX_GAP_COLS
EVENTS_MAX_GAP_ROWS = 1 << 16   # FSEA_EVENTS_MAX_GAP_ROWS
EVENTS_NO_EVENT = 0xFFFFFFFF    # FSEA_EVENTS_NO_EVENT: event_of_run of a run whose event the filters dropped
EVENTS_RUN = np.dtype([("row", "<u4"), ("first", "<u4"), ("last", "<u4"), ("hits", "<u4"), ("peak", "<i4"), ("peak_col", "<u4"),
                       ("level_sum", "<i8")])   # fsea_events_run
EVENTS_EVENT = np.dtype([("row_first", "<u4"), ("row_last", "<u4"), ("col_first", "<u4"), ("col_last", "<u4"), ("runs", "<u4"),
                         ("peak", "<i4"), ("peak_row", "<u4"), ("peak_col", "<u4"), ("hits", "<u8"), ("level_sum", "<i8")])   # fsea_events_event
IQ_U8, IQ_F32, IQ_F64 = 0, 1, 2   # FSEA_IQ_* input types (include/fsea.h)
EXTRACT_MAX_JOBS = 65536        # FSEA_EXTRACT_MAX_JOBS
MEASURE_TILE_PAIRS = 4096       # FSEA_MEASURE_TILE_PAIRS: pairs per workgroup of fsea_measure_tiles
MEASURE_MAX_JOBS = 65536        # FSEA_MEASURE_MAX_JOBS
MEASURE_MAX_PAIRS = 1 << 24     # FSEA_MEASURE_MAX_PAIRS, per job
MEASURE_MAX_LAG = 65536         # FSEA_MEASURE_MAX_LAG
AUDIO_FM, AUDIO_AM = 0, 1       # FSEA_AUDIO_*: kind
AUDIO_MAX_DECIMATION = 64       # FSEA_AUDIO_MAX_DECIMATION
AUDIO_MAX_JOBS = 65536          # FSEA_AUDIO_MAX_JOBS
AUDIO_MAX_PAIRS = 1 << 24       # FSEA_AUDIO_MAX_PAIRS, per job
SPECTRA_Z, SPECTRA_ENVELOPE, SPECTRA_SQUARE, SPECTRA_FOURTH = 0, 1, 2, 3   # FSEA_SPECTRA_*: kind
SPECTRA_KINDS = {"z": 0, "env": 1, "sq": 2, "fourth": 3}
SPECTRA_MIN_N, SPECTRA_MAX_N = 64, 4096   # FSEA_SPECTRA_MIN_N, FSEA_SPECTRA_MAX_N
SPECTRA_TILE_SEGMENTS = 32      # FSEA_SPECTRA_TILE_SEGMENTS: segments per workgroup of fsea_spectra_tiles_<n>
SPECTRA_MAX_JOBS = 65536        # FSEA_SPECTRA_MAX_JOBS
SPECTRA_MAX_PAIRS = 1 << 24     # FSEA_SPECTRA_MAX_PAIRS, per job
IQ_MAX_MULTIPLIER = 16      # FSEA_IQ_MAX_MULTIPLIER
DEMOD_RAW, DEMOD_WBFM = 0, 1        # FSEA_DEMOD_* (= nrf_demodulate_type)
DEMOD_MAX_CHANNELS = 256            # FSEA_DEMOD_MAX_CHANNELS
DEMOD_MAX_SAMPLES = 1 << 24         # FSEA_DEMOD_MAX_SAMPLES

class InterpGeometry(ctypes.Structure):
    """fsea_interp_geometry (include/fsea.h)."""
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("iq_size", ctypes.c_int), ("flip", ctypes.c_int)]


class TraceConfig(ctypes.Structure):
    """fsea_trace_config (include/fsea.h)."""
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("size_multiplier", ctypes.c_int),
                ("pixel_inc", ctypes.c_int), ("fade", ctypes.c_int)]


class ChainStage(ctypes.Structure):
    """fsea_chain_stage (include/fsea.h)."""
    _fields_ = [("flip", ctypes.c_int), ("shift", ctypes.c_int), ("cycles_per_sample", ctypes.c_double),
                ("phase0_cycles", ctypes.c_double), ("sample_offset", ctypes.c_uint64), ("n_zero", ctypes.c_size_t)]


class ChainOutputs(ctypes.Structure):
    """fsea_chain_outputs (include/fsea.h)."""
    _fields_ = [("points", ctypes.c_void_p), ("lines", ctypes.c_void_p), ("size_multiplier", ctypes.c_int),
                ("n_line_points", ctypes.c_size_t), ("pairs", ctypes.c_void_p)]


class ExtractJob(ctypes.Structure):
    """fsea_extract_job (include/fsea.h): one cut-out of a resident recording."""
    _fields_ = [("first", ctypes.c_uint64), ("n_samples", ctypes.c_uint64), ("sample_offset", ctypes.c_uint64),
                ("cycles_per_sample", ctypes.c_double), ("phase0_cycles", ctypes.c_double), ("out_first", ctypes.c_uint64)]


class MeasureJob(ctypes.Structure):
    """fsea_measure_job (include/fsea.h): a span of a resident buffer of pairs."""
    _fields_ = [("first_pair", ctypes.c_uint64), ("n_pairs", ctypes.c_uint64)]


class MeasureSums(ctypes.Structure):
    """fsea_measure_sums (include/fsea.h): the moment sums of one job."""
    _fields_ = [("s_re", ctypes.c_double), ("s_im", ctypes.c_double), ("p", ctypes.c_double), ("q", ctypes.c_double),
                ("r_re", ctypes.c_double), ("r_im", ctypes.c_double), ("peak", ctypes.c_double), ("peak_index", ctypes.c_uint64),
                ("n_pairs", ctypes.c_uint64), ("n_lagged", ctypes.c_uint64)]


class MeasureResult(ctypes.Structure):
    """fsea_measure_result (include/fsea.h): what fsea_measure_finish makes of the sums."""
    _fields_ = [("mean_power", ctypes.c_double), ("power_db", ctypes.c_double), ("dc_re", ctypes.c_double), ("dc_im", ctypes.c_double),
                ("freq_cycles", ctypes.c_double), ("coherence", ctypes.c_double), ("width_cycles", ctypes.c_double),
                ("kurtosis", ctypes.c_double), ("crest", ctypes.c_double), ("peak_index", ctypes.c_uint64), ("n_pairs", ctypes.c_uint64)]


class AudioJob(ctypes.Structure):
    """fsea_audio_job (include/fsea.h): a span of a resident buffer of pairs and the place of its audio."""
    _fields_ = [("first_pair", ctypes.c_uint64), ("n_pairs", ctypes.c_uint64), ("out_first", ctypes.c_uint64)]


class SpectraJob(ctypes.Structure):
    """fsea_spectra_job (include/fsea.h): a span of a resident buffer of pairs and the place of its n powers."""
    _fields_ = [("first_pair", ctypes.c_uint64), ("n_pairs", ctypes.c_uint64), ("out_first", ctypes.c_uint64)]


class SpectraResult(ctypes.Structure):
    """fsea_spectra_result (include/fsea.h): what fsea_spectra_finish makes of one row of powers."""
    _fields_ = [("total", ctypes.c_double), ("centroid_cycles", ctypes.c_double), ("obw_centre_cycles", ctypes.c_double),
                ("peak_power", ctypes.c_double), ("peak_cycles", ctypes.c_double), ("floor", ctypes.c_double), ("line_db", ctypes.c_double),
                ("obw_lo", ctypes.c_int32), ("obw_hi", ctypes.c_int32), ("obw_bins", ctypes.c_int32), ("peak_bin", ctypes.c_int32)]


class CaptureRun(ctypes.Structure):
    """fsea_capture_run (include/fsea.h)."""
    _fields_ = [("first_block", ctypes.c_size_t), ("n_blocks", ctypes.c_size_t), ("continues", ctypes.c_int),
                ("open", ctypes.c_int)]


class CaptureBurstInfo(ctypes.Structure):
    """fsea_capture_burst_info (include/fsea.h)."""
    _fields_ = [("first_block", ctypes.c_size_t), ("n_blocks", ctypes.c_size_t), ("n_pairs", ctypes.c_size_t),
                ("open", ctypes.c_int), ("d_pairs", ctypes.c_void_p)]


# Every function include/fsea.h declares, once: name -> (restype, argtypes).  hip_lib() applies the table, EXPORTS is its
# names; tests check both against the header and the built library.
_vp, _sz, _ci, _f64, _u32, _u64, _str = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_uint32,
                                         ctypes.c_uint64, ctypes.c_char_p)
_out = ctypes.POINTER(_vp)        # where a create / alloc function puts its handle
_f32p, _uip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint)
_stage, _outputs, _geo = ctypes.POINTER(ChainStage), ctypes.POINTER(ChainOutputs), ctypes.POINTER(InterpGeometry)
_f64p, _szp = ctypes.POINTER(_f64), ctypes.POINTER(_sz)
API = {
    "fsea_device_count": (_ci, [ctypes.POINTER(_ci)]),
    "fsea_last_error_string": (_str, []),
    "fsea_plan_create": (_ci, [_out, _ci, _ci, _ci, _ci]),
    "fsea_plan_destroy": (_ci, [_vp]),
    "fsea_plan_reset": (_ci, [_vp]),
    "fsea_plan_release_stream": (_ci, [_vp, _vp]),
    "fsea_plan_grid": (_ci, [_vp, _sz, _uip, _uip, ctypes.POINTER(_sz)]),
    "fsea_plan_row_bytes": (_sz, [_vp]),
    "fsea_plan_fft_size": (_ci, [_vp]),
    "fsea_plan_kernel_name": (_str, [_vp]),
    "fsea_plan_set_unit_distribution": (_ci, [_vp, _ci]),
    "fsea_plan_set_window": (_ci, [_vp, _vp]),
    "fsea_plan_window_form": (_ci, [_vp]),
    "fsea_window_fill": (_ci, [_ci, _ci, _vp]),
    "fsea_exec_u8_device": (_ci, [_vp, _vp, _sz, _ci, _vp, _vp]),
    "fsea_exec_u8_tiled_device": (_ci, [_vp, _vp, _sz, _ci, _vp, _sz, _sz, _sz, _sz, _sz, _vp]),
    "fsea_exec_u8_host": (_ci, [_vp, _vp, _sz, _ci, _vp]),
    "fsea_exec_f64_host": (_ci, [_vp, _vp, _sz, _vp]),
    "fsea_exec_u8_shifted_device": (_ci, [_vp, _vp, _sz, _ci, _f64, _f64, _vp, _vp]),
    "fsea_exec_u8_shifted_host": (_ci, [_vp, _vp, _sz, _ci, _f64, _f64, _vp]),
    "fsea_mean_magnitude_u8_device": (_ci, [_vp, _vp, _sz, _ci, ctypes.POINTER(_f64), _vp]),
    "fsea_composite_max_device": (_ci, [_vp, _vp] + [_u32] * 7 + [_ci, _vp]),
    "fsea_stitch_tiles_device": (_ci, [_vp, _vp] + [_u32] * 6 + [_ci, _vp]),
    "fsea_device_alloc": (_ci, [_ci, _sz, _out]),
    "fsea_device_free": (_ci, [_ci, _vp]),
    "fsea_copy_to_device": (_ci, [_ci, _vp, _vp, _sz]),
    "fsea_copy_to_host": (_ci, [_ci, _vp, _vp, _sz]),
    "fsea_stream_create": (_ci, [_ci, _out]),
    "fsea_stream_destroy": (_ci, [_ci, _vp]),
    "fsea_stream_synchronize": (_ci, [_vp, _vp]),
    "fsea_copy_to_device_async": (_ci, [_ci, _vp, _vp, _sz, _vp]),
    "fsea_copy_to_host_async": (_ci, [_ci, _vp, _vp, _sz, _vp]),
    "fsea_host_alloc": (_ci, [_sz, _out]),
    "fsea_host_free": (_ci, [_vp]),
    "fsea_history_create": (_ci, [_vp, _ci, _out]),
    "fsea_history_destroy": (_ci, [_vp]),
    "fsea_history_push_u8_host": (_ci, [_vp, _vp, _ci]),
    "fsea_history_push_f64_host": (_ci, [_vp, _vp]),
    "fsea_history_shift": (_ci, [_vp, _ci]),
    "fsea_history_get_f64": (_ci, [_vp, _vp]),
    "fsea_fir_lowpass_taps": (_ci, [_f64, _f64, _ci, _vp]),
    "fsea_fir_create": (_ci, [_out, _vp, _ci, _ci]),
    "fsea_fir_destroy": (_ci, [_vp]),
    "fsea_fir_reset": (_ci, [_vp]),
    "fsea_fir_n_taps": (_ci, [_vp]),
    "fsea_fir_u8_device": (_ci, [_vp, _vp, _sz, _ci, _vp, _vp]),
    "fsea_fir_u8_host": (_ci, [_vp, _vp, _sz, _ci, _vp]),
    "fsea_fir_f64_host": (_ci, [_vp, _vp, _sz, _vp]),
    "fsea_fir_u8_shifted_device": (_ci, [_vp, _vp, _sz, _ci, _f64, _f64, _u64, _vp, _vp]),
    "fsea_fir_u8_shifted_host": (_ci, [_vp, _vp, _sz, _ci, _f64, _f64, _u64, _vp]),
    "fsea_chain_create": (_ci, [_out, _vp, _ci, _ci]),
    "fsea_chain_destroy": (_ci, [_vp]),
    "fsea_chain_reset": (_ci, [_vp]),
    "fsea_chain_n_pairs": (_sz, [_vp]),
    "fsea_chain_run_host": (_ci, [_vp, _vp, _sz, _stage, _outputs]),
    "fsea_chain_run_f64_host": (_ci, [_vp, _vp, _sz, _outputs]),
    "fsea_chain_fetch_host": (_ci, [_vp, _outputs]),
    "fsea_chain_run_device": (_ci, [_vp, _vp, _sz, _ci, _stage, _outputs, _vp]),
    "fsea_zoom_create": (_ci, [_out, _vp, _ci, _ci, _ci, _ci, _ci, _ci]),
    "fsea_zoom_destroy": (_ci, [_vp]),
    "fsea_zoom_reset": (_ci, [_vp]),
    "fsea_zoom_set_window": (_ci, [_vp, _vp]),
    "fsea_zoom_out_pairs": (_sz, [_vp, _sz]),
    "fsea_zoom_out_rows": (_sz, [_vp, _sz]),
    "fsea_zoom_row_bytes": (_sz, [_vp]),
    "fsea_zoom_run_device": (_ci, [_vp, _vp, _sz, _ci, _f64, _f64, _u64, _vp, _vp, _vp]),
    "fsea_zoom_run_host": (_ci, [_vp, _vp, _sz, _ci, _f64, _f64, _u64, _vp, _vp]),
    "fsea_pfb_prototype": (_ci, [_ci, _ci, _vp]),
    "fsea_pfb_create": (_ci, [_out, _vp, _ci, _ci, _ci, _ci, _ci]),
    "fsea_pfb_destroy": (_ci, [_vp]),
    "fsea_pfb_reset": (_ci, [_vp]),
    "fsea_pfb_out_frames": (_sz, [_vp, _sz]),
    "fsea_pfb_row_bytes": (_sz, [_vp]),
    "fsea_pfb_run_device": (_ci, [_vp, _vp, _sz, _ci, _vp, _vp, _vp, _vp]),
    "fsea_pfb_run_host": (_ci, [_vp, _vp, _sz, _ci, _vp, _vp, _vp]),
    "fsea_persist_create": (_ci, [_out, _ci, _ci]),
    "fsea_persist_destroy": (_ci, [_vp]),
    "fsea_persist_reset": (_ci, [_vp]),
    "fsea_persist_set_range": (_ci, [_vp, ctypes.c_float, ctypes.c_float]),
    "fsea_persist_width": (_ci, [_vp]),
    "fsea_persist_rows": (_u64, [_vp]),
    "fsea_persist_add_device": (_ci, [_vp, _vp, _ci, _sz, _sz, _vp]),
    "fsea_persist_add_host": (_ci, [_vp, _vp, _ci, _sz, _sz]),
    "fsea_persist_decay": (_ci, [_vp, _u32, _u32, _vp]),
    "fsea_persist_counts_host": (_ci, [_vp, _vp]),
    "fsea_persist_image_device": (_ci, [_vp, _ci, _u64, _vp, _vp]),
    "fsea_persist_image_host": (_ci, [_vp, _ci, _u64, _vp]),
    "fsea_persist_trace": (_ci, [_vp, _ci, _ci, _f64, _vp]),
    "fsea_cfar_create": (_ci, [_out, _ci, _ci]),
    "fsea_cfar_destroy": (_ci, [_vp]),
    "fsea_cfar_reset": (_ci, [_vp]),
    "fsea_cfar_set": (_ci, [_vp, _ci, _ci, _ci, _ci]),
    "fsea_cfar_width": (_ci, [_vp]),
    "fsea_cfar_rows": (_u64, [_vp]),
    "fsea_cfar_add_device": (_ci, [_vp, _vp, _ci, _sz, _sz, _vp, _vp, _vp]),
    "fsea_cfar_add_host": (_ci, [_vp, _vp, _ci, _sz, _sz, _vp, _vp]),
    "fsea_cfar_hits_host": (_ci, [_vp, _vp]),
    "fsea_cfar_bands": (_ci, [_vp, _ci, _u64, _f64, _ci, _ci, _vp, _sz, _szp]),
    "fsea_oscfar_create": (_ci, [_out, _ci, _ci]),
    "fsea_oscfar_destroy": (_ci, [_vp]),
    "fsea_oscfar_reset": (_ci, [_vp]),
    "fsea_oscfar_set": (_ci, [_vp, _ci, _ci, _ci, _ci]),
    "fsea_oscfar_width": (_ci, [_vp]),
    "fsea_oscfar_rows": (_u64, [_vp]),
    "fsea_oscfar_rank": (_ci, [_vp]),
    "fsea_oscfar_add_device": (_ci, [_vp, _vp, _ci, _sz, _sz, _vp, _vp, _vp]),
    "fsea_oscfar_add_host": (_ci, [_vp, _vp, _ci, _sz, _sz, _vp, _vp]),
    "fsea_oscfar_hits_host": (_ci, [_vp, _vp]),
    "fsea_tcfar_create": (_ci, [_out, _ci, _ci]),
    "fsea_tcfar_destroy": (_ci, [_vp]),
    "fsea_tcfar_reset": (_ci, [_vp]),
    "fsea_tcfar_set": (_ci, [_vp, _ci, _ci, _ci, _ci, _ci]),
    "fsea_tcfar_width": (_ci, [_vp]),
    "fsea_tcfar_rows": (_u64, [_vp]),
    "fsea_tcfar_run_rows": (_ci, [_vp]),
    "fsea_tcfar_add_device": (_ci, [_vp, _vp, _ci, _sz, _sz, _sz, _sz, _vp, _vp, _vp]),
    "fsea_tcfar_add_host": (_ci, [_vp, _vp, _ci, _sz, _sz, _sz, _sz, _vp, _vp]),
    "fsea_tcfar_hits_host": (_ci, [_vp, _vp]),
    "fsea_events_create": (_ci, [_out, _ci, _ci]),
    "fsea_events_destroy": (_ci, [_vp]),
    "fsea_events_reset": (_ci, [_vp]),
    "fsea_events_set_gap": (_ci, [_vp, _ci]),
    "fsea_events_width": (_ci, [_vp]),
    "fsea_events_rows": (_u64, [_vp]),
    "fsea_events_runs_device": (_ci, [_vp, _vp, _sz, _vp, _ci, _sz, _sz, _vp, _sz, _szp, _vp]),
    "fsea_events_runs_host": (_ci, [_vp, _vp, _sz, _vp, _ci, _sz, _sz, _vp, _sz, _szp]),
    "fsea_events_link": (_ci, [_vp, _sz, _ci, _ci, _u32, _u32, _u64, _vp, _vp, _sz, _szp]),
    "fsea_events_paint_device": (_ci, [_vp, _vp, _vp, _sz, _u64, _sz, _vp, _sz, _vp]),
    "fsea_events_paint_host": (_ci, [_vp, _vp, _vp, _sz, _u64, _sz, _vp, _sz]),
    "fsea_extract_create": (_ci, [_out, _vp, _ci, _ci, _ci]),
    "fsea_extract_destroy": (_ci, [_vp]),
    "fsea_extract_decimation": (_ci, [_vp]),
    "fsea_extract_n_taps": (_ci, [_vp]),
    "fsea_extract_out_pairs": (_sz, [_vp, _sz]),
    "fsea_extract_lead": (_sz, [_ci, _ci]),
    "fsea_extract_layout": (_ci, [_vp, _vp, _sz, _szp]),
    "fsea_extract_run_device": (_ci, [_vp, _vp, _sz, _ci, _vp, _sz, _vp, _sz, _vp]),
    "fsea_extract_run_host": (_ci, [_vp, _vp, _sz, _ci, _vp, _sz, _vp, _sz]),
    "fsea_extract_jobs": (_ci, [_vp, _sz, _ci, _ci, _u64, _ci, _ci, _f64, _vp, _vp]),
    "fsea_measure_create": (_ci, [_out, _ci]),
    "fsea_measure_destroy": (_ci, [_vp]),
    "fsea_measure_run_device": (_ci, [_vp, _vp, _sz, _vp, _sz, _f64, _f64, _ci, _vp, _vp]),
    "fsea_measure_run_host": (_ci, [_vp, _vp, _sz, _vp, _sz, _f64, _f64, _ci, _vp]),
    "fsea_measure_jobs": (_ci, [_vp, _sz, _ci, _sz, _vp]),
    "fsea_measure_finish": (_ci, [_vp, _ci, _vp]),
    "fsea_audio_create": (_ci, [_out, _ci, _vp, _ci, _ci, _ci]),
    "fsea_audio_destroy": (_ci, [_vp]),
    "fsea_audio_kind": (_ci, [_vp]),
    "fsea_audio_decimation": (_ci, [_vp]),
    "fsea_audio_n_taps": (_ci, [_vp]),
    "fsea_audio_layout": (_ci, [_vp, _vp, _sz, _szp]),
    "fsea_audio_run_device": (_ci, [_vp, _vp, _sz, _vp, _sz, _f64, _f64, _f64, _vp, _sz, _vp]),
    "fsea_audio_run_host": (_ci, [_vp, _vp, _sz, _vp, _sz, _f64, _f64, _f64, _vp, _sz]),
    "fsea_spectra_create": (_ci, [_out, _ci, _ci, _ci, _vp, _ci]),
    "fsea_spectra_destroy": (_ci, [_vp]),
    "fsea_spectra_n": (_ci, [_vp]),
    "fsea_spectra_hop": (_ci, [_vp]),
    "fsea_spectra_kind": (_ci, [_vp]),
    "fsea_spectra_segments": (_sz, [_vp, _sz]),
    "fsea_spectra_layout": (_ci, [_vp, _vp, _sz, _szp]),
    "fsea_spectra_run_device": (_ci, [_vp, _vp, _sz, _vp, _sz, _f64, _f64, _vp, _sz, _vp]),
    "fsea_spectra_run_host": (_ci, [_vp, _vp, _sz, _vp, _sz, _f64, _f64, _vp, _sz]),
    "fsea_spectra_jobs": (_ci, [_vp, _sz, _ci, _sz, _vp]),
    "fsea_spectra_finish": (_ci, [_vp, _ci, _ci, _f64, _vp]),
    "fsea_iq_draw_create": (_ci, [_out, _ci]),
    "fsea_iq_draw_destroy": (_ci, [_vp]),
    "fsea_iq_points_device": (_ci, [_vp, _vp, _ci, _ci, _sz, _ci, _vp, _vp]),
    "fsea_iq_lines_device": (_ci, [_vp, _vp, _ci, _ci, _sz, _ci, _ci, _vp, _vp]),
    "fsea_iq_points_host": (_ci, [_vp, _vp, _ci, _ci, _sz, _vp]),
    "fsea_iq_lines_host": (_ci, [_vp, _vp, _ci, _ci, _sz, _ci, _vp]),
    "fsea_demod_create": (_ci, [_out, _ci, _ci, _ci, _ci, _ci]),
    "fsea_demod_destroy": (_ci, [_vp]),
    "fsea_demod_reset": (_ci, [_vp]),
    "fsea_demod_set_channel": (_ci, [_vp, _ci, _ci, _f64, _f64]),
    "fsea_demod_get_channel": (_ci, [_vp, _ci, ctypes.POINTER(_ci), ctypes.POINTER(_f64), ctypes.POINTER(_f64)]),
    "fsea_demod_out_length": (_sz, [_vp, _sz]),
    "fsea_demod_u8_device": (_ci, [_vp, _vp, _sz, _ci, _vp, _vp]),
    "fsea_demod_u8_host": (_ci, [_vp, _vp, _sz, _ci, _vp]),
    "fsea_demod_f64_host": (_ci, [_vp, _vp, _vp, _sz, _vp]),
    "fsea_interp_create": (_ci, [_out, _ci, _sz, _ci]),
    "fsea_interp_destroy": (_ci, [_vp]),
    "fsea_interp_reset": (_ci, [_vp]),
    "fsea_interp_n_elements": (_sz, [_vp]),
    "fsea_interp_push_device": (_ci, [_vp, _vp, _vp]),
    "fsea_interp_push_host": (_ci, [_vp, _vp]),
    "fsea_interp_frames_device": (_ci, [_vp, _vp, _ci, _vp, _vp]),
    "fsea_interp_frames_host": (_ci, [_vp, _vp, _ci, _vp]),
    "fsea_interp_image_tables": (_ci, [_ci, _ci, _ci, _vp, _vp]),
    "fsea_interp_image_frames_device": (_ci, [_vp, _vp, _ci, _geo, _vp, _vp]),
    "fsea_interp_image_frames_host": (_ci, [_vp, _vp, _ci, _geo, _vp]),
    "fsea_trace_create": (_ci, [_out, ctypes.POINTER(TraceConfig), _ci]),
    "fsea_trace_destroy": (_ci, [_vp]),
    "fsea_trace_reset": (_ci, [_vp]),
    "fsea_trace_frames_device": (_ci, [_vp, _vp, _sz, _ci, _sz, _ci, _vp, _vp]),
    "fsea_trace_frames_host": (_ci, [_vp, _vp, _sz, _ci, _sz, _ci, _vp]),
    "fsea_trace_canvas_host": (_ci, [_vp, _vp]),
    "fsea_detect_create": (_ci, [_out, _ci]),
    "fsea_detect_destroy": (_ci, [_vp]),
    "fsea_detect_u8_device": (_ci, [_vp, _vp, _sz, _sz, _ci, _vp, _vp]),
    "fsea_detect_u8_host": (_ci, [_vp, _vp, _sz, _sz, _ci, _vp, _vp]),
    "fsea_detect_moments": (_ci, [_vp, _sz, _f64p, _f64p]),
    "fsea_detect_finish": (_ci, [_vp, _sz, _f64p, _f64p]),
    "fsea_capture_create": (_ci, [_out, _vp, _ci, _ci]),
    "fsea_capture_destroy": (_ci, [_vp]),
    "fsea_capture_reset": (_ci, [_vp]),
    "fsea_capture_scan_device": (_ci, [_vp, _vp, _sz, _sz, _ci, _f64, _vp]),
    "fsea_capture_scan_host": (_ci, [_vp, _vp, _sz, _sz, _ci, _f64]),
    "fsea_capture_segment": (_ci, [_vp, _sz, _f64, _ci, ctypes.POINTER(CaptureRun), _szp]),
    "fsea_capture_n_blocks": (_sz, [_vp]),
    "fsea_capture_stats": (_ci, [_vp, _sz, _f64p, _f64p]),
    "fsea_capture_n_bursts": (_sz, [_vp]),
    "fsea_capture_burst": (_ci, [_vp, _sz, ctypes.POINTER(CaptureBurstInfo)]),
    "fsea_capture_burst_pairs_host": (_ci, [_vp, _sz, _vp]),
    "fsea_capture_burst_lines_device": (_ci, [_vp, _sz, _ci, _sz, _vp, _vp]),
    "fsea_capture_burst_lines_host": (_ci, [_vp, _sz, _ci, _sz, _vp]),
}
# include/fsea_tune.h: only libfsea_hip_tune.so (scripts/tune.py and friends) has these
TUNE_API = {
    "fsea_plan_create_variant": (_ci, [_out, _ci, _ci, _ci, _ci, _str]),
    "fsea_time_exec_u8_device": (_ci, [_vp, _vp, _sz, _ci, _vp, _vp, _ci, _f32p]),
    "fsea_time_exec_u8_rotating": (_ci, [_vp, _out, _out, _ci, _sz, _ci, _vp, _ci, _f32p]),
    "fsea_plan_read_trace": (_ci, [_vp, _vp, ctypes.c_uint]),
    "fsea_tune_stream_1to2": (_ci, [_out, _out, _ci, _sz, _ci, _vp, _ci, _f32p]),
}
EXPORTS, TUNE_EXPORTS = list(API), list(TUNE_API)


def declare(L, names=None):
    """Attach restype and argtypes to the functions of a loaded build of the library: the one place they are assigned.
    Without names: all of include/fsea.h, and of include/fsea_tune.h where the build is the tuning library.  With names:
    those only (a script that loads another build of the library, which may not have every function)."""
    if names is None:
        names = EXPORTS + (TUNE_EXPORTS if hasattr(L, "fsea_plan_create_variant") else [])
    for name in names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = API[name] if name in API else TUNE_API[name]
    return L


class FseaError(RuntimeError):
    pass


_USE_TUNE = False


def use_tune_library():
    """Measurement scripts call this first: load libfsea_hip_tune.so (a superset build with kernel
    variants, ablations, traces and the timing helper) instead of the product library."""
    global _USE_TUNE
    if _LIB is not None and not _USE_TUNE:
        raise FseaError("use_tune_library() must be called before the library is first used")
    _USE_TUNE = True


def tune_lib_path():
    return os.path.join(_HERE, "libfsea_hip_tune.so")


def lib_path():
    # FSEA_HIP_LIB: load an alternative build of the same library
    if os.environ.get("FSEA_HIP_LIB"):
        return os.environ["FSEA_HIP_LIB"]
    return tune_lib_path() if _USE_TUNE else os.path.join(_HERE, "libfsea_hip.so")


def build(jobs=8):
    """Compile libfsea_hip.so and libfsea_nrf.so in-tree (hipcc cross-compiles gfx950)."""
    subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", os.path.join(_HERE, "csrc")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "host")])


_LIB = None


def hip_lib():
    """Load libfsea_hip.so; raises loudly if it was not built (no fallback)."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise FseaError("libfsea_hip.so is missing: run frequensea_amd.build() / __graft_entry__.build()")
        _LIB = declare(ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL))
    return _LIB


def _check(rc):
    if rc != 0:
        raise FseaError("fsea error %d: %s" % (rc, hip_lib().fsea_last_error_string().decode()))


def window(kind, n):
    """fsea_window_fill: the periodic cosine-sum taper `kind` (a name of WINDOW_KINDS or a number) as n float32 weights."""
    w = np.empty(n, dtype=np.float32)
    _check(hip_lib().fsea_window_fill(WINDOW_KINDS[kind] if isinstance(kind, str) else int(kind), n, w.ctypes.data))
    return w


def device_count():
    n = ctypes.c_int(0)
    hip_lib().fsea_device_count(ctypes.byref(n))
    return n.value


class _Handle:
    """An object behind the C ABI: the library (self._L), the handle fsea_<kind>_create gave (self._p), and its destroy."""
    _kind = None    # "plan", "fir", ...: the X of fsea_X_destroy and fsea_X_reset
    _p = None

    def _create(self, create, *args):
        self._L = hip_lib()
        self._p = ctypes.c_void_p()
        _check(getattr(self._L, create)(ctypes.byref(self._p), *args))

    def close(self):
        if self._p:
            getattr(self._L, "fsea_%s_destroy" % self._kind)(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ResettableHandle(_Handle):
    """A _Handle whose kind has an fsea_<kind>_reset."""

    def reset(self):
        _check(getattr(self._L, "fsea_%s_reset" % self._kind)(self._p))


class Plan(_ResettableHandle):
    """One (fft_size, hop, mode) plan on one device; thin wrapper over fsea_plan_*."""
    _kind = "plan"

    def __init__(self, fft_size, hop=None, mode=MODE_MAG_F32, device=0, variant=None):
        self.fft_size = fft_size
        self.hop = fft_size if hop is None else hop
        self.mode = mode
        self.device = device
        # variant None: the product plan (its mode's configuration of the size); "" (tuning library): the size's first
        # configuration whatever the mode; a name: that tuning / per-mode configuration
        tuning = hasattr(hip_lib(), "fsea_plan_create_variant")
        if variant is None or (variant == "" and not tuning):
            self._create("fsea_plan_create", fft_size, self.hop, mode, device)
        elif not tuning:
            raise FseaError("kernel variants live in libfsea_hip_tune.so: call fsea.use_tune_library() first")
        else:
            self._create("fsea_plan_create_variant", fft_size, self.hop, mode, device, variant.encode())

    @property
    def row_bytes(self):
        return self._L.fsea_plan_row_bytes(self._p)

    @property
    def out_dtype(self):
        return _MODE_DTYPE[self.mode]

    @property
    def kernel_name(self):
        return self._L.fsea_plan_kernel_name(self._p).decode()

    def grid(self, n_frames):
        g, b, l = ctypes.c_uint(0), ctypes.c_uint(0), ctypes.c_size_t(0)
        _check(self._L.fsea_plan_grid(self._p, n_frames, ctypes.byref(g), ctypes.byref(b), ctypes.byref(l)))
        return g.value, b.value, l.value

    def in_bytes(self, n_frames):
        return 2 * ((n_frames - 1) * self.hop + self.fft_size) if n_frames else 0

    def exec_device(self, d_iq_ptr, n_frames, d_out_ptr, flip=True, stream=0):
        """Device pointers (ints), asynchronous on `stream` (hipStream_t as int, 0 = null stream)."""
        _check(self._L.fsea_exec_u8_device(self._p, d_iq_ptr, n_frames, int(bool(flip)), d_out_ptr,
                                           stream or None))

    def exec_tiled_device(self, d_iq_ptr, n_frames, d_image_ptr, image_rows, image_stride, first_x, tile_rows, tile_step,
                          flip=True, stream=0):
        """Rows written straight into a stitched image (fsea_exec_u8_tiled_device): frame f = row f % tile_rows of
        tile f // tile_rows, tile k at columns first_x + k * tile_step."""
        _check(self._L.fsea_exec_u8_tiled_device(self._p, d_iq_ptr, n_frames, int(bool(flip)), d_image_ptr, image_rows,
                                                 image_stride, first_x, tile_rows, tile_step, stream or None))

    def set_window(self, w):
        """fsea_plan_set_window: fft_size float32 weights (a name of WINDOW_KINDS is filled in first), None removes it."""
        if w is None:
            _check(self._L.fsea_plan_set_window(self._p, None))
            return
        if isinstance(w, str):
            w = window(w, self.fft_size)
        wf = np.ascontiguousarray(w, dtype=np.float32).ravel()
        if wf.size != self.fft_size:
            raise ValueError("a window has fft_size weights")
        _check(self._L.fsea_plan_set_window(self._p, wf.ctypes.data))

    @property
    def window_form(self):
        """0 = no window, 1 = centred form, 2 = offset-binary form (include/fsea.h)."""
        return self._L.fsea_plan_window_form(self._p)

    def set_unit_distribution(self, policy):
        """UNITS_AUTO (default), UNITS_STATIC or UNITS_TICKETS: fsea_plan_set_unit_distribution."""
        _check(self._L.fsea_plan_set_unit_distribution(self._p, policy))

    def release_stream(self, stream):
        """fsea_plan_release_stream: give back the counter slot `stream` holds (after its captured graphs are destroyed)."""
        _check(self._L.fsea_plan_release_stream(self._p, stream))

    def time_device(self, d_iq_ptr, n_frames, d_out_ptr, reps, flip=True, stream=0):
        """Tuning library only (fsea_time_exec_u8_device)."""
        if not hasattr(self._L, "fsea_time_exec_u8_device"):
            raise FseaError("the timing helper lives in libfsea_hip_tune.so: call fsea.use_tune_library() first")
        ms = ctypes.c_float(0)
        _check(self._L.fsea_time_exec_u8_device(self._p, d_iq_ptr, n_frames, int(bool(flip)), d_out_ptr,
                                                stream or None, reps, ctypes.byref(ms)))
        return ms.value

    def time_rotating(self, d_iq_ptrs, n_frames, d_out_ptrs, reps, flip=True, stream=0):
        """Tuning library only (fsea_time_exec_u8_rotating): launch i uses buffer set i % len(sets)."""
        n = len(d_iq_ptrs)
        ins = (ctypes.c_void_p * n)(*[p.value if isinstance(p, ctypes.c_void_p) else p for p in d_iq_ptrs])
        outs = (ctypes.c_void_p * n)(*[p.value if isinstance(p, ctypes.c_void_p) else p for p in d_out_ptrs])
        ms = ctypes.c_float(0)
        _check(self._L.fsea_time_exec_u8_rotating(self._p, ins, outs, n, n_frames, int(bool(flip)), stream or None, reps,
                                                  ctypes.byref(ms)))
        return ms.value

    def synchronize(self, stream=0):
        _check(self._L.fsea_stream_synchronize(self._p, stream or None))

    def exec_host(self, iq_u8, n_frames=None, flip=True):
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        if n_frames is None:
            n_frames = 0 if iq.size < 2 * self.fft_size else (iq.size // 2 - self.fft_size) // self.hop + 1
        if iq.size < self.in_bytes(n_frames):
            raise ValueError("iq too short for %d frames" % n_frames)
        out = np.empty((n_frames, self.fft_size), dtype=self.out_dtype)
        _check(self._L.fsea_exec_u8_host(self._p, iq.ctypes.data, n_frames, int(bool(flip)), out.ctypes.data))
        return out

    def exec_host_into(self, iq_u8, n_frames, out, flip=True):
        """fsea_exec_u8_host into a caller-owned array (any host memory: pageable numpy, or pinned_array())."""
        if iq_u8.nbytes < self.in_bytes(n_frames) or out.nbytes < n_frames * self.row_bytes:
            raise ValueError("buffers too short for %d frames" % n_frames)
        _check(self._L.fsea_exec_u8_host(self._p, iq_u8.ctypes.data, n_frames, int(bool(flip)), out.ctypes.data))
        return out

    def exec_shifted_device(self, d_iq_ptr, n_frames, d_out_ptr, cycles_per_sample, phase0_cycles=0.0, flip=True,
                            stream=0):
        """fsea_exec_u8_shifted_device: the frequency shifter fused into the FFT's load."""
        _check(self._L.fsea_exec_u8_shifted_device(self._p, d_iq_ptr, n_frames, int(bool(flip)), cycles_per_sample,
                                                   phase0_cycles, d_out_ptr, stream or None))

    def exec_shifted_host(self, iq_u8, n_frames, cycles_per_sample, phase0_cycles=0.0, flip=True):
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        if iq.size < self.in_bytes(n_frames):
            raise ValueError("iq too short for %d frames" % n_frames)
        out = np.empty((n_frames, self.fft_size), dtype=self.out_dtype)
        _check(self._L.fsea_exec_u8_shifted_host(self._p, iq.ctypes.data, n_frames, int(bool(flip)),
                                                 cycles_per_sample, phase0_cycles, out.ctypes.data))
        return out

    def exec_host_f64(self, iq_f64, n_frames):
        iq = np.ascontiguousarray(iq_f64, dtype=np.float64).ravel()
        if iq.size < self.in_bytes(n_frames):
            raise ValueError("iq too short for %d frames" % n_frames)
        out = np.empty((n_frames, self.fft_size), dtype=self.out_dtype)
        _check(self._L.fsea_exec_f64_host(self._p, iq.ctypes.data, n_frames, out.ctypes.data))
        return out

    def mean_magnitude_device(self, d_iq_ptr, n_frames, flip=True, stream=0):
        m = ctypes.c_double(0)
        _check(self._L.fsea_mean_magnitude_u8_device(self._p, d_iq_ptr, n_frames, int(bool(flip)),
                                                     ctypes.byref(m), stream or None))
        return m.value


def lowpass_taps(sample_rate, half_ampl_freq, length):
    """fsea_fir_lowpass_taps: the reference's low-pass design (nrf_fir_get_low_pass_coefficients), its first `length` taps."""
    taps = np.empty(max(int(length), 1), dtype=np.float64)
    _check(hip_lib().fsea_fir_lowpass_taps(float(sample_rate), float(half_ampl_freq), int(length), taps.ctypes.data))
    return taps[:length]


class Fir(_ResettableHandle):
    """A streaming complex FIR filter with real taps on one device; thin wrapper over fsea_fir_*.  Each call continues
    the signal of the previous ones (the last n_taps - 1 samples are carried over); reset() starts a new one."""
    _kind = "fir"

    def __init__(self, taps, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        self.n_taps = t.size
        self.device = device
        self._create("fsea_fir_create", t.ctypes.data if t.size else None, t.size, device)

    def run_device(self, d_iq_ptr, n_samples, d_out_ptr, flip=False, stream=0):
        """Device pointers (ints, 16-byte aligned): 2 * n_samples bytes in, n_samples complex64 out; asynchronous."""
        _check(self._L.fsea_fir_u8_device(self._p, d_iq_ptr, n_samples, int(bool(flip)), d_out_ptr, stream or None))

    def run_u8(self, iq_u8, flip=False):
        """Interleaved 8-bit IQ (host) -> complex64 of len(iq_u8) // 2 filtered samples."""
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        out = np.empty(iq.size // 2, dtype=np.complex64)
        _check(self._L.fsea_fir_u8_host(self._p, iq.ctypes.data, out.size, int(bool(flip)), out.ctypes.data))
        return out

    def run_shifted_device(self, d_iq_ptr, n_samples, d_out_ptr, cycles_per_sample, phase0_cycles=0.0, sample_offset=0,
                           flip=False, stream=0):
        """fsea_fir_u8_shifted_device: run_device with the frequency shifter fused into the load; sample_offset is the
        number of samples the stream's earlier calls consumed."""
        _check(self._L.fsea_fir_u8_shifted_device(self._p, d_iq_ptr, n_samples, int(bool(flip)), cycles_per_sample,
                                                  phase0_cycles, sample_offset, d_out_ptr, stream or None))

    def run_u8_shifted(self, iq_u8, cycles_per_sample, phase0_cycles=0.0, sample_offset=0, flip=False):
        """fsea_fir_u8_shifted_host: run_u8 with the frequency shifter fused into the load."""
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        out = np.empty(iq.size // 2, dtype=np.complex64)
        _check(self._L.fsea_fir_u8_shifted_host(self._p, iq.ctypes.data, out.size, int(bool(flip)), cycles_per_sample,
                                                phase0_cycles, sample_offset, out.ctypes.data))
        return out

    def run_f64(self, iq):
        """Complex (or interleaved float64) IQ (host) -> complex64 filtered samples."""
        a = np.asarray(iq)
        if np.iscomplexobj(a):
            flat = np.ascontiguousarray(a, dtype=np.complex128).ravel().view(np.float64)
        else:
            flat = np.ascontiguousarray(a, dtype=np.float64).ravel()
        out = np.empty(flat.size // 2, dtype=np.complex64)
        _check(self._L.fsea_fir_f64_host(self._p, flat.ctypes.data, out.size, out.ctypes.data))
        return out


class Chain(_ResettableHandle):
    """Shift -> low-pass filter -> constellation images per block, the filtered block resident on the device; thin wrapper
    over fsea_chain_*.  run() takes one 8-bit block from the host and returns what was asked for as a dict with the keys
    "points", "lines", "pairs"; fetch() draws more from the block of the last run."""
    _kind = "chain"

    def __init__(self, taps, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        self.n_taps, self.device = t.size, device
        self._create("fsea_chain_create", t.ctypes.data if t.size else None, t.size, device)

    @property
    def n_pairs(self):
        return self._L.fsea_chain_n_pairs(self._p)

    @staticmethod
    def stage(flip=False, cycles_per_sample=None, phase0_cycles=0.0, sample_offset=0, n_zero=0):
        """A ChainStage; cycles_per_sample None = no shift."""
        return ChainStage(int(bool(flip)), int(cycles_per_sample is not None), float(cycles_per_sample or 0.0),
                          float(phase0_cycles), int(sample_offset), int(n_zero))

    def _outputs(self, n_pairs, points, lines_m, n_line_points, pairs):
        res, o = {}, ChainOutputs(None, None, 1, 0, None)
        if points:
            res["points"] = np.empty((256, 256), dtype=np.uint8)
            o.points = res["points"].ctypes.data
        if lines_m:
            res["lines"] = np.empty((256 * lines_m, 256 * lines_m), dtype=np.uint8)
            o.lines, o.size_multiplier = res["lines"].ctypes.data, int(lines_m)
            o.n_line_points = n_pairs if n_line_points is None else int(n_line_points)
        if pairs:
            res["pairs"] = np.empty(n_pairs, dtype=np.complex64)
            o.pairs = res["pairs"].ctypes.data
        return res, o

    def run(self, iq_u8, stage=None, points=False, lines_m=0, n_line_points=None, pairs=False):
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        n = iq.size // 2
        res, o = self._outputs(n + (stage.n_zero if stage is not None else 0), points, lines_m, n_line_points, pairs)
        _check(self._L.fsea_chain_run_host(self._p, iq.ctypes.data, n, ctypes.byref(stage) if stage is not None else None,
                                           ctypes.byref(o)))
        return res

    def run_f64(self, iq, points=False, lines_m=0, n_line_points=None, pairs=False):
        flat = np.ascontiguousarray(np.asarray(iq, dtype=np.complex128)).ravel().view(np.float64)
        res, o = self._outputs(flat.size // 2, points, lines_m, n_line_points, pairs)
        _check(self._L.fsea_chain_run_f64_host(self._p, flat.ctypes.data, flat.size // 2, ctypes.byref(o)))
        return res

    def fetch(self, points=False, lines_m=0, n_line_points=None, pairs=False):
        res, o = self._outputs(self.n_pairs, points, lines_m, n_line_points, pairs)
        _check(self._L.fsea_chain_fetch_host(self._p, ctypes.byref(o)))
        return res

    def run_device(self, d_iq_ptr, n_samples, n_frames, stage=None, d_points=None, d_lines=None, lines_m=1,
                   n_line_points=None, d_pairs=None, stream=0):
        """Device pointers (ints, 16-byte aligned): n_frames blocks of n_samples pairs in, per frame a points image, a
        lines image and / or the filtered pairs out; asynchronous."""
        per_frame = n_samples + (stage.n_zero if stage is not None else 0)
        o = ChainOutputs(d_points, d_lines, int(lines_m), per_frame if n_line_points is None else int(n_line_points), d_pairs)
        _check(self._L.fsea_chain_run_device(self._p, d_iq_ptr, n_samples, n_frames,
                                             ctypes.byref(stage) if stage is not None else None, ctypes.byref(o),
                                             stream or None))


class Zoom(_ResettableHandle):
    """Shift -> decimating low-pass -> FFT on one device, the decimated pairs resident between the two; thin wrapper over
    fsea_zoom_*.  run() takes 8-bit IQ from the host and returns (rows, pairs): the rows of the inner (fft_size, hop, mode)
    plan on the len // decimation decimated pairs of this call, and those pairs where asked for.  Each call continues the
    filter of the previous ones; sample_offset is the number of samples they consumed."""
    _kind = "zoom"

    def __init__(self, taps, decimation, fft_size, hop=None, mode=MODE_MAG_F32, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        self.n_taps, self.decimation, self.device = t.size, decimation, device
        self.fft_size, self.hop, self.mode = fft_size, fft_size if hop is None else hop, mode
        self._create("fsea_zoom_create", t.ctypes.data if t.size else None, t.size, decimation, fft_size, self.hop, mode, device)

    def set_window(self, w):
        """fsea_zoom_set_window: Plan.set_window on the inner plan."""
        if w is None:
            _check(self._L.fsea_zoom_set_window(self._p, None))
            return
        if isinstance(w, str):
            w = window(w, self.fft_size)
        wf = np.ascontiguousarray(w, dtype=np.float32).ravel()
        if wf.size != self.fft_size:
            raise ValueError("a window has fft_size weights")
        _check(self._L.fsea_zoom_set_window(self._p, wf.ctypes.data))

    def out_pairs(self, n_samples):
        return self._L.fsea_zoom_out_pairs(self._p, n_samples)

    def out_rows(self, n_samples):
        return self._L.fsea_zoom_out_rows(self._p, n_samples)

    @property
    def row_bytes(self):
        return self._L.fsea_zoom_row_bytes(self._p)

    def run(self, iq_u8, cycles_per_sample, phase0_cycles=0.0, sample_offset=0, flip=False, pairs=False):
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        n = iq.size // 2
        rows = np.empty((self.out_rows(n), self.fft_size), dtype=_MODE_DTYPE[self.mode])
        out = np.empty(self.out_pairs(n), dtype=np.complex64) if pairs else None
        _check(self._L.fsea_zoom_run_host(self._p, iq.ctypes.data, n, int(bool(flip)), cycles_per_sample, phase0_cycles,
                                          sample_offset, rows.ctypes.data, out.ctypes.data if pairs else None))
        return rows, out

    def run_device(self, d_iq_ptr, n_samples, d_rows_ptr, cycles_per_sample, phase0_cycles=0.0, sample_offset=0, flip=False,
                   d_pairs_ptr=None, stream=0):
        """Device pointers (ints, 16-byte aligned): 2 * n_samples bytes in, out_rows(n_samples) rows and, where asked for,
        out_pairs(n_samples) complex64 out; asynchronous."""
        _check(self._L.fsea_zoom_run_device(self._p, d_iq_ptr, n_samples, int(bool(flip)), cycles_per_sample, phase0_cycles,
                                            sample_offset, d_rows_ptr, d_pairs_ptr, stream or None))


def pfb_prototype(channels, branch_taps):
    """fsea_pfb_prototype: the bank's default prototype, channels * lowpass_taps(2 channels, 1, channels * branch_taps)."""
    taps = np.empty(max(int(channels) * int(branch_taps), 1), dtype=np.float64)
    _check(hip_lib().fsea_pfb_prototype(int(channels), int(branch_taps), taps.ctypes.data))
    return taps


class Pfb(_ResettableHandle):
    """A polyphase filter bank on one device: the band split into `channels` channels, a frame every channels /
    oversampling samples; thin wrapper over fsea_pfb_*.  run() takes 8-bit IQ from the host and returns (rows, frames,
    series): the rows of the inner (channels, channels, mode) plan on the len // (channels / oversampling) polyphase frames
    of this call, and where asked for those frames and the rows transposed (one channel's outputs in a row; COMPLEX mode),
    None otherwise.  Each call continues the stream of the previous ones; reset() starts a new one."""
    _kind = "pfb"

    def __init__(self, taps, channels, oversampling=1, mode=MODE_MAG_F32, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        if channels < 1 or t.size % channels:
            raise ValueError("the prototype has channels * branch_taps taps")
        self.channels, self.branch_taps, self.oversampling = channels, t.size // channels, oversampling
        self.mode, self.device = mode, device
        self._create("fsea_pfb_create", t.ctypes.data if t.size else None, channels, self.branch_taps, oversampling, mode, device)

    def out_frames(self, n_samples):
        return self._L.fsea_pfb_out_frames(self._p, n_samples)

    @property
    def row_bytes(self):
        return self._L.fsea_pfb_row_bytes(self._p)

    def run(self, iq_u8, flip=False, frames=False, series=False):
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        n = iq.size // 2
        F, M = self.out_frames(n), self.channels
        rows = np.empty((F, M), dtype=_MODE_DTYPE[self.mode])
        fr = np.empty((F, M), dtype=np.complex64) if frames else None
        se = np.empty((M, F), dtype=np.complex64) if series else None
        _check(self._L.fsea_pfb_run_host(self._p, iq.ctypes.data, n, int(bool(flip)), rows.ctypes.data,
                                         fr.ctypes.data if frames else None, se.ctypes.data if series else None))
        return rows, fr, se

    def run_device(self, d_iq_ptr, n_samples, d_rows_ptr, flip=False, d_frames_ptr=None, d_series_ptr=None, stream=0):
        """Device pointers (ints, 16-byte aligned): 2 * n_samples bytes in, out_frames(n_samples) rows and, where asked for,
        as many frames of `channels` complex64 and the `channels` series out; asynchronous."""
        _check(self._L.fsea_pfb_run_device(self._p, d_iq_ptr, n_samples, int(bool(flip)), d_rows_ptr, d_frames_ptr,
                                           d_series_ptr, stream or None))


def _rows_2d(a, dtypes, what):
    """A 2-D array whose rows are contiguous and a whole number of elements apart (copied where they are not: only such
    rows go to the library as they are), and its pitch in elements."""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype not in dtypes:
        raise ValueError("%s is a 2-D array of %s" % (what, " or ".join(np.dtype(d).name for d in dtypes)))
    if a.strides[1] != a.itemsize or (a.shape[0] > 1 and (a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize)):
        a = np.ascontiguousarray(a)
    return a, (a.strides[0] // a.itemsize if a.shape[0] > 1 else a.shape[1])


class _RowsHandle(_ResettableHandle):
    """What consumes rows of `width` levels (Persist, Cfar, OsCfar, Tcfar, Events): the width and the rows offered so far."""

    def __init__(self, width, device=0):
        self.device = device
        self._create("fsea_%s_create" % self._kind, int(width), device)

    @property
    def width(self):
        return getattr(self._L, "fsea_%s_width" % self._kind)(self._p)

    @property
    def rows(self):
        return getattr(self._L, "fsea_%s_rows" % self._kind)(self._p)

    def _host_rows(self, rows):
        """(array, pitch, type) of a 2-D uint8 or float32 array of rows of `width` elements"""
        a, pitch = _rows_2d(rows, (np.uint8, np.float32), "rows")
        if a.shape[1] != self.width:
            raise ValueError("a row has `width` elements")
        return a, pitch, CFAR_U8 if a.dtype == np.uint8 else CFAR_F32   # PERSIST_U8 and PERSIST_F32 are the same two


def persist_trace(counts, kind, fraction=0.5):
    """fsea_persist_trace (host arithmetic): one level per column of a (256, width) array of counts -- the highest
    (PERSIST_TRACE_MAX) or lowest (PERSIST_TRACE_MIN) occupied level, or the level at which the cumulative count reaches
    `fraction` of the column's total (PERSIST_TRACE_QUANTILE; 0.5: the median level)."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    if c.ndim != 2 or c.shape[0] != PERSIST_LEVELS:
        raise ValueError("counts has shape (256, width)")
    levels = np.empty(c.shape[1], dtype=np.uint8)
    _check(hip_lib().fsea_persist_trace(c.ctypes.data, c.shape[1], int(kind), float(fraction), levels.ctypes.data))
    return levels


class Persist(_RowsHandle):
    """A persistence spectrum on one device: counts[level, column] over all the rows offered; thin wrapper over
    fsea_persist_*.  add() takes a 2-D uint8 or float32 array from the host (any row stride), add_device() resident rows;
    counts() and image() fetch the (256, width) counts and the (256, width) uint8 picture, strongest level on top."""
    _kind = "persist"

    def set_range(self, lo, hi):
        _check(self._L.fsea_persist_set_range(self._p, lo, hi))

    def add(self, rows):
        a, pitch, type = self._host_rows(rows)
        _check(self._L.fsea_persist_add_host(self._p, a.ctypes.data, type, a.shape[0], pitch))

    def add_device(self, d_rows_ptr, type, n_rows, pitch=None, stream=0):
        """d_rows_ptr (an int, 16-byte aligned): n_rows rows of `width` elements, `pitch` elements apart; asynchronous."""
        _check(self._L.fsea_persist_add_device(self._p, d_rows_ptr, int(type), n_rows, self.width if pitch is None else pitch,
                                               stream or None))

    def decay(self, numerator, denominator, stream=0):
        _check(self._L.fsea_persist_decay(self._p, numerator, denominator, stream or None))

    def counts(self):
        out = np.empty((PERSIST_LEVELS, self.width), dtype=np.uint32)
        _check(self._L.fsea_persist_counts_host(self._p, out.ctypes.data))
        return out

    def image(self, map=PERSIST_MAP_LOG, full=0):
        out = np.empty((PERSIST_LEVELS, self.width), dtype=np.uint8)
        _check(self._L.fsea_persist_image_host(self._p, int(map), int(full), out.ctypes.data))
        return out

    def image_device(self, d_image_ptr, map=PERSIST_MAP_LOG, full=0, stream=0):
        _check(self._L.fsea_persist_image_device(self._p, int(map), int(full), d_image_ptr, stream or None))


def cfar_bands(hits, rows, min_fraction, max_gap=0, min_width=1):
    """fsea_cfar_bands (host arithmetic): the bands of occupied columns of `hits` (width uint32, a Cfar's hits()) over
    `rows` rows as a structured array of dtype CFAR_BAND (first, last, peak, peak_hits, hits_sum).  A column is occupied
    when hits[k] >= max(1, ceil(min_fraction * rows)); up to max_gap unoccupied columns do not end a band; a band narrower
    than min_width is dropped."""
    h = np.ascontiguousarray(hits, dtype=np.uint32)
    if h.ndim != 1:
        raise ValueError("hits is a 1-D array")
    n = ctypes.c_size_t()
    args = (h.ctypes.data, h.shape[0], int(rows), float(min_fraction), int(max_gap), int(min_width))
    _check(hip_lib().fsea_cfar_bands(*args, None, 0, ctypes.byref(n)))
    out = np.zeros(n.value, dtype=CFAR_BAND)
    if n.value:
        _check(hip_lib().fsea_cfar_bands(*args, out.ctypes.data, n.value, ctypes.byref(n)))
    return out


class _Detector(_RowsHandle):
    """What Cfar and OsCfar have in common, fsea_<kind>_add_host, _add_device and _hits_host (Tcfar keeps hits() and has
    adds of its own, with context rows): add() takes a 2-D uint8 or
    float32 array from the host (any row stride) and returns what was asked for; add_device() takes resident rows; hits()
    fetches hits[column] over all the rows offered."""

    def add(self, rows, mask=False, row_hits=False):
        """None, the (n_rows, width) uint8 mask, the (n_rows,) uint32 row hits, or (mask, row_hits)."""
        a, pitch, type = self._host_rows(rows)
        m = np.empty(a.shape, dtype=np.uint8) if mask else None
        h = np.empty(a.shape[0], dtype=np.uint32) if row_hits else None
        _check(getattr(self._L, "fsea_%s_add_host" % self._kind)(self._p, a.ctypes.data, type, a.shape[0], pitch,
                                                                 m.ctypes.data if mask else None, h.ctypes.data if row_hits else None))
        return (m, h) if mask and row_hits else m if mask else h

    def add_device(self, d_rows_ptr, type, n_rows, pitch=None, d_mask_ptr=None, d_row_hits_ptr=None, stream=0):
        """d_rows_ptr (an int, 16-byte aligned): n_rows rows of `width` elements, `pitch` elements apart; d_mask_ptr
        (n_rows * width bytes) and d_row_hits_ptr (n_rows uint32) are optional; asynchronous."""
        _check(getattr(self._L, "fsea_%s_add_device" % self._kind)(
            self._p, d_rows_ptr, int(type), n_rows, self.width if pitch is None else pitch, d_mask_ptr or None,
            d_row_hits_ptr or None, stream or None))

    def hits(self):
        out = np.empty(self.width, dtype=np.uint32)
        _check(getattr(self._L, "fsea_%s_hits_host" % self._kind)(self._p, out.ctypes.data))
        return out


class Cfar(_Detector):
    """A CFAR detector across frequency on one device: which cells of a dB row stand above the mean level of their
    neighbours, and hits[column] over all the rows offered; thin wrapper over fsea_cfar_*."""
    _kind = "cfar"

    def set(self, guard=2, train=16, offset=60, method=CFAR_CA):
        _check(self._L.fsea_cfar_set(self._p, int(guard), int(train), int(offset), int(method)))


class OsCfar(_Detector):
    """An ordered-statistic CFAR detector across frequency on one device: which cells of a dB row stand above the rank-th
    smallest level of their training cells -- the weaker of two close emissions keeps its hit -- and hits[column] over all
    the rows offered; thin wrapper over fsea_oscfar_*.  cfar_bands() takes the hits."""
    _kind = "oscfar"

    def set(self, guard=2, train=16, offset=60, rank=24):
        _check(self._L.fsea_oscfar_set(self._p, int(guard), int(train), int(offset), int(rank)))

    @property
    def rank(self):
        return self._L.fsea_oscfar_rank(self._p)


class Tcfar(_Detector):
    """A CFAR detector down the time axis on one device: which cells stand above the mean level of the cells of their own
    column in the rows before and after them -- a burst wider than any frequency window -- and hits[column] over all the
    rows decided; thin wrapper over fsea_tcfar_*.  cfar_bands() takes the hits."""
    _kind = "tcfar"

    def set(self, guard=2, train=16, offset=60, method=CFAR_CA, mask_op=TCFAR_MASK_SET):
        _check(self._L.fsea_tcfar_set(self._p, int(guard), int(train), int(offset), int(method), int(mask_op)))

    @property
    def run_rows(self):
        """The rows a workgroup decides under the current settings: where the seams of a call lie."""
        return self._L.fsea_tcfar_run_rows(self._p)

    def add(self, rows, before=0, after=0, mask=False, row_hits=False):
        """`rows` is the whole array, context included: its first `before` and last `after` rows are context, the rows
        between are decided.  `mask`: True for a new (n_rows, width) uint8 mask, or a C-contiguous uint8 array of that
        shape, which TCFAR_MASK_OR and TCFAR_MASK_AND combine with and every operation writes.  Returns None, the mask,
        the (n_rows,) uint32 row hits, or (mask, row_hits)."""
        a, pitch, type = self._host_rows(rows)
        n = a.shape[0] - int(before) - int(after)
        if before < 0 or after < 0 or n < 0:
            raise ValueError("before and after are row counts within the array")
        want_mask = mask is not False and mask is not None
        m = np.empty((n, a.shape[1]), dtype=np.uint8) if mask is True else mask if want_mask else None
        if want_mask and (not isinstance(m, np.ndarray) or m.dtype != np.uint8 or m.shape != (n, a.shape[1])
                          or not m.flags.c_contiguous or not m.flags.writeable):
            raise ValueError("mask is True or a writeable C-contiguous uint8 array of shape (n_rows, width)")
        h = np.empty(n, dtype=np.uint32) if row_hits else None
        _check(self._L.fsea_tcfar_add_host(self._p, a.ctypes.data + int(before) * pitch * a.itemsize, type, n, pitch, int(before),
                                           int(after), m.ctypes.data if want_mask else None, h.ctypes.data if row_hits else None))
        return (m, h) if want_mask and row_hits else m if want_mask else h

    def add_device(self, d_rows_ptr, type, n_rows, pitch=None, before=0, after=0, d_mask_ptr=None, d_row_hits_ptr=None, stream=0):
        """d_rows_ptr (an int, 16-byte aligned): the first of n_rows decided rows of `width` elements, `pitch` elements
        apart, `before` context rows in front of it and `after` behind the last; d_mask_ptr (n_rows * width bytes, read
        as well under TCFAR_MASK_OR and TCFAR_MASK_AND) and d_row_hits_ptr (n_rows uint32) are optional; asynchronous."""
        _check(self._L.fsea_tcfar_add_device(self._p, d_rows_ptr, int(type), n_rows, self.width if pitch is None else pitch,
                                             int(before), int(after), d_mask_ptr or None, d_row_hits_ptr or None, stream or None))


class Events(_RowsHandle):
    """Spectrum events on one device: a detection mask (and the level rows under it) as a sorted list of runs, the runs
    linked into time-frequency events, runs painted back as an image; thin wrapper over fsea_events_*.  runs() and paint()
    take and give host arrays, runs_device() and paint_device() work on resident memory; link() is host arithmetic."""
    _kind = "events"

    def set_gap(self, gap_cols):
        _check(self._L.fsea_events_set_gap(self._p, int(gap_cols)))

    def runs(self, mask, levels=None):
        """The runs of a 2-D uint8 mask (any row stride), with the statistics of `levels` (uint8 or float32, the mask's shape)
        under its hits: a structured array of dtype EVENTS_RUN, sorted by (row, first)."""
        m, mp = _rows_2d(mask, (np.uint8,), "mask")
        if m.shape[1] != self.width:
            raise ValueError("a row has `width` elements")
        lp, lptr, type = m.shape[1], None, CFAR_U8
        if levels is not None:
            lv, lp = _rows_2d(levels, (np.uint8, np.float32), "levels")
            if lv.shape != m.shape:
                raise ValueError("levels has the mask's shape")
            lptr, type = lv.ctypes.data, CFAR_U8 if lv.dtype == np.uint8 else CFAR_F32
        # room for the records: the hits with no hit to their left are the runs at a gap of 0 and no fewer at any other
        hit = m != 0
        room = int(hit[:, 0].sum()) + int((hit[:, 1:] & ~hit[:, :-1]).sum())
        out = np.zeros(room, dtype=EVENTS_RUN)
        n = ctypes.c_size_t()
        _check(self._L.fsea_events_runs_host(self._p, m.ctypes.data, mp, lptr, type, lp, m.shape[0],
                                             out.ctypes.data if room else None, room, ctypes.byref(n)))
        assert n.value <= room
        return out[:n.value]

    def runs_device(self, d_mask_ptr, n_rows, d_runs_ptr, capacity, mask_pitch=None, d_levels_ptr=None, type=CFAR_U8,
                    level_pitch=None, stream=0):
        """d_mask_ptr (an int, 16-byte aligned): n_rows rows of `width` bytes, mask_pitch bytes apart; d_levels_ptr (optional)
        the level rows, level_pitch elements apart; at most `capacity` records to d_runs_ptr.  Returns the number of runs
        found, which may exceed capacity; the records are in place when it returns."""
        n = ctypes.c_size_t()
        _check(self._L.fsea_events_runs_device(self._p, d_mask_ptr, self.width if mask_pitch is None else mask_pitch,
                                               d_levels_ptr or None, int(type), self.width if level_pitch is None else level_pitch,
                                               n_rows, d_runs_ptr or None, capacity, ctypes.byref(n), stream or None))
        return n.value

    @staticmethod
    def link(runs, gap_cols=0, gap_rows=0, min_rows=1, min_cols=1, min_hits=1):
        """fsea_events_link (host arithmetic): (events, event_of_run) of a sorted array of EVENTS_RUN -- a structured array
        of dtype EVENTS_EVENT for the events that pass the filters, and per run the number of its event or EVENTS_NO_EVENT."""
        r = np.ascontiguousarray(runs, dtype=EVENTS_RUN)
        if r.ndim != 1:
            raise ValueError("runs is a 1-D array")
        of_run = np.empty(r.size, dtype=np.uint32)
        n = ctypes.c_size_t()
        args = (r.ctypes.data if r.size else None, r.size, int(gap_cols), int(gap_rows), int(min_rows), int(min_cols), int(min_hits))
        _check(hip_lib().fsea_events_link(*args, None, None, 0, ctypes.byref(n)))
        events = np.zeros(n.value, dtype=EVENTS_EVENT)
        _check(hip_lib().fsea_events_link(*args, of_run.ctypes.data if r.size else None, events.ctypes.data if n.value else None,
                                          n.value, ctypes.byref(n)))
        return events, of_run

    def paint(self, runs, values, n_rows, row0=0):
        """The (n_rows, width) uint8 image of `runs` with one uint8 value per run; image row 0 is row `row0`."""
        r = np.ascontiguousarray(runs, dtype=EVENTS_RUN)
        v = np.ascontiguousarray(values, dtype=np.uint8)
        if r.ndim != 1 or v.shape != r.shape:
            raise ValueError("runs is a 1-D array and values has one uint8 per run")
        out = np.empty((n_rows, self.width), dtype=np.uint8)
        _check(self._L.fsea_events_paint_host(self._p, r.ctypes.data if r.size else None, v.ctypes.data if r.size else None, r.size,
                                              int(row0), n_rows, out.ctypes.data if n_rows else None, self.width))
        return out

    def paint_device(self, d_runs_ptr, d_values_ptr, n_runs, n_rows, d_image_ptr, row0=0, pitch=None, stream=0):
        """d_runs_ptr, d_image_ptr (ints, 16-byte aligned) and d_values_ptr: n_runs records and values, an image of n_rows rows
        `pitch` bytes apart; asynchronous."""
        _check(self._L.fsea_events_paint_device(self._p, d_runs_ptr or None, d_values_ptr or None, n_runs, int(row0), n_rows,
                                                d_image_ptr or None, self.width if pitch is None else pitch, stream or None))


def extract_lead(n_taps, decimation):
    """fsea_extract_lead: ceil((n_taps - 1) / decimation) * decimation, the samples a cut-out starts in front of its event."""
    return hip_lib().fsea_extract_lead(int(n_taps), int(decimation))


def extract_jobs(events, width, hop, n_samples, n_taps, decimation, max_fill=0.8):
    """fsea_extract_jobs (host arithmetic): (jobs, fits) of an array of EVENTS_EVENT whose rows are the frames of `width`
    samples, one every `hop`, of a recording of n_samples samples -- a ctypes array of ExtractJob, one per event with
    out_first 0, and a uint8 array: 1 where the event's columns times the decimation fit max_fill * width."""
    e = np.ascontiguousarray(events, dtype=EVENTS_EVENT)
    if e.ndim != 1:
        raise ValueError("events is a 1-D array")
    jobs = (ExtractJob * e.size)()
    fits = np.zeros(e.size, dtype=np.uint8)
    _check(hip_lib().fsea_extract_jobs(e.ctypes.data if e.size else None, e.size, int(width), int(hop), int(n_samples), int(n_taps),
                                       int(decimation), float(max_fill), _address(jobs), fits.ctypes.data if e.size else None))
    return jobs, fits


def _table_of(kind, jobs):
    """a sequence of `kind` records as one ctypes array (a ctypes array of them passes through)"""
    if isinstance(jobs, ctypes.Array) and jobs._type_ is kind:
        return jobs
    jobs = list(jobs)
    return (kind * len(jobs))(*jobs)


def _address(array):
    """the address of a ctypes array, None for an empty one"""
    return ctypes.addressof(array) if len(array) else None


class _JobRunner(_Handle):
    """What Extract, Measure, Audio and Spectra have in common, the objects that run a table of `_job` records over one
    resident buffer: _table() makes the jobs the (array, address, length) a call takes.  A run_device names its function
    and takes the offset apart itself: what it spends before the call is the host time the rate scripts print, and a
    call forwarded through a method of this class took 2.4 us where it takes 1.6 (profiles/jobs_scaffold.txt)."""
    _job = None    # the record of the table

    def _table(self, jobs):
        """(the jobs as one ctypes array, its address or None for an empty one, its length)"""
        table = _table_of(self._job, jobs)
        return table, _address(table), len(table)


class _PlacingJobRunner(_JobRunner):
    """The three that place their outputs, Extract, Audio and Spectra (Measure writes one record per job): layout() is
    fsea_<kind>_layout, _run_placed() their host form: a copy of the jobs laid out, one call, one array per job."""

    def layout(self, jobs):
        """fsea_<kind>_layout: (the jobs as a ctypes array with out_first filled in, the outputs they need in all: pairs
        for Extract, floats for Audio and Spectra)."""
        table, at, n = self._table(jobs)
        total = ctypes.c_size_t()
        _check(getattr(self._L, "fsea_%s_layout" % self._kind)(self._p, at, n, ctypes.byref(total)))
        return table, total.value

    def _run_placed(self, before, jobs, dtype, count, *between):
        """fsea_<kind>_run_host(object, *before, table, n_jobs, *between, out, total) on a copy of the jobs laid out with
        layout(): a list of `dtype` arrays, count(job) long, one per job."""
        table, total = self.layout([self._job.from_buffer_copy(j) for j in jobs])
        out = np.zeros(max(total, 1), dtype=dtype)
        _check(getattr(self._L, "fsea_%s_run_host" % self._kind)(self._p, *before, _address(table), len(table), *between,
                                                                 out.ctypes.data, total))
        return [out[j.out_first:j.out_first + count(j)].copy() for j in table]


class Extract(_PlacingJobRunner):
    """Event cut-outs on one device: a table of shift -> low-pass -> keep every decimation-th sample jobs over one recording
    in one launch, stateless; thin wrapper over fsea_extract_*.  run() takes 8-bit IQ and the jobs from the host and
    returns one complex64 array per job; run_device() works on resident memory with the jobs' own out_first."""
    _kind, _job = "extract", ExtractJob

    def __init__(self, taps, decimation, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        self.n_taps, self.decimation, self.device = t.size, decimation, device
        self._create("fsea_extract_create", t.ctypes.data if t.size else None, t.size, decimation, device)

    def out_pairs(self, n_samples):
        return self._L.fsea_extract_out_pairs(self._p, n_samples)

    def run(self, iq_u8, jobs, flip=False):
        """The host form on a copy of the jobs laid out with layout(): a list of complex64 arrays, one per job."""
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        return self._run_placed((iq.ctypes.data, iq.size // 2, int(bool(flip))), jobs, np.complex64,
                                lambda j: j.n_samples // self.decimation)

    def run_device(self, d_iq_ptr, n_iq_samples, jobs, d_pairs_ptr, pairs_capacity, flip=False, stream=0):
        """Device pointers (ints, 16-byte aligned): 2 * n_iq_samples bytes in, pairs_capacity complex64 out, every job at its
        own out_first; asynchronous.  The jobs are read before the call returns."""
        table, at, n = self._table(jobs)
        _check(self._L.fsea_extract_run_device(self._p, d_iq_ptr or None, n_iq_samples, int(bool(flip)), at, n, d_pairs_ptr or None,
                                               pairs_capacity, stream or None))


def _jobs_of_extract(kind, record, extract_jobs_laid_out, decimation, skip_pairs):
    """fsea_<kind>_jobs: a ctypes array of `record`, one per extract job"""
    table = _table_of(ExtractJob, extract_jobs_laid_out)
    jobs = (record * len(table))()
    _check(getattr(hip_lib(), "fsea_%s_jobs" % kind)(_address(table), len(table), int(decimation), int(skip_pairs), _address(jobs)))
    return jobs


def measure_jobs(extract_jobs_laid_out, decimation, skip_pairs=0):
    """fsea_measure_jobs (host arithmetic): the spans of the outputs of extract jobs that Extract.layout laid out, each
    without its first skip_pairs pairs, as a ctypes array of MeasureJob."""
    return _jobs_of_extract("measure", MeasureJob, extract_jobs_laid_out, decimation, skip_pairs)


def measure_finish(sums, lag=1):
    """fsea_measure_finish (host arithmetic, no GPU needed): a MeasureSums made with `lag` to a MeasureResult."""
    result = MeasureResult()
    _check(hip_lib().fsea_measure_finish(ctypes.byref(sums), int(lag), ctypes.byref(result)))
    return result


class Measure(_JobRunner):
    """Signal measures on one device: a table of spans of one buffer of complex64 in, one record of moment sums per span out,
    in two launches, stateless; thin wrapper over fsea_measure_*.  run() takes the pairs and the jobs from the host and
    returns a ctypes array of MeasureSums; run_device() works on resident memory."""
    _kind, _job = "measure", MeasureJob

    def __init__(self, device=0):
        self.device = device
        self._create("fsea_measure_create", device)

    def run(self, pairs, jobs, offset=0j, lag=1):
        z = np.ascontiguousarray(pairs, dtype=np.complex64).ravel()
        table, at, n = self._table(jobs)
        sums = (MeasureSums * n)()
        offset = complex(offset)
        _check(self._L.fsea_measure_run_host(self._p, z.ctypes.data, z.size, at, n, offset.real, offset.imag, int(lag), _address(sums)))
        return sums

    def run_device(self, d_pairs_ptr, n_buffer_pairs, jobs, d_sums_ptr, offset=0j, lag=1, stream=0):
        """Device pointers (ints): n_buffer_pairs complex64 in (8-byte aligned), one 80-byte record per job out (16-byte
        aligned); asynchronous.  The jobs are read before the call returns."""
        table, at, n = self._table(jobs)
        offset = complex(offset)
        _check(self._L.fsea_measure_run_device(self._p, d_pairs_ptr or None, n_buffer_pairs, at, n, offset.real, offset.imag, int(lag),
                                               d_sums_ptr or None, stream or None))


def audio_layout(jobs, decimation):
    """What fsea_audio_layout does, without an object: (the jobs as a ctypes array of AudioJob with out_first filled in back
    to back in table order, the floats they need in all); a job of n pairs has n // decimation outputs."""
    table = _table_of(AudioJob, jobs)
    at = 0
    for j in table:
        j.out_first = at
        at += j.n_pairs // int(decimation)
    return table, at


class Audio(_PlacingJobRunner):
    """Cut-out audio on one device: a table of spans of one buffer of complex64 in, every span's FM-discriminated
    (kind "fm") or envelope-detected ("am"), low-passed and decimated float32 audio out, in one launch, stateless; thin
    wrapper over fsea_audio_*.  run() takes the pairs and the jobs from the host and returns one float32 array per job;
    run_device() works on resident memory with the jobs' own out_first."""
    _kind, _job = "audio", AudioJob

    def __init__(self, kind, taps, decimation, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        self.kind = {"fm": AUDIO_FM, "am": AUDIO_AM}.get(kind, kind)
        self.n_taps, self.decimation, self.device = t.size, decimation, device
        self._create("fsea_audio_create", self.kind, t.ctypes.data if t.size else None, t.size, decimation, device)

    def run(self, pairs, jobs, offset=0j, gain=1.0):
        """The host form on a copy of the jobs laid out with layout(): a list of float32 arrays, one per job."""
        z = np.ascontiguousarray(pairs, dtype=np.complex64).ravel()
        offset = complex(offset)
        return self._run_placed((z.ctypes.data, z.size), jobs, np.float32, lambda j: j.n_pairs // self.decimation,
                                offset.real, offset.imag, float(gain))

    def run_device(self, d_pairs_ptr, n_buffer_pairs, jobs, d_audio_ptr, n_audio, offset=0j, gain=1.0, stream=0):
        """Device pointers (ints): n_buffer_pairs complex64 in (8-byte aligned), n_audio float32 out (4-byte aligned), every
        job at its own out_first; asynchronous.  The jobs are read before the call returns."""
        table, at, n = self._table(jobs)
        offset = complex(offset)
        _check(self._L.fsea_audio_run_device(self._p, d_pairs_ptr or None, n_buffer_pairs, at, n, offset.real, offset.imag,
                                             float(gain), d_audio_ptr or None, n_audio, stream or None))


def spectra_jobs(extract_jobs_laid_out, decimation, skip_pairs=0):
    """fsea_spectra_jobs (host arithmetic): the spans of the outputs of extract jobs that Extract.layout laid out, each
    without its first skip_pairs pairs, as a ctypes array of SpectraJob (out_first 0: Spectra.layout places them)."""
    return _jobs_of_extract("spectra", SpectraJob, extract_jobs_laid_out, decimation, skip_pairs)


def spectra_finish(power, guard_bins=0, fraction=0.99):
    """fsea_spectra_finish (host arithmetic, no GPU needed): one row of n float32 powers to a SpectraResult."""
    p = np.ascontiguousarray(power, dtype=np.float32).ravel()
    result = SpectraResult()
    _check(hip_lib().fsea_spectra_finish(p.ctypes.data, p.size, int(guard_bins), float(fraction), ctypes.byref(result)))
    return result


class Spectra(_PlacingJobRunner):
    """Cut-out spectra on one device: a table of spans of one buffer of complex64 in, every span's averaged periodogram of n
    bins out -- of the span itself (kind "z"), of |z|^2 ("env"), z^2 ("sq") or z^4 ("fourth") -- in two launches, stateless;
    thin wrapper over fsea_spectra_*.  run() takes the pairs and the jobs from the host and returns one float32 array per
    job (empty for a span shorter than n); run_device() works on resident memory with the jobs' own out_first."""
    _kind, _job = "spectra", SpectraJob

    def __init__(self, n, hop=None, kind="z", window=None, device=0):
        self.n, self.hop, self.device = int(n), int(n) // 2 if hop is None else int(hop), device
        self.kind = SPECTRA_KINDS.get(kind, kind)
        w = None if window is None else np.ascontiguousarray(window, dtype=np.float32).ravel()
        if w is not None and w.size != self.n:
            raise FseaError("the window must have n weights")
        self._create("fsea_spectra_create", self.n, self.hop, self.kind, w.ctypes.data if w is not None else None, device)

    def segments(self, n_pairs):
        return self._L.fsea_spectra_segments(self._p, n_pairs)

    def run(self, pairs, jobs, offset=0j):
        """The host form on a copy of the jobs laid out with layout(): a list of float32 arrays, one per job."""
        z = np.ascontiguousarray(pairs, dtype=np.complex64).ravel()
        offset = complex(offset)
        return self._run_placed((z.ctypes.data, z.size), jobs, np.float32, lambda j: self.n if self.segments(j.n_pairs) else 0,
                                offset.real, offset.imag)

    def run_device(self, d_pairs_ptr, n_buffer_pairs, jobs, d_power_ptr, n_power, offset=0j, stream=0):
        """Device pointers (ints): n_buffer_pairs complex64 in (8-byte aligned), n_power float32 out (4-byte aligned), every
        job with a segment at its own out_first; asynchronous.  The jobs are read before the call returns."""
        table, at, n = self._table(jobs)
        offset = complex(offset)
        _check(self._L.fsea_spectra_run_device(self._p, d_pairs_ptr or None, n_buffer_pairs, at, n, offset.real, offset.imag,
                                               d_power_ptr or None, n_power, stream or None))


class Demod(_ResettableHandle):
    """The reference's audio chain (RAW or WBFM, nrf_decoder's conversion and frequency shift) on n_channels channels of
    one input stream; thin wrapper over fsea_demod_*.  Each call continues every channel's signal; reset() starts anew."""
    _kind = "demod"

    def __init__(self, kind, in_rate, out_rate=48000, n_channels=1, device=0):
        self.kind = {"raw": DEMOD_RAW, "wbfm": DEMOD_WBFM}.get(kind, kind)
        self.in_rate, self.out_rate, self.n_channels, self.device = in_rate, out_rate, n_channels, device
        self._create("fsea_demod_create", self.kind, in_rate, out_rate, n_channels, device)

    def set_channel(self, ch, freq_offset, cosine=1.0, sine=0.0):
        _check(self._L.fsea_demod_set_channel(self._p, ch, int(freq_offset), float(cosine), float(sine)))

    def get_channel(self, ch):
        """(freq_offset, cosine, sine) the channel starts its next call with."""
        o, c, s = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        _check(self._L.fsea_demod_get_channel(self._p, ch, ctypes.byref(o), ctypes.byref(c), ctypes.byref(s)))
        return o.value, c.value, s.value

    def out_length(self, n_samples):
        return self._L.fsea_demod_out_length(self._p, n_samples)

    def run_device(self, d_iq_ptr, n_samples, d_audio_ptr, flip=False, stream=0):
        """Device pointers (ints): 2 * n_samples bytes in, n_channels x out_length f64 out; asynchronous."""
        _check(self._L.fsea_demod_u8_device(self._p, d_iq_ptr, n_samples, int(bool(flip)), d_audio_ptr, stream or None))

    def run_u8(self, iq_u8, flip=False):
        """Interleaved 8-bit IQ (host) -> float64 array (n_channels, out_length)."""
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        n = iq.size // 2
        out = np.empty((self.n_channels, self.out_length(n)), dtype=np.float64)
        _check(self._L.fsea_demod_u8_host(self._p, iq.ctypes.data, n, int(bool(flip)), out.ctypes.data))
        return out

    def run_f64(self, i, q):
        """Separate I and Q float64 arrays (host), converted by nothing -> float64 array (n_channels, out_length)."""
        i = np.ascontiguousarray(i, dtype=np.float64).ravel()
        q = np.ascontiguousarray(q, dtype=np.float64).ravel()
        if i.size != q.size:
            raise ValueError("I and Q differ in length")
        out = np.empty((self.n_channels, self.out_length(i.size)), dtype=np.float64)
        _check(self._L.fsea_demod_f64_host(self._p, i.ctypes.data, q.ctypes.data, i.size, out.ctypes.data))
        return out


def _iq_input(iq):
    """A host IQ array -> (contiguous flat array, FSEA_IQ_* type, pairs).  uint8, float32 and float64 pass as they are;
    complex64 / complex128 as their interleaved float parts."""
    a = np.asarray(iq)
    if a.dtype == np.complex64:
        a = a.view(np.float32)
    elif a.dtype == np.complex128:
        a = a.view(np.float64)
    kinds = {np.dtype(np.uint8): IQ_U8, np.dtype(np.float32): IQ_F32, np.dtype(np.float64): IQ_F64}
    if a.dtype not in kinds:
        raise TypeError("IQ input must be uint8, float32, float64 or complex, got %s" % a.dtype)
    a = np.ascontiguousarray(a).ravel()
    return a, kinds[a.dtype], a.size // 2


class IqDraw(_Handle):
    """IQ constellation images on one device; thin wrapper over fsea_iq_*.  points(): the 256 x 256 histogram of the
    reference's nrf_buffer_to_iq_points (bin I * 256 + Q, counts modulo 256); lines(): the (256 m)^2 image of
    nrf_buffer_to_iq_lines (consecutive points joined by its Bresenham lines, pixel (I m, Q m) at row Q m, counts clamped to
    255).  Coordinates as nut_buffer_get_u8: u8 as is, floats as x86-64's (uint8_t)(v * 256.0)."""
    _kind = "iq_draw"

    def __init__(self, device=0):
        self.device = device
        self._create("fsea_iq_draw_create", device)

    def points(self, iq, flip=False):
        """Host IQ (uint8, float32, float64 interleaved, or complex) -> (256, 256) uint8, row I."""
        a, kind, n = _iq_input(iq)
        img = np.empty((256, 256), dtype=np.uint8)
        _check(self._L.fsea_iq_points_host(self._p, a.ctypes.data, kind, int(bool(flip)), n, img.ctypes.data))
        return img

    def lines(self, iq, m=1, n_points=None, flip=False):
        """Host IQ -> (256 m, 256 m) uint8, row y = Q m; the first n_points points (default all) joined in order."""
        a, kind, n = _iq_input(iq)
        if n_points is not None:
            if not 0 <= int(n_points) <= n:
                raise ValueError("n_points must be in [0, %d] (the pairs of iq), got %d" % (n, int(n_points)))
            n = int(n_points)
        img = np.empty((256 * m, 256 * m), dtype=np.uint8)
        _check(self._L.fsea_iq_lines_host(self._p, a.ctypes.data, kind, int(bool(flip)), n, int(m), img.ctypes.data))
        return img

    def points_device(self, d_iq_ptr, kind, n_pairs, n_frames, d_image_ptr, flip=False, stream=0):
        """Device pointers (ints, 16-byte aligned): n_frames frames of n_pairs pairs in, n_frames 65536-byte images out;
        asynchronous."""
        _check(self._L.fsea_iq_points_device(self._p, d_iq_ptr, kind, int(bool(flip)), n_pairs, n_frames, d_image_ptr,
                                             stream or None))

    def lines_device(self, d_iq_ptr, kind, n_points, n_frames, m, d_image_ptr, flip=False, stream=0):
        """Device pointers (ints, 16-byte aligned): n_frames frames of n_points points in, n_frames (256 m)^2-byte images
        out; asynchronous."""
        _check(self._L.fsea_iq_lines_device(self._p, d_iq_ptr, kind, int(bool(flip)), n_points, n_frames, int(m),
                                            d_image_ptr, stream or None))


def interp_image_tables(width, height, iq_size):
    """fsea_interp_image_tables: (col, row) int32 arrays, the sample whose colour each pixel column / row shows (host
    arithmetic, needs no GPU)."""
    col, row = np.empty(max(width, 0), dtype=np.int32), np.empty(max(height, 0), dtype=np.int32)
    _check(hip_lib().fsea_interp_image_tables(width, height, iq_size, col.ctypes.data, row.ctypes.data))
    return col, row


class Interp(_ResettableHandle):
    """Two resident sample blocks A and B (uint8 or float64, n_elements each, zero at first) and their blends
    a (1 - t) + b t for arrays of weights; thin wrapper over fsea_interp_*.  frames(): the reference's
    nrf_interpolator_get_buffer per weight; image_frames(): the frames of its gradual-noise movie tool."""
    _kind = "interp"

    def __init__(self, dtype, n_elements, device=0):
        self.dtype = np.dtype(dtype)
        kinds = {np.dtype(np.uint8): IQ_U8, np.dtype(np.float64): IQ_F64}
        if self.dtype not in kinds:
            raise TypeError("blocks must be uint8 or float64, got %s" % self.dtype)
        self.n, self.device = int(n_elements), device
        self._create("fsea_interp_create", kinds[self.dtype], self.n, device)

    def push(self, block):
        """A takes what B held, B the host array `block` (n_elements of the object's dtype)."""
        b = np.ascontiguousarray(block, dtype=self.dtype).ravel()
        if b.size != self.n:
            raise ValueError("a block has %d elements, got %d" % (self.n, b.size))
        _check(self._L.fsea_interp_push_host(self._p, b.ctypes.data))

    def push_device(self, d_block_ptr, stream=0):
        _check(self._L.fsea_interp_push_device(self._p, d_block_ptr, stream or None))

    def frames(self, weights):
        """Host float64 weights -> (len(weights), n_elements) array of the object's dtype."""
        w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        out = np.empty((w.size, self.n), dtype=self.dtype)
        _check(self._L.fsea_interp_frames_host(self._p, w.ctypes.data, w.size, out.ctypes.data))
        return out

    def frames_device(self, d_weights_ptr, n_frames, d_out_ptr, stream=0):
        """Device pointers (ints; output 16-byte aligned): n_frames weights in, n_frames blocks out; asynchronous."""
        _check(self._L.fsea_interp_frames_device(self._p, d_weights_ptr, n_frames, d_out_ptr, stream or None))

    def image_frames(self, weights, width, height, iq_size, flip=True):
        """Host float64 (already eased) weights -> (len(weights), height, width) uint8 images."""
        w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        g = InterpGeometry(width, height, iq_size, int(bool(flip)))
        out = np.empty((w.size, max(height, 0), max(width, 0)), dtype=np.uint8)
        _check(self._L.fsea_interp_image_frames_host(self._p, w.ctypes.data, w.size, ctypes.byref(g), out.ctypes.data))
        return out

    def image_frames_device(self, d_weights_ptr, n_frames, width, height, iq_size, d_images_ptr, flip=True, stream=0):
        """Device pointers (ints; images 16-byte aligned): n_frames width x height images out; asynchronous."""
        g = InterpGeometry(width, height, iq_size, int(bool(flip)))
        _check(self._L.fsea_interp_image_frames_device(self._p, d_weights_ptr, n_frames, ctypes.byref(g), d_images_ptr,
                                                       stream or None))


class Trace(_ResettableHandle):
    """The IQ trace movie of the reference's single-sample tool on one device; thin wrapper over fsea_trace_*.  A
    width x height canvas (zero at first) with the (256 m)^2 IQ square at its centre; every frame fades it by `fade`, joins
    the points of its frame_bytes bytes with lines, each hit adding pixel_inc unless that reaches 255, and is one image."""
    _kind = "trace"

    def __init__(self, width=1920, height=1080, m=4, pixel_inc=4, fade=0, device=0):
        self.width, self.height, self.m, self.device = int(width), int(height), int(m), device
        cfg = TraceConfig(self.width, self.height, self.m, int(pixel_inc), int(fade))
        self._create("fsea_trace_create", ctypes.byref(cfg), device)

    def frames(self, data, frame_bytes, n_frames=None, flip=True, images=True):
        """Host uint8 bytes -> (n_frames, height, width) uint8, frame f from byte f * frame_bytes on (n_frames defaults to
        every frame that starts inside `data`); images=False advances the canvas and returns None."""
        b = np.ascontiguousarray(data, dtype=np.uint8).ravel()
        if n_frames is None:
            n_frames = -(-b.size // int(frame_bytes)) if int(frame_bytes) > 0 else 0
        out = np.empty((max(n_frames, 0), self.height, self.width), dtype=np.uint8) if images else None
        _check(self._L.fsea_trace_frames_host(self._p, b.ctypes.data if b.size else None, b.size, int(bool(flip)),
                                              frame_bytes, n_frames, out.ctypes.data if images else None))
        return out

    def frames_device(self, d_bytes_ptr, n_bytes, frame_bytes, n_frames, d_images_ptr, flip=True, stream=0):
        """Device pointers (ints; images 16-byte aligned or 0 for none): n_bytes readable bytes in, n_frames images out;
        asynchronous."""
        _check(self._L.fsea_trace_frames_device(self._p, d_bytes_ptr, n_bytes, int(bool(flip)), frame_bytes, n_frames,
                                                d_images_ptr or None, stream or None))

    def canvas(self):
        """The canvas as it stands, (height, width) uint8."""
        out = np.empty((self.height, self.width), dtype=np.uint8)
        _check(self._L.fsea_trace_canvas_host(self._p, out.ctypes.data))
        return out


def detect_finish(sums, n_elements):
    """fsea_detect_finish: (mean, sd) of a block of n_elements bytes from its three integer sums (host arithmetic, needs no
    GPU)."""
    a = np.ascontiguousarray(sums, dtype=np.uint64).ravel()
    mean, sd = ctypes.c_double(), ctypes.c_double()
    _check(hip_lib().fsea_detect_finish(a.ctypes.data, n_elements, ctypes.byref(mean), ctypes.byref(sd)))
    return mean.value, sd.value


def capture_segment(sd, threshold, capturing=False):
    """fsea_capture_segment: the scene's state machine over the standard deviations of a scan's blocks -> a list of
    (first_block, n_blocks, continues, open) (host arithmetic, needs no GPU)."""
    a = np.ascontiguousarray(sd, dtype=np.float64).ravel()
    runs, n = (CaptureRun * (a.size // 2 + 1))(), ctypes.c_size_t(0)
    _check(hip_lib().fsea_capture_segment(a.ctypes.data if a.size else None, a.size, float(threshold), int(bool(capturing)),
                                          runs, ctypes.byref(n)))
    return [(r.first_block, r.n_blocks, bool(r.continues), bool(r.open)) for r in runs[:n.value]]


class Detect(_Handle):
    """The burst detector of the reference's signal scene on one device; thin wrapper over fsea_detect_*: per block of
    8-bit samples the three integer sums of nrf_signal_detector_process, or its mean and standard deviation."""
    _kind = "detect"

    def __init__(self, device=0):
        self.device = device
        self._create("fsea_detect_create", device)

    def sums_device(self, d_iq_ptr, block_bytes, n_blocks, d_sums_ptr, flip=False, stream=0):
        """Device pointers (ints, 16-byte aligned): n_blocks blocks in, three uint64 per block out; asynchronous."""
        _check(self._L.fsea_detect_u8_device(self._p, d_iq_ptr, block_bytes, n_blocks, int(bool(flip)), d_sums_ptr,
                                             stream or None))

    def run(self, iq_u8, block_bytes, flip=False):
        """Host uint8 bytes -> (mean, sd), one float64 each per whole block of block_bytes."""
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        n = iq.size // int(block_bytes) if int(block_bytes) > 0 else 0
        mean, sd = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        _check(self._L.fsea_detect_u8_host(self._p, iq.ctypes.data, block_bytes, n, int(bool(flip)), mean.ctypes.data,
                                           sd.ctypes.data))
        return mean, sd


class Capture(_ResettableHandle):
    """The signal scene on a recording that stays on the device; thin wrapper over fsea_capture_*.  scan() finds the
    bursts and filters their blocks; the bursts accumulate until reset()."""
    _kind = "capture"

    def __init__(self, taps, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        self.n_taps, self.device = t.size, device
        self._create("fsea_capture_create", t.ctypes.data if t.size else None, t.size, device)

    def scan(self, iq_u8, block_bytes, threshold, flip=False):
        """Host uint8 bytes, every whole block of block_bytes; returns the number of bursts so far."""
        iq = np.ascontiguousarray(iq_u8, dtype=np.uint8).ravel()
        n = iq.size // int(block_bytes) if int(block_bytes) > 0 else 0
        _check(self._L.fsea_capture_scan_host(self._p, iq.ctypes.data, block_bytes, n, int(bool(flip)), float(threshold)))
        return self.n_bursts

    def scan_device(self, d_iq_ptr, block_bytes, n_blocks, threshold, flip=False, stream=0):
        _check(self._L.fsea_capture_scan_device(self._p, d_iq_ptr, block_bytes, n_blocks, int(bool(flip)), float(threshold),
                                                stream or None))
        return self.n_bursts

    def stats(self):
        """(mean, sd) of the last scan's blocks."""
        n = self._L.fsea_capture_n_blocks(self._p)
        out = np.empty((2, n), dtype=np.float64)
        m, s = ctypes.c_double(), ctypes.c_double()
        for b in range(n):
            _check(self._L.fsea_capture_stats(self._p, b, ctypes.byref(m), ctypes.byref(s)))
            out[:, b] = m.value, s.value
        return out[0], out[1]

    @property
    def n_bursts(self):
        return self._L.fsea_capture_n_bursts(self._p)

    def burst(self, k):
        """CaptureBurstInfo of burst k."""
        info = CaptureBurstInfo()
        _check(self._L.fsea_capture_burst(self._p, k, ctypes.byref(info)))
        return info

    def burst_pairs(self, k):
        out = np.empty(self.burst(k).n_pairs, dtype=np.complex64)
        _check(self._L.fsea_capture_burst_pairs_host(self._p, k, out.ctypes.data))
        return out

    def burst_lines(self, k, m=1, n_points=None):
        """(256 m, 256 m) uint8: the burst's first n_points points (default all) joined in order."""
        n = self.burst(k).n_pairs if n_points is None else int(n_points)
        img = np.empty((256 * m, 256 * m), dtype=np.uint8)
        _check(self._L.fsea_capture_burst_lines_host(self._p, k, int(m), n, img.ctypes.data))
        return img

    def burst_lines_device(self, k, m, n_points, d_image_ptr, stream=0):
        _check(self._L.fsea_capture_burst_lines_device(self._p, k, int(m), n_points, d_image_ptr, stream or None))


class PinnedArray:
    """A numpy view of fsea_host_alloc'ed (page-locked) memory; .array is valid until close()."""

    def __init__(self, shape, dtype):
        self._ptr = ctypes.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _check(hip_lib().fsea_host_alloc(n, ctypes.byref(self._ptr)))
        buf = (ctypes.c_char * n).from_address(self._ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def close(self):
        if self._ptr:
            self.array = None
            hip_lib().fsea_host_free(self._ptr)
            self._ptr = ctypes.c_void_p()


class DeviceBuffer:
    """nbytes of device memory (fsea_device_alloc; at least 16, so that an empty buffer has an address too).  .ptr is a
    ctypes.c_void_p: pass it, or an int made of .ptr.value plus an offset, wherever a device pointer is taken."""

    def __init__(self, nbytes, device=0):
        self.ptr, self.nbytes, self.device = ctypes.c_void_p(), nbytes, device
        _check(hip_lib().fsea_device_alloc(device, max(nbytes, 16), ctypes.byref(self.ptr)))

    def upload(self, arr):
        """The bytes of a host array to the start of the buffer (fsea_copy_to_device); returns the buffer."""
        arr = np.ascontiguousarray(arr)
        _check(hip_lib().fsea_copy_to_device(self.device, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, shape, byte_offset=0):
        """A new host array of `shape` and `dtype` from byte_offset on (fsea_copy_to_host)."""
        out = np.empty(shape, dtype=dtype)
        _check(hip_lib().fsea_copy_to_host(self.device, out.ctypes.data, self.ptr.value + byte_offset, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            hip_lib().fsea_device_free(self.device, self.ptr)
            self.ptr = ctypes.c_void_p()


class Stream:
    """A non-blocking stream on one device (fsea_stream_create); pass it wherever a `stream=` argument is taken, or to the
    library's functions themselves.  .handle is the hipStream_t as a ctypes.c_void_p."""

    def __init__(self, device=0):
        self.device, self.handle = device, ctypes.c_void_p()
        _check(hip_lib().fsea_stream_create(device, ctypes.byref(self.handle)))
        self._as_parameter_ = self.handle

    def close(self):
        if self.handle:
            _check(hip_lib().fsea_stream_destroy(self.device, self.handle))
            self.handle = self._as_parameter_ = ctypes.c_void_p()


def composite_max_device(d_dst, d_src, dst_x, dst_y, width, height, dst_stride, dst_height, src_stride, device=0,
                         stream=0):
    _check(hip_lib().fsea_composite_max_device(d_dst, d_src, dst_x, dst_y, width, height, dst_stride, dst_height,
                                               src_stride, device, stream or None))


def stitch_tiles_device(d_image, d_tiles, n_tiles, first_x, width_step, width, height, image_stride, device=0,
                        stream=0):
    _check(hip_lib().fsea_stitch_tiles_device(d_image, d_tiles, n_tiles, first_x, width_step, width, height,
                                              image_stride, device, stream or None))
