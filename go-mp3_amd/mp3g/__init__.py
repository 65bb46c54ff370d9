"""mp3g -- Python binding of libmp3g.so (the MI355X granule-decode C-ABI).

The C-ABI (include/mp3g.h) is the product boundary; this module is a thin
ctypes layer used by the tests and bench.py.  It never falls back to a CPU
implementation: if libmp3g.so is missing or no gfx950 device is present the
calls raise.

Boundary structs mirror include/mp3g.h exactly (asserted sizes below).
"""
import ctypes as C
import os
import time

import numpy as np

__all__ = ["CHANNEL_DTYPE", "GRANULE_DTYPE", "STREAM_DTYPE", "STATE_DTYPE", "MODE_EXACT",
           "MODE_FAST", "FLAG_CHECKED", "FLAG_KERNEL_V1", "FLAG_KERNEL_V2", "FLAG_HOT_STATS", "FLAG_HOST_HUFFMAN", "STATE_IN", "STATE_OUT", "Mp3gError", "lib", "lib_path",
           "decode_host", "validate", "Plan", "device_count", "streams_for", "parse_stream",
           "parse_streams", "Decoder", "HJOB_DTYPE", "scan_streams", "huffman_execute", "HUFF_ROWS_COUNT1",
           "HUFF_STAGE_WIDE", "HUFF_STAGE_MID", "huffman_stage_flags", "decode_streams",
           "WINDOW_DTYPE", "WINDOW_ROW_DTYPE", "WINDOW_GAPLESS", "scan_windows", "WindowPlan",
           "decode_windows_tensor", "RESAMPLE_ROW_DTYPE", "RESAMPLE_FAST", "RESAMPLE_BEST", "Resampler",
           "stream_rates", "decode_windows_resampled_tensor", "VARRESAMPLE_ROW_DTYPE", "VarResampler"]

HERE = os.path.dirname(os.path.abspath(__file__))

CHANNEL_DTYPE = np.dtype([
    ("count1", "<u2"), ("global_gain", "u1"), ("scalefac_scale", "u1"), ("preflag", "u1"),
    ("win_switch_flag", "u1"), ("block_type", "u1"), ("mixed_block_flag", "u1"),
    ("subblock_gain", "u1", (3,)), ("scalefac_l", "u1", (22,)), ("scalefac_s", "u1", (13, 3)),
])
GRANULE_DTYPE = np.dtype([("header", "<u4"), ("gr", "<u4"), ("ch", CHANNEL_DTYPE, (2,)),
                          ("reserved", "u1", (8,))])
STREAM_DTYPE = np.dtype([("first_granule", "<u8"), ("n_granules", "<u4"), ("flags", "<u4")])
STATE_DTYPE = np.dtype([("store", "<f4", (2, 32, 18)), ("vvec", "<f4", (2, 1024))])
# one Huffman job per (granule, channel) of the GPU main-data path (mp3g_hjob)
HJOB_DTYPE = np.dtype([("part2_start", "<u8"), ("bit_end", "<u8"), ("scf0_delta", "<u4"),
                       ("part2_3_length", "<u2"), ("big_values", "<u2"), ("region1_start", "<u2"),
                       ("region2_start", "<u2"), ("table_select", "u1", (3,)), ("count1_table", "u1"),
                       ("sf_kind", "u1"), ("scfsi", "u1"), ("slen", "u1", (4,)), ("nsf", "u1", (4,)),
                       ("sf0_kind", "u1"), ("sf0_slen", "u1", (2,)), ("reserved", "u1", (3,))])
# sample windows (mp3g_window) and the layout a windowed scan returns (mp3g_window_row)
WINDOW_DTYPE = np.dtype([("start", "<u8"), ("n_samples", "<u4"), ("flags", "<u4")])
WINDOW_ROW_DTYPE = np.dtype([("lead", "<u4"), ("skip", "<u4"), ("n_valid", "<u4"), ("reserved", "<u4")])
WINDOW_GAPLESS = 1
assert WINDOW_DTYPE.itemsize == 16 and WINDOW_ROW_DTYPE.itemsize == 16
assert CHANNEL_DTYPE.itemsize == 72 and GRANULE_DTYPE.itemsize == 160 and HJOB_DTYPE.itemsize == 48
assert STREAM_DTYPE.itemsize == 16 and STATE_DTYPE.itemsize == 12800

MODE_EXACT, MODE_FAST, FLAG_CHECKED, FLAG_KERNEL_V1, FLAG_HOST_HUFFMAN = 0, 1, 0x100, 0x200, 0x400
FLAG_KERNEL_V2 = 0x800  # exact mode via the workgroup v2 kernel (cross-check of the default v4)
FLAG_HOT_STATS = 0x1000  # fast plans: count the hot-granule fallback's work (Plan.hot_stats)
STATE_IN, STATE_OUT = 1, 2
MP3G_PCM_BYTES_PER_GRANULE = 2304  # include/mp3g.h: 576 stereo s16 samples
# output formats (include/mp3g.h MP3G_OUT_*): s16 [n, 576, 2]; float32 in the
# same order; float32 planar -- stream (first F, n granules) owns floats
# [F * 1152, (F + n) * 1152), plane ch at F * 1152 + ch * n * 576; the mono
# downmixes [n, 576]: (L + R) >> 1 of the s16 samples, (fL + fR) * 0.5f of the
# float samples (a mono granule: channel 0 as it is)
OUT_S16, OUT_F32, OUT_F32_PLANAR, OUT_S16_MONO, OUT_F32_MONO = 0, 1, 2, 3, 4
_OUT_INT16 = (OUT_S16, OUT_S16_MONO)  # (the others hold float32)
_OUT_MONO = (OUT_S16_MONO, OUT_F32_MONO)

STATUS = {0: "ok", 1: "invalid argument", 2: "invalid granule", 3: "no device", 4: "device error",
          5: "out of memory", 6: "parse error", 7: "eof", 8: "unsupported", 9: "no Xing/Info header",
          10: "unexpected EOF", 11: "reader error"}
ERR_NO_XING_HEADER, ERR_UNEXPECTED_EOF, EOF, ERR_READ = 9, 10, 7, 11

# include/mp3g.h mp3g_reader: io.Reader.Read / io.Seeker.Seek as C callbacks
READ_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)
SEEK_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_int64, C.c_int)


class _Reader(C.Structure):
    _fields_ = [("read", READ_FN), ("seek", SEEK_FN), ("user", C.c_void_p)]


class _AugmentArgs(C.Structure):  # include/mp3g.h mp3g_augment_args
    _fields_ = ([(k, C.c_void_p) for k in ("x", "out", "lengths", "rir_index", "noise", "noise_lengths",
                                            "noise_power", "slots", "stats")]
                + [(k, C.c_uint32) for k in ("n_rows", "n_planes", "T", "n_noise", "Tn", "A", "flags", "zero")])


class Mp3gError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__(f"mp3g status {status} ({STATUS.get(status, '?')}): {msg}")
        self.status = status


_lib = None


def lib_path():
    # MP3G_LIB: another build of the same library (kernel experiments)
    return os.environ.get("MP3G_LIB") or os.path.join(HERE, "libmp3g.so")


def lib():
    """Load libmp3g.so (import torch first when sharing the process with it)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise Mp3gError(3, f"{path} not built (run __graft_entry__.build())")
        L = C.CDLL(path)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.mp3g_abi_version.restype = C.c_int
        L.mp3g_status_string.argtypes = [C.c_int]
        L.mp3g_status_string.restype = C.c_char_p
        L.mp3g_last_error.restype = C.c_char_p
        L.mp3g_device_count.argtypes = [C.POINTER(C.c_int)]
        L.mp3g_validate.argtypes = [vp, vp, u64, C.POINTER(u64)]
        L.mp3g_plan_create.argtypes = [C.c_int, vp, u32, u32, u32, C.POINTER(vp)]
        L.mp3g_plan_destroy.argtypes = [vp]
        L.mp3g_plan_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.mp3g_plan_execute.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.mp3g_plan_synth_execute.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "mp3g_plan_hot_stats"):  # ABI 5 (an older build through MP3G_LIB: A/B runs)
            L.mp3g_plan_hot_stats.argtypes = [vp, C.POINTER(u64), C.c_int]
        L.mp3g_decode_host.argtypes = [C.c_int, vp, vp, u64, vp, u32, vp, vp, vp, u32]
        if hasattr(L, "mp3g_plan_execute_out"):  # (an older build through MP3G_LIB: A/B runs)
            L.mp3g_out_bytes_per_granule.argtypes = [u32]
            L.mp3g_out_bytes_per_granule.restype = C.c_size_t
            L.mp3g_plan_execute_out.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp]
            L.mp3g_decode_host_out.argtypes = [C.c_int, vp, vp, u64, vp, u32, vp, vp, vp, u32, u32]
        L.mp3g_plan_debug_phases.argtypes = [vp, vp, vp, vp, C.POINTER(u64), vp]
        L.mp3g_plan_debug_timeline.argtypes = [vp, vp, vp, vp, C.POINTER(u64), vp]
        if hasattr(L, "mp3g_debug_clock_probe"):  # (an older build through MP3G_LIB: A/B runs)
            L.mp3g_debug_clock_probe.argtypes = [C.c_int, vp, vp, u32, u32, vp]
        i64, sz = C.c_int64, C.c_size_t
        L.mp3g_parse_stream.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64),
                                        C.POINTER(C.c_int)]
        L.mp3g_parse_streams.argtypes = [u32, vp, vp, C.c_int, C.POINTER(vp), C.POINTER(vp),
                                         C.POINTER(u64), vp, vp]
        L.mp3g_free.argtypes = [vp]
        L.mp3g_scan_streams.argtypes = [u32, vp, vp, C.c_int, C.POINTER(vp)]
        L.mp3g_scan_buffers.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)] + [C.POINTER(vp)] * 5
        L.mp3g_scan_free.argtypes = [vp]
        if hasattr(L, "mp3g_scan_windows"):  # (an older build through MP3G_LIB: A/B runs)
            L.mp3g_scan_windows.argtypes = [u32, vp, vp, vp, C.c_int, C.POINTER(vp)]
            L.mp3g_scan_window_rows.argtypes = [vp, C.POINTER(vp)]
            L.mp3g_plan_create_windows.argtypes = [C.c_int, vp, vp, u32, u32, u32, u32, C.POINTER(vp)]
            L.mp3g_plan_execute_windows.argtypes = [vp, vp, vp, vp, u32, vp]
        if hasattr(L, "mp3g_resampler_create"):  # (an older build through MP3G_LIB: A/B runs)
            L.mp3g_resampler_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                C.POINTER(vp)]
            L.mp3g_resampler_free.argtypes = [vp]
            L.mp3g_resampler_free.restype = None
            L.mp3g_resampler_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(vp),
                                              C.POINTER(u32)]
            L.mp3g_resample_host.argtypes = [vp, vp, u64, u64, u64, u64, vp]
            L.mp3g_resample_rows.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, vp]
            L.mp3g_stream_rates.argtypes = [u32, vp, vp, C.c_int, vp, vp]
        if hasattr(L, "mp3g_varresampler_create"):  # (an older build through MP3G_LIB: A/B runs)
            L.mp3g_varresampler_create.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(vp)]
            L.mp3g_varresampler_free.argtypes = [vp]
            L.mp3g_varresampler_free.restype = None
            L.mp3g_varresampler_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(vp),
                                                 C.POINTER(u32), C.POINTER(u32)]
            L.mp3g_varresample_host.argtypes = [vp, vp, u64, u64, u64, u64, vp, u32, u32, C.c_float]
            L.mp3g_varresample_rows.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, vp]
        if hasattr(L, "mp3g_logmel_create"):  # (an older build through MP3G_LIB: A/B runs)
            L.mp3g_logmel_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, u32,
                                             C.POINTER(vp)]
            L.mp3g_logmel_free.argtypes = [vp]
            L.mp3g_logmel_free.restype = None
            L.mp3g_logmel_info.argtypes = [vp, C.POINTER(u32)] + [C.POINTER(vp)] * 4 + [C.POINTER(u32)]
            L.mp3g_logmel_frames.argtypes = [vp, u64]
            L.mp3g_logmel_frames.restype = u64
            L.mp3g_logmel_host.argtypes = [vp, vp, u64, u64, vp, u64]
            L.mp3g_logmel_execute.argtypes = [vp, vp, u32, u32, u32, vp, u32, u32, vp]
            L.mp3g_logmel_log10f.argtypes = [vp, u64, vp]
            L.mp3g_logmel_log10f.restype = None
        if hasattr(L, "mp3g_fbank_create"):  # (an older build through MP3G_LIB: A/B runs)
            L.mp3g_fbank_create.argtypes = [C.c_int] * 5 + [C.c_double] * 4 + [C.c_int, u32, C.POINTER(vp)]
            L.mp3g_fbank_free.argtypes = [vp]
            L.mp3g_fbank_free.restype = None
            L.mp3g_fbank_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)] + [C.POINTER(vp)] * 5 + [C.POINTER(u32)]
            L.mp3g_fbank_frames.argtypes = [vp, u64]
            L.mp3g_fbank_frames.restype = u64
            L.mp3g_fbank_host.argtypes = [vp, vp, u64, u64, vp, u64]
            L.mp3g_fbank_execute.argtypes = [vp, vp, u32, u32, u32, vp, u32, u32, vp]
            L.mp3g_fbank_logf.argtypes = [vp, u64, vp]
            L.mp3g_fbank_logf.restype = None
        if hasattr(L, "mp3g_stft_create"):
            L.mp3g_stft_create.argtypes = [C.c_int] * 7 + [C.c_double] * 2 + [C.c_int, C.c_float, u32, C.POINTER(vp)]
            L.mp3g_stft_free.argtypes = [vp]
            L.mp3g_stft_free.restype = None
            L.mp3g_stft_info.argtypes = [vp, C.POINTER(u32)] + [C.POINTER(vp)] * 4 + [C.POINTER(u32)]
            L.mp3g_stft_frames.argtypes = [vp, u64]
            L.mp3g_stft_frames.restype = u64
            L.mp3g_stft_host.argtypes = [vp, vp, u64, u64, vp, u64]
            L.mp3g_stft_execute.argtypes = [vp, vp, u32, u32, u32, vp, u32, u32, vp]
        if hasattr(L, "mp3g_mfcc_create"):
            L.mp3g_mfcc_create.argtypes = [C.c_int] * 6 + [C.c_double] * 6 + [C.c_int, u32, C.POINTER(vp)]
            L.mp3g_mfcc_free.argtypes = [vp]
            L.mp3g_mfcc_free.restype = None
            L.mp3g_mfcc_info.argtypes = [vp, C.POINTER(vp), C.POINTER(u32), C.POINTER(vp), C.POINTER(vp),
                                         C.POINTER(C.c_float), C.POINTER(u32)]
            L.mp3g_mfcc_frames.argtypes = [vp, u64]
            L.mp3g_mfcc_frames.restype = u64
            L.mp3g_mfcc_host.argtypes = [vp, vp, u64, u64, vp, u64]
            L.mp3g_mfcc_execute.argtypes = [vp, vp, u32, u32, u32, vp, u32, u32, vp]
            L.mp3g_cmvn_rows.argtypes = [C.c_int, vp, u32, u32, u32, u32, u32, vp, u32, vp]
            L.mp3g_cmvn_host.argtypes = [vp, u32, u32, u32, u32, u32, vp, u32]
        if hasattr(L, "mp3g_sliding_cmn_rows"):
            f32 = C.c_float
            L.mp3g_sliding_cmn_rows.argtypes = [C.c_int, vp, vp, u32, u32, u32, u32, u32, vp, u32, u32, u32, vp]
            L.mp3g_sliding_cmn_host.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, u32, u32, u32]
            L.mp3g_vad_energy_rows.argtypes = [C.c_int, vp, u32, u32, u32, u32, u32, u32, vp, f32, f32, f32, u32, vp,
                                               vp, vp]
            L.mp3g_vad_energy_host.argtypes = [vp, u32, u32, u32, u32, u32, u32, vp, f32, f32, f32, u32, vp, vp]
            L.mp3g_select_frames_rows.argtypes = [C.c_int, vp, u32, u32, u32, u32, u32, vp, vp, vp, u32, u32, vp, vp]
            L.mp3g_select_frames_host.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp, vp, u32, u32, vp]
        if hasattr(L, "mp3g_specaug_rows"):
            L.mp3g_specaug_rows.argtypes = [C.c_int, vp, vp, u32, u32, u32, u32, u32, vp, vp, u32, C.c_float, vp, vp]
            L.mp3g_specaug_host.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, vp, u32, C.c_float, vp]
        if hasattr(L, "mp3g_add_deltas_rows"):
            L.mp3g_delta_scales.argtypes = [u32, u32, vp]
            L.mp3g_add_deltas_rows.argtypes = [C.c_int, vp, vp] + [u32] * 6 + [vp, u32, u32, u32, vp]
            L.mp3g_add_deltas_host.argtypes = [vp, vp] + [u32] * 6 + [vp, u32, u32, u32]
            L.mp3g_stack_frames_count.argtypes = [u32, u32, u32]
            L.mp3g_stack_frames_count.restype = u32
            L.mp3g_stack_frames_rows.argtypes = [C.c_int, vp] + [u32] * 5 + [vp] + [u32] * 5 + [vp, u32, u32, vp, vp]
            L.mp3g_stack_frames_host.argtypes = [vp] + [u32] * 5 + [vp] + [u32] * 5 + [vp, u32, u32, vp]
        if hasattr(L, "mp3g_loudness_create"):
            dp = C.POINTER(vp)
            L.mp3g_loudness_create.argtypes = [C.c_int, C.c_int, dp]
            L.mp3g_loudness_free.argtypes = [vp]
            L.mp3g_loudness_free.restype = None
            L.mp3g_loudness_info.argtypes = [vp, C.POINTER(u32), dp, dp, dp, dp, dp]
            L.mp3g_loudness_blocks.argtypes = [vp, u64]
            L.mp3g_loudness_blocks.restype = u64
            L.mp3g_loudness_host.argtypes = [vp, vp, u32, u32, u32, vp, vp]
            L.mp3g_loudness_scratch_bytes.argtypes = [vp, u32, u32, u32]
            L.mp3g_loudness_scratch_bytes.restype = u64
            L.mp3g_loudness_rows.argtypes = [vp, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
            L.mp3g_loudness_target_energy.argtypes = [C.c_double]
            L.mp3g_loudness_target_energy.restype = C.c_double
            L.mp3g_gain_rows.argtypes = [C.c_int, vp, u32, u32, u32, vp, vp, C.c_double, C.c_float, vp, vp]
            L.mp3g_gain_host.argtypes = [vp, u32, u32, u32, vp, vp, C.c_double, C.c_float, vp]
        if hasattr(L, "mp3g_true_peak_rows"):
            L.mp3g_true_peak_coefs.argtypes = [C.POINTER(vp)]
            L.mp3g_true_peak_tile.argtypes = []
            L.mp3g_true_peak_tile.restype = u32
            L.mp3g_true_peak_scratch_bytes.argtypes = [u32, u32, u32]
            L.mp3g_true_peak_scratch_bytes.restype = u64
            L.mp3g_true_peak_host.argtypes = [vp, u32, u32, u32, vp, vp]
            L.mp3g_true_peak_rows.argtypes = [C.c_int, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
            L.mp3g_loudness_range_host.argtypes = [vp, vp, u32, u32, u32, vp, vp]
            L.mp3g_loudness_range_scratch_bytes.argtypes = [vp, u32, u32, u32]
            L.mp3g_loudness_range_scratch_bytes.restype = u64
            L.mp3g_loudness_range_rows.argtypes = [vp, u32, u32, u32, vp, vp, u32, vp, vp, vp, vp]
            L.mp3g_gain_rows_peak.argtypes = [C.c_int, vp, u32, u32, u32, vp, vp, C.c_double, C.c_float, vp, vp, vp]
            L.mp3g_gain_host_peak.argtypes = [vp, u32, u32, u32, vp, vp, C.c_double, C.c_float, vp, vp]
        if hasattr(L, "mp3g_augment_rows"):
            L.mp3g_reverb_create.argtypes = [C.c_int, C.c_int, vp, u32, u32, vp, C.POINTER(vp)]
            L.mp3g_reverb_free.argtypes = [vp]
            L.mp3g_reverb_free.restype = None
            L.mp3g_reverb_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(vp), C.POINTER(vp),
                                           C.POINTER(vp), C.POINTER(u64)]
            L.mp3g_reverb_read_spectra.argtypes = [vp, vp]
            L.mp3g_reverb_scratch_bytes.argtypes = [vp, u32, u32, u32]
            L.mp3g_reverb_scratch_bytes.restype = u64
            L.mp3g_augment_host.argtypes = [vp, C.POINTER(_AugmentArgs)]
            L.mp3g_augment_rows.argtypes = [vp, C.c_int, C.POINTER(_AugmentArgs), vp, vp, vp, vp, u64, vp]
            L.mp3g_augment_debug_launch.argtypes = L.mp3g_augment_rows.argtypes + [u32]
            L.mp3g_row_power_scratch_bytes.argtypes = [u32, u32]
            L.mp3g_row_power_scratch_bytes.restype = u64
            L.mp3g_row_power_host.argtypes = [vp, u32, u32, vp, vp]
            L.mp3g_row_power_rows.argtypes = [C.c_int, vp, u32, u32, vp, vp, vp, vp]
        L.mp3g_lame_parse.argtypes = [vp, C.c_size_t, C.POINTER(_LameInfo)]
        L.mp3g_lame_parse_reader.argtypes = [vp, C.c_size_t, C.POINTER(_LameInfo), C.POINTER(C.c_size_t)]
        L.mp3g_lame_total_delay.argtypes = [C.POINTER(_LameInfo)]
        L.mp3g_lame_total_padding.argtypes = [C.POINTER(_LameInfo)]
        L.mp3g_lame_trim.argtypes = [C.POINTER(_LameInfo), u64, u32, C.POINTER(u64), C.POINTER(u64)]
        L.mp3g_lame_toc_offset.argtypes = [C.POINTER(_LameInfo), C.c_double, u64, C.POINTER(u64)]
        L.mp3g_lame_toc_offset.restype = C.c_int
        L.mp3g_huffman_execute.argtypes = [C.c_int, vp, u64, vp, vp, vp, vp]
        L.mp3g_huffman_execute_ex.argtypes = [C.c_int, vp, u64, vp, vp, vp, u32, vp]
        L.mp3g_huffman_stage_flags.argtypes = [vp, u64]
        L.mp3g_huffman_stage_flags.restype = u32
        L.mp3g_decode_streams.argtypes = [C.c_int, u32, vp, vp, C.c_int, u32, C.POINTER(vp), C.POINTER(u64),
                                          vp, vp]
        if hasattr(L, "mp3g_decode_streams_into_out"):  # (an older build through MP3G_LIB: A/B runs)
            L.mp3g_decode_streams_into_out.argtypes = [C.c_int, u32, vp, vp, C.c_int, u32, u32, vp, u32, u64,
                                                       C.POINTER(u64), vp, vp]
        L.mp3g_decode_streams_into.argtypes = [C.c_int, u32, vp, vp, C.c_int, u32, u32, vp, u64, C.POINTER(u64),
                                               vp, vp]
        L.mp3g_release_cached_buffers.argtypes = []
        L.mp3g_release_cached_buffers.restype = None
        L.mp3g_decoder_new.argtypes = [vp, sz, C.c_int, C.c_int, u32, C.POINTER(vp)]
        L.mp3g_decoder_new_reader.argtypes = [C.POINTER(_Reader), C.c_int, u32, C.POINTER(vp)]
        L.mp3g_decoder_free.argtypes = [vp]
        L.mp3g_decoder_read.argtypes = [vp, vp, sz, C.POINTER(sz)]
        L.mp3g_decoder_read_full.argtypes = [vp, vp, sz, C.POINTER(sz)]
        L.mp3g_decoder_seek.argtypes = [vp, i64, C.c_int, C.POINTER(i64)]
        L.mp3g_decoder_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(i64),
                                        C.POINTER(i64)]
        for fn in ("duration_ns", "position_ns", "remaining_ns", "sample_position", "sample_count"):
            getattr(L, "mp3g_decoder_" + fn).argtypes = [vp]
            getattr(L, "mp3g_decoder_" + fn).restype = i64
        L.mp3g_decoder_progress.argtypes = [vp]
        L.mp3g_decoder_progress.restype = C.c_double
        for fn in ("seek_to_sample", "seek_to_time_ns", "skip_ns"):
            getattr(L, "mp3g_decoder_" + fn).argtypes = [vp, i64]
        _lib = L
    return _lib


def _check(st):
    if st != 0:
        raise Mp3gError(st, lib().mp3g_last_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int()
    _check(lib().mp3g_device_count(C.byref(n)))
    return n.value


def streams_for(lengths, flags=0):
    """Stream table for consecutive runs of granules with the given lengths."""
    lengths = np.asarray(lengths, dtype=np.int64)
    s = np.zeros(len(lengths), STREAM_DTYPE)
    s["first_granule"] = np.concatenate([[0], np.cumsum(lengths)[:-1]]) if len(lengths) else []
    s["n_granules"] = lengths
    s["flags"] = flags
    return s


def validate(granules, coeffs):
    granules = np.ascontiguousarray(granules, dtype=GRANULE_DTYPE)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
    bad = C.c_uint64()
    st = lib().mp3g_validate(_ptr(granules), _ptr(coeffs), len(granules), C.byref(bad))
    return st, bad.value


def out_bytes_per_granule(out_format):
    """Output bytes per granule of OUT_* (2304 / 4608 / 4608 / 1152 / 2304); 0 for an unknown format."""
    return int(lib().mp3g_out_bytes_per_granule(int(out_format)))


def planar_views(out, streams):
    """The [2, n * 576] view of each stream in an OUT_F32_PLANAR buffer (a flat
    numpy array or torch tensor of float32, 1152 per granule slot): plane ch
    of stream (F, n) starts at float F * 1152 + ch * n * 576."""
    views = []
    for s in np.asarray(streams, dtype=STREAM_DTYPE):
        f, n = int(s["first_granule"]), int(s["n_granules"])
        views.append(out[f * 1152:(f + n) * 1152].reshape(2, n * 576))
    return views


def decode_host(granules, coeffs, streams=None, state_in=None, state_out=None, mode=MODE_EXACT,
                device=0, out_format=OUT_S16):
    """Synchronous decode of host arrays (the cgo drop-in entry, mp3g_decode_host /
    mp3g_decode_host_out).

    granules: GRANULE_DTYPE[n]; coeffs: int16[n, 2, 576]; streams: STREAM_DTYPE[s]
    (default: one stream covering everything).  Returns (pcm, state_out): pcm is
    int16[n, 576, 2] (OUT_S16), float32[n, 576, 2] (OUT_F32), a flat float32
    array of n * 1152 (OUT_F32_PLANAR: planar_views(pcm, streams) gives each
    stream's [2, n * 576]), or the mono downmix int16[n, 576] (OUT_S16_MONO) /
    float32[n, 576] (OUT_F32_MONO).  trunc(float * 32768) is the s16 sample
    (stereo formats).
    """
    granules = np.ascontiguousarray(granules, dtype=GRANULE_DTYPE)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
    n = len(granules)
    assert coeffs.shape == (n, 2, 576), coeffs.shape
    if streams is None:
        streams = streams_for([n])
    streams = np.ascontiguousarray(streams, dtype=STREAM_DTYPE)
    if state_in is not None:
        state_in = np.ascontiguousarray(state_in, dtype=STATE_DTYPE)
    if state_out is None:
        state_out = np.zeros(len(streams), STATE_DTYPE)
    if out_format == OUT_S16:
        pcm = np.zeros((n, 576, 2), np.int16)
        _check(lib().mp3g_decode_host(device, _ptr(granules), _ptr(coeffs), n, _ptr(streams),
                                      len(streams), _ptr(state_in), _ptr(state_out), _ptr(pcm), mode))
        return pcm, state_out
    if out_format in _OUT_MONO:
        pcm = np.zeros((n, 576), np.int16 if out_format == OUT_S16_MONO else np.float32)
    else:
        pcm = np.zeros(n * 1152 if out_format == OUT_F32_PLANAR else (n, 576, 2), np.float32)
    _check(lib().mp3g_decode_host_out(device, _ptr(granules), _ptr(coeffs), n, _ptr(streams), len(streams),
                                      _ptr(state_in), _ptr(state_out), _ptr(pcm), int(out_format), mode))
    return pcm, state_out


def _take(ptr, n, dtype, shape):
    """Copy a library-allocated buffer into numpy and free it (no 2 GiB limit)."""
    nbytes = n * np.dtype(dtype).itemsize * int(np.prod(shape[1:]))
    if n:
        raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))
        out = raw.view(dtype).reshape(shape).copy()
    else:
        out = np.zeros(shape, dtype)
    lib().mp3g_free(ptr)
    return out


def parse_stream(data: bytes):
    """Host bitstream parse (mp3g_parse_stream): (granules, coeffs [n,2,576], end_status)."""
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    g, c, n, st = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_int()
    _check(lib().mp3g_parse_stream(_ptr(buf), len(data), C.byref(g), C.byref(c), C.byref(n), C.byref(st)))
    k = n.value
    return (_take(g, k, GRANULE_DTYPE, (k,)), _take(c, k, np.int16, (k, 2, 576)), st.value)


def parse_streams(datas, n_threads=0):
    """Many streams in parallel: (granules, coeffs, streams[STREAM_DTYPE], end_status[])."""
    bufs, ptrs, lens = _stream_args(datas)
    streams = np.zeros(len(datas), STREAM_DTYPE)
    status = np.zeros(max(1, len(datas)), np.int32)
    g, c, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    _check(lib().mp3g_parse_streams(len(datas), ptrs, lens, n_threads, C.byref(g), C.byref(c), C.byref(n),
                                    _ptr(streams), _ptr(status)))
    k = n.value
    return (_take(g, k, GRANULE_DTYPE, (k,)), _take(c, k, np.int16, (k, 2, 576)), streams,
            status[:len(datas)])


def _copy_out(ptr, nbytes, dtype):
    if nbytes == 0:
        return np.zeros(0, dtype)
    raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))
    return raw.view(dtype).copy()


def _stream_args(datas):
    bufs = [np.frombuffer(d, dtype=np.uint8) if len(d) else np.zeros(1, np.uint8) for d in datas]
    ptrs = (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * max(1, len(bufs)))(*[len(d) for d in datas])
    return bufs, ptrs, lens


def scan_streams(datas, n_threads=0):
    """Host scan of the GPU main-data path (mp3g_scan_streams).

    Returns numpy copies: granules (side-info fields set), jobs [HJOB_DTYPE]
    (two per granule), main_data (uint8, padded), streams, end_status."""
    bufs, ptrs, lens = _stream_args(datas)
    h = C.c_void_p()
    t0 = time.perf_counter()
    _check(lib().mp3g_scan_streams(len(datas), ptrs, lens, n_threads, C.byref(h)))
    return _scan_result(h, len(datas), time.perf_counter() - t0)


def _scan_result(h, n_streams, scan_s, rows=False):
    """The buffers of scan handle h as numpy copies (scan_streams' dict; rows:
    a windowed scan's "rows" with them), and the handle freed."""
    try:
        ng, nmd = C.c_uint64(), C.c_uint64()
        pg, pj, pm, ps, pst, pr = (C.c_void_p() for _ in range(6))
        _check(lib().mp3g_scan_buffers(h, C.byref(ng), C.byref(nmd), C.byref(pg), C.byref(pj), C.byref(pm),
                                       C.byref(ps), C.byref(pst)))
        n = ng.value
        s = {"granules": _copy_out(pg, n * GRANULE_DTYPE.itemsize, GRANULE_DTYPE),
             "jobs": _copy_out(pj, 2 * n * HJOB_DTYPE.itemsize, HJOB_DTYPE),
             "main_data": _copy_out(pm, nmd.value, np.uint8),
             "streams": _copy_out(ps, n_streams * STREAM_DTYPE.itemsize, STREAM_DTYPE),
             "end_status": _copy_out(pst, n_streams * 4, np.int32)}
        if rows:
            _check(lib().mp3g_scan_window_rows(h, C.byref(pr)))
            s["rows"] = _copy_out(pr, n_streams * WINDOW_ROW_DTYPE.itemsize, WINDOW_ROW_DTYPE)
        s["scan_s"] = scan_s
        return s
    finally:
        lib().mp3g_scan_free(h)


HUFF_ROWS_COUNT1 = 1  # mp3g_huffman_execute_ex: rows written only up to count1 (+ padding)
HUFF_STAGE_WIDE = 2  # mp3g_huffman_execute_ex: 68 KB main-data stage per block (~320 kbps)
HUFF_STAGE_MID = 4  # mp3g_huffman_execute_ex: 42 KB main-data stage per block (~160-200 kbps)
# fast mode's magnitude bounds (granule_fast.hip kHotS / kHotL1, checked by
# tests/test_abi_cpu.py): a granule with max |S| > FAST_HOT_S and a time slot
# whose sum of |S| over the 32 subbands exceeds FAST_HOT_L1 runs in the
# reference's operation order
FAST_HOT_S, FAST_HOT_L1 = 4.0, 64.0


def huffman_execute(d_jobs, n_granules, d_main_data, d_granules, d_coeffs, stream=None, device=0, flags=0):
    """Device scale-factor + Huffman decode of 2 * n_granules jobs (mp3g_huffman_execute,
    or mp3g_huffman_execute_ex with flags, e.g. HUFF_ROWS_COUNT1 when the rows feed a
    default-kernel plan); buffers are device pointers (ints) or torch tensors, stream a
    hipStream_t int."""
    def p(x):
        return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
    st = C.c_void_p(stream) if stream else None
    if flags:
        _check(lib().mp3g_huffman_execute_ex(device, p(d_jobs), n_granules, p(d_main_data), p(d_granules),
                                             p(d_coeffs), flags, st))
    else:
        _check(lib().mp3g_huffman_execute(device, p(d_jobs), n_granules, p(d_main_data), p(d_granules),
                                          p(d_coeffs), st))


def huffman_stage_flags(jobs, n_granules=None):
    """mp3g_huffman_stage_flags: the main-data stage (0, HUFF_STAGE_MID,
    HUFF_STAGE_WIDE) of least modelled time for the batch's 256-job blocks
    (jobs: the scan's HJOB_DTYPE array, host memory)."""
    jobs = np.ascontiguousarray(jobs, dtype=HJOB_DTYPE)
    n = len(jobs) // 2 if n_granules is None else int(n_granules)
    return int(lib().mp3g_huffman_stage_flags(jobs.ctypes.data, n))


class _LameInfo(C.Structure):
    """mp3g_lame_info (include/mp3g.h)."""
    _fields_ = [("is_xing", C.c_uint32), ("flags", C.c_uint32), ("frame_count", C.c_uint32),
                ("byte_count", C.c_uint32), ("toc", C.c_uint8 * 100), ("vbr_scale", C.c_uint32),
                ("has_lame", C.c_uint32), ("lame_version", C.c_uint8 * 12), ("encoder_delay", C.c_uint16),
                ("encoder_padding", C.c_uint16)]


assert C.sizeof(_LameInfo) == 140

FLAG_FRAME_COUNT, FLAG_BYTE_COUNT, FLAG_TOC, FLAG_VBR_SCALE = 0x1, 0x2, 0x4, 0x8
DECODER_DELAY = 529


class LameInfo:
    """lameinfo.Info (lameinfo/lameinfo.go:20-111), parsed by libmp3g (row f4)."""

    def __init__(self, raw):
        self._raw = raw
        self.is_xing = bool(raw.is_xing)
        self.flags = raw.flags
        self.frame_count = raw.frame_count
        self.byte_count = raw.byte_count
        self.toc = bytes(raw.toc)
        self.vbr_scale = raw.vbr_scale
        # the 9 stored bytes, NULs included, as Go's string(frame[pos:pos+9])
        self.lame_version = bytes(raw.lame_version[:9]).decode("latin-1") if raw.has_lame else ""
        self.encoder_delay = raw.encoder_delay
        self.encoder_padding = raw.encoder_padding

    def has_frame_count(self):
        return bool(self.flags & FLAG_FRAME_COUNT)

    def has_byte_count(self):
        return bool(self.flags & FLAG_BYTE_COUNT)

    def has_toc(self):
        return bool(self.flags & FLAG_TOC)

    def has_vbr_scale(self):
        return bool(self.flags & FLAG_VBR_SCALE)

    def has_lame_info(self):
        return self.lame_version != ""

    def total_delay(self):
        return lib().mp3g_lame_total_delay(C.byref(self._raw))

    def total_padding(self):
        return lib().mp3g_lame_total_padding(C.byref(self._raw))

    def trim(self, n_samples, tag_frame_samples=1152):
        """(first, count) of the samples to keep after gapless trimming (mp3g_lame_trim)."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().mp3g_lame_trim(C.byref(self._raw), n_samples, tag_frame_samples, C.byref(a), C.byref(b)))
        return a.value, b.value

    def toc_offset(self, percent, stream_bytes=0):
        """Byte offset of `percent` of the playback time from the Xing TOC; the
        tag's byte count, else `stream_bytes` (Mp3gError when neither is known)."""
        out = C.c_uint64()
        _check(lib().mp3g_lame_toc_offset(C.byref(self._raw), float(percent), int(stream_bytes), C.byref(out)))
        return out.value


def lame_parse(frame):
    """lameinfo.Parse: raises Mp3gError(ERR_NO_XING_HEADER) like ErrNoXingHeader."""
    raw = _LameInfo()
    b = bytes(frame)
    st = lib().mp3g_lame_parse(b, len(b), C.byref(raw))
    if st:
        raise Mp3gError(st, STATUS.get(st, ""))
    return LameInfo(raw)


def lame_parse_reader(data):
    """lameinfo.ParseFromReader on a reader over `data`: (LameInfo, bytes read);
    io.EOF / io.ErrUnexpectedEOF / ErrNoXingHeader raise Mp3gError(EOF /
    ERR_UNEXPECTED_EOF / ERR_NO_XING_HEADER)."""
    raw = _LameInfo()
    b = bytes(data)
    used = C.c_size_t()
    st = lib().mp3g_lame_parse_reader(b, len(b), C.byref(raw), C.byref(used))
    if st:
        raise Mp3gError(st, STATUS.get(st, ""))
    return LameInfo(raw), used.value


def decode_streams(datas, mode=MODE_EXACT, n_threads=0, device=0):
    """Bitstreams in, PCM out on the GPU (mp3g_decode_streams): scan on the host,
    Huffman + DSP on the device.  Returns (pcm int16[n, 576, 2], streams, end_status)."""
    bufs, ptrs, lens = _stream_args(datas)
    streams = np.zeros(len(datas), STREAM_DTYPE)
    status = np.zeros(max(1, len(datas)), np.int32)
    pcm, n = C.c_void_p(), C.c_uint64()
    _check(lib().mp3g_decode_streams(device, len(datas), ptrs, lens, n_threads, mode, C.byref(pcm), C.byref(n),
                                     _ptr(streams), _ptr(status)))
    k = n.value
    return _take(pcm, k, np.int16, (k, 576, 2)), streams, status[:len(datas)]


def _decode_scan(s, make_plan, d_out, out_format, mode, device, then=None):
    """The device side of the *_tensor calls, on the current torch stream: the
    scan's granules, jobs and main data uploaded, the main-data kernel into
    torch-owned coefficient rows, then the plan (make_plan()) into d_out and
    then(stream), if given.  Returns when the kernels are done (the plan and the
    input buffers, which the kernels read, are released then).  A scan without
    granules launches nothing."""
    import torch
    n = len(s["granules"])
    if not n:
        return
    dev = torch.device("cuda", device)
    d_g = torch.from_numpy(s["granules"].view(np.uint8)).to(dev)
    d_j = torch.from_numpy(s["jobs"].view(np.uint8)).to(dev)
    d_m = torch.from_numpy(s["main_data"]).to(dev)
    d_c = torch.empty(n * 1152, dtype=torch.int16, device=dev)
    plan = make_plan()
    st = torch.cuda.current_stream(dev)
    # (rows to count1: the one-wave plan kernels read no further)
    flags = (0 if mode & FLAG_KERNEL_V2 else HUFF_ROWS_COUNT1) | huffman_stage_flags(s["jobs"], n)
    huffman_execute(d_j, n, d_m, d_g, d_c, stream=st.cuda_stream, device=device, flags=flags)
    plan.execute(d_g, d_c, d_out, stream=st.cuda_stream, out_format=out_format)
    if then is not None:
        then(st)
    st.synchronize()
    plan.close()


def decode_streams_tensor(datas, mode=MODE_EXACT, out_format=OUT_F32_PLANAR, n_threads=0, device=0):
    """Bitstreams in, one device tensor out: the host scan, one upload, then the
    main-data kernel and the plan kernel on torch-owned buffers and the
    current torch stream -- no PCM comes back to the host.  Returns when the
    kernels are done (the plan and the input buffers are released then).

    Returns (out, views, streams, end_status).  out: a float32 (OUT_S16 /
    OUT_S16_MONO: int16) tensor of 1152 samples per granule (the mono formats:
    576) on cuda:device; views[k] is stream k's part of it, a slice --
    [2, T] for OUT_F32_PLANAR, [T, 2] for the interleaved formats, [T] for
    the mono formats, T = 576 * n_granules.  streams / end_status as
    decode_streams.  Whole streams, untrimmed: decode_windows_tensor decodes
    a crop of each stream (gapless=True: counted from the first sample
    LameInfo.trim keeps) straight into a dense batch."""
    import torch
    if not out_bytes_per_granule(out_format):
        raise Mp3gError(1, "unknown output format")
    s = scan_streams(datas, n_threads=n_threads)
    streams, n = s["streams"], len(s["granules"])
    dev = torch.device("cuda", device)
    per = 576 if out_format in _OUT_MONO else 1152  # samples per granule slot
    out = torch.empty(n * per, dtype=torch.int16 if out_format in _OUT_INT16 else torch.float32, device=dev)
    _decode_scan(s, lambda: Plan(streams, mode=mode, device=device), out, out_format, mode, device)
    if out_format == OUT_F32_PLANAR:
        views = planar_views(out, streams)
    elif out_format in _OUT_MONO:
        views = [out[int(f) * 576:(int(f) + int(k)) * 576]
                 for f, k in zip(streams["first_granule"], streams["n_granules"])]
    else:
        views = [out[int(f) * 1152:(int(f) + int(k)) * 1152].reshape(int(k) * 576, 2)
                 for f, k in zip(streams["first_granule"], streams["n_granules"])]
    return out, views, streams, s["end_status"]


def scan_windows(datas, starts, n_samples, gapless=False, n_threads=0):
    """Windowed host scan (mp3g_scan_windows): only the frames the window
    (starts[k], n_samples) of each stream needs.  Returns scan_streams' dict
    (the stream table describes each stream's decoded run) plus "rows"
    [WINDOW_ROW_DTYPE]: lead (granules decoded with PCM off), skip (samples of
    the window's first granule in front of it) and n_valid (samples the row
    receives).  gapless: a bool, or one per stream."""
    return _scan_windows(datas, starts, int(n_samples), gapless, n_threads)


def _scan_windows(datas, starts, lengths, gapless, n_threads=0):
    """scan_windows with a window length per stream (or one for all), as
    mp3g_scan_windows takes them."""
    B = len(datas)
    win = np.zeros(max(1, B), WINDOW_DTYPE)
    win["start"][:B] = np.asarray(starts, dtype=np.uint64)
    win["n_samples"][:B] = lengths
    win["flags"][:B] = np.where(np.broadcast_to(np.asarray(gapless, dtype=bool), (B,)), WINDOW_GAPLESS, 0)
    bufs, ptrs, lens = _stream_args(datas)
    h = C.c_void_p()
    t0 = time.perf_counter()
    _check(lib().mp3g_scan_windows(B, ptrs, lens, _ptr(win), n_threads, C.byref(h)))
    return _scan_result(h, B, time.perf_counter() - t0, rows=True)


def _check_window_format(out_format):
    if out_format not in (OUT_F32_PLANAR, OUT_F32_MONO):
        raise Mp3gError(8 if out_bytes_per_granule(out_format) else 1, "windowed output is OUT_F32_PLANAR or OUT_F32_MONO")


def decode_windows_tensor(datas, starts, n_samples, mode=MODE_EXACT, out_format=OUT_F32_PLANAR, gapless=False,
                          n_threads=0, device=0):
    """A crop of every stream, decoded straight into one dense batch tensor:
    row k holds samples [starts[k], starts[k] + lengths[k]) of stream k's full
    decode (gapless=True: counted from the first sample LameInfo.trim keeps,
    and capped by its count), zero-padded to n_samples.  Only the frames each
    window needs are scanned and decoded (scan_windows, WindowPlan); the
    samples are bit-identical to the same slice of decode_streams_tensor in
    the same mode and format.

    Returns (batch, lengths, end_status): batch a torch.zeros tensor
    [B, 2, n_samples] (OUT_F32_PLANAR) or [B, n_samples] (OUT_F32_MONO) on
    cuda:device, lengths int64[B], end_status as scan_windows (0 when the
    window was filled before the stream's end).  Runs on the current torch
    stream and returns when the kernels are done."""
    import torch
    _check_window_format(out_format)
    s = scan_windows(datas, starts, n_samples, gapless=gapless, n_threads=n_threads)
    B, T = len(datas), int(n_samples)
    dev = torch.device("cuda", device)
    batch = torch.zeros((B, 2, T) if out_format == OUT_F32_PLANAR else (B, T), dtype=torch.float32, device=dev)
    _decode_scan(s, lambda: WindowPlan(s["streams"], s["rows"], T, mode=mode, device=device), batch, out_format, mode,
                 device)
    return batch, s["rows"]["n_valid"].astype(np.int64), s["end_status"]


# ---- sample-rate conversion of decoded rows (include/mp3g.h) ----------------
# one row of Resampler.rows (mp3g_resample_row)
RESAMPLE_ROW_DTYPE = np.dtype([("out_start", "<u8"), ("src_origin", "<u8"), ("src_row", "<u4"), ("out_row", "<u4"),
                               ("n_src", "<u4"), ("n_out", "<u4")])
assert RESAMPLE_ROW_DTYPE.itemsize == 32
RESAMPLE_MAX_TAPS = 1 << 18
# the presets (resampy's kaiser_fast / kaiser_best): zeros, rolloff, beta
RESAMPLE_FAST = (16, 0.85, 8.555504641634386)
RESAMPLE_BEST = (64, 0.9475937167399596, 14.769656459379492)
RESAMPLE_QUALITY = {"fast": RESAMPLE_FAST, "best": RESAMPLE_BEST}


class Resampler:
    """Polyphase windowed-sinc resampler fi -> fo (mp3g_resampler_*): y[n] is
    ONE float32 FMA chain over 2 W taps in ascending order, so the device
    call (rows) equals the host reference (host) bit for bit.  device=None (or
    -1) makes a host-only object; fi == fo is a copy (W = 0, no taps)."""

    def __init__(self, fi, fo, zeros=RESAMPLE_FAST[0], rolloff=RESAMPLE_FAST[1], beta=RESAMPLE_FAST[2], device=None):
        self._h = C.c_void_p()
        self.device = -1 if device is None else int(device)
        self.fi, self.fo = int(fi), int(fo)
        _check(lib().mp3g_resampler_create(self.device, self.fi, self.fo, int(zeros), float(rolloff), float(beta),
                                           C.byref(self._h)))
        a, b, c, t, p = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_void_p()
        _check(lib().mp3g_resampler_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(p), C.byref(t)))
        self.L, self.M, self.W, self.tile = a.value, b.value, c.value, t.value
        n = self.L * 2 * self.W
        # a view of the library's table: valid while this object lives
        self.taps = (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,)).reshape(self.L, 2 * self.W)
                     if n else np.zeros((self.L, 0), np.float32))
        self._keep = None

    def out_len(self, n_src):
        """Samples of the resampled signal of n_src source samples: ceil(n L / M)."""
        return -((-int(n_src) * self.L) // self.M)

    def src_window(self, out_start, n_out):
        """The source samples [a, b) the outputs [out_start, out_start + n_out)
        read (a >= 0), n_out >= 1."""
        s, T = int(out_start), int(n_out)
        if self.W == 0:
            return s, s + T
        return max(0, s * self.M // self.L - self.W + 1), (s + T - 1) * self.M // self.L + self.W + 1

    def host(self, src, src_origin, out_start, n_out):
        """The reference on the CPU (mp3g_resample_host): outputs [out_start,
        out_start + n_out) of the signal whose samples [src_origin, src_origin
        + len(src)) are `src` (float32) and zero elsewhere."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        out = np.zeros(int(n_out), np.float32)
        _check(lib().mp3g_resample_host(self._h, _ptr(src) if len(src) else None, int(src_origin), len(src),
                                        int(out_start), int(n_out), _ptr(out) if n_out else None))
        return out

    def rows(self, d_src, d_out, rows, stream=None):
        """The device call (mp3g_resample_rows): d_src float32 [*, C, S] (or
        [*, S]) and d_out float32 [*, C, T] (or [*, T]) contiguous tensors on
        this resampler's device, C = 1 or 2; rows: RESAMPLE_ROW_DTYPE[n] (numpy:
        uploaded and kept until the next call; or a uint8 device tensor of n *
        32 bytes).  Writes the n_out samples of each row and plane, nothing
        else.  Asynchronous on `stream` (a hipStream_t; None = the current
        torch stream)."""
        import torch
        for t in (d_src, d_out):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() not in (2, 3) or not t.is_cuda:
                raise ValueError("Resampler.rows: contiguous float32 device tensors [*, C, S] or [*, S]")
        nch = d_out.shape[1] if d_out.dim() == 3 else 1
        if (d_src.shape[1] if d_src.dim() == 3 else 1) != nch:
            raise ValueError("Resampler.rows: source and output differ in channels")
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows, dtype=RESAMPLE_ROW_DTYPE)
            n = len(rows)
            if n and (int(rows["src_row"].max()) >= d_src.shape[0] or int(rows["out_row"].max()) >= d_out.shape[0]
                      or int(rows["n_src"].max()) > d_src.shape[-1] or int(rows["n_out"].max()) > d_out.shape[-1]):
                raise ValueError("Resampler.rows: a row lies outside the tensors")
            d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(d_out.device) if n else None
        else:
            d_rows, n = rows, rows.numel() // RESAMPLE_ROW_DTYPE.itemsize
        self._keep = d_rows
        if stream is None:
            stream = torch.cuda.current_stream(d_out.device).cuda_stream
        _check(lib().mp3g_resample_rows(self._h, C.c_void_p(d_src.data_ptr()), int(d_src.shape[-1]),
                                        C.c_void_p(d_out.data_ptr()), int(d_out.shape[-1]), int(nch),
                                        C.c_void_p(d_rows.data_ptr()) if n else None, n,
                                        C.c_void_p(stream) if stream else None))
        return d_rows

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.taps = None
            lib().mp3g_resampler_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- variable-ratio resampling of decoded rows (include/mp3g.h) -------------
# one row of VarResampler.rows (mp3g_varresample_row)
VARRESAMPLE_ROW_DTYPE = np.dtype([("out_start", "<u8"), ("src_origin", "<u8"), ("src_row", "<u4"), ("out_row", "<u4"),
                                  ("n_src", "<u4"), ("n_out", "<u4"), ("num", "<u4"), ("den", "<u4"),
                                  ("gain", "<f4"), ("reserved", "<u4")])
assert VARRESAMPLE_ROW_DTYPE.itemsize == 48


class VarResampler:
    """Windowed-sinc resampler whose ratio num / den (source samples per
    output sample) and gain belong to the row, not the object
    (mp3g_varresampler_*): speed and volume perturbation.  One prototype table
    of (F, D) pairs at 2^precision entries per zero crossing; y[n] is ONE
    float32 FMA chain over the row's taps in ascending source order, so the
    device call (rows, one launch whatever the ratios) equals the host
    reference (host) bit for bit.  device=None (or -1) makes a host-only
    object."""

    def __init__(self, zeros=RESAMPLE_FAST[0], rolloff=RESAMPLE_FAST[1], beta=RESAMPLE_FAST[2], precision=9,
                 device=None):
        self._h = C.c_void_p()
        self.device = -1 if device is None else int(device)
        _check(lib().mp3g_varresampler_create(self.device, int(zeros), float(rolloff), float(beta), int(precision),
                                              C.byref(self._h)))
        a, b, c, t, g, p = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_void_p()
        _check(lib().mp3g_varresampler_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(p), C.byref(t),
                                            C.byref(g)))
        self.zeros, self.P, self.Z, self.R, self.tile, self.stage = int(zeros), a.value, b.value, c.value, t.value, g.value
        # a view of the library's table [Z + 1, 2] of (F, D): valid while this object lives
        self.table = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(2 * (self.Z + 1),)).reshape(-1, 2)
        self._keep = None

    @staticmethod
    def ratio(fi, fo, speed=1):
        """Reduced (num, den) with num / den = speed fi / fo.  speed: an int, a
        Fraction, a (p, q) pair, or a float taken through
        Fraction(speed).limit_denominator(10000)."""
        from fractions import Fraction
        if isinstance(speed, tuple):
            sp = Fraction(int(speed[0]), int(speed[1]))
        elif isinstance(speed, (int, Fraction, np.integer)):
            sp = Fraction(speed)
        else:
            sp = Fraction(float(speed)).limit_denominator(10000)
        if sp <= 0 or int(fi) <= 0 or int(fo) <= 0:
            raise Mp3gError(1, "speed and rates must be positive")
        f = sp * Fraction(int(fi), int(fo))
        if f.numerator >= 1 << 31 or f.denominator >= 1 << 31:
            raise Mp3gError(1, "ratio beyond 2^31")
        return f.numerator, f.denominator

    def step(self, num, den):
        """The row's table step I (cutoff c = I / 2^P): R, or floor(R den / num)."""
        return self.R if num <= den else self.R * int(den) // int(num)

    def half_width(self, num, den):
        """Wr = ceil(Z / I): the row's half width in source samples (0: a copy)."""
        if num == den:
            return 0
        i = self.step(num, den)
        if i == 0:
            raise Mp3gError(1, "ratio beyond the table's resolution")
        return -(-self.Z // i)

    @staticmethod
    def out_len(n_src, num, den):
        """Samples of the resampled signal of n_src source samples: ceil(n den / num)."""
        return -((-int(n_src) * int(den)) // int(num))

    def src_window(self, out_start, n_out, num, den):
        """The source samples [a, b) the outputs [out_start, out_start + n_out)
        read (a >= 0), n_out >= 1."""
        s, T, w = int(out_start), int(n_out), self.half_width(num, den)
        if w == 0:
            return s, s + T
        return max(0, s * num // den - w + 1), (s + T - 1) * num // den + w + 1

    def host(self, src, src_origin, out_start, n_out, num, den, gain=1.0):
        """The reference on the CPU (mp3g_varresample_host): outputs [out_start,
        out_start + n_out) of the signal whose samples [src_origin, src_origin
        + len(src)) are `src` (float32) and zero elsewhere, at num / den source
        samples per output, times gain."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        out = np.zeros(int(n_out), np.float32)
        if not (0 <= int(num) < 1 << 32 and 0 <= int(den) < 1 << 32):
            raise Mp3gError(1, "num and den in [1, 2^31)")
        _check(lib().mp3g_varresample_host(self._h, _ptr(src) if len(src) else None, int(src_origin), len(src),
                                           int(out_start), int(n_out), _ptr(out) if n_out else None, int(num),
                                           int(den), float(gain)))
        return out

    def rows(self, d_src, d_out, rows, stream=None):
        """The device call (mp3g_varresample_rows): tensors as Resampler.rows;
        rows: VARRESAMPLE_ROW_DTYPE[n] (numpy: checked -- a row outside the
        tensors, with num or den outside [1, 2^31) or with a ratio beyond the
        table's resolution is refused -- uploaded and kept until the next
        call; or a uint8 device tensor of n * 48 bytes, taken as it is).  ONE
        launch for all rows.  Asynchronous on `stream` (a hipStream_t; None =
        the current torch stream)."""
        import torch
        for t in (d_src, d_out):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() not in (2, 3) or not t.is_cuda:
                raise ValueError("VarResampler.rows: contiguous float32 device tensors [*, C, S] or [*, S]")
        nch = d_out.shape[1] if d_out.dim() == 3 else 1
        if (d_src.shape[1] if d_src.dim() == 3 else 1) != nch:
            raise ValueError("VarResampler.rows: source and output differ in channels")
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows, dtype=VARRESAMPLE_ROW_DTYPE)
            n = len(rows)
            if n and (int(rows["src_row"].max()) >= d_src.shape[0] or int(rows["out_row"].max()) >= d_out.shape[0]
                      or int(rows["n_src"].max()) > d_src.shape[-1] or int(rows["n_out"].max()) > d_out.shape[-1]):
                raise ValueError("VarResampler.rows: a row lies outside the tensors")
            if n:
                num, den = rows["num"].astype(np.uint64), rows["den"].astype(np.uint64)
                if (int(num.min()) < 1 or int(den.min()) < 1 or int(num.max()) >= 1 << 31 or int(den.max()) >= 1 << 31
                        or bool((num > np.uint64(self.R) * den).any())):
                    raise Mp3gError(1, "VarResampler.rows: num or den outside [1, 2^31), or a ratio beyond the "
                                       "table's resolution")
            d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(d_out.device) if n else None
        else:
            d_rows, n = rows, rows.numel() // VARRESAMPLE_ROW_DTYPE.itemsize
        self._keep = d_rows
        if stream is None:
            stream = torch.cuda.current_stream(d_out.device).cuda_stream
        _check(lib().mp3g_varresample_rows(self._h, C.c_void_p(d_src.data_ptr()), int(d_src.shape[-1]),
                                           C.c_void_p(d_out.data_ptr()), int(d_out.shape[-1]), int(nch),
                                           C.c_void_p(d_rows.data_ptr()) if n else None, n,
                                           C.c_void_p(stream) if stream else None))
        return d_rows

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.table = None
            lib().mp3g_varresampler_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_rates(datas, n_threads=0, channels=False):
    """The sample rate of each stream's first valid frame (mp3g_stream_rates; 0:
    no valid frame) as int32[B]; channels=True: (rates, channel counts)."""
    bufs, ptrs, lens = _stream_args(datas)
    rates = np.zeros(max(1, len(datas)), np.int32)
    nch = np.zeros(max(1, len(datas)), np.int32)
    _check(lib().mp3g_stream_rates(len(datas), ptrs, lens, n_threads, _ptr(rates), _ptr(nch)))
    return (rates[:len(datas)], nch[:len(datas)]) if channels else rates[:len(datas)]


def decode_windows_resampled_tensor(datas, starts, n_samples, rate, mode=MODE_EXACT, out_format=OUT_F32_PLANAR,
                                    gapless=False, quality="fast", n_threads=0, device=0, speed=None, gain=None):
    """decode_windows_tensor at ONE sample rate: starts[k] and n_samples count
    samples at `rate`, and row k holds y_k[starts[k], starts[k] + lengths[k]),
    zero-padded to n_samples, where y_k is the resample (Resampler, preset
    `quality`: "fast" or "best", or a (zeros, rolloff, beta) tuple) of what the
    windowed decode exposes as stream k -- its full decode, or with gapless the
    trimmed one -- at the rate of its first valid frame (stream_rates).  A
    stream already at `rate` is copied.  lengths[k] = ceil(N_k L / M) -
    starts[k] clamped to [0, n_samples], N_k the stream's samples.

    One windowed decode of all streams into an intermediate [B, C, T_src]
    tensor (each stream's source window: Resampler.src_window), then one
    Resampler.rows launch per distinct source rate; every sample equals
    Resampler.host on the same slice of the full decode bit for bit.

    Returns (batch, lengths, end_status, rates): batch [B, 2, n_samples]
    (OUT_F32_PLANAR) or [B, n_samples] (OUT_F32_MONO) on cuda:device, lengths
    int64[B], end_status of the windowed scan, rates int32[B] (0: no valid
    frame, an all-zero row).

    speed, gain: speed and volume perturbation, one entry per stream each
    (speed as VarResampler.ratio takes it; None for either: 1 for every
    stream).  With both None this is the polyphase path above.  Otherwise
    stream k is played speed[k] times faster -- num / den = speed[k] fi / rate
    source samples per output sample -- and scaled by gain[k]; starts and
    n_samples count samples of the perturbed signal, lengths[k] = ceil(N_k den
    / num) - starts[k] clamped to [0, n_samples], and every row goes through
    ONE VarResampler.rows launch behind the windowed decode: every sample
    equals VarResampler.host on the same slice of the full decode bit for
    bit."""
    import torch
    _check_window_format(out_format)
    if int(rate) <= 0:
        raise Mp3gError(1, "rate not positive")
    zeros, rolloff, beta = RESAMPLE_QUALITY[quality] if isinstance(quality, str) else quality
    B, T = len(datas), int(n_samples)
    starts = [int(s) for s in starts]
    if len(starts) != B or T < 0 or any(s < 0 for s in starts):
        raise ValueError("decode_windows_resampled_tensor: one start >= 0 per stream")
    if speed is not None or gain is not None:
        return _decode_windows_perturbed(datas, starts, T, int(rate), mode, out_format, gapless,
                                         (zeros, rolloff, beta), n_threads, device, speed, gain)
    rates = stream_rates(datas, n_threads=n_threads)
    rs = {int(f): Resampler(int(f), int(rate), zeros, rolloff, beta, device=device) for f in set(rates.tolist()) if f}
    dev = torch.device("cuda", device)
    planar = out_format == OUT_F32_PLANAR
    batch = torch.zeros((B, 2, T) if planar else (B, T), dtype=torch.float32, device=dev)
    lengths = np.zeros(B, np.int64)
    # each stream's source window [src0, src0 + src_n) (none: no valid frame)
    src0, src_n = np.zeros(B, np.uint64), np.zeros(B, np.uint64)
    for k in range(B):
        if rates[k] and T:
            a, b = rs[int(rates[k])].src_window(starts[k], T)
            if b - a > (1 << 26):
                raise Mp3gError(1, "source window of more than MP3G_WINDOW_MAX_SAMPLES samples")
            src0[k], src_n[k] = a, b - a
    s = _scan_windows(datas, src0, src_n, gapless, n_threads)
    T_src = int(src_n.max()) if B else 0
    inter = (torch.zeros((B, 2, T_src) if planar else (B, T_src), dtype=torch.float32, device=dev)
             if len(s["granules"]) else None)

    def resample(st):  # one launch per source rate, behind the windowed decode
        n_valid = s["rows"]["n_valid"].astype(np.int64)
        for f, r in rs.items():
            ks = [k for k in range(B) if rates[k] == f and n_valid[k] > 0]
            rows = np.zeros(len(ks), RESAMPLE_ROW_DTYPE)
            for i, k in enumerate(ks):
                a, want = int(src0[k]), int(src_n[k])
                # fewer samples than asked for: the stream ends at N = a + n_valid
                ln = T if n_valid[k] >= want else min(T, max(0, r.out_len(a + int(n_valid[k])) - starts[k]))
                lengths[k] = ln
                rows[i] = (starts[k], a, k, k, int(n_valid[k]), ln)
            rows = rows[rows["n_out"] > 0]
            if len(rows):
                r.rows(inter, batch, rows, stream=st.cuda_stream)

    _decode_scan(s, lambda: WindowPlan(s["streams"], s["rows"], T_src, mode=mode, device=device), inter, out_format,
                 mode, device, then=resample)
    for r in rs.values():
        r.close()
    return batch, lengths, s["end_status"], rates


def _decode_windows_perturbed(datas, starts, T, rate, mode, out_format, gapless, quality, n_threads, device, speed,
                              gain):
    """decode_windows_resampled_tensor with a speed and a gain per stream: the
    windowed decode of each stream's source window, then one VarResampler.rows
    launch for all rows."""
    import torch
    B = len(datas)
    speed = [1] * B if speed is None else list(speed)
    gain = [1.0] * B if gain is None else [float(g) for g in gain]
    if len(speed) != B or len(gain) != B:
        raise ValueError("decode_windows_resampled_tensor: one speed and one gain per stream")
    rates = stream_rates(datas, n_threads=n_threads)
    vr = VarResampler(*quality, device=device)
    try:
        dev = torch.device("cuda", device)
        planar = out_format == OUT_F32_PLANAR
        batch = torch.zeros((B, 2, T) if planar else (B, T), dtype=torch.float32, device=dev)
        lengths = np.zeros(B, np.int64)
        ratio = [vr.ratio(int(rates[k]), rate, speed[k]) if rates[k] else (1, 1) for k in range(B)]
        # each stream's source window [src0, src0 + src_n) (none: no valid frame)
        src0, src_n = np.zeros(B, np.uint64), np.zeros(B, np.uint64)
        for k in range(B):
            if rates[k] and T:
                a, b = vr.src_window(starts[k], T, *ratio[k])
                if b - a > (1 << 26):
                    raise Mp3gError(1, "source window of more than MP3G_WINDOW_MAX_SAMPLES samples")
                src0[k], src_n[k] = a, b - a
        s = _scan_windows(datas, src0, src_n, gapless, n_threads)
        T_src = int(src_n.max()) if B else 0
        inter = (torch.zeros((B, 2, T_src) if planar else (B, T_src), dtype=torch.float32, device=dev)
                 if len(s["granules"]) else None)

        def resample(st):  # one launch for every row, behind the windowed decode
            n_valid = s["rows"]["n_valid"].astype(np.int64)
            ks = [k for k in range(B) if rates[k] and n_valid[k] > 0]
            rows = np.zeros(len(ks), VARRESAMPLE_ROW_DTYPE)
            for i, k in enumerate(ks):
                a, want = int(src0[k]), int(src_n[k])
                # fewer samples than asked for: the stream ends at N = a + n_valid
                ln = T if n_valid[k] >= want else min(T, max(0, vr.out_len(a + int(n_valid[k]), *ratio[k])
                                                             - starts[k]))
                lengths[k] = ln
                rows[i] = (starts[k], a, k, k, int(n_valid[k]), ln, ratio[k][0], ratio[k][1], gain[k], 0)
            rows = rows[rows["n_out"] > 0]
            if len(rows):
                vr.rows(inter, batch, rows, stream=st.cuda_stream)

        _decode_scan(s, lambda: WindowPlan(s["streams"], s["rows"], T_src, mode=mode, device=device), inter,
                     out_format, mode, device, then=resample)
    finally:
        vr.close()
    return batch, lengths, s["end_status"], rates


# ---- log-mel features of decoded rows (include/mp3g.h) ----------------------
LOGMEL_CENTER = 1
LOGMEL_CLAMP = 2


def log10f(x):
    """mp3g_log10f of every element of x (float32; normal, positive, finite):
    the features' logarithm, for tests."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    lib().mp3g_logmel_log10f(_ptr(x), x.size, _ptr(y))
    return y


class LogMel:
    """Log-mel features of float32 rows (mp3g_logmel_*): a Hann-windowed STFT
    power spectrum by direct DFT, Slaney's mel filter bank, log10 of the power
    floored at 1e-10 and, with clamp, Whisper's (max(y, max y - 8) + 4) / 4.
    Every sum is ONE float32 FMA chain in ascending order, so the device call
    (execute) equals the host reference (host) bit for bit.  device=None (or
    -1) makes a host-only object; fmax=0 means rate / 2."""

    def __init__(self, rate=16000, n_fft=400, hop=160, n_mels=80, fmin=0.0, fmax=0.0, center=True, clamp=True,
                 device=None):
        self._h = C.c_void_p()
        self.device = -1 if device is None else int(device)
        self.rate, self.n_fft, self.hop, self.n_mels = int(rate), int(n_fft), int(hop), int(n_mels)
        self.center, self.clamp = bool(center), bool(clamp)
        self.flags = (LOGMEL_CENTER if center else 0) | (LOGMEL_CLAMP if clamp else 0)
        _check(lib().mp3g_logmel_create(self.device, self.rate, self.n_fft, self.hop, self.n_mels, float(fmin),
                                        float(fmax), self.flags, C.byref(self._h)))
        k, t = C.c_uint32(), C.c_uint32()
        p = [C.c_void_p() for _ in range(4)]
        _check(lib().mp3g_logmel_info(self._h, C.byref(k), *[C.byref(q) for q in p], C.byref(t)))
        self.K, self.tile_frames = k.value, t.value
        self.pad = self.n_fft // 2 if center else 0

        def view(q, ctype, shape):  # a view of the library's table: valid while this object lives
            return np.ctypeslib.as_array(C.cast(q, C.POINTER(ctype)), shape=shape)
        self.cw = view(p[0], C.c_float, (self.K, self.n_fft))
        self.sw = view(p[1], C.c_float, (self.K, self.n_fft))
        self.wm = view(p[2], C.c_float, (self.n_mels, self.K))
        self.support = view(p[3], C.c_uint32, (self.n_mels, 2))

    def frames(self, T):
        """The frames a row of T samples has (mp3g_logmel_frames)."""
        return int(lib().mp3g_logmel_frames(self._h, int(T)))

    def host(self, x, n_frames=None, frame_stride=None):
        """The reference on the CPU (mp3g_logmel_host): features [n_mels,
        n_frames] of the float32 row x (n_frames: all by default); with a
        frame_stride the full [n_mels, frame_stride] buffer, zeros where
        nothing is written."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.frames(len(x)) if n_frames is None else int(n_frames)
        stride = n if frame_stride is None else int(frame_stride)
        out = np.zeros((self.n_mels, max(stride, 0)), np.float32)
        _check(lib().mp3g_logmel_host(self._h, _ptr(x) if len(x) else None, len(x), n, _ptr(out) if out.size else None,
                                      stride))
        return out

    def execute(self, d_src, d_out=None, n_frames=None, stream=None):
        """The device call (mp3g_logmel_execute): d_src float32 [B, C, T] (C = 1
        or 2) or [B, T], contiguous on this object's device; d_out float32
        [B, C, n_mels, S] or [B, n_mels, S] with S >= n_frames (made here when
        None: S = n_frames, all frames by default).  Writes the n_frames
        features of each mel row, nothing else.  Asynchronous on `stream` (a
        hipStream_t; None = the current torch stream).  Returns d_out."""
        import torch
        if d_src.dtype != torch.float32 or not d_src.is_contiguous() or d_src.dim() not in (2, 3) or not d_src.is_cuda:
            raise ValueError("LogMel.execute: a contiguous float32 device tensor [B, C, T] or [B, T]")
        B, T = int(d_src.shape[0]), int(d_src.shape[-1])
        planes = int(d_src.shape[1]) if d_src.dim() == 3 else 1
        n = self.frames(T) if n_frames is None else int(n_frames)
        lead = (B, planes) if d_src.dim() == 3 else (B,)
        if d_out is None:
            d_out = torch.empty(lead + (self.n_mels, n), dtype=torch.float32, device=d_src.device)
        if (d_out.dtype != torch.float32 or not d_out.is_contiguous() or not d_out.is_cuda
                or tuple(d_out.shape[:-1]) != lead + (self.n_mels,)):
            raise ValueError("LogMel.execute: d_out is a contiguous float32 device tensor [B, (C,) n_mels, S]")
        if stream is None:
            stream = torch.cuda.current_stream(d_src.device).cuda_stream
        _check(lib().mp3g_logmel_execute(self._h, C.c_void_p(d_src.data_ptr()) if d_src.numel() else None, B, planes, T,
                                         C.c_void_p(d_out.data_ptr()) if d_out.numel() else None, n,
                                         int(d_out.shape[-1]), C.c_void_p(stream) if stream else None))
        return d_out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.cw = self.sw = self.wm = self.support = None
            lib().mp3g_logmel_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_windows_logmel_tensor(datas, starts, n_samples, rate=16000, n_fft=400, hop=160, n_mels=80, clamp=True,
                                 center=True, fmin=0.0, fmax=0.0, n_frames=None, mode=MODE_EXACT,
                                 out_format=OUT_F32_MONO, gapless=False, quality="fast", n_threads=0, device=0,
                                 speed=None, gain=None, spec_augment=None):
    """decode_windows_resampled_tensor followed by LogMel.execute on the same
    torch stream: the log-mel features of each stream's window [starts[k],
    starts[k] + n_samples) at `rate`, zero padding included.  F = n_frames, by
    default n_samples // hop with center (Whisper's count, which drops the last
    frame) and every frame without.

    Returns (features, frame_lengths, end_status, rates): features [B, n_mels,
    F] (OUT_F32_MONO) or [B, 2, n_mels, F] (OUT_F32_PLANAR) on cuda:device,
    equal to LogMel.host on the rows of decode_windows_resampled_tensor bit for
    bit; frame_lengths int64[B] = min(F, ceil(lengths / hop)), the frames that
    start inside each stream's valid samples.

    speed, gain: speed and volume perturbation before everything else, one
    entry per stream each (decode_windows_resampled_tensor); starts and
    n_samples then count samples of the perturbed signal.

    spec_augment: None, or SpecAugment of the features in the frequency-major
    layout (spec_augment with freq_major=True) on the same stream: a
    descriptor array [B], or a dict of spec_augment_rows' options plus `rng`
    and `fill`, whose rows are drawn from the returned frame_lengths."""
    import torch
    lm = LogMel(rate, n_fft, hop, n_mels, fmin, fmax, center=center, clamp=clamp, device=device)
    try:
        T = int(n_samples)
        avail = lm.frames(T)
        F = (min(avail, T // lm.hop) if center else avail) if n_frames is None else int(n_frames)
        if F < 0 or F > avail:
            raise Mp3gError(1, "more frames than a row of n_samples has")
        batch, lengths, end_status, rates = decode_windows_resampled_tensor(
            datas, starts, T, rate, mode=mode, out_format=out_format, gapless=gapless, quality=quality,
            n_threads=n_threads, device=device, speed=speed, gain=gain)
        feats = lm.execute(batch, n_frames=F)
        flen = np.minimum(F, -(-lengths // lm.hop))
        if spec_augment is not None:
            feats = _specaug_after("decode_windows_logmel_tensor", feats, flen, spec_augment, lm.n_mels, True)
        torch.cuda.current_stream(feats.device).synchronize()
    finally:
        lm.close()
    return feats, flen, end_status, rates


# ---- Kaldi filter-bank features of decoded rows (include/mp3g.h) -------------
FBANK_REMOVE_DC = 1
FBANK_SNIP_EDGES = 2
FBANK_WINDOWS = {"povey": 0, "hamming": 1, "hanning": 2, "rectangular": 3}


def logf(x):
    """mp3g_logf of every element of x (float32; normal, positive, finite):
    the filter-bank features' natural logarithm, for tests."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    lib().mp3g_fbank_logf(_ptr(x), x.size, _ptr(y))
    return y


class FBank:
    """Kaldi's log mel filter-bank features of float32 rows (mp3g_fbank_*; what
    compute-fbank-feats and torchaudio.compliance.kaldi.fbank compute, without
    dither, energy, VTLN and subtract_mean): per frame DC removal and
    pre-emphasis, the window, the power spectrum of the frame zero-padded to
    P = the next power of two, Kaldi's mel triangles and the natural logarithm
    floored at float32 epsilon, time-major.  Samples are multiplied by `scale`
    first (Kaldi models read int16-range samples).  Every sum is ONE float32
    FMA chain in ascending order, so the device call (execute) equals the host
    reference (host) bit for bit.  device=None (or -1) makes a host-only
    object; high_freq <= 0 means rate / 2 + high_freq."""

    def __init__(self, rate=16000, frame_length_ms=25.0, frame_shift_ms=10.0, n_mels=80, low_freq=20.0, high_freq=0.0,
                 preemphasis=0.97, remove_dc=True, window="povey", snip_edges=True, scale=32768.0, device=None):
        self._h = C.c_void_p()
        if window not in FBANK_WINDOWS:
            raise Mp3gError(1, "FBank: window is one of " + ", ".join(FBANK_WINDOWS))
        self.device = -1 if device is None else int(device)
        self.rate, self.n_mels = int(rate), int(n_mels)
        # Kaldi's conversion of the durations to samples
        self.N, self.hop = int(self.rate * 0.001 * frame_length_ms), int(self.rate * 0.001 * frame_shift_ms)
        self.preemphasis, self.scale, self.window = float(preemphasis), float(scale), window
        self.remove_dc, self.snip_edges = bool(remove_dc), bool(snip_edges)
        self.flags = (FBANK_REMOVE_DC if remove_dc else 0) | (FBANK_SNIP_EDGES if snip_edges else 0)
        _check(lib().mp3g_fbank_create(self.device, self.rate, self.N, self.hop, self.n_mels, float(low_freq),
                                       float(high_freq), self.preemphasis, self.scale, FBANK_WINDOWS[window],
                                       self.flags, C.byref(self._h)))
        pp, k, t = C.c_uint32(), C.c_uint32(), C.c_uint32()
        p = [C.c_void_p() for _ in range(5)]
        _check(lib().mp3g_fbank_info(self._h, C.byref(pp), C.byref(k), *[C.byref(q) for q in p], C.byref(t)))
        self.P, self.K, self.tile_frames = pp.value, k.value, t.value

        def view(q, ctype, shape):  # a view of the library's table: valid while this object lives
            return np.ctypeslib.as_array(C.cast(q, C.POINTER(ctype)), shape=shape)
        self.cw = view(p[0], C.c_float, (self.K, self.N))
        self.sw = view(p[1], C.c_float, (self.K, self.N))
        self.wm = view(p[2], C.c_float, (self.n_mels, self.K))
        self.support = view(p[3], C.c_uint32, (self.n_mels, 2))
        self.w = view(p[4], C.c_float, (self.N,))

    def frames(self, T):
        """The frames a row of T samples has (mp3g_fbank_frames)."""
        return int(lib().mp3g_fbank_frames(self._h, int(T)))

    def host(self, x, n_frames=None, mel_stride=None):
        """The reference on the CPU (mp3g_fbank_host): features [n_frames,
        n_mels] of the float32 row x (n_frames: all by default); with a
        mel_stride the full [n_frames, mel_stride] buffer, zeros where nothing
        is written."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.frames(len(x)) if n_frames is None else int(n_frames)
        stride = self.n_mels if mel_stride is None else int(mel_stride)
        out = np.zeros((max(n, 0), max(stride, 0)), np.float32)
        _check(lib().mp3g_fbank_host(self._h, _ptr(x) if len(x) else None, len(x), n, _ptr(out) if out.size else None,
                                     stride))
        return out

    def execute(self, d_src, d_out=None, stream=None):
        """The device call (mp3g_fbank_execute): d_src float32 [B, C, T] (C = 1
        or 2) or [B, T], contiguous on this object's device; d_out float32
        [B, C, F, S] or [B, F, S] with F <= frames(T) and S >= n_mels (made here
        when None: every frame, S = n_mels).  Writes the n_mels features of each
        of the F frames, nothing else.  One launch, asynchronous on `stream` (a
        hipStream_t; None = the current torch stream).  Returns d_out."""
        import torch
        if d_src.dtype != torch.float32 or not d_src.is_contiguous() or d_src.dim() not in (2, 3) or not d_src.is_cuda:
            raise ValueError("FBank.execute: a contiguous float32 device tensor [B, C, T] or [B, T]")
        B, T = int(d_src.shape[0]), int(d_src.shape[-1])
        planes = int(d_src.shape[1]) if d_src.dim() == 3 else 1
        lead = (B, planes) if d_src.dim() == 3 else (B,)
        if d_out is None:
            d_out = torch.empty(lead + (self.frames(T), self.n_mels), dtype=torch.float32, device=d_src.device)
        if (d_out.dtype != torch.float32 or not d_out.is_contiguous() or not d_out.is_cuda
                or d_out.dim() != len(lead) + 2 or tuple(d_out.shape[:-2]) != lead):
            raise ValueError("FBank.execute: d_out is a contiguous float32 device tensor [B, (C,) F, S]")
        if stream is None:
            stream = torch.cuda.current_stream(d_src.device).cuda_stream
        _check(lib().mp3g_fbank_execute(self._h, C.c_void_p(d_src.data_ptr()) if d_src.numel() else None, B, planes, T,
                                        C.c_void_p(d_out.data_ptr()) if d_out.numel() else None,
                                        int(d_out.shape[-2]), int(d_out.shape[-1]), C.c_void_p(stream) if stream else None))
        return d_out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.cw = self.sw = self.wm = self.support = self.w = None
            lib().mp3g_fbank_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_windows_fbank_tensor(datas, starts, n_samples, rate=16000, frame_length_ms=25.0, frame_shift_ms=10.0,
                                n_mels=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97, remove_dc=True,
                                window="povey", snip_edges=True, scale=32768.0, n_frames=None, mode=MODE_EXACT,
                                out_format=OUT_F32_MONO, gapless=False, quality="fast", n_threads=0, device=0,
                                speed=None, gain=None, cmvn=None, spec_augment=None, deltas=None, stack=None):
    """decode_windows_resampled_tensor followed by FBank.execute on the same
    torch stream: Kaldi's filter-bank features of each stream's window
    [starts[k], starts[k] + n_samples) at `rate`, zero padding included.
    F = n_frames, by default every frame a row of n_samples has.

    Returns (features, frame_lengths, end_status, rates): features [B, F,
    n_mels] (OUT_F32_MONO) or [B, 2, F, n_mels] (OUT_F32_PLANAR) on cuda:device,
    equal to FBank.host on the rows of decode_windows_resampled_tensor bit for
    bit; frame_lengths int64[B], the frames that lie wholly inside each stream's
    valid samples: clamp((len - N) // hop + 1, 0, F) with snip_edges, else
    min(F, (len + hop // 2) // hop).  A frameless stream's rows are all
    logf(2^-23).

    speed, gain: speed and volume perturbation before everything else, one
    entry per stream each (decode_windows_resampled_tensor); starts and
    n_samples then count samples of the perturbed signal.

    cmvn: None, "mean" or "mean_var": the per-row normalisation of
    decode_windows_mfcc_tensor (cmvn) over each stream's frame_lengths frames,
    in place on the same stream.  spec_augment: None, or SpecAugment of the
    (normalised) features (spec_augment, time-major) on the same stream: a
    descriptor array [B], or a dict of spec_augment_rows' options plus `rng`
    and `fill`, whose rows are drawn from the returned frame_lengths.  The
    recipes normalise before they mask: a fill of 0 is then the mean.

    deltas: None or dict(order=, window=): add_deltas of the result, n_mels *
    (order + 1) columns.  stack: None or dict(left=, right=, step=, first=)
    (lfr_options(7, 6) is the Paraformer front end): stack_frames after that;
    the features then have stack_frames_count(F, step, first) frames and the
    returned frame_lengths are the stacked counts.  Both on the same stream."""
    import torch
    if cmvn not in CMVN_MODES:
        raise Mp3gError(1, "decode_windows_fbank_tensor: cmvn is None, 'mean' or 'mean_var'")
    _framectx_options("decode_windows_fbank_tensor", deltas, stack)
    fb = FBank(rate, frame_length_ms, frame_shift_ms, n_mels, low_freq, high_freq, preemphasis, remove_dc, window,
               snip_edges, scale, device=device)
    try:
        T = int(n_samples)
        avail = fb.frames(T)
        F = avail if n_frames is None else int(n_frames)
        if F < 0 or F > avail:
            raise Mp3gError(1, "more frames than a row of n_samples has")
        batch, lengths, end_status, rates = decode_windows_resampled_tensor(
            datas, starts, T, rate, mode=mode, out_format=out_format, gapless=gapless, quality=quality,
            n_threads=n_threads, device=device, speed=speed, gain=gain)
        feats = torch.empty(tuple(batch.shape[:-1]) + (F, fb.n_mels), dtype=torch.float32, device=batch.device)
        fb.execute(batch, feats)
        if snip_edges:
            flen = np.clip((lengths - fb.N) // fb.hop + 1, 0, F)
        else:
            flen = np.minimum(F, (lengths + fb.hop // 2) // fb.hop)
        if CMVN_MODES[cmvn] is not None:
            _cmvn_rows(feats, flen, norm_vars=CMVN_MODES[cmvn])
        if spec_augment is not None:
            feats = _specaug_after("decode_windows_fbank_tensor", feats, flen, spec_augment, fb.n_mels, False)
        if deltas is not None or stack is not None:
            feats, flen = _framectx_after(feats, flen, deltas, stack)
        torch.cuda.current_stream(feats.device).synchronize()
    finally:
        fb.close()
    return feats, flen, end_status, rates


# ---- Kaldi MFCC features of decoded rows, per-row normalisation (include/mp3g.h) --
MFCC_USE_ENERGY = 4
MFCC_RAW_ENERGY = 8
CMVN_NORM_VARS = 1
CMVN_MODES = {None: None, "mean": False, "mean_var": True}


class MFCC:
    """Kaldi's MFCC features of float32 rows (mp3g_mfcc_*; what
    compute-mfcc-feats and torchaudio.compliance.kaldi.mfcc compute, without
    dither, VTLN and htk_compat): FBank's log mel energies through Kaldi's DCT
    matrix cut to n_ceps rows and the cepstral lifter, time-major; with
    use_energy coefficient 0 is the frame's log energy -- raw_energy: after DC
    removal, before pre-emphasis and window; else after the window -- floored at
    log(energy_floor) when that is positive.  Every sum is ONE float32 FMA chain
    in ascending order, so the device call (execute) equals the host reference
    (host) bit for bit.  The object owns an FBank-equivalent front end whose
    tables are the views cw, sw, wm, support and w; dct [n_ceps, n_mels] and
    lifter [n_ceps] are its own.  device=None (or -1) makes a host-only
    object."""

    def __init__(self, rate=16000, frame_length_ms=25.0, frame_shift_ms=10.0, n_mels=23, n_ceps=13,
                 cepstral_lifter=22.0, use_energy=True, raw_energy=True, energy_floor=0.0, low_freq=20.0,
                 high_freq=0.0, preemphasis=0.97, remove_dc=True, window="povey", snip_edges=True, scale=32768.0,
                 device=None):
        self._h = C.c_void_p()
        if window not in FBANK_WINDOWS:
            raise Mp3gError(1, "MFCC: window is one of " + ", ".join(FBANK_WINDOWS))
        self.device = -1 if device is None else int(device)
        self.rate, self.n_mels, self.n_ceps = int(rate), int(n_mels), int(n_ceps)
        # Kaldi's conversion of the durations to samples
        self.N, self.hop = int(self.rate * 0.001 * frame_length_ms), int(self.rate * 0.001 * frame_shift_ms)
        self.preemphasis, self.scale, self.window = float(preemphasis), float(scale), window
        self.cepstral_lifter, self.energy_floor = float(cepstral_lifter), float(energy_floor)
        self.remove_dc, self.snip_edges = bool(remove_dc), bool(snip_edges)
        self.use_energy, self.raw_energy = bool(use_energy), bool(raw_energy)
        self.flags = ((FBANK_REMOVE_DC if remove_dc else 0) | (FBANK_SNIP_EDGES if snip_edges else 0)
                      | (MFCC_USE_ENERGY if use_energy else 0) | (MFCC_RAW_ENERGY if raw_energy else 0))
        _check(lib().mp3g_mfcc_create(self.device, self.rate, self.N, self.hop, self.n_mels, self.n_ceps,
                                      float(low_freq), float(high_freq), self.preemphasis, self.scale,
                                      self.cepstral_lifter, self.energy_floor, FBANK_WINDOWS[window], self.flags,
                                      C.byref(self._h)))
        fb, nc, lef, in_lds = C.c_void_p(), C.c_uint32(), C.c_float(), C.c_uint32()
        d, lf = C.c_void_p(), C.c_void_p()
        _check(lib().mp3g_mfcc_info(self._h, C.byref(fb), C.byref(nc), C.byref(d), C.byref(lf), C.byref(lef),
                                    C.byref(in_lds)))
        pp, k, t = C.c_uint32(), C.c_uint32(), C.c_uint32()
        p = [C.c_void_p() for _ in range(5)]
        _check(lib().mp3g_fbank_info(fb, C.byref(pp), C.byref(k), *[C.byref(q) for q in p], C.byref(t)))
        self.P, self.K, self.tile_frames = pp.value, k.value, t.value
        self.log_energy_floor, self.dct_in_lds = float(lef.value), bool(in_lds.value)

        def view(q, ctype, shape):  # a view of the library's table: valid while this object lives
            return np.ctypeslib.as_array(C.cast(q, C.POINTER(ctype)), shape=shape)
        self.dct = view(d, C.c_float, (self.n_ceps, self.n_mels))
        self.lifter = view(lf, C.c_float, (self.n_ceps,))
        self.cw = view(p[0], C.c_float, (self.K, self.N))
        self.sw = view(p[1], C.c_float, (self.K, self.N))
        self.wm = view(p[2], C.c_float, (self.n_mels, self.K))
        self.support = view(p[3], C.c_uint32, (self.n_mels, 2))
        self.w = view(p[4], C.c_float, (self.N,))

    def frames(self, T):
        """The frames a row of T samples has (mp3g_mfcc_frames)."""
        return int(lib().mp3g_mfcc_frames(self._h, int(T)))

    def host(self, x, n_frames=None, cep_stride=None):
        """The reference on the CPU (mp3g_mfcc_host): features [n_frames,
        n_ceps] of the float32 row x (n_frames: all by default); with a
        cep_stride the full [n_frames, cep_stride] buffer, zeros where nothing
        is written."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.frames(len(x)) if n_frames is None else int(n_frames)
        stride = self.n_ceps if cep_stride is None else int(cep_stride)
        out = np.zeros((max(n, 0), max(stride, 0)), np.float32)
        _check(lib().mp3g_mfcc_host(self._h, _ptr(x) if len(x) else None, len(x), n, _ptr(out) if out.size else None,
                                    stride))
        return out

    def execute(self, d_src, d_out=None, stream=None):
        """The device call (mp3g_mfcc_execute): d_src float32 [B, C, T] (C = 1
        or 2) or [B, T], contiguous on this object's device; d_out float32
        [B, C, F, S] or [B, F, S] with F <= frames(T) and S >= n_ceps (made here
        when None: every frame, S = n_ceps).  Writes the n_ceps features of each
        of the F frames, nothing else.  One launch, asynchronous on `stream` (a
        hipStream_t; None = the current torch stream).  Returns d_out."""
        import torch
        if d_src.dtype != torch.float32 or not d_src.is_contiguous() or d_src.dim() not in (2, 3) or not d_src.is_cuda:
            raise ValueError("MFCC.execute: a contiguous float32 device tensor [B, C, T] or [B, T]")
        B, T = int(d_src.shape[0]), int(d_src.shape[-1])
        planes = int(d_src.shape[1]) if d_src.dim() == 3 else 1
        lead = (B, planes) if d_src.dim() == 3 else (B,)
        if d_out is None:
            d_out = torch.empty(lead + (self.frames(T), self.n_ceps), dtype=torch.float32, device=d_src.device)
        if (d_out.dtype != torch.float32 or not d_out.is_contiguous() or not d_out.is_cuda
                or d_out.dim() != len(lead) + 2 or tuple(d_out.shape[:-2]) != lead):
            raise ValueError("MFCC.execute: d_out is a contiguous float32 device tensor [B, (C,) F, S]")
        if stream is None:
            stream = torch.cuda.current_stream(d_src.device).cuda_stream
        _check(lib().mp3g_mfcc_execute(self._h, C.c_void_p(d_src.data_ptr()) if d_src.numel() else None, B, planes, T,
                                       C.c_void_p(d_out.data_ptr()) if d_out.numel() else None,
                                       int(d_out.shape[-2]), int(d_out.shape[-1]), C.c_void_p(stream) if stream else None))
        return d_out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.dct = self.lifter = self.cw = self.sw = self.wm = self.support = self.w = None
            lib().mp3g_mfcc_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cmvn_host(feats, frame_lengths, norm_vars=False, n_cols=None):
    """The reference on the CPU (mp3g_cmvn_host): a normalised copy of the
    float32 array feats [B, F, S] or [B, C, F, S] -- per row and plane, over
    the row's first min(frame_lengths[b], F) frames, every column below n_cols
    (all S by default) minus its mean in double, with norm_vars divided by its
    standard deviation (the variance floored at 1e-20).  Frames past the length
    and columns from n_cols on are copied."""
    out = np.array(feats, dtype=np.float32, order="C", copy=True)
    if out.ndim not in (3, 4):
        raise ValueError("cmvn_host: feats is [B, F, S] or [B, C, F, S]")
    B, planes = out.shape[0], (out.shape[1] if out.ndim == 4 else 1)
    lengths = np.ascontiguousarray(frame_lengths, dtype=np.uint32)
    if lengths.shape != (B,):
        raise ValueError("cmvn_host: one frame length per row")
    cols = out.shape[-1] if n_cols is None else int(n_cols)
    _check(lib().mp3g_cmvn_host(_ptr(out) if out.size else None, B, planes, out.shape[-2], out.shape[-1], cols,
                                _ptr(lengths) if B else None, CMVN_NORM_VARS if norm_vars else 0))
    return out


def cmvn(feats, frame_lengths, norm_vars=False, stream=None, n_cols=None):
    """The device call (mp3g_cmvn_rows): normalises the contiguous float32
    device tensor feats [B, F, S] or [B, C, F, S] in place, as cmvn_host
    states it and bit for bit.  frame_lengths: a device tensor or anything
    array-like, one count per row (copied to the device as int32 when it is not
    there; values above F mean F).  One launch, asynchronous on `stream` (a
    hipStream_t; None = the current torch stream).  Returns feats."""
    import torch
    if (not torch.is_tensor(feats) or feats.dtype != torch.float32 or not feats.is_contiguous() or not feats.is_cuda
            or feats.dim() not in (3, 4)):
        raise ValueError("cmvn: a contiguous float32 device tensor [B, F, S] or [B, C, F, S]")
    B, planes = int(feats.shape[0]), (int(feats.shape[1]) if feats.dim() == 4 else 1)
    if torch.is_tensor(frame_lengths) and frame_lengths.is_cuda:
        lengths = frame_lengths.to(torch.int32).contiguous()
    else:
        host = np.ascontiguousarray(np.minimum(np.asarray(frame_lengths, dtype=np.int64), 2 ** 31 - 1), dtype=np.int32)
        lengths = torch.from_numpy(host).to(feats.device)
    if tuple(lengths.shape) != (B,):
        raise ValueError("cmvn: one frame length per row")
    cols = int(feats.shape[-1]) if n_cols is None else int(n_cols)
    if stream is None:
        stream = torch.cuda.current_stream(feats.device).cuda_stream
    _check(lib().mp3g_cmvn_rows(feats.device.index or 0, C.c_void_p(feats.data_ptr()) if feats.numel() else None, B,
                                planes, int(feats.shape[-2]), int(feats.shape[-1]), cols,
                                C.c_void_p(lengths.data_ptr()) if B else None, CMVN_NORM_VARS if norm_vars else 0,
                                C.c_void_p(stream) if stream else None))
    return feats


_cmvn_rows = cmvn  # (decode_windows_mfcc_tensor has a parameter of that name)


# ---- sliding-window CMN, energy VAD and voiced-frame selection (include/mp3g.h) --
SCMN_CENTER = 1
SCMN_NORM_VARS = 2
SLIDING_CMVN_MODES = {"sliding": False, "sliding_var": True}
VAD_OPTIONS = ("energy_threshold", "energy_mean_scale", "proportion_threshold", "frames_context")


def _host_feats(name, feats, frame_lengths, n_cols):
    """(x float32 C-order [B, (C,) F, S], B, planes, lengths uint32 [B], cols) of a host call."""
    x = np.ascontiguousarray(feats, dtype=np.float32)
    if x.ndim not in (3, 4):
        raise ValueError(name + ": feats is [B, F, S] or [B, C, F, S]")
    B, planes = x.shape[0], (x.shape[1] if x.ndim == 4 else 1)
    lengths = np.ascontiguousarray(np.minimum(np.asarray(frame_lengths, dtype=np.int64), 2 ** 32 - 1), dtype=np.uint32)
    if lengths.shape != (B,):
        raise ValueError(name + ": one frame length per row")
    return x, B, planes, lengths, (x.shape[-1] if n_cols is None else int(n_cols))


def _device_feats(name, feats, frame_lengths, n_cols):
    """(B, planes, lengths int32 device tensor [B], cols) of a device call on feats."""
    import torch
    if (not torch.is_tensor(feats) or feats.dtype != torch.float32 or not feats.is_contiguous() or not feats.is_cuda
            or feats.dim() not in (3, 4)):
        raise ValueError(name + ": a contiguous float32 device tensor [B, F, S] or [B, C, F, S]")
    B, planes = int(feats.shape[0]), (int(feats.shape[1]) if feats.dim() == 4 else 1)
    if torch.is_tensor(frame_lengths) and frame_lengths.is_cuda:
        lengths = frame_lengths.to(torch.int32).contiguous()
    else:
        host = np.ascontiguousarray(np.minimum(np.asarray(frame_lengths, dtype=np.int64), 2 ** 31 - 1), dtype=np.int32)
        lengths = torch.from_numpy(host).to(feats.device)
    if tuple(lengths.shape) != (B,):
        raise ValueError(name + ": one frame length per row")
    return B, planes, lengths, (int(feats.shape[-1]) if n_cols is None else int(n_cols))


def _dptr(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def _stream_of(t, stream):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(t.device).cuda_stream
    return C.c_void_p(stream) if stream else None


def sliding_cmn_host(feats, frame_lengths, cmn_window=600, min_window=100, center=False, norm_vars=False, n_cols=None):
    """The reference on the CPU (mp3g_sliding_cmn_host; Kaldi's
    apply-cmvn-sliding, torchaudio.functional.sliding_window_cmn): a copy of the
    float32 array feats [B, F, S] or [B, C, F, S] in which every column below
    n_cols of each row's first min(frame_lengths[b], F) frames has the mean of
    its window of up to cmn_window frames subtracted (centred on the frame, or
    the frames before it and at least min_window of them at a row's start) and,
    with norm_vars, is divided by the window's standard deviation (the variance
    floored at 1e-10).  The sums are float64, in the blocked order of
    include/mp3g.h."""
    x, B, planes, lengths, cols = _host_feats("sliding_cmn_host", feats, frame_lengths, n_cols)
    out = x.copy()
    flags = (SCMN_CENTER if center else 0) | (SCMN_NORM_VARS if norm_vars else 0)
    _check(lib().mp3g_sliding_cmn_host(_ptr(x) if x.size else None, _ptr(out) if out.size else None, B, planes,
                                       x.shape[-2], x.shape[-1], cols, _ptr(lengths) if B else None, int(cmn_window),
                                       int(min_window), flags))
    return out


def sliding_cmn(feats, frame_lengths, cmn_window=600, min_window=100, center=False, norm_vars=False, out=None,
                n_cols=None, stream=None):
    """The device call (mp3g_sliding_cmn_rows): as sliding_cmn_host states it
    and bit for bit, from the contiguous float32 device tensor feats [B, F, S]
    or [B, C, F, S] into `out` (another tensor like it; made here when None, and
    then columns from n_cols on are copies too).  frame_lengths as for cmvn.  One
    launch, asynchronous on `stream` (a hipStream_t; None = the current torch
    stream).  Returns out."""
    import torch
    B, planes, lengths, cols = _device_feats("sliding_cmn", feats, frame_lengths, n_cols)
    if out is None:
        out = feats.clone() if cols < int(feats.shape[-1]) else torch.empty_like(feats)
    if (not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or out.shape != feats.shape
            or out.device != feats.device):
        raise ValueError("sliding_cmn: out is a contiguous float32 tensor like feats")
    flags = (SCMN_CENTER if center else 0) | (SCMN_NORM_VARS if norm_vars else 0)
    _check(lib().mp3g_sliding_cmn_rows(feats.device.index or 0, _dptr(feats), _dptr(out), B, planes,
                                       int(feats.shape[-2]), int(feats.shape[-1]), cols, _dptr(lengths),
                                       int(cmn_window), int(min_window), flags, _stream_of(feats, stream)))
    return out


def vad_energy_host(feats, frame_lengths, energy_threshold=5.0, energy_mean_scale=0.5, proportion_threshold=0.6,
                    frames_context=0, col=0, n_cols=None):
    """The reference on the CPU (mp3g_vad_energy_host; Kaldi's
    compute-vad-energy): (voiced uint8 [B, (C,) F], counts int32 [B, (C)]).
    Frame t of a row's first min(frame_lengths[b], F) is voiced when, of the
    frames within frames_context of it, at least proportion_threshold have
    feats[..., col] above energy_threshold + energy_mean_scale * (the column's
    mean over the row); the comparison of the proportion is float32, as
    Kaldi's.  Frames past the length are 0."""
    x, B, planes, lengths, cols = _host_feats("vad_energy_host", feats, frame_lengths, n_cols)
    voiced = np.zeros(x.shape[:-1], np.uint8)
    counts = np.zeros(x.shape[:-2], np.uint32)
    _check(lib().mp3g_vad_energy_host(_ptr(x) if x.size else None, B, planes, x.shape[-2], x.shape[-1], cols, int(col),
                                      _ptr(lengths) if B else None, float(energy_threshold), float(energy_mean_scale),
                                      float(proportion_threshold), int(frames_context),
                                      _ptr(voiced) if voiced.size else None, _ptr(counts) if counts.size else None))
    return voiced, counts.astype(np.int32)


def vad_energy(feats, frame_lengths, energy_threshold=5.0, energy_mean_scale=0.5, proportion_threshold=0.6,
               frames_context=0, col=0, n_cols=None, out=None, stream=None):
    """The device call (mp3g_vad_energy_rows): as vad_energy_host states it and
    bit for bit, on the contiguous float32 device tensor feats [B, F, S] or
    [B, C, F, S].  Returns device tensors (voiced uint8 [B, (C,) F], counts
    int32 [B, (C)]): `out`, a pair of such contiguous tensors, when given.  One
    launch, asynchronous on `stream`."""
    import torch
    B, planes, lengths, cols = _device_feats("vad_energy", feats, frame_lengths, n_cols)
    if out is None:
        out = (torch.empty(tuple(feats.shape[:-1]), dtype=torch.uint8, device=feats.device),
               torch.empty(tuple(feats.shape[:-2]), dtype=torch.int32, device=feats.device))
    voiced, counts = out
    if (voiced.dtype != torch.uint8 or counts.dtype != torch.int32 or not voiced.is_contiguous()
            or not counts.is_contiguous() or voiced.shape != feats.shape[:-1] or counts.shape != feats.shape[:-2]
            or voiced.device != feats.device or counts.device != feats.device):
        raise ValueError("vad_energy: out is (uint8 [B, (C,) F], int32 [B, (C)]), contiguous on feats' device")
    _check(lib().mp3g_vad_energy_rows(feats.device.index or 0, _dptr(feats), B, planes, int(feats.shape[-2]),
                                      int(feats.shape[-1]), cols, int(col), _dptr(lengths), float(energy_threshold),
                                      float(energy_mean_scale), float(proportion_threshold), int(frames_context),
                                      _dptr(voiced), _dptr(counts), _stream_of(feats, stream)))
    return voiced, counts


def select_frames_host(feats, voiced, frame_lengths, n_frames_out=None, n_cols=None, out=None):
    """The reference on the CPU (mp3g_select_frames_host; Kaldi's
    select-voiced-frames, kept dense): (out float32 [B, (C,) n_frames_out, S],
    lengths_out int32 [B, (C)]).  out[b, j] is the j-th frame of feats[b] below
    the row's length with voiced != 0, columns below n_cols; the frames after
    the last one are +0; lengths_out = min(count, n_frames_out).  n_frames_out:
    F by default.  `out`, when given, is an array [B, (C,) n_frames_out, S_out]
    whose other words are kept (a copy is returned)."""
    x, B, planes, lengths, cols = _host_feats("select_frames_host", feats, frame_lengths, n_cols)
    v = np.ascontiguousarray(voiced, dtype=np.uint8)
    if v.shape != x.shape[:-1]:
        raise ValueError("select_frames_host: voiced is [B, (C,) F]")
    if out is None:
        Fo = x.shape[-2] if n_frames_out is None else int(n_frames_out)
        y = np.zeros(x.shape[:-2] + (Fo, x.shape[-1]), np.float32)
    else:
        y = np.array(out, dtype=np.float32, order="C", copy=True)
        if y.ndim != x.ndim or y.shape[:-2] != x.shape[:-2]:
            raise ValueError("select_frames_host: out is [B, (C,) n_frames_out, S_out]")
    m = np.zeros(x.shape[:-2], np.uint32)
    _check(lib().mp3g_select_frames_host(_ptr(x) if x.size else None, B, planes, x.shape[-2], x.shape[-1], cols,
                                         _ptr(v) if v.size else None, _ptr(lengths) if B else None,
                                         _ptr(y) if y.size else None, y.shape[-2], y.shape[-1],
                                         _ptr(m) if m.size else None))
    return y, m.astype(np.int32)


def select_frames(feats, voiced, frame_lengths, n_frames_out=None, n_cols=None, out=None, stream=None):
    """The device call (mp3g_select_frames_rows): as select_frames_host states
    it and bit for bit.  feats as for vad_energy, voiced a uint8 device tensor
    [B, (C,) F] (vad_energy's).  out: a contiguous float32 device tensor [B,
    (C,) n_frames_out, S_out] (made here when None: n_frames_out frames, F by
    default, of S columns).  No frame count is read back: the output keeps its
    static shape.  Returns (out, lengths_out int32 [B, (C)]).  One launch,
    asynchronous on `stream`."""
    import torch
    B, planes, lengths, cols = _device_feats("select_frames", feats, frame_lengths, n_cols)
    if (not torch.is_tensor(voiced) or voiced.dtype != torch.uint8 or not voiced.is_contiguous()
            or voiced.device != feats.device or voiced.shape != feats.shape[:-1]):
        raise ValueError("select_frames: voiced is a contiguous uint8 device tensor [B, (C,) F]")
    if out is None:
        Fo = int(feats.shape[-2]) if n_frames_out is None else int(n_frames_out)
        out = torch.empty(tuple(feats.shape[:-2]) + (Fo, int(feats.shape[-1])), dtype=torch.float32,
                          device=feats.device)
        if cols < int(feats.shape[-1]):
            out.zero_()
    if (not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != feats.device
            or out.dim() != feats.dim() or out.shape[:-2] != feats.shape[:-2]):
        raise ValueError("select_frames: out is a contiguous float32 device tensor [B, (C,) n_frames_out, S_out]")
    m = torch.empty(tuple(feats.shape[:-2]), dtype=torch.int32, device=feats.device)
    _check(lib().mp3g_select_frames_rows(feats.device.index or 0, _dptr(feats), B, planes, int(feats.shape[-2]),
                                         int(feats.shape[-1]), cols, _dptr(voiced), _dptr(lengths), _dptr(out),
                                         int(out.shape[-2]), int(out.shape[-1]), _dptr(m), _stream_of(feats, stream)))
    return out, m


# ---- SpecAugment: time warp, frequency and time masks (include/mp3g.h) ------------
SPECAUG_FREQ_MAJOR = 1
SPECAUG_WARP = 2
SPECAUG_FILL_MEAN = 4
SPECAUG_MAX_TIME_MASKS = 16
SPECAUG_MAX_FREQ_MASKS = 4
SPECAUG_ROW_DTYPE = np.dtype([("warp_center", "<u4"), ("warp_to", "<u4"), ("n_time", "<u4"), ("n_freq", "<u4"),
                              ("time", "<u4", (SPECAUG_MAX_TIME_MASKS, 2)),
                              ("freq", "<u4", (SPECAUG_MAX_FREQ_MASKS, 2))])
assert SPECAUG_ROW_DTYPE.itemsize == 176


def _specaug_flags(name, fill, freq_major, warp):
    """(flags, fill_value) of a spec_augment call."""
    flags = (SPECAUG_FREQ_MAJOR if freq_major else 0) | (SPECAUG_WARP if warp else 0)
    if isinstance(fill, str):
        if fill != "mean":
            raise ValueError(name + ": fill is a number or 'mean'")
        return flags | SPECAUG_FILL_MEAN, 0.0
    return flags, float(fill)


def spec_augment_host(feats, frame_lengths, rows, fill=0.0, freq_major=False, warp=True, n_cols=None):
    """The reference on the CPU (mp3g_specaug_host): SpecAugment of the float32
    array feats -- [B, F, S] or [B, C, F, S], or with freq_major [B, bins, S] or
    [B, C, bins, S] with the frames along the last axis -- as include/mp3g.h
    states it: per row, from rows[b] (SPECAUG_ROW_DTYPE; spec_augment_rows
    draws them), first the two-segment cubic time warp (when `warp`), then the
    union of the row's time and frequency masks written with `fill`, a number or
    "mean" (the mean of the row's live input per plane, in float64).  Only the
    row's first min(frame_lengths[b], F) frames are warped and masked; later
    frames are copied.  n_cols: the live count of the last axis (bins in
    time-major, frames in frequency-major; all S by default); words past it keep
    feats' values.  Returns out, or (out, fills float32 [B, (C)]) with "mean"."""
    x, B, planes, lengths, live = _host_feats("spec_augment_host", feats, frame_lengths, n_cols)
    desc = np.ascontiguousarray(rows, dtype=SPECAUG_ROW_DTYPE)
    if desc.shape != (B,):
        raise ValueError("spec_augment_host: one descriptor per row")
    flags, value = _specaug_flags("spec_augment_host", fill, freq_major, warp)
    n_frames, n_bins = (live, x.shape[-2]) if freq_major else (x.shape[-2], live)
    out = x.copy()
    fills = np.zeros(x.shape[:-2], np.float32)
    _check(lib().mp3g_specaug_host(_ptr(x) if x.size else None, _ptr(out) if out.size else None, B, planes, n_frames,
                                   n_bins, x.shape[-1], _ptr(lengths) if B else None, _ptr(desc) if B else None, flags,
                                   value, _ptr(fills) if fills.size else None))
    return (out, fills) if flags & SPECAUG_FILL_MEAN else out


def spec_augment(feats, frame_lengths, rows, fill=0.0, freq_major=False, warp=True, out=None, n_cols=None, stream=None):
    """The device call (mp3g_specaug_rows): as spec_augment_host states it and
    bit for bit, from the contiguous float32 device tensor feats into `out`
    (another tensor like it; made here when None).  rows: a host array of
    SPECAUG_ROW_DTYPE [B], or a uint8 or int32 device tensor of B x 176 bytes.
    frame_lengths as for cmvn.  out=feats works in place and is allowed only
    with warp=False: then only the masked words are written.  One launch, two
    with fill="mean", asynchronous on `stream` (a hipStream_t; None = the
    current torch stream).  Returns out, or (out, fills) with "mean"."""
    import torch
    B, planes, lengths, live = _device_feats("spec_augment", feats, frame_lengths, n_cols)
    flags, value = _specaug_flags("spec_augment", fill, freq_major, warp)
    if torch.is_tensor(rows):
        if (not rows.is_cuda or rows.device != feats.device or rows.dtype not in (torch.uint8, torch.int32)
                or not rows.is_contiguous() or rows.numel() * rows.element_size() != B * SPECAUG_ROW_DTYPE.itemsize):
            raise ValueError("spec_augment: rows is a contiguous uint8 or int32 device tensor of B x 176 bytes")
        d_rows = rows
    else:
        desc = np.ascontiguousarray(rows, dtype=SPECAUG_ROW_DTYPE)
        if desc.shape != (B,):
            raise ValueError("spec_augment: one descriptor per row")
        d_rows = torch.from_numpy(desc.view(np.uint8).copy()).to(feats.device)
    if out is feats and warp:
        raise ValueError("spec_augment: out=feats needs warp=False (the warp is out of place)")
    if out is None:
        out = feats.clone() if live < int(feats.shape[-1]) else torch.empty_like(feats)
    if (not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or out.shape != feats.shape
            or out.device != feats.device):
        raise ValueError("spec_augment: out is a contiguous float32 tensor like feats")
    n_frames, n_bins = (live, int(feats.shape[-2])) if freq_major else (int(feats.shape[-2]), live)
    fills = None
    if flags & SPECAUG_FILL_MEAN:
        fills = torch.empty(tuple(feats.shape[:-2]), dtype=torch.float32, device=feats.device)
    _check(lib().mp3g_specaug_rows(feats.device.index or 0, _dptr(feats), _dptr(out), B, planes, n_frames, n_bins,
                                   int(feats.shape[-1]), _dptr(lengths), _dptr(d_rows), flags, value,
                                   _dptr(fills) if fills is not None else None, _stream_of(feats, stream)))
    return (out, fills) if fills is not None else out


def spec_augment_rows(rng, frame_lengths, n_bins, time_warp=0, n_freq_masks=2, freq_mask_width=27, n_time_masks=2,
                      time_mask_width=100, time_mask_ratio=None):
    """Draws one SpecAugment descriptor per row from rng (a
    numpy.random.Generator) and returns the SPECAUG_ROW_DTYPE array [B] that
    spec_augment takes.  Pure numpy.  Per row of n = frame_lengths[b] frames:

    warp, as ESPnet's time_warp draws it with window W = time_warp: none when
    W = 0 or n - W <= W; otherwise the centre c uniform in [W, n - W) and its
    destination w uniform in [c - W + 1, c + W];
    n_freq_masks frequency masks: width uniform in [0, freq_mask_width] (at
    most n_bins), start uniform in [0, n_bins - width];
    n_time_masks time masks: width uniform in [0, T], T = time_mask_width,
    capped at floor(time_mask_ratio * n) when a ratio is given (the paper's p,
    ESPnet's ratio range) and at n; start uniform in [0, n - width].  Time masks
    are drawn against n: the warp leaves the length unchanged.

    The LibriSpeech policies of Park et al. 2019 as parameter sets:
      LB: time_warp=80, freq_mask_width=27, n_freq_masks=1, time_mask_width=100, n_time_masks=1, time_mask_ratio=1.0
      LD: time_warp=80, freq_mask_width=27, n_freq_masks=2, time_mask_width=100, n_time_masks=2, time_mask_ratio=1.0
    and Switchboard's
      SM: time_warp=40, freq_mask_width=15, n_freq_masks=2, time_mask_width=70, n_time_masks=2, time_mask_ratio=0.2
      SS: time_warp=40, freq_mask_width=27, n_freq_masks=2, time_mask_width=70, n_time_masks=2, time_mask_ratio=0.2
    icefall's default is n_time_masks=10 with time_mask_ratio=0.2 shared among
    them; here the ratio caps each mask."""
    lengths = np.asarray(frame_lengths, dtype=np.int64).reshape(-1)
    n_bins, W = int(n_bins), int(time_warp)
    n_f, n_t = int(n_freq_masks), int(n_time_masks)
    if not 0 <= n_f <= SPECAUG_MAX_FREQ_MASKS or not 0 <= n_t <= SPECAUG_MAX_TIME_MASKS:
        raise ValueError("spec_augment_rows: at most %d frequency and %d time masks"
                         % (SPECAUG_MAX_FREQ_MASKS, SPECAUG_MAX_TIME_MASKS))
    if n_bins < 0 or W < 0 or int(freq_mask_width) < 0 or int(time_mask_width) < 0 or (lengths < 0).any():
        raise ValueError("spec_augment_rows: negative count or width")
    rows = np.zeros(len(lengths), SPECAUG_ROW_DTYPE)
    for b, n in enumerate(lengths):
        n = int(min(n, 2 ** 32 - 1))
        r = rows[b]
        if W > 0 and n - W > W:
            c = int(rng.integers(W, n - W))
            r["warp_center"], r["warp_to"] = c, int(rng.integers(c - W + 1, c + W + 1))
        r["n_freq"], r["n_time"] = n_f, n_t
        fmax = min(int(freq_mask_width), n_bins)
        for k in range(n_f):
            width = int(rng.integers(0, fmax + 1))
            r["freq"][k] = (int(rng.integers(0, n_bins - width + 1)), width)
        tmax = min(int(time_mask_width), n)
        if time_mask_ratio is not None:
            tmax = min(tmax, int(float(time_mask_ratio) * n))
        for k in range(n_t):
            width = int(rng.integers(0, tmax + 1))
            r["time"][k] = (int(rng.integers(0, n - width + 1)), width)
    return rows


_spec_augment = spec_augment  # (the decode_windows_*_tensor calls have a parameter of that name)


def _specaug_after(name, feats, flen, spec, n_bins, freq_major):
    """The spec_augment= keyword of a decode_windows_*_tensor call: spec is a
    descriptor array [B], or a dict of spec_augment_rows' options plus `rng` and
    `fill`, whose rows are drawn from the call's own frame lengths.  Returns the
    augmented tensor."""
    fill = 0.0
    if isinstance(spec, dict):
        opts = dict(spec)
        fill = opts.pop("fill", 0.0)
        rng = opts.pop("rng", None)
        if rng is None:
            raise Mp3gError(1, name + ": spec_augment as a dict needs rng, a numpy.random.Generator")
        try:
            rows = spec_augment_rows(rng, flen, n_bins, **opts)
        except (TypeError, ValueError) as e:
            raise Mp3gError(1, name + ": spec_augment: " + str(e))
    else:
        rows = np.ascontiguousarray(spec, dtype=SPECAUG_ROW_DTYPE)
        if rows.shape != (len(flen),):
            raise Mp3gError(1, name + ": spec_augment is one descriptor per stream")
    out = _spec_augment(feats, flen, rows, fill=fill, freq_major=freq_major, warp=True)
    return out[0] if isinstance(out, tuple) else out


# ---- delta features and frame context (include/mp3g.h) ----------------------------
DELTA_OPTIONS = ("order", "window")
STACK_OPTIONS = ("left", "right", "step", "first")
DELTA_MAX_ORDER = 4
DELTA_MAX_HALO = 32
STACK_MAX_CONTEXT = 64


def _plane_lengths_host(name, frame_lengths, B, planes):
    """(lengths uint32 C-order, len_planes) of frame_lengths [B] or [B, planes]."""
    lengths = np.ascontiguousarray(np.minimum(np.asarray(frame_lengths, dtype=np.int64), 2 ** 32 - 1), dtype=np.uint32)
    if lengths.shape == (B,):
        return lengths, 1
    if lengths.shape == (B, planes):
        return lengths, planes
    raise ValueError(name + ": frame_lengths is [B] or [B, planes]")


def _plane_lengths_device(name, frame_lengths, B, planes, device):
    """(lengths int32 device tensor, len_planes) of frame_lengths [B] or [B, planes], host or device."""
    import torch
    if torch.is_tensor(frame_lengths) and frame_lengths.is_cuda:
        lengths = frame_lengths.to(torch.int32).contiguous()
    else:
        host = np.ascontiguousarray(np.minimum(np.asarray(frame_lengths, dtype=np.int64), 2 ** 31 - 1), dtype=np.int32)
        lengths = torch.from_numpy(host).to(device)
    if tuple(lengths.shape) == (B,):
        return lengths, 1
    if tuple(lengths.shape) == (B, planes):
        return lengths, planes
    raise ValueError(name + ": frame_lengths is [B] or [B, planes]")


def _host_tensor(name, feats, n_cols):
    """(x float32 C-order [B, (C,) F, S], B, planes, cols) of a host call."""
    x = np.ascontiguousarray(feats, dtype=np.float32)
    if x.ndim not in (3, 4):
        raise ValueError(name + ": feats is [B, F, S] or [B, C, F, S]")
    return x, x.shape[0], (x.shape[1] if x.ndim == 4 else 1), (x.shape[-1] if n_cols is None else int(n_cols))


def _device_tensor(name, feats, n_cols):
    """(B, planes, cols) of a device call on feats."""
    import torch
    if (not torch.is_tensor(feats) or feats.dtype != torch.float32 or not feats.is_contiguous() or not feats.is_cuda
            or feats.dim() not in (3, 4)):
        raise ValueError(name + ": a contiguous float32 device tensor [B, F, S] or [B, C, F, S]")
    return (int(feats.shape[0]), (int(feats.shape[1]) if feats.dim() == 4 else 1),
            (int(feats.shape[-1]) if n_cols is None else int(n_cols)))


def _host_out(name, out, lead, frames, width):
    """The array a host call writes: zeros [lead.., frames, width], or a copy of `out`
    [lead.., frames or any, S_out] whose other words are kept."""
    if out is None:
        return np.zeros(tuple(lead) + (frames, width), np.float32)
    y = np.array(out, dtype=np.float32, order="C", copy=True)
    if y.ndim != len(lead) + 2 or y.shape[:-2] != tuple(lead):
        raise ValueError(name + ": out is [B, (C,) frames, S_out]")
    return y


def _device_out(name, out, feats, frames, width):
    """The tensor a device call writes: made here when None (of exactly the live
    width), else a contiguous float32 tensor [B, (C,) frames, S_out]."""
    import torch
    if out is None:
        out = torch.empty(tuple(feats.shape[:-2]) + (frames, width), dtype=torch.float32, device=feats.device)
    if (not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != feats.device
            or out.dim() != feats.dim() or out.shape[:-2] != feats.shape[:-2]):
        raise ValueError(name + ": out is a contiguous float32 device tensor [B, (C,) frames, S_out]")
    return out


def delta_scales(order, window):
    """Kaldi's delta scales in float32 (mp3g_delta_scales): a list of order + 1
    arrays, the i-th of 2 * i * window + 1 taps; [array([1.])] for order 0.  Order
    i is made from the already rounded order i - 1."""
    order, window = int(order), int(window)
    sizes = [2 * i * window + 1 for i in range(order + 1)]
    buf = np.zeros(max(1, sum(sizes)) if 0 <= order <= DELTA_MAX_ORDER and 0 < window <= DELTA_MAX_HALO else 1,
                   np.float32)
    _check(lib().mp3g_delta_scales(order, window, _ptr(buf)))
    return [a.copy() for a in np.split(buf, np.cumsum(sizes)[:-1])]


def add_deltas_host(feats, frame_lengths, order=2, window=2, n_cols=None, out=None):
    """The reference on the CPU (mp3g_add_deltas_host; Kaldi's add-deltas): the
    float32 array [B, (C,) F, (order + 1) * n_cols] whose block 0 is a bit copy
    of feats' columns below n_cols (all S by default) and whose block i is the
    i-th order delta -- fmaf over delta_scales(order, window)[i], the neighbours
    clamped to the row's first min(frame_lengths, F) frames, every order on the
    original frames.  Frames past the length are +0.  frame_lengths: [B], or
    [B, C] with one count per plane.  `out`, when given, is an array [B, (C,) F,
    S_out] whose other words are kept (a copy is returned)."""
    x, B, planes, cols = _host_tensor("add_deltas_host", feats, n_cols)
    lengths, lp = _plane_lengths_host("add_deltas_host", frame_lengths, B, planes)
    order, window = int(order), int(window)
    y = _host_out("add_deltas_host", out, x.shape[:-2], x.shape[-2], (max(order, 0) + 1) * cols)
    if y.shape[-2] != x.shape[-2]:
        raise ValueError("add_deltas_host: out has feats' frames")
    _check(lib().mp3g_add_deltas_host(_ptr(x) if x.size else None, _ptr(y) if y.size else None, B, planes, x.shape[-2],
                                      x.shape[-1], cols, y.shape[-1], _ptr(lengths) if B else None, lp, order, window))
    return y


def add_deltas(feats, frame_lengths, order=2, window=2, out=None, n_cols=None, stream=None):
    """The device call (mp3g_add_deltas_rows): as add_deltas_host states it and
    bit for bit, from the contiguous float32 device tensor feats [B, (C,) F, S]
    into `out` [B, (C,) F, S_out], S_out >= (order + 1) * n_cols (made here when
    None, with exactly that width).  frame_lengths: [B] or [B, C], anything
    array-like or an int32 device tensor.  One launch, asynchronous on `stream`
    (a hipStream_t; None = the current torch stream).  Returns out."""
    B, planes, cols = _device_tensor("add_deltas", feats, n_cols)
    lengths, lp = _plane_lengths_device("add_deltas", frame_lengths, B, planes, feats.device)
    order, window = int(order), int(window)
    width = (max(order, 0) + 1) * cols
    out = _device_out("add_deltas", out, feats, int(feats.shape[-2]), width)
    if out.shape[-2] != feats.shape[-2]:
        raise ValueError("add_deltas: out has feats' frames")
    _check(lib().mp3g_add_deltas_rows(feats.device.index or 0, _dptr(feats), _dptr(out), B, planes,
                                      int(feats.shape[-2]), int(feats.shape[-1]), cols, int(out.shape[-1]),
                                      _dptr(lengths), lp, order, window, _stream_of(feats, stream)))
    return out


def stack_frames_count(n_frames, step=1, first=0):
    """The frames a stack leaves of n_frames (mp3g_stack_frames_count): 0 when
    n_frames <= first, else ceil((n_frames - first) / step)."""
    return int(lib().mp3g_stack_frames_count(int(n_frames), int(step), int(first)))


def lfr_options(m=7, n=6):
    """The stack parameters of FunASR's apply_lfr(m, n): m frames stacked at a
    stride of n, the first padded on the left with frame 0, the last repeated."""
    left = (int(m) - 1) // 2
    return dict(left=left, right=int(m) - 1 - left, step=int(n), first=0)


def stack_frames_host(feats, frame_lengths, left=0, right=0, step=1, first=0, n_frames_out=None, n_cols=None, out=None):
    """The reference on the CPU (mp3g_stack_frames_host): (out float32 [B, (C,)
    n_frames_out, (left + right + 1) * n_cols], lengths_out int32 [B, (C)]).
    Output frame j of a row of n = min(frame_lengths, F) frames has the anchor
    t = first + j * step and is the bit copy of frames t - left .. t + right,
    each clamped to [0, n - 1], side by side; there are lengths_out =
    min(stack_frames_count(n, step, first), n_frames_out) of them and the frames
    after them are +0.  splice-feats is (L, R, 1, 0), apply_lfr lfr_options(m,
    n), subsample-feats (0, 0, N, offset).  n_frames_out: stack_frames_count(F,
    step, first) by default.  frame_lengths: [B] or [B, C].  `out`, when given,
    is an array [B, (C,) n_frames_out, S_out] whose other words are kept (a copy
    is returned)."""
    x, B, planes, cols = _host_tensor("stack_frames_host", feats, n_cols)
    lengths, lp = _plane_lengths_host("stack_frames_host", frame_lengths, B, planes)
    left, right, step, first = int(left), int(right), int(step), int(first)
    Fo = stack_frames_count(x.shape[-2], step, first) if n_frames_out is None else int(n_frames_out)
    y = _host_out("stack_frames_host", out, x.shape[:-2], Fo, (max(left, 0) + max(right, 0) + 1) * cols)
    m = np.zeros(x.shape[:-2], np.uint32)
    _check(lib().mp3g_stack_frames_host(_ptr(x) if x.size else None, B, planes, x.shape[-2], x.shape[-1], cols,
                                        _ptr(lengths) if B else None, lp, left, right, step, first,
                                        _ptr(y) if y.size else None, y.shape[-2], y.shape[-1],
                                        _ptr(m) if m.size else None))
    return y, m.astype(np.int32)


def stack_frames(feats, frame_lengths, left=0, right=0, step=1, first=0, n_frames_out=None, n_cols=None, out=None,
                 stream=None):
    """The device call (mp3g_stack_frames_rows): as stack_frames_host states it
    and bit for bit, from the contiguous float32 device tensor feats into `out`
    [B, (C,) n_frames_out, S_out] (made here when None).  No frame count is read
    back: the output keeps its static shape.  Returns (out, lengths_out int32
    [B, (C)]).  One launch, asynchronous on `stream`."""
    import torch
    B, planes, cols = _device_tensor("stack_frames", feats, n_cols)
    lengths, lp = _plane_lengths_device("stack_frames", frame_lengths, B, planes, feats.device)
    left, right, step, first = int(left), int(right), int(step), int(first)
    Fo = stack_frames_count(int(feats.shape[-2]), step, first) if n_frames_out is None else int(n_frames_out)
    width = (max(left, 0) + max(right, 0) + 1) * cols
    out = _device_out("stack_frames", out, feats, Fo, width)
    m = torch.empty(tuple(feats.shape[:-2]), dtype=torch.int32, device=feats.device)
    _check(lib().mp3g_stack_frames_rows(feats.device.index or 0, _dptr(feats), B, planes, int(feats.shape[-2]),
                                        int(feats.shape[-1]), cols, _dptr(lengths), lp, left, right, step, first,
                                        _dptr(out), int(out.shape[-2]), int(out.shape[-1]), _dptr(m),
                                        _stream_of(feats, stream)))
    return out, m


def _framectx_options(name, deltas, stack):
    """The deltas= and stack= keywords of a decode_windows_*_tensor call, checked before any work."""
    for key, value, allowed in (("deltas", deltas, DELTA_OPTIONS), ("stack", stack, STACK_OPTIONS)):
        if value is not None and (not isinstance(value, dict) or set(value) - set(allowed)):
            raise Mp3gError(1, "%s: %s is None or a dict of %s" % (name, key, ", ".join(allowed)))


def _framectx_after(feats, flen, deltas, stack):
    """deltas, then stack, of the features on the current stream.  Returns (feats, frame_lengths)."""
    if deltas is not None:
        feats = add_deltas(feats, flen, **deltas)
    if stack is not None:
        feats, counts = stack_frames(feats, flen, **stack)
        flen = counts.cpu().numpy().astype(np.int64)  # (the copy waits for the stream)
    return feats, flen


def decode_windows_mfcc_tensor(datas, starts, n_samples, rate=16000, frame_length_ms=25.0, frame_shift_ms=10.0,
                               n_mels=23, n_ceps=13, cepstral_lifter=22.0, use_energy=True, raw_energy=True,
                               energy_floor=0.0, low_freq=20.0, high_freq=0.0, preemphasis=0.97, remove_dc=True,
                               window="povey", snip_edges=True, scale=32768.0, cmvn=None, n_frames=None,
                               mode=MODE_EXACT, out_format=OUT_F32_MONO, gapless=False, quality="fast", n_threads=0,
                               device=0, cmn_window=300, min_cmn_window=100, center=True, vad=None,
                               speed=None, gain=None, deltas=None, stack=None):
    """decode_windows_resampled_tensor, MFCC.execute and, with cmvn = "mean"
    or "mean_var", the per-row normalisation over each stream's own frames, all
    on the current torch stream: Kaldi's MFCC features of each stream's window
    [starts[k], starts[k] + n_samples) at `rate`, zero padding included.
    F = n_frames, by default every frame a row of n_samples has.

    Returns (features, frame_lengths, end_status, rates): features [B, F,
    n_ceps] (OUT_F32_MONO) or [B, 2, F, n_ceps] (OUT_F32_PLANAR) on cuda:device,
    equal to MFCC.host (then cmvn_host) on the rows of
    decode_windows_resampled_tensor bit for bit; frame_lengths int64[B] as
    decode_windows_fbank_tensor counts them.  Frames past a stream's
    frame_lengths are not normalised.

    The speaker recipes' front end: cmvn = "sliding" or "sliding_var" is the
    sliding-window normalisation instead (sliding_cmn with cmn_window,
    min_cmn_window and center), and vad, a dict of vad_energy's options
    (energy_threshold, energy_mean_scale, proportion_threshold,
    frames_context), selects the voiced frames: the decision is taken on the raw
    features' coefficient 0 (use_energy is required), the normalisation of
    whichever kind runs over all of a stream's frames, the selection comes last
    (select_frames; the frames after the voiced ones are zeros).  frame_lengths
    are then the voiced counts, int64 [B] or, planar, [B, 2].

    speed, gain: speed and volume perturbation before everything else, one
    entry per stream each (decode_windows_resampled_tensor); starts and
    n_samples then count samples of the perturbed signal.

    deltas: None or dict(order=, window=): add_deltas after the selection (the
    GMM recipes' apply-cmvn | add-deltas), n_ceps * (order + 1) columns.  stack:
    None or dict(left=, right=, step=, first=): stack_frames after that (the
    TDNN recipes' splice-feats; subsampling); the features then have
    stack_frames_count(F, step, first) frames and the returned frame_lengths are
    the stacked counts.  Both take the voiced counts per plane as they are."""
    import torch
    if cmvn not in CMVN_MODES and cmvn not in SLIDING_CMVN_MODES:
        raise Mp3gError(1, "decode_windows_mfcc_tensor: cmvn is None, 'mean', 'mean_var', 'sliding' or 'sliding_var'")
    _framectx_options("decode_windows_mfcc_tensor", deltas, stack)
    if vad is not None:
        if not isinstance(vad, dict) or set(vad) - set(VAD_OPTIONS):
            raise Mp3gError(1, "decode_windows_mfcc_tensor: vad is None or a dict of " + ", ".join(VAD_OPTIONS))
        if not use_energy:
            raise Mp3gError(1, "decode_windows_mfcc_tensor: vad needs use_energy (coefficient 0 is the log energy)")
    mf = MFCC(rate, frame_length_ms, frame_shift_ms, n_mels, n_ceps, cepstral_lifter, use_energy, raw_energy,
              energy_floor, low_freq, high_freq, preemphasis, remove_dc, window, snip_edges, scale, device=device)
    try:
        T = int(n_samples)
        avail = mf.frames(T)
        F = avail if n_frames is None else int(n_frames)
        if F < 0 or F > avail:
            raise Mp3gError(1, "more frames than a row of n_samples has")
        batch, lengths, end_status, rates = decode_windows_resampled_tensor(
            datas, starts, T, rate, mode=mode, out_format=out_format, gapless=gapless, quality=quality,
            n_threads=n_threads, device=device, speed=speed, gain=gain)
        feats = torch.empty(tuple(batch.shape[:-1]) + (F, mf.n_ceps), dtype=torch.float32, device=batch.device)
        mf.execute(batch, feats)
        if snip_edges:
            flen = np.clip((lengths - mf.N) // mf.hop + 1, 0, F)
        else:
            flen = np.minimum(F, (lengths + mf.hop // 2) // mf.hop)
        if vad is not None:  # (on the raw features)
            voiced, _ = vad_energy(feats, flen, **vad)
        if cmvn in SLIDING_CMVN_MODES:
            feats = sliding_cmn(feats, flen, cmn_window, min_cmn_window, center, SLIDING_CMVN_MODES[cmvn])
        elif CMVN_MODES[cmvn] is not None:
            _cmvn_rows(feats, flen, norm_vars=CMVN_MODES[cmvn])
        if vad is not None:
            feats, counts = select_frames(feats, voiced, flen)
            flen = counts.cpu().numpy().astype(np.int64)  # (the copy waits for the stream)
        if deltas is not None or stack is not None:
            feats, flen = _framectx_after(feats, flen, deltas, stack)
        torch.cuda.current_stream(feats.device).synchronize()
    finally:
        mf.close()
    return feats, flen, end_status, rates


# ---- integrated loudness of decoded rows (include/mp3g.h) -----------------------
# one record per row (mp3g_loudness_stats)
LOUDNESS_STATS_DTYPE = np.dtype([("energy", "<f8"), ("lufs", "<f4"), ("peak", "<f4"), ("n_blocks", "<u4"),
                                 ("n_abs", "<u4"), ("n_gated", "<u4"), ("zero", "<u4")])
assert LOUDNESS_STATS_DTYPE.itemsize == 32
LOUDNESS_ABS_GATE = 1.1724653045822964e-07
# one record per row (mp3g_loudness_range)
LOUDNESS_RANGE_DTYPE = np.dtype([("momentary_max", "<f4"), ("shortterm_max", "<f4"), ("lra", "<f4"),
                                 ("range_lo", "<f4"), ("range_hi", "<f4"), ("n_short", "<u4"), ("n_range", "<u4"),
                                 ("zero", "<u4")])
assert LOUDNESS_RANGE_DTYPE.itemsize == 32


def loudness_target_energy(lufs):
    """The mean gated block energy of `lufs`: 10^((lufs + 0.691) / 10)
    (mp3g_loudness_target_energy)."""
    return float(lib().mp3g_loudness_target_energy(float(lufs)))


def _device_lengths(lengths, B, device, what):
    """One length per row as an int32 device tensor (None stays None; values
    above the row length mean the row length)."""
    import torch
    if lengths is None:
        return None
    if torch.is_tensor(lengths) and lengths.is_cuda:
        d = lengths.to(torch.int32).contiguous()
    else:
        host = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64), 0, 2 ** 31 - 1), dtype=np.int32)
        d = torch.from_numpy(host).to(device)
    if tuple(d.shape) != (B,):
        raise ValueError(what + ": one length per row")
    return d


class Loudness:
    """ITU-R BS.1770-4 integrated loudness and the sample peak of float32 rows
    at `rate` (8000 .. 192000 Hz; mp3g_loudness_*): K-weighting, 400 ms blocks
    every H = (rate + 5) // 10 samples, the absolute gate at -70 LUFS and the
    relative gate 10 LU under the mean.  One or two planes, each of weight 1.
    The filter runs per 100 ms segment from zero state and a scan over the
    segments adds what the carried-in state contributes, all in float64 in one
    fixed order, so the device call (execute) equals the host reference (host)
    byte for byte.  shelf and highpass are the two sections as b0 b1 b2 a1 a2;
    V [H, 4], AH [4, 4] and G [4, 4] the segment tables.  The largest
    momentary and short-term loudness and the loudness range (EBU Tech 3342)
    come from the same pass: range_host, and execute(d_range=); the true peak
    is mp3g.true_peak.  Surround channel weights and the momentary and
    short-term time series are not offered.
    device=None (or -1) makes a host-only object."""

    def __init__(self, rate, device=None):
        self._h = C.c_void_p()
        self.device = -1 if device is None else int(device)
        self.rate = int(rate)
        _check(lib().mp3g_loudness_create(self.device, self.rate, C.byref(self._h)))
        h = C.c_uint32()
        p = [C.c_void_p() for _ in range(5)]
        _check(lib().mp3g_loudness_info(self._h, C.byref(h), *[C.byref(q) for q in p]))
        self.H = h.value

        def view(q, shape):  # a view of the library's table: valid while this object lives
            return np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_double)), shape=shape)
        self.shelf, self.highpass = view(p[0], (5,)), view(p[1], (5,))
        self.V, self.AH, self.G = view(p[2], (self.H, 4)), view(p[3], (4, 4)), view(p[4], (4, 4))
        self._scratch = self._range_scratch = self._keep = None

    def blocks(self, n):
        """The 400 ms blocks a row of n samples has (mp3g_loudness_blocks)."""
        return int(lib().mp3g_loudness_blocks(self._h, int(n)))

    def host(self, x, lengths=None):
        """The reference on the CPU (mp3g_loudness_host): x float32 [B, C, T]
        (C = 1 or 2) or [B, T]; lengths: one sample count per row (None: T).
        Returns LOUDNESS_STATS_DTYPE[B]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim not in (2, 3):
            raise ValueError("Loudness.host: x is [B, C, T] or [B, T]")
        B, T = x.shape[0], x.shape[-1]
        planes = x.shape[1] if x.ndim == 3 else 1
        ln = None
        if lengths is not None:
            ln = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64), 0, 2 ** 32 - 1), dtype=np.uint32)
            if ln.shape != (B,):
                raise ValueError("Loudness.host: one length per row")
        stats = np.zeros(B, LOUDNESS_STATS_DTYPE)
        _check(lib().mp3g_loudness_host(self._h, _ptr(x) if x.size else None, B, planes, T,
                                        _ptr(ln) if ln is not None and B else None, _ptr(stats) if B else None))
        return stats

    def range_host(self, x, lengths=None):
        """The reference on the CPU of the momentary and short-term maxima and
        the loudness range (mp3g_loudness_range_host): x and lengths as in
        host().  Returns LOUDNESS_RANGE_DTYPE[B]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim not in (2, 3):
            raise ValueError("Loudness.range_host: x is [B, C, T] or [B, T]")
        B, T = x.shape[0], x.shape[-1]
        planes = x.shape[1] if x.ndim == 3 else 1
        ln = None
        if lengths is not None:
            ln = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64), 0, 2 ** 32 - 1), dtype=np.uint32)
            if ln.shape != (B,):
                raise ValueError("Loudness.range_host: one length per row")
        out = np.zeros(B, LOUDNESS_RANGE_DTYPE)
        _check(lib().mp3g_loudness_range_host(self._h, _ptr(x) if x.size else None, B, planes, T,
                                              _ptr(ln) if ln is not None and B else None, _ptr(out) if B else None))
        return out

    def execute(self, d_src, lengths=None, rows=None, stream=None, d_stats=None, d_range=None):
        """The device call (mp3g_loudness_rows): d_src float32 [B, C, T] (C = 1
        or 2) or [B, T], contiguous on this object's device; lengths: one
        sample count per row (a device tensor or array-like; None: T); rows: the
        rows to measure (array-like or an int32 device tensor; None: all).
        Returns the records as a uint8 device tensor [B, 32] (d_stats when
        given, else a new zero-filled one): only the records of the measured
        rows are written.  The scratch is a tensor this object keeps and grows.
        Two launches, asynchronous on `stream` (a hipStream_t; None = the
        current torch stream); read the records with stats().  d_range: a
        contiguous uint8 device tensor [B, 32] that receives the measured rows'
        mp3g_loudness_range records (range_stats() reads them), from a third
        launch behind the two on the same stream (mp3g_loudness_range_rows)."""
        import torch
        if d_src.dtype != torch.float32 or not d_src.is_contiguous() or d_src.dim() not in (2, 3) or not d_src.is_cuda:
            raise ValueError("Loudness.execute: a contiguous float32 device tensor [B, C, T] or [B, T]")
        B, T = int(d_src.shape[0]), int(d_src.shape[-1])
        planes = int(d_src.shape[1]) if d_src.dim() == 3 else 1
        dev = d_src.device
        if d_stats is None:
            d_stats = torch.zeros((B, LOUDNESS_STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        if (d_stats.dtype != torch.uint8 or not d_stats.is_contiguous() or not d_stats.is_cuda
                or tuple(d_stats.shape) != (B, LOUDNESS_STATS_DTYPE.itemsize)):
            raise ValueError("Loudness.execute: d_stats is a contiguous uint8 device tensor [B, 32]")
        if d_range is not None and (not torch.is_tensor(d_range) or d_range.dtype != torch.uint8
                                    or not d_range.is_contiguous() or d_range.device != dev
                                    or tuple(d_range.shape) != (B, LOUDNESS_RANGE_DTYPE.itemsize)):
            raise ValueError("Loudness.execute: d_range is a contiguous uint8 device tensor [B, 32]")
        d_len = _device_lengths(lengths, B, dev, "Loudness.execute")
        d_rows, n_index = None, 0
        if rows is not None:
            if torch.is_tensor(rows) and rows.is_cuda:
                d_rows = rows.to(torch.int32).contiguous()
            else:
                host = np.ascontiguousarray(rows, dtype=np.int64)
                if host.ndim != 1 or (len(host) and (host.min() < 0 or host.max() >= B)):
                    raise ValueError("Loudness.execute: rows lie in [0, B)")
                d_rows = torch.from_numpy(host.astype(np.int32)).to(dev)
            n_index = int(d_rows.numel())
            if n_index > B:
                raise ValueError("Loudness.execute: more rows than the batch has")
            if n_index == 0:
                return d_stats
        need = int(lib().mp3g_loudness_scratch_bytes(self._h, B, planes, T))
        if B and need == 0:
            _check(lib().mp3g_loudness_rows(self._h, None, B, planes, T, None, None, 0, None, None, None))
        if self._scratch is None or self._scratch.numel() * 8 < need or self._scratch.device != dev:
            self._scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        self._keep = (d_len, d_rows)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream

        def p(t):
            return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        _check(lib().mp3g_loudness_rows(self._h, p(d_src), B, planes, T, p(d_len), p(d_rows), n_index,
                                        p(self._scratch), p(d_stats), C.c_void_p(stream) if stream else None))
        if d_range is not None and B:
            need = int(lib().mp3g_loudness_range_scratch_bytes(self._h, B, planes, T))
            if (self._range_scratch is None or self._range_scratch.numel() * 8 < need
                    or self._range_scratch.device != dev):
                self._range_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
            _check(lib().mp3g_loudness_range_rows(self._h, B, planes, T, p(d_len), p(d_rows), n_index,
                                                  p(self._scratch), p(self._range_scratch), p(d_range),
                                                  C.c_void_p(stream) if stream else None))
        return d_stats

    @staticmethod
    def stats(t):
        """The records of execute() as a numpy LOUDNESS_STATS_DTYPE array
        (synchronises with the device)."""
        return t.cpu().numpy().reshape(-1).view(LOUDNESS_STATS_DTYPE).copy()

    @staticmethod
    def range_stats(t):
        """The records execute() left in d_range as a numpy
        LOUDNESS_RANGE_DTYPE array (synchronises with the device)."""
        return t.cpu().numpy().reshape(-1).view(LOUDNESS_RANGE_DTYPE).copy()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.shelf = self.highpass = self.V = self.AH = self.G = None
            self._scratch = self._range_scratch = self._keep = None
            lib().mp3g_loudness_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def loudness_gain_host(x, stats, target_lufs, peak_ceiling=None, lengths=None, peaks=None):
    """The reference on the CPU (mp3g_gain_host): (y, gains) with y a copy of
    the float32 array x [B, C, T] or [B, T] whose row b is multiplied over its
    first min(lengths[b], T) samples by gains[b] = float32(sqrt(target energy /
    stats[b].energy)), capped at peak_ceiling / stats[b].peak when a ceiling is
    given; a row of energy 0 is copied and has gain 1.  peaks: float32 [B] that
    takes the place of stats[b].peak (a true peak, say; mp3g_gain_host_peak)."""
    y = np.array(x, dtype=np.float32, order="C", copy=True)
    if y.ndim not in (2, 3):
        raise ValueError("loudness_gain_host: x is [B, C, T] or [B, T]")
    B, T = y.shape[0], y.shape[-1]
    planes = y.shape[1] if y.ndim == 3 else 1
    stats = np.ascontiguousarray(stats, dtype=LOUDNESS_STATS_DTYPE)
    if stats.shape != (B,):
        raise ValueError("loudness_gain_host: one record per row")
    ln = None
    if lengths is not None:
        ln = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64), 0, 2 ** 32 - 1), dtype=np.uint32)
        if ln.shape != (B,):
            raise ValueError("loudness_gain_host: one length per row")
    gains = np.ones(B, np.float32)
    args = (_ptr(y) if y.size else None, B, planes, T, _ptr(ln) if ln is not None and B else None,
            _ptr(stats) if B else None, loudness_target_energy(target_lufs),
            0.0 if peak_ceiling is None else float(peak_ceiling), _ptr(gains) if B else None)
    if peaks is None:
        _check(lib().mp3g_gain_host(*args))
    else:
        peaks = np.ascontiguousarray(peaks, dtype=np.float32)
        if peaks.shape != (B,):
            raise ValueError("loudness_gain_host: one peak per row")
        _check(lib().mp3g_gain_host_peak(*args, _ptr(peaks) if B else None))
    return y, gains


def loudness_gain(d_x, d_stats, target_lufs, peak_ceiling=None, lengths=None, stream=None, d_peak=None):
    """The device call (mp3g_gain_rows): multiplies the contiguous float32
    device tensor d_x [B, C, T] or [B, T] in place, row b over its first
    min(lengths[b], T) samples, by the gain that brings the loudness d_stats
    (Loudness.execute's records) reports to target_lufs, capped so that the
    sample peak stays at or below peak_ceiling when one is given -- as
    loudness_gain_host states it and bit for bit.  One launch, asynchronous on
    `stream` (a hipStream_t; None = the current torch stream).  d_peak: a
    contiguous float32 device tensor [B] that takes the place of the records'
    sample peak (mp3g.true_peak's result, say; mp3g_gain_rows_peak).  Returns
    the gains, a float32 device tensor [B]."""
    import torch
    if (not torch.is_tensor(d_x) or d_x.dtype != torch.float32 or not d_x.is_contiguous() or not d_x.is_cuda
            or d_x.dim() not in (2, 3)):
        raise ValueError("loudness_gain: a contiguous float32 device tensor [B, C, T] or [B, T]")
    B, T = int(d_x.shape[0]), int(d_x.shape[-1])
    planes = int(d_x.shape[1]) if d_x.dim() == 3 else 1
    if (not torch.is_tensor(d_stats) or d_stats.dtype != torch.uint8 or not d_stats.is_contiguous()
            or d_stats.device != d_x.device or tuple(d_stats.shape) != (B, LOUDNESS_STATS_DTYPE.itemsize)):
        raise ValueError("loudness_gain: d_stats is a contiguous uint8 tensor [B, 32] on d_x's device")
    if d_peak is not None and (not torch.is_tensor(d_peak) or d_peak.dtype != torch.float32
                               or not d_peak.is_contiguous() or d_peak.device != d_x.device
                               or tuple(d_peak.shape) != (B,)):
        raise ValueError("loudness_gain: d_peak is a contiguous float32 tensor [B] on d_x's device")
    d_len = _device_lengths(lengths, B, d_x.device, "loudness_gain")
    gains = torch.empty(B, dtype=torch.float32, device=d_x.device)  # (every row's gain is written)
    if stream is None:
        stream = torch.cuda.current_stream(d_x.device).cuda_stream
    args = (d_x.device.index or 0, C.c_void_p(d_x.data_ptr()) if d_x.numel() else None, B, planes,
            T, C.c_void_p(d_len.data_ptr()) if d_len is not None and B else None,
            C.c_void_p(d_stats.data_ptr()) if B else None, loudness_target_energy(target_lufs),
            0.0 if peak_ceiling is None else float(peak_ceiling),
            C.c_void_p(gains.data_ptr()) if B else None, C.c_void_p(stream) if stream else None)
    if d_peak is None:
        _check(lib().mp3g_gain_rows(*args))
    else:
        _check(lib().mp3g_gain_rows_peak(*args, C.c_void_p(d_peak.data_ptr()) if B else None))
    return gains


# ---- true peak of decoded rows (include/mp3g.h) ---------------------------------------
def true_peak_coefs():
    """The interpolator's coefficients, float32 [3, 12]: phases 1..3, delays
    0..11 (mp3g_true_peak_coefs)."""
    q = C.c_void_p()
    _check(lib().mp3g_true_peak_coefs(C.byref(q)))
    return np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_float)), shape=(3, 12)).copy()


def true_peak_tile():
    """The samples of a plane one workgroup of the true-peak kernel takes."""
    return int(lib().mp3g_true_peak_tile())


def true_peak_host(x, lengths=None):
    """The reference on the CPU (mp3g_true_peak_host): the peak of the 4x
    oversampled signal (libebur128's 49-tap interpolator) of every row of the
    float32 array x [B, C, T] (C = 1 or 2) or [B, T], over its first
    min(lengths[b], T) samples.  Returns float32 [B]; 20 log10 of it is dBTP."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim not in (2, 3):
        raise ValueError("true_peak_host: x is [B, C, T] or [B, T]")
    B, T = x.shape[0], x.shape[-1]
    planes = x.shape[1] if x.ndim == 3 else 1
    ln = None
    if lengths is not None:
        ln = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64), 0, 2 ** 32 - 1), dtype=np.uint32)
        if ln.shape != (B,):
            raise ValueError("true_peak_host: one length per row")
    tp = np.zeros(B, np.float32)
    _check(lib().mp3g_true_peak_host(_ptr(x) if x.size else None, B, planes, T,
                                     _ptr(ln) if ln is not None and B else None, _ptr(tp) if B else None))
    return tp


_tp_scratch = {}  # per device: the partial maxima of the last call (grown, never shrunk)
_tp_keep = {}  # per device: the last call's lengths and rows, alive while its launches may run


def true_peak(d_x, lengths=None, rows=None, stream=None, d_out=None):
    """The device call (mp3g_true_peak_rows): the true peak of the rows of the
    contiguous float32 device tensor d_x [B, C, T] (C = 1 or 2) or [B, T], as
    true_peak_host states it and bit for bit.  lengths: one sample count per row
    (a device tensor or array-like; None: T); rows: the rows to measure
    (array-like or an int32 device tensor; None: all).  Returns a float32
    device tensor [B] (d_out when given, else a new zero-filled one): only the
    measured rows' entries are written.  Two launches, asynchronous on `stream`
    (a hipStream_t; None = the current torch stream); the scratch is a tensor
    kept per device, so calls on one device must be stream-ordered."""
    import torch
    if (not torch.is_tensor(d_x) or d_x.dtype != torch.float32 or not d_x.is_contiguous() or not d_x.is_cuda
            or d_x.dim() not in (2, 3)):
        raise ValueError("true_peak: a contiguous float32 device tensor [B, C, T] or [B, T]")
    B, T = int(d_x.shape[0]), int(d_x.shape[-1])
    planes = int(d_x.shape[1]) if d_x.dim() == 3 else 1
    dev = d_x.device
    if d_out is None:
        d_out = torch.zeros(B, dtype=torch.float32, device=dev)
    if (not torch.is_tensor(d_out) or d_out.dtype != torch.float32 or not d_out.is_contiguous()
            or d_out.device != dev or tuple(d_out.shape) != (B,)):
        raise ValueError("true_peak: d_out is a contiguous float32 tensor [B] on d_x's device")
    d_len = _device_lengths(lengths, B, dev, "true_peak")
    d_rows, n_index = None, 0
    if rows is not None:
        if torch.is_tensor(rows) and rows.is_cuda:
            d_rows = rows.to(torch.int32).contiguous()
        else:
            host = np.ascontiguousarray(rows, dtype=np.int64)
            if host.ndim != 1 or (len(host) and (host.min() < 0 or host.max() >= B)):
                raise ValueError("true_peak: rows lie in [0, B)")
            d_rows = torch.from_numpy(host.astype(np.int32)).to(dev)
        n_index = int(d_rows.numel())
        if n_index > B:
            raise ValueError("true_peak: more rows than the batch has")
        if n_index == 0:
            return d_out
    need = int(lib().mp3g_true_peak_scratch_bytes(B, planes, T))
    if B and T and need == 0:
        _check(lib().mp3g_true_peak_rows(dev.index or 0, None, B, planes, T, None, None, 0, None, None, None))
    scratch = _tp_scratch.get(dev)
    if scratch is None or scratch.numel() * 4 < need:
        scratch = _tp_scratch[dev] = torch.empty(max(1, (need + 3) // 4), dtype=torch.float32, device=dev)
    _tp_keep[dev] = (d_len, d_rows)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    _check(lib().mp3g_true_peak_rows(dev.index or 0, p(d_x), B, planes, T, p(d_len), p(d_rows), n_index, p(scratch),
                                     p(d_out), C.c_void_p(stream) if stream else None))
    return d_out


def decode_windows_normalized_tensor(datas, starts, n_samples, target_lufs=-23.0, peak_ceiling=None, rate=None,
                                     mode=MODE_EXACT, out_format=OUT_F32_PLANAR, gapless=False, quality="fast",
                                     n_threads=0, device=0, peak="sample", extended=False, speed=None, gain=None):
    """A windowed decode, its loudness and the gain to target_lufs, all on the
    GPU.  rate=None: decode_windows_tensor, each row measured at its stream's
    own rate (stream_rates; one Loudness and one measurement per distinct
    rate); with a rate: decode_windows_resampled_tensor and one Loudness(rate).
    Every row is measured over its own samples (lengths) and then multiplied in
    place by loudness_gain; target_lufs=None measures only and leaves the batch
    as decoded.  The loudness is that of the WINDOW: a caller who wants a
    file's loudness passes a window that covers the file.  A stream with no
    valid frame is an all-zero row with lufs = -inf and gain 1.

    peak="true": the true peak of every row is measured (mp3g.true_peak: one
    call, the interpolator does not depend on the rate) and peak_ceiling caps
    the gain against it instead of the sample peak -- the ceiling of EBU R128
    and of delivery specifications, in dBTP.  extended=True appends range_stats
    (LOUDNESS_RANGE_DTYPE[B], numpy: Loudness.range_host of the un-normalised
    batch byte for byte) and true_peaks (float32[B], numpy: true_peak_host of
    it bit for bit) to the result; a row no meter measures has -inf maxima,
    lra 0, counts 0 and true peak 0.

    Returns what the underlying call returns -- (batch, lengths, end_status)
    or (batch, lengths, end_status, rates) -- followed by stats
    (LOUDNESS_STATS_DTYPE[B], numpy: Loudness.host of the un-normalised batch
    byte for byte) and gains (float32[B], numpy; ones when only measuring).

    speed, gain: speed and volume perturbation before everything else, one
    entry per stream each (decode_windows_resampled_tensor); starts and
    n_samples then count samples of the perturbed signal."""
    import torch
    if peak not in ("sample", "true"):
        raise ValueError("decode_windows_normalized_tensor: peak is 'sample' or 'true'")
    B = len(datas)
    if rate is None and (speed is not None or gain is not None):
        raise Mp3gError(1, "decode_windows_normalized_tensor: speed and gain need a rate")
    if rate is None:
        res = decode_windows_tensor(datas, starts, n_samples, mode=mode, out_format=out_format, gapless=gapless,
                                    n_threads=n_threads, device=device)
        row_rates = stream_rates(datas, n_threads=n_threads)
    else:
        res = decode_windows_resampled_tensor(datas, starts, n_samples, rate, mode=mode, out_format=out_format,
                                              gapless=gapless, quality=quality, n_threads=n_threads, device=device,
                                              speed=speed, gain=gain)
        row_rates = np.where(res[3] > 0, int(rate), 0)
    batch, lengths = res[0], res[1]
    # a row no Loudness measures keeps this record: the zero row's
    blank = np.zeros(B, LOUDNESS_STATS_DTYPE)
    blank["lufs"] = -np.inf
    d_stats = torch.from_numpy(blank.view(np.uint8).reshape(B, -1).copy()).to(batch.device)
    d_len = torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(batch.device)
    d_range = d_tp = None
    if extended:
        blank_range = np.zeros(B, LOUDNESS_RANGE_DTYPE)
        for name in ("momentary_max", "shortterm_max", "range_lo", "range_hi"):
            blank_range[name] = -np.inf
        d_range = torch.from_numpy(blank_range.view(np.uint8).reshape(B, -1).copy()).to(batch.device)
    meters = {int(f): Loudness(int(f), device=device) for f in set(row_rates.tolist()) if f}
    try:
        for f, m in meters.items():
            m.execute(batch, lengths=d_len, rows=np.nonzero(row_rates == f)[0], d_stats=d_stats, d_range=d_range)
        if (extended or peak == "true") and B:
            # (a row without a frame has length 0: its true peak is 0)
            d_tp = true_peak(batch, lengths=d_len)
        gains = None
        if target_lufs is not None and B:
            gains = loudness_gain(batch, d_stats, target_lufs, peak_ceiling=peak_ceiling, lengths=d_len,
                                  d_peak=d_tp if peak == "true" else None)
        torch.cuda.current_stream(batch.device).synchronize()
    finally:
        for m in meters.values():
            m.close()
    stats = Loudness.stats(d_stats)
    gains = np.ones(B, np.float32) if gains is None else gains.cpu().numpy()
    if not extended:
        return tuple(res) + (stats, gains)
    true_peaks = np.zeros(B, np.float32) if d_tp is None else d_tp.cpu().numpy()
    return tuple(res) + (stats, gains, Loudness.range_stats(d_range), true_peaks)


# ---- room reverberation and noise at an SNR (include/mp3g.h) -------------------
AUGMENT_NORMALIZE = 1
AUGMENT_MAX_SLOTS = 8
AUGMENT_SLOT_DTYPE = np.dtype([("noise_index", "<i4"), ("start", "<u4"), ("offset", "<u4"), ("wrap", "<u4"),
                               ("snr_ratio", "<f8")])
assert AUGMENT_SLOT_DTYPE.itemsize == 24 and C.sizeof(_AugmentArgs) == 104
_AUGMENT_KEYS = ("reverb", "rir_index", "noise", "noise_lengths", "noise_power", "additive", "normalize", "out",
                 "stats", "stream")


class Reverb:
    """A bank of room impulse responses for augment (mp3g_reverb_*): rirs float32
    [R, S] (or one response [S]), rir_lengths the taps of each (None: S), 1 ..
    65,536, at `rate` (20 .. 384000 Hz).  Per response the peak (the first index of the largest
    value), the early window [es, ee) = [peak - rate // 1000, peak + rate // 20)
    cut to the response, and the spectra of its P = ceil(L / 1024) partitions of
    h + i h_early, which one partitioned overlap-save pipeline turns into the
    reverberated signal and the early-reverberation energy.  device=None (or
    -1) makes a host-only object."""

    def __init__(self, rirs, rir_lengths=None, rate=16000, device=0):
        h = np.ascontiguousarray(rirs, dtype=np.float32)
        if h.ndim == 1:
            h = h[None]
        if h.ndim != 2:
            raise ValueError("Reverb: rirs is [R, S] or [S]")
        R, stride = h.shape
        ln = (np.full(R, stride, np.uint32) if rir_lengths is None else
              np.ascontiguousarray(np.clip(np.asarray(rir_lengths, dtype=np.int64), 0, 2 ** 32 - 1), dtype=np.uint32))
        if ln.shape != (R,):
            raise ValueError("Reverb: one length per response")
        self._h = C.c_void_p()
        self.device = -1 if device is None else int(device)
        self.rate = int(rate)
        _check(lib().mp3g_reverb_create(self.device, self.rate, _ptr(h) if h.size else None, R, stride,
                                        _ptr(ln) if R else None, C.byref(self._h)))
        n, lmax, ns = C.c_uint32(), C.c_uint32(), C.c_uint64()
        p = [C.c_void_p() for _ in range(3)]
        _check(lib().mp3g_reverb_info(self._h, C.byref(n), C.byref(lmax), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]),
                                      C.byref(ns)))
        self.n_rirs, self.max_taps, self.n_spectra = n.value, lmax.value, ns.value
        # views of the library's tables: valid while this object lives
        self._table = np.ctypeslib.as_array(C.cast(p[0], C.POINTER(C.c_uint32)), shape=(self.n_rirs, 8))
        self.twiddles = np.ctypeslib.as_array(C.cast(p[1], C.POINTER(C.c_float)), shape=(4096, 2))
        self._spectra = np.ctypeslib.as_array(C.cast(p[2], C.POINTER(C.c_float)), shape=(self.n_spectra, 2))

    def info(self):
        """Per response: L, peak, es, ee, P (int64 arrays [R]) and offset, where
        its first partition's 2,048 slots start in spectra()."""
        t = self._table.astype(np.int64)
        return {"L": t[:, 0], "peak": t[:, 1], "es": t[:, 2], "ee": t[:, 3], "P": t[:, 4],
                "offset": t[:, 6] | (t[:, 7] << 32)}

    def spectra(self):
        """The host copy of the partition spectra, float32 [n_spectra, 2], bins in slot order."""
        return self._spectra.copy()

    def device_spectra(self):
        """What the device holds of them (mp3g_reverb_read_spectra; synchronous)."""
        out = np.empty((self.n_spectra, 2), np.float32)
        _check(lib().mp3g_reverb_read_spectra(self._h, _ptr(out)))
        return out

    def close(self):
        if self._h:
            self._table = self.twiddles = self._spectra = None
            lib().mp3g_reverb_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _row_lengths(lengths, B, what):
    if lengths is None:
        return None
    ln = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64), 0, 2 ** 32 - 1), dtype=np.uint32)
    if ln.shape != (B,):
        raise ValueError(what + ": one length per row")
    return ln


def row_power_host(x, lengths=None):
    """The reference on the CPU (mp3g_row_power_host): sum(v^2) / len of every
    row of the float32 array x [B, T] over its first min(lengths[b], T) samples,
    float64 in include/mp3g.h's blocked order (a row of no samples: 0)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("row_power_host: x is [B, T]")
    B, T = x.shape
    ln = _row_lengths(lengths, B, "row_power_host")
    power = np.zeros(B, np.float64)
    _check(lib().mp3g_row_power_host(_ptr(x) if x.size else None, B, T, _ptr(ln) if ln is not None and B else None,
                                     _ptr(power) if B else None))
    return power


_aug_scratch = {}  # per device: the scratch of the last call (grown, never shrunk)
_aug_keep = {}  # per device: the last call's small tensors, alive while its launches may run


def _scratch_for(dev, need):
    import torch
    scratch = _aug_scratch.get(dev)
    if scratch is None or scratch.numel() * 8 < need:
        if scratch is not None:  # launches of an earlier call, on whatever stream, may still use the old one
            torch.cuda.synchronize(dev)
        scratch = _aug_scratch[dev] = torch.empty(max(1, (need + 7) // 8), dtype=torch.float64, device=dev)
    return scratch


def row_power(d_x, lengths=None, stream=None, d_out=None):
    """The device call (mp3g_row_power_rows): as row_power_host states it and
    bit for bit, of the contiguous float32 device tensor d_x [B, T].  Returns a
    float64 device tensor [B] (d_out when given).  Two launches, asynchronous on
    `stream` (None = the current torch stream); the scratch is a tensor kept per
    device, shared with augment, so calls on one device must be stream-ordered."""
    import torch
    if (not torch.is_tensor(d_x) or d_x.dtype != torch.float32 or not d_x.is_contiguous() or not d_x.is_cuda
            or d_x.dim() != 2):
        raise ValueError("row_power: a contiguous float32 device tensor [B, T]")
    B, T = int(d_x.shape[0]), int(d_x.shape[1])
    dev = d_x.device
    if d_out is None:
        d_out = torch.zeros(B, dtype=torch.float64, device=dev)
    if (not torch.is_tensor(d_out) or d_out.dtype != torch.float64 or not d_out.is_contiguous()
            or d_out.device != dev or tuple(d_out.shape) != (B,)):
        raise ValueError("row_power: d_out is a contiguous float64 tensor [B] on d_x's device")
    d_len = _device_lengths(lengths, B, dev, "row_power")
    need = int(lib().mp3g_row_power_scratch_bytes(B, T))
    scratch = _scratch_for(dev, need)
    _aug_keep[dev] = (d_len,)
    _check(lib().mp3g_row_power_rows(dev.index or 0, _dptr(d_x), B, T, None if d_len is None else _dptr(d_len),
                                     _dptr(scratch), _dptr(d_out), _stream_of(d_x, stream)))
    return d_out


def _augment_slots(additive, B):
    """additive (a dict of [B, A] arrays: index, snr_db, start, offset, wrap) as
    mp3g_augment_slot records [B, A]; snr_ratio = 10^(-snr_db / 10) in float64."""
    if additive is None:
        return np.zeros((B, 0), AUGMENT_SLOT_DTYPE)
    unknown = set(additive) - {"index", "snr_db", "start", "offset", "wrap"}
    if unknown or "index" not in additive:
        raise ValueError("augment: additive holds index and optionally snr_db, start, offset, wrap")
    idx = np.asarray(additive["index"], dtype=np.int64)
    if idx.ndim == 1:
        idx = idx[:, None]
    if idx.ndim != 2 or idx.shape[0] != B:
        raise ValueError("augment: additive arrays are [B, A]")
    s = np.zeros(idx.shape, AUGMENT_SLOT_DTYPE)

    def field(key, dtype):
        v = np.asarray(additive.get(key, 0), dtype=dtype)
        return np.broadcast_to(v[:, None] if v.ndim == 1 and idx.shape[1] != v.shape[0] else v, idx.shape)
    s["noise_index"] = np.clip(idx, -1, 2 ** 31 - 1)
    s["snr_ratio"] = np.power(10.0, -field("snr_db", np.float64) / 10.0)
    for key, name in (("start", "start"), ("offset", "offset")):
        v = field(key, np.int64)
        if (v < 0).any():
            raise ValueError("augment: a negative " + key)
        s[name] = np.minimum(v, 2 ** 32 - 1)
    s["wrap"] = field("wrap", np.int64) != 0
    return s


def augment_host(x, lengths=None, reverb=None, rir_index=None, noise=None, noise_lengths=None, noise_power=None,
                 additive=None, normalize=True):
    """The reference on the CPU (mp3g_augment_host; Kaldi's wav-reverberate is
    the model): x float32 [B, C, T] (C = 1 or 2) or [B, T], over each row's first
    n = min(lengths[b], T) samples.  Row b is convolved with response
    rir_index[b] of `reverb` (< 0 or None: none) and shifted by the response's
    peak, so the length stays n; then for each slot of additive (a dict of
    [B, A] arrays, A <= 8: index into the float32 noise bank noise [M, Tn], < 0:
    none; snr_db; start in output samples; offset into the noise; wrap) the
    noise is added with the gain sqrt(10^(-snr_db / 10) signal_power /
    noise_power), signal_power the EARLY reverberation's (the row's own power
    without a response) and noise_power [M] row_power_host of the bank unless
    given; with normalize the result is scaled back to the row's power.  Every
    plane gets the row's response and noises; the powers are per plane.
    Returns (out like x, +0 past n; stats float64 [B, C, 4] or [B, 4]:
    power_before, signal_power, power_after, scale)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim not in (2, 3):
        raise ValueError("augment_host: x is [B, C, T] or [B, T]")
    B, T = x.shape[0], x.shape[-1]
    planes = x.shape[1] if x.ndim == 3 else 1
    ln = _row_lengths(lengths, B, "augment_host")
    ri = None
    if rir_index is not None:
        ri = np.ascontiguousarray(np.clip(np.asarray(rir_index, dtype=np.int64), -1, 2 ** 31 - 1), dtype=np.int32)
        if ri.shape != (B,):
            raise ValueError("augment_host: one rir_index per row")
    nz = nl = npow = None
    if noise is not None:
        nz = np.ascontiguousarray(noise, dtype=np.float32)
        if nz.ndim != 2:
            raise ValueError("augment_host: noise is [M, Tn]")
        nl = _row_lengths(np.full(len(nz), nz.shape[1]) if noise_lengths is None else noise_lengths, len(nz),
                          "augment_host (noise)")
        npow = (row_power_host(nz, nl) if noise_power is None else
                np.ascontiguousarray(noise_power, dtype=np.float64))
        if npow.shape != (len(nz),):
            raise ValueError("augment_host: one noise_power per noise")
    slots = _augment_slots(additive, B)
    out = np.zeros_like(x)
    stats = np.zeros((B, planes, 4), np.float64)
    a = _AugmentArgs()
    a.x, a.out, a.lengths, a.rir_index = _ptr(x) if x.size else None, _ptr(out) if x.size else None, _ptr(ln), _ptr(ri)
    if nz is not None and len(nz):
        a.noise, a.noise_lengths, a.noise_power = _ptr(nz) if nz.size else None, _ptr(nl), _ptr(npow)
        a.n_noise, a.Tn = nz.shape
    a.slots = _ptr(slots) if slots.size else None
    a.stats = _ptr(stats) if stats.size else None
    a.n_rows, a.n_planes, a.T, a.A = B, planes, T, slots.shape[1]
    a.flags = AUGMENT_NORMALIZE if normalize else 0
    _check(lib().mp3g_augment_host(reverb._h if reverb is not None else None, C.byref(a)))
    return out, (stats if x.ndim == 3 else stats[:, 0])


def augment(d_x, lengths=None, reverb=None, rir_index=None, noise=None, noise_lengths=None, noise_power=None,
            additive=None, normalize=True, out=None, stats=None, stream=None, _launch=None):
    """The device call (mp3g_augment_rows): as augment_host states it and bit
    for bit, out and stats, from the contiguous float32 device tensor d_x
    [B, C, T] or [B, T] into `out` (another tensor like it, not overlapping;
    made here when None).  noise is a float32 device tensor [M, Tn] (an array is
    uploaded), noise_power a float64 device tensor [M] (None: row_power of the
    bank); lengths as for true_peak; rir_index, noise_lengths and additive are
    host arrays, uploaded here.  Five launches whose shapes depend on B, C, T
    and the bank's longest response only, asynchronous on `stream` (None = the
    current torch stream); the scratch is a tensor kept per device, so calls on
    one device must be stream-ordered (a call that needs a larger one
    synchronises the device before the old one is released).  Returns (out, stats float64 device
    tensor [B, C, 4] or [B, 4])."""
    import torch
    if (not torch.is_tensor(d_x) or d_x.dtype != torch.float32 or not d_x.is_contiguous() or not d_x.is_cuda
            or d_x.dim() not in (2, 3)):
        raise ValueError("augment: a contiguous float32 device tensor [B, C, T] or [B, T]")
    B, T = int(d_x.shape[0]), int(d_x.shape[-1])
    planes = int(d_x.shape[1]) if d_x.dim() == 3 else 1
    dev = d_x.device
    if out is None:
        out = torch.empty_like(d_x)
    if (not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or out.shape != d_x.shape
            or out.device != dev):
        raise ValueError("augment: out is a contiguous float32 tensor like d_x")
    stats_shape = (B, planes, 4) if d_x.dim() == 3 else (B, 4)
    if stats is None:
        stats = torch.zeros(stats_shape, dtype=torch.float64, device=dev)
    if (not torch.is_tensor(stats) or stats.dtype != torch.float64 or not stats.is_contiguous()
            or tuple(stats.shape) != stats_shape or stats.device != dev):
        raise ValueError("augment: stats is a contiguous float64 tensor [B, C, 4] (or [B, 4]) on d_x's device")
    d_len = _device_lengths(lengths, B, dev, "augment")
    ri = d_ri = None
    if rir_index is not None:
        ri = np.ascontiguousarray(np.clip(np.asarray(rir_index, dtype=np.int64), -1, 2 ** 31 - 1), dtype=np.int32)
        if ri.shape != (B,):
            raise ValueError("augment: one rir_index per row")
        d_ri = torch.from_numpy(ri).to(dev)
    nl = d_nl = d_np = None
    M = Tn = 0
    if noise is not None:
        if not torch.is_tensor(noise):
            noise = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).to(dev)
        if (noise.dtype != torch.float32 or not noise.is_contiguous() or noise.device != dev or noise.dim() != 2):
            raise ValueError("augment: noise is a contiguous float32 tensor [M, Tn] on d_x's device")
        M, Tn = int(noise.shape[0]), int(noise.shape[1])
        nl = _row_lengths(np.full(M, Tn) if noise_lengths is None else noise_lengths, M, "augment (noise)")
        nl = np.minimum(nl, Tn)
        d_nl = torch.from_numpy(nl.astype(np.int32)).to(dev)
        if noise_power is None:
            d_np = row_power(noise, d_nl, stream=stream)
        elif torch.is_tensor(noise_power):
            d_np = noise_power
        else:
            d_np = torch.from_numpy(np.ascontiguousarray(noise_power, dtype=np.float64)).to(dev)
        if (d_np.dtype != torch.float64 or not d_np.is_contiguous() or d_np.device != dev
                or tuple(d_np.shape) != (M,)):
            raise ValueError("augment: noise_power is a contiguous float64 tensor [M] on d_x's device")
    slots = _augment_slots(additive, B)
    d_slots = torch.from_numpy(slots.view(np.uint8).reshape(-1).copy()).to(dev) if slots.size else None
    h = reverb._h if reverb is not None else None
    need = int(lib().mp3g_reverb_scratch_bytes(h, B, planes, T))
    scratch = _scratch_for(dev, need)
    _aug_keep[dev] = (d_len, d_ri, d_nl, d_np, d_slots, noise)

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    a = _AugmentArgs()
    a.x, a.out, a.lengths, a.rir_index = p(d_x), p(out), p(d_len), p(d_ri)
    if M:
        a.noise, a.noise_lengths, a.noise_power = p(noise), p(d_nl), p(d_np)
        a.n_noise, a.Tn = M, Tn
    a.slots, a.stats = p(d_slots), p(stats)
    a.n_rows, a.n_planes, a.T, a.A = B, planes, T, slots.shape[1]
    a.flags = AUGMENT_NORMALIZE if normalize else 0
    call = (h, dev.index or 0, C.byref(a), _ptr(ri), _ptr(nl) if M else None, _ptr(slots) if slots.size else None,
            p(scratch), scratch.numel() * 8, _stream_of(d_x, stream))
    if _launch is None:
        _check(lib().mp3g_augment_rows(*call))
    else:  # (diagnostic: one launch of the five, for timing)
        _check(lib().mp3g_augment_debug_launch(*call, int(_launch)))
    return out, stats


def decode_windows_augmented_tensor(datas, starts, n_samples, rate, mode=MODE_EXACT, out_format=OUT_F32_PLANAR,
                                    gapless=False, quality="fast", n_threads=0, device=0, speed=None, gain=None,
                                    **augment_keywords):
    """decode_windows_resampled_tensor, then augment on its batch and lengths
    with the keywords of augment (reverb, rir_index, noise, noise_lengths,
    noise_power, additive, normalize, out, stats, stream): the augmented
    training batch at one sample rate with no copy to the host; it equals
    augment_host of the resampled tensor bit for bit.  Returns (out, lengths,
    end_status, rates, stats).  Without any augment keyword it is
    decode_windows_resampled_tensor, and returns what that returns.

    speed, gain: speed and volume perturbation before everything else, one
    entry per stream each (decode_windows_resampled_tensor); starts and
    n_samples then count samples of the perturbed signal."""
    unknown = set(augment_keywords) - set(_AUGMENT_KEYS)
    if unknown:
        raise TypeError("decode_windows_augmented_tensor: unknown keyword " + sorted(unknown)[0])
    res = decode_windows_resampled_tensor(datas, starts, n_samples, rate, mode=mode, out_format=out_format,
                                          gapless=gapless, quality=quality, n_threads=n_threads, device=device,
                                          speed=speed, gain=gain)
    if not augment_keywords:
        return res
    out, stats = augment(res[0], res[1], **augment_keywords)
    return (out,) + tuple(res[1:]) + (stats,)


# ---- STFT and mel spectrograms of decoded rows (include/mp3g.h) ----------------
STFT_CENTER = 1
STFT_MEL_HTK = 2
STFT_MEL_NORM = 4
STFT_OUTPUTS = {"complex": 0, "power": 1, "magnitude": 2}
STFT_LOGS = {None: 0, "ln": 1, "log10": 2}


class STFT:
    """STFT and mel spectrograms of float32 rows (mp3g_stft_*): a Hann-windowed
    STFT by FFT for n_fft in {256, .., 4096}, stored as "complex" bins, "power"
    or "magnitude", optionally through a mel filter bank (n_mels > 0; Slaney's
    scale or htk, norm = Slaney's area normalisation) and a logarithm (log =
    "ln" or "log10" of max(value, floor)).  The transform is one fixed network
    of float32 butterflies that host and device both compile, so the device call
    (execute) equals the host reference (host) bit for bit.  device=None (or -1)
    makes a host-only object; fmax=0 means rate / 2; win_length=None means
    n_fft."""

    def __init__(self, rate, n_fft=2048, hop=512, win_length=None, output="power", n_mels=0, fmin=0.0, fmax=0.0,
                 htk=False, norm=True, log=None, floor=None, center=True, device=None):
        self._h = C.c_void_p()
        if output not in STFT_OUTPUTS or log not in STFT_LOGS:
            raise Mp3gError(1, "STFT: output is complex, power or magnitude; log is None, ln or log10")
        self.device = -1 if device is None else int(device)
        self.rate, self.n_fft, self.hop, self.n_mels = int(rate), int(n_fft), int(hop), int(n_mels)
        self.win_length = self.n_fft if win_length is None else int(win_length)
        self.output, self.log, self.floor = output, log, floor
        self.center, self.htk, self.norm = bool(center), bool(htk), bool(norm)
        self.flags = (STFT_CENTER if center else 0) | (STFT_MEL_HTK if htk else 0) | (STFT_MEL_NORM if norm else 0)
        _check(lib().mp3g_stft_create(self.device, self.rate, self.n_fft, self.win_length, self.hop,
                                      STFT_OUTPUTS[output], self.n_mels, float(fmin), float(fmax), STFT_LOGS[log],
                                      0.0 if floor is None else float(floor), self.flags, C.byref(self._h)))
        k, t = C.c_uint32(), C.c_uint32()
        p = [C.c_void_p() for _ in range(4)]
        _check(lib().mp3g_stft_info(self._h, C.byref(k), *[C.byref(q) for q in p], C.byref(t)))
        self.K, self.tile_frames = k.value, t.value
        self.pad = self.n_fft // 2 if center else 0
        self.complex = output == "complex"
        self.bins = self.n_mels or self.K

        def view(q, ctype, shape):  # a view of the library's table: valid while this object lives
            return np.ctypeslib.as_array(C.cast(q, C.POINTER(ctype)), shape=shape)
        self.window = view(p[0], C.c_float, (self.n_fft,))
        self.twiddles = view(p[1], C.c_float, (self.n_fft, 2))
        self.wm = view(p[2], C.c_float, (self.n_mels, self.K)) if self.n_mels else None
        self.support = view(p[3], C.c_uint32, (self.n_mels, 2)) if self.n_mels else None

    def frames(self, T):
        """The frames a row of T samples has (mp3g_stft_frames)."""
        return int(lib().mp3g_stft_frames(self._h, int(T)))

    def host(self, x, n_frames=None, frame_stride=None):
        """The reference on the CPU (mp3g_stft_host): [bins, n_frames] float32 of
        the float32 row x (n_frames: all by default), complex64 for "complex";
        with a frame_stride the full [bins, frame_stride] buffer, zeros where
        nothing is written."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.frames(len(x)) if n_frames is None else int(n_frames)
        stride = n if frame_stride is None else int(frame_stride)
        out = np.zeros((self.bins, max(stride, 0)) + ((2,) if self.complex else ()), np.float32)
        _check(lib().mp3g_stft_host(self._h, _ptr(x) if len(x) else None, len(x), n, _ptr(out) if out.size else None,
                                    stride))
        return out.view(np.complex64)[..., 0] if self.complex else out

    def execute(self, d_src, d_out=None, n_frames=None, stream=None):
        """The device call (mp3g_stft_execute): d_src float32 [B, C, T] (C = 1 or
        2) or [B, T], contiguous on this object's device; d_out float32 [B, (C,)
        bins, S] -- "complex": [B, (C,) K, S, 2] -- with S >= n_frames (made
        here when None: S = n_frames, all frames by default).  Writes n_frames
        entries of each bin row, nothing else.  One launch, asynchronous on
        `stream` (a hipStream_t; None = the current torch stream).  Returns
        d_out, for "complex" as a complex64 view [B, (C,) K, S]."""
        import torch
        if d_src.dtype != torch.float32 or not d_src.is_contiguous() or d_src.dim() not in (2, 3) or not d_src.is_cuda:
            raise ValueError("STFT.execute: a contiguous float32 device tensor [B, C, T] or [B, T]")
        B, T = int(d_src.shape[0]), int(d_src.shape[-1])
        planes = int(d_src.shape[1]) if d_src.dim() == 3 else 1
        n = self.frames(T) if n_frames is None else int(n_frames)
        lead = (B, planes) if d_src.dim() == 3 else (B,)
        tail = (2,) if self.complex else ()
        if d_out is None:
            d_out = torch.empty(lead + (self.bins, n) + tail, dtype=torch.float32, device=d_src.device)
        if d_out.is_complex():
            d_out = torch.view_as_real(d_out)
        S = int(d_out.shape[len(lead) + 1]) if d_out.dim() == len(lead) + 2 + len(tail) else -1
        if (d_out.dtype != torch.float32 or not d_out.is_contiguous() or not d_out.is_cuda
                or tuple(d_out.shape) != lead + (self.bins, S) + tail):
            raise ValueError("STFT.execute: d_out is a contiguous float32 device tensor [B, (C,) bins, S(, 2)]")
        if stream is None:
            stream = torch.cuda.current_stream(d_src.device).cuda_stream
        _check(lib().mp3g_stft_execute(self._h, C.c_void_p(d_src.data_ptr()) if d_src.numel() else None, B, planes, T,
                                       C.c_void_p(d_out.data_ptr()) if d_out.numel() else None, n, S,
                                       C.c_void_p(stream) if stream else None))
        return torch.view_as_complex(d_out) if self.complex else d_out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.window = self.twiddles = self.wm = self.support = None
            lib().mp3g_stft_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_windows_stft_tensor(datas, starts, n_samples, rate, n_fft=2048, hop=512, win_length=None, output="power",
                               n_mels=0, fmin=0.0, fmax=0.0, htk=False, norm=True, log=None, floor=None, center=True,
                               n_frames=None, mode=MODE_EXACT, out_format=OUT_F32_MONO, gapless=False, quality="fast",
                               n_threads=0, device=0, speed=None, gain=None, spec_augment=None):
    """decode_windows_resampled_tensor followed by one STFT.execute on the same
    torch stream: the spectrogram (or mel spectrogram) of each stream's window
    [starts[k], starts[k] + n_samples) at `rate`, zero padding included.  F =
    n_frames, by default n_samples // hop with center (which drops the last
    frame, as decode_windows_logmel_tensor does) and every frame without.

    Returns (features, frame_lengths, end_status, rates): features [B, bins, F]
    (OUT_F32_MONO) or [B, 2, bins, F] (OUT_F32_PLANAR) on cuda:device, float32
    or, for output="complex", complex64; equal to STFT.host on the rows of
    decode_windows_resampled_tensor bit for bit; frame_lengths int64[B] = min(F,
    ceil(lengths / hop)), the frames that start inside each stream's valid
    samples.

    speed, gain: speed and volume perturbation before everything else, one
    entry per stream each (decode_windows_resampled_tensor); starts and
    n_samples then count samples of the perturbed signal.

    spec_augment: None, or SpecAugment of the float32 features in the
    frequency-major layout (spec_augment with freq_major=True) on the same
    stream, as for decode_windows_logmel_tensor; complex output is refused."""
    import torch
    if spec_augment is not None and output == "complex":
        raise Mp3gError(1, "decode_windows_stft_tensor: spec_augment needs a float32 output, not 'complex'")
    st = STFT(rate, n_fft, hop, win_length, output, n_mels, fmin, fmax, htk, norm, log, floor, center, device=device)
    try:
        T = int(n_samples)
        avail = st.frames(T)
        F = (min(avail, T // st.hop) if center else avail) if n_frames is None else int(n_frames)
        if F < 0 or F > avail:
            raise Mp3gError(1, "more frames than a row of n_samples has")
        batch, lengths, end_status, rates = decode_windows_resampled_tensor(
            datas, starts, T, rate, mode=mode, out_format=out_format, gapless=gapless, quality=quality,
            n_threads=n_threads, device=device, speed=speed, gain=gain)
        feats = st.execute(batch, n_frames=F)
        flen = np.minimum(F, -(-lengths // st.hop))
        if spec_augment is not None:
            feats = _specaug_after("decode_windows_stft_tensor", feats, flen, spec_augment, int(feats.shape[-2]), True)
        torch.cuda.current_stream(feats.device).synchronize()
    finally:
        st.close()
    return feats, flen, end_status, rates


def _host_buffer(out, want_int16, want_float32=False):
    """(pointer, size in bytes) of a caller's writable, C-contiguous HOST
    buffer -- a numpy array or a CPU torch tensor (pinned or not).  The
    library writes host memory through the pointer, so device tensors,
    non-contiguous views and read-only arrays are refused, and so is any
    dtype but int16 (or float32, for the float output formats) where the PCM
    is addressed in samples."""
    if hasattr(out, "data_ptr"):  # torch.Tensor
        if out.device.type != "cpu":
            raise ValueError("output buffer must be in host memory (got a %s tensor)" % out.device)
        if not out.is_contiguous():
            raise ValueError("output buffer must be contiguous")
        if want_int16 and str(out.dtype) != "torch.int16":
            raise ValueError("output buffer must be int16 (got %s)" % out.dtype)
        if want_float32 and str(out.dtype) != "torch.float32":
            raise ValueError("output buffer must be float32 (got %s)" % out.dtype)
        return out.data_ptr(), out.numel() * out.element_size()
    a = out
    if not isinstance(a, np.ndarray):
        raise TypeError("output buffer must be a numpy array or a torch tensor")
    if not a.flags.c_contiguous or not a.flags.writeable:
        raise ValueError("output buffer must be C-contiguous and writable")
    if want_int16 and a.dtype != np.int16:
        raise ValueError("output buffer must be int16 (got %s)" % a.dtype)
    if want_float32 and a.dtype != np.float32:
        raise ValueError("output buffer must be float32 (got %s)" % a.dtype)
    return a.ctypes.data, a.nbytes


def decode_streams_into(datas, out, mode=MODE_EXACT, n_threads=0, n_groups=0, device=0, out_format=OUT_S16):
    """Pipelined bitstreams-in, PCM-out (mp3g_decode_streams_into_out): groups
    of streams, each group's host scan overlapping the previous group's
    transfers and kernels.  `out` is a writable, C-contiguous host buffer
    (numpy array or a pinned CPU torch tensor) of the format's dtype -- int16
    for OUT_S16 / OUT_S16_MONO, float32 otherwise -- and of at least
    out_bytes_per_granule(out_format) * (total granules) bytes; the layout
    comes from a header-only pre-pass: stream k starts at granule slot
    streams[k].first_granule.  Returns (n_granules, streams, end_status)."""
    bpg = out_bytes_per_granule(out_format)
    if not bpg:
        raise Mp3gError(1, "unknown output format")
    bufs, ptrs, lens = _stream_args(datas)
    streams = np.zeros(len(datas), STREAM_DTYPE)
    status = np.zeros(max(1, len(datas)), np.int32)
    n = C.c_uint64()
    ptr, nbytes = _host_buffer(out, want_int16=out_format in _OUT_INT16, want_float32=out_format not in _OUT_INT16)
    cap = nbytes // bpg
    if out_format == OUT_S16 and not hasattr(lib(), "mp3g_decode_streams_into_out"):  # (an older build: A/B runs)
        _check(lib().mp3g_decode_streams_into(device, len(datas), ptrs, lens, n_threads, mode, n_groups,
                                              C.c_void_p(ptr), cap, C.byref(n), _ptr(streams), _ptr(status)))
        return n.value, streams, status[:len(datas)]
    _check(lib().mp3g_decode_streams_into_out(device, len(datas), ptrs, lens, n_threads, mode, n_groups,
                                              C.c_void_p(ptr), int(out_format), cap, C.byref(n), _ptr(streams),
                                              _ptr(status)))
    return n.value, streams, status[:len(datas)]


def clock_probe(d_flag, d_out, n_waves=8, max_ms=5000, stream=None, device=0):
    """mp3g_debug_clock_probe (diagnostic): n_waves one-wave workgroups spin on
    `stream` until the int32 device word d_flag turns non-zero (or max_ms
    pass), writing (s_memtime, s_memtime, s_memrealtime, s_memrealtime, seen)
    at both ends of their window into the int64 device tensor d_out
    (5 x n_waves).  Asynchronous: set the flag from another stream after the
    work whose clock is measured."""
    if d_out.numel() < 5 * n_waves or d_out.element_size() != 8 or d_flag.element_size() != 4:
        raise ValueError("clock_probe: d_out needs 5 x n_waves int64, d_flag one int32")
    _check(lib().mp3g_debug_clock_probe(device, C.c_void_p(d_flag.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                        n_waves, max_ms, C.c_void_p(stream or 0)))


class Decoder:
    """mp3.Decoder (reference decode.go:27-388) backed by the GPU path.

    read(n) -> (status, bytes): status 0 with >= 1 byte, 7 (EOF) or an error
    status, like Decoder.Read.  seek(off, whence) -> (status, newpos)."""

    def __init__(self, data: bytes, seekable=True, mode=MODE_EXACT, device=0):
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        self._h = C.c_void_p()
        _check(lib().mp3g_decoder_new(_ptr(buf), len(data), int(seekable), device, mode, C.byref(self._h)))

    @classmethod
    def from_reader(cls, read, seek=None, mode=MODE_EXACT, device=0):
        """mp3.NewDecoder(r) on a streaming source (mp3g_decoder_new_reader):
        read(n) -> bytes (io.Reader.Read: 1..n bytes, b"" = io.EOF, an
        exception = a reader error); seek(offset, whence) -> new offset, or
        None when the source is no io.Seeker.  Returns once the tags and frame
        0 are in (non-seekable) -- the decoder pulls the rest as Read needs it."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.read_errors = []

        def _read(_user, buf, cap):
            # (everything inside the try: an exception escaping a ctypes
            # callback would return 0, a silent EOF)
            try:
                b = read(int(cap))
                if not isinstance(b, (bytes, bytearray, memoryview)):
                    raise TypeError(f"read() returned {type(b).__name__}, not bytes")
                if len(b) > int(cap):
                    raise ValueError(f"read({int(cap)}) returned {len(b)} bytes")
                k = len(b)
                if k:
                    C.memmove(buf, bytes(b), k)
                return k
            except Exception as e:  # a reader error: the decoder returns MP3G_ERR_READ
                self.read_errors.append(e)
                return -1

        def _seek(_user, off, whence):
            try:
                return int(seek(int(off), int(whence)))
            except Exception as e:  # the Seeker's error: MP3G_ERR_READ
                self.read_errors.append(e)
                return -1

        # the callbacks must outlive the decoder
        self._cb = (READ_FN(_read), SEEK_FN(_seek) if seek is not None else SEEK_FN())
        r = _Reader(self._cb[0], self._cb[1], None)
        _check(lib().mp3g_decoder_new_reader(C.byref(r), device, mode, C.byref(self._h)))
        return self

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().mp3g_decoder_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def read(self, n):
        out = np.zeros(max(n, 1), np.uint8)
        k = C.c_size_t()
        st = lib().mp3g_decoder_read(self._h, _ptr(out), n, C.byref(k))
        return st, out[:k.value].tobytes()

    def read_full(self, out):
        """io.ReadFull into a writable, C-contiguous host buffer (numpy array
        or CPU torch tensor of any dtype; filled as bytes): (status, bytes delivered)."""
        ptr, cap = _host_buffer(out, want_int16=False)
        k = C.c_size_t()
        st = lib().mp3g_decoder_read_full(self._h, C.c_void_p(ptr), cap, C.byref(k))
        return st, k.value

    def read_all(self):
        chunks = []
        while True:
            st, b = self.read(1 << 16)
            if st != 0:
                return st, b"".join(chunks)
            chunks.append(b)

    def seek(self, off, whence=0):
        np_ = C.c_int64()
        st = lib().mp3g_decoder_seek(self._h, off, whence, C.byref(np_))
        return st, np_.value

    def _info(self):
        sr, ln, bpf, pos = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().mp3g_decoder_info(self._h, C.byref(sr), C.byref(ln), C.byref(bpf), C.byref(pos)))
        return sr.value, ln.value, bpf.value, pos.value

    sample_rate = property(lambda self: self._info()[0])
    length = property(lambda self: self._info()[1])
    bytes_per_frame = property(lambda self: self._info()[2])
    pos = property(lambda self: self._info()[3])
    duration_ns = property(lambda self: lib().mp3g_decoder_duration_ns(self._h))
    position_ns = property(lambda self: lib().mp3g_decoder_position_ns(self._h))
    remaining_ns = property(lambda self: lib().mp3g_decoder_remaining_ns(self._h))
    progress = property(lambda self: lib().mp3g_decoder_progress(self._h))
    sample_position = property(lambda self: lib().mp3g_decoder_sample_position(self._h))
    sample_count = property(lambda self: lib().mp3g_decoder_sample_count(self._h))

    def seek_to_sample(self, s):
        return lib().mp3g_decoder_seek_to_sample(self._h, s)

    def seek_to_time_ns(self, t):
        return lib().mp3g_decoder_seek_to_time_ns(self._h, t)

    def skip_ns(self, d):
        return lib().mp3g_decoder_skip_ns(self._h, d)


class Plan:
    """Device-resident plan (mp3g_plan_*): execute on device pointers / torch tensors."""

    @staticmethod
    def chunks(c):
        """granules_per_chunk value for about c chunks in total (MP3G_PLAN_CHUNKS)."""
        return 0x80000000 | int(c)

    def __init__(self, streams, granules_per_chunk=0, mode=MODE_EXACT, device=0):
        streams = np.ascontiguousarray(streams, dtype=STREAM_DTYPE)
        self._h = C.c_void_p()
        self.device = device
        _check(lib().mp3g_plan_create(device, _ptr(streams), len(streams), granules_per_chunk,
                                      mode, C.byref(self._h)))

    def info(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().mp3g_plan_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"chunks": a.value, "granules": b.value, "halo_granules": c.value}

    def execute(self, d_gran, d_coef, d_pcm, d_state_in=None, d_state_out=None, stream=None, out_format=OUT_S16):
        """Pointers are ints (device addresses) or torch tensors; stream: hipStream_t int.
        out_format: OUT_* -- d_pcm holds out_bytes_per_granule(out_format) bytes per
        granule slot (mp3g_plan_execute_out)."""
        def p(x):
            if x is None:
                return None
            return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        if out_format == OUT_S16:
            _check(lib().mp3g_plan_execute(self._h, p(d_gran), p(d_coef), p(d_state_in),
                                           p(d_state_out), p(d_pcm),
                                           C.c_void_p(stream) if stream else None))
        else:
            _check(lib().mp3g_plan_execute_out(self._h, p(d_gran), p(d_coef), p(d_state_in),
                                               p(d_state_out), p(d_pcm), int(out_format),
                                               C.c_void_p(stream) if stream else None))

    def synth_execute(self, d_gran, d_lines, d_pcm, d_state_in=None, d_state_out=None, stream=None):
        """Standalone polyphase synthesis (mp3g_plan_synth_execute, frame.go:630-688) on
        float32 frequency-inverted lines [n, 2, 576]; fast-mode plans only."""
        def p(x):
            if x is None:
                return None
            return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        _check(lib().mp3g_plan_synth_execute(self._h, p(d_gran), p(d_lines), p(d_state_in),
                                             p(d_state_out), p(d_pcm),
                                             C.c_void_p(stream) if stream else None))

    def hot_stats(self, reset=False):
        """Fast plans created with FLAG_HOT_STATS: the hot-granule fallback's
        work summed over this plan's launches (mp3g_plan_hot_stats,
        synchronous): granules whose PCM the reference-order pass rewrites,
        hot zones, hot granules the fast pass flagged, granules re-run inside
        a chunk's own wave (zones beyond the plan's zone list)."""
        out = (C.c_uint64 * 4)()
        _check(lib().mp3g_plan_hot_stats(self._h, out, 1 if reset else 0))
        return {"rewritten": out[0], "zones": out[1], "hot": out[2], "in_wave": out[3]}

    PHASES = ("params", "requantize", "stereo+antialias", "imdct", "S rows (transpose)",
              "dct32 (matrixing)", "window+store", "history")

    def debug_phases(self, d_gran, d_coef, d_pcm, stream=None):
        """Diagnostic (fast plans): summed shader cycles per kernel phase."""
        out = (C.c_uint64 * 8)()
        p = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        _check(lib().mp3g_plan_debug_phases(self._h, p(d_gran), p(d_coef), p(d_pcm), out,
                                            C.c_void_p(stream) if stream else None))
        return dict(zip(self.PHASES, list(out)))

    def debug_timeline(self, d_gran, d_coef, d_pcm, stream=None):
        """Diagnostic (fast plans): [chunks, 4] s_memrealtime ticks (100 MHz) of
        each wave at entry, loop start, loop end, exit."""
        n = self.info()["chunks"]
        out = (C.c_uint64 * max(1, 4 * n))()
        p = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        _check(lib().mp3g_plan_debug_timeline(self._h, p(d_gran), p(d_coef), p(d_pcm), out,
                                              C.c_void_p(stream) if stream else None))
        return np.frombuffer(out, dtype=np.uint64)[:4 * n].reshape(n, 4).copy()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().mp3g_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WindowPlan(Plan):
    """Plan over windowed runs (mp3g_plan_create_windows): streams / rows as
    scan_windows returns them, T the row length in samples."""

    def __init__(self, streams, rows, T, granules_per_chunk=0, mode=MODE_EXACT, device=0):
        streams = np.ascontiguousarray(streams, dtype=STREAM_DTYPE)
        rows = np.ascontiguousarray(rows, dtype=WINDOW_ROW_DTYPE)
        if len(rows) != len(streams):
            raise ValueError("WindowPlan: one row per stream")
        self._h = C.c_void_p()
        self.device = device
        _check(lib().mp3g_plan_create_windows(device, _ptr(streams), _ptr(rows), len(streams), int(T),
                                              granules_per_chunk, mode, C.byref(self._h)))

    def execute(self, d_gran, d_coef, d_out, stream=None, out_format=OUT_F32_PLANAR):
        """d_out: float32 [B, 2, T] (OUT_F32_PLANAR) or [B, T] (OUT_F32_MONO) on
        the device; only the rows' n_valid samples are written
        (mp3g_plan_execute_windows)."""
        def p(x):
            return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        _check(lib().mp3g_plan_execute_windows(self._h, p(d_gran), p(d_coef), p(d_out), int(out_format),
                                               C.c_void_p(stream) if stream else None))
