"""ctypes mirror of include/tbf.h (the drop-in C-ABI)."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from .params import LIMIT_METER_DTYPE, MIX_ROW_DTYPE

# TBF_LIB overrides the library path (build variants for A/B measurements)
LIB_PATH = Path(os.environ.get("TBF_LIB", Path(__file__).resolve().parent / "libtbf.so"))

_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_u32p = C.POINTER(C.c_uint32)


# the render kernels of one launch chunk, in stream order (tbf_debug_kernel_times)
STAGES = ("k_tonegen", "k_mixpre", "k_rv_pre", "k_rv_core", "k_rv_post", "k_whirl")


class TbfError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("device", C.c_int32), ("chain_mode", C.c_uint32),
                ("debug_flags", C.c_uint32), ("whirl_out", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RotorOut(C.Structure):
    """tbf_rotor_out: the four planes of a rotor render and their common stride (in floats)"""
    _fields_ = [("hornL", C.c_void_p), ("hornR", C.c_void_p), ("drumL", C.c_void_p), ("drumR", C.c_void_p),
                ("stride", C.c_uint64)]


class CabinetOut(C.Structure):
    """tbf_cabinet_out: the mixed pair, the optional wet pair and their common stride (in floats)"""
    _fields_ = [("L", C.c_void_p), ("R", C.c_void_p), ("wetL", C.c_void_p), ("wetR", C.c_void_p),
                ("stride", C.c_uint64)]


class ResampledOut(C.Structure):
    """tbf_resampled_out: the converted pair, the optional engine-rate pair, their strides (in
    floats) and the host array of counts"""
    _fields_ = [("L", C.c_void_p), ("R", C.c_void_p), ("rawL", C.c_void_p), ("rawR", C.c_void_p),
                ("stride", C.c_uint64), ("raw_stride", C.c_uint64), ("counts", C.c_void_p)]


class PcmOut(C.Structure):
    """tbf_pcm_out: the frames and their row stride in bytes, the optional meters, the format and
    flags, and the dither's seed and frame numbering"""
    _fields_ = [("out", C.c_void_p), ("out_stride_bytes", C.c_uint64), ("meters", C.c_void_p), ("format", C.c_uint32),
                ("flags", C.c_uint32), ("seed", C.c_uint32), ("frame0", C.c_uint64), ("row_frame0", C.c_void_p)]


# tbf_pcm_out.format / .flags (include/tbf.h TBF_PCM_*), bytes per frame by format, and tbf_pcm_meter
PCM_S16, PCM_S24_3LE, PCM_F32 = 0, 1, 2
PCM_DITHER = 1
PCM_FRAME_BYTES = (4, 6, 8)
METER_DTYPE = np.dtype([("peakL", "<f4"), ("peakR", "<f4"), ("clipL", "<u4"), ("clipR", "<u4")])


class MixRow(C.Structure):
    """tbf_mix_row: the row's bus (MIX_NONE: none) and its four coefficients L -> busL, R -> busL,
    L -> busR, R -> busR; arrays of them are MIX_ROW_DTYPE records (params.mix_rows builds them)"""
    _fields_ = [("bus", C.c_uint32), ("ll", C.c_float), ("lr", C.c_float), ("rl", C.c_float), ("rr", C.c_float)]


class MixOut(C.Structure):
    """tbf_mix_out: the two bus planes and their common stride (in floats)"""
    _fields_ = [("L", C.c_void_p), ("R", C.c_void_p), ("stride", C.c_uint64)]


# tbf_mix_row.bus of a row in no bus (include/tbf.h TBF_MIX_NONE)
MIX_NONE = 0xFFFFFFFF


class LimiterConfig(C.Structure):
    """tbf_limiter_config: the ceiling, the look-ahead A (a power of two) and the hold, in frames"""
    _fields_ = [("ceiling", C.c_float), ("ahead", C.c_uint32), ("hold", C.c_uint32)]


class LimiterDetect(C.Structure):
    """tbf_limiter_detect: the oversampling factor (2 or 4) of a limiter's true-peak detector"""
    _fields_ = [("oversample", C.c_uint32), ("reserved", C.c_uint32)]


class LimitMeter(C.Structure):
    """tbf_limit_meter: the least gain, the frames below unity and the clamped samples of a row in
    one call; arrays of them are LIMIT_METER_DTYPE records"""
    _fields_ = [("min_gain", C.c_float), ("reduced", C.c_uint32), ("clamped", C.c_uint32)]


class LimitOut(C.Structure):
    """tbf_limit_out: the two output planes, their common stride (in floats) and the optional meters"""
    _fields_ = [("L", C.c_void_p), ("R", C.c_void_p), ("stride", C.c_uint64), ("meters", C.c_void_p)]


class LoudnessConfig(C.Structure):
    """tbf_loudness_config: the rate (a multiple of 10 in [8000, 192000]) and the most 100 ms hops a
    row holds between resets"""
    _fields_ = [("rate_hz", C.c_uint32), ("max_hops", C.c_uint32)]


class LoudnessResult(C.Structure):
    """tbf_loudness_result: integrated, largest momentary and largest short-term loudness in LUFS
    (-inf where there is no block to take one from), the complete hops, the 400 ms blocks and the
    blocks behind `integrated`; arrays of them are LOUDNESS_RESULT_DTYPE records"""
    _fields_ = [("integrated", C.c_double), ("momentary_max", C.c_double), ("short_term_max", C.c_double),
                ("hops", C.c_uint32), ("blocks", C.c_uint32), ("gated", C.c_uint32), ("reserved", C.c_uint32)]


class CompConfig(C.Structure):
    """tbf_comp_config: the gain curves of a compressor (1 .. 8)"""
    _fields_ = [("n_curves", C.c_uint32)]


class EqConfig(C.Structure):
    """tbf_eq_config: the rate (in [8000, 192000]) and the most bands of a row (1 .. 8)"""
    _fields_ = [("rate_hz", C.c_uint32), ("max_bands", C.c_uint32)]


class TruePeakConfig(C.Structure):
    """tbf_true_peak_config: the oversampling factor (1, 2 or 4)"""
    _fields_ = [("oversample", C.c_uint32), ("reserved", C.c_uint32)]


class TruePeakResult(C.Structure):
    """tbf_true_peak_result: the largest sample and interpolated magnitudes of L and R, the frames
    taken and 20 log10 of the largest of the four (-inf for silence, NaN for a NaN); arrays of them
    are TRUE_PEAK_RESULT_DTYPE records"""
    _fields_ = [("sample_peak", C.c_float * 2), ("inter_peak", C.c_float * 2), ("frames", C.c_uint64), ("dbtp", C.c_double)]


# tbf_engine_config.debug_flags / tbf_error_flags bits (include/tbf.h)
DEBUG_FORCE_SERIAL = 1
# tbf_engine_config.whirl_out (include/tbf.h TBF_WHIRL_OUT_*): whirlProc3's mic mix, whirlProc's direct sum
WHIRL_OUT_MIC, WHIRL_OUT_DIRECT = 0, 1
PATH_VIB_SERIAL, PATH_WH_ANGLE, PATH_WH_MOTION, PATH_RV_PHASE, PATH_RV_WINDOW, PATH_RV_SYNC = 1, 2, 4, 8, 16, 32


# every symbol include/tbf.h declares, with its ctypes signature
SIGNATURES = {
    "tbf_abi_version": (C.c_int, []),
    "tbf_last_error": (C.c_char_p, []),
    "tbf_engine_create": (C.c_int, [C.POINTER(_Config), C.POINTER(C.c_void_p)]),
    "tbf_engine_destroy": (C.c_int, [C.c_void_p]),
    "tbf_template_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, _u32p]),
    "tbf_templates_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, _u32p, _u32p]),
    "tbf_instances_add": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _u32p, _u32p]),
    "tbf_instance_count": (C.c_uint32, [C.c_void_p]),
    "tbf_instance_retune": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "tbf_instances_clone": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _u32p]),
    "tbf_instances_save": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "tbf_instances_load": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, C.c_void_p, C.c_uint64]),
    "tbf_instances_remove": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _u32p]),
    "tbf_note": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32]),
    "tbf_set_param": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int32, C.c_double]),
    "tbf_render": (C.c_int, [C.c_void_p, C.c_uint32, _fp, _fp, C.c_uint64]),
    "tbf_render_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "tbf_synth_sound": (C.c_int, [C.c_void_p, C.c_uint32, _fp, _fp, C.c_uint64]),
    "tbf_synchronize": (C.c_int, [C.c_void_p]),
    "tbf_error_flags": (C.c_int, [C.c_void_p, _u32p]),
    "tbf_template_bank": (C.c_int, [C.c_void_p, C.c_uint32, _fp, C.c_uint64, _u32p]),
    "tbf_midi_control": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int32]),
    "tbf_config_set": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "tbf_config_parse": (C.c_int, [C.c_void_p, C.c_char_p]),
    "tbf_program_parse": (C.c_int, [C.c_void_p, C.c_char_p]),
    "tbf_program_install": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "tbf_program_name": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32]),
    "tbf_midi_control_id": (C.c_int, [C.c_char_p]),
    "tbf_set_steady_chunk": (C.c_int, [C.c_void_p, C.c_uint32]),
    "tbf_render_events": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_uint64, C.c_void_p]),
    "tbf_process": (C.c_int, [C.c_void_p, C.c_uint32, _fp, C.c_uint64, _fp, _fp, C.c_uint64]),
    "tbf_process_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p]),
    "tbf_process_events": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "tbf_render_rotors": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RotorOut)]),
    "tbf_render_rotors_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_uint64, C.POINTER(RotorOut), C.c_void_p]),
    "tbf_process_rotors": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.POINTER(RotorOut)]),
    "tbf_process_rotors_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                            C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RotorOut), C.c_void_p]),
    "tbf_cabinet_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "tbf_render_cabinet": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(CabinetOut), C.POINTER(RotorOut)]),
    "tbf_render_cabinet_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(CabinetOut),
                                            C.POINTER(RotorOut), C.c_void_p]),
    "tbf_process_cabinet": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(CabinetOut),
                                      C.POINTER(RotorOut)]),
    "tbf_process_cabinet_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                             C.POINTER(CabinetOut), C.POINTER(RotorOut), C.c_void_p]),
    "tbf_resampler_set": (C.c_int, [C.c_void_p, C.c_uint32]),
    "tbf_resampled_frames": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "tbf_render_resampled": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(ResampledOut)]),
    "tbf_render_resampled_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(ResampledOut),
                                              C.c_void_p]),
    "tbf_process_resampled": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(ResampledOut)]),
    "tbf_process_resampled_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                               C.POINTER(ResampledOut), C.c_void_p]),
    "tbf_pcm_convert_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                         C.c_void_p, C.POINTER(PcmOut), C.c_void_p]),
    "tbf_render_pcm": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(PcmOut)]),
    "tbf_render_pcm_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(PcmOut), C.c_void_p]),
    "tbf_process_pcm": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(PcmOut)]),
    "tbf_process_pcm_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.POINTER(PcmOut), C.c_void_p]),
    "tbf_mix_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                 C.c_void_p, C.c_uint32, C.POINTER(MixOut), C.c_void_p]),
    "tbf_render_mix": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(MixOut)]),
    "tbf_render_mix_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                        C.POINTER(MixOut), C.c_void_p]),
    "tbf_process_mix": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                  C.POINTER(MixOut)]),
    "tbf_process_mix_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_uint32, C.POINTER(MixOut), C.c_void_p]),
    "tbf_limiter_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(LimiterConfig), C.POINTER(C.c_void_p)]),
    "tbf_limiter_create_tp": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(LimiterConfig), C.POINTER(LimiterDetect),
                                        C.POINTER(C.c_void_p)]),
    "tbf_limiter_destroy": (C.c_int, [C.c_void_p]),
    "tbf_limiter_reset": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_limiter_latency": (C.c_int, [C.c_void_p, _u32p]),
    "tbf_limit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                   C.POINTER(LimitOut), C.c_void_p]),
    "tbf_loudness_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(LoudnessConfig), C.POINTER(C.c_void_p)]),
    "tbf_loudness_destroy": (C.c_int, [C.c_void_p]),
    "tbf_loudness_reset": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_loudness_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_loudness_read": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_loudness_hops": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _u32p]),
    "tbf_loudness_range": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tbf_true_peak_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(TruePeakConfig), C.POINTER(C.c_void_p)]),
    "tbf_true_peak_destroy": (C.c_int, [C.c_void_p]),
    "tbf_true_peak_reset": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_true_peak_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_true_peak_read": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_eq_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(EqConfig), C.POINTER(C.c_void_p)]),
    "tbf_eq_destroy": (C.c_int, [C.c_void_p]),
    "tbf_eq_reset": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_eq_set": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tbf_eq_bands": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _u32p]),
    "tbf_eq_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                C.c_void_p, C.c_void_p]),
    "tbf_comp_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(CompConfig), C.POINTER(C.c_void_p)]),
    "tbf_comp_destroy": (C.c_int, [C.c_void_p]),
    "tbf_comp_reset": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_comp_curve_set": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "tbf_comp_rows_set": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tbf_comp_curve_get": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "tbf_comp_row_get": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "tbf_comp_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tbf_comp_curve_design": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_void_p]),
}
# the stages' timing hooks (_stage_time), which share one signature; debug calls stay out of SIGNATURES
STAGE_TIME = {f"tbf_debug_{stage}_time": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.POINTER(C.c_uint64)])
              for stage in ("cabinet", "resample", "pcm", "mix", "limit", "loudness", "true_peak", "eq", "comp")}

# tbf_engine_config.chain_mode of the effects-only chains (include/tbf.h TBF_CHAIN_FX*)
CHAIN_FX, CHAIN_FX_TAP_PREAMP, CHAIN_FX_TAP_REVERB = 4, 5, 6

# tbf_event kinds (include/tbf.h)
EV_NOTE, EV_PARAM, EV_CONTROL, EV_PROGRAM = 0, 1, 2, 3
EVENT_DTYPE = np.dtype([("block", "<u4"), ("inst", "<u4"), ("kind", "<i4"), ("id", "<i4"), ("value", "<f8")])

# tbf_debug_launches index order (include/tbf.h TBF_LAUNCH_*)
LAUNCH_KINDS = ("k_tonegen", "k_tonegen_ranges", "k_rv_core", "k_rv_core_lds", "k_whirl", "k_whirl_split")

_lib = None


def load_library():
    """Load the in-tree libtbf.so; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise TbfError(f"{LIB_PATH} not built -- run __graft_entry__.build() or `make -C tunebfree_amd`")
        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in {**SIGNATURES, **STAGE_TIME}.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _check(rc):
    if rc < 0:
        raise TbfError(f"tbf error {rc}: {load_library().tbf_last_error().decode(errors='replace')}")
    return rc


def _stage_time(fn, handle, enable):
    """a stage's tbf_debug_*_time call fn on its engine or object: enable True / False switches its
    timing on / off and returns None; None returns (milliseconds, launch sets) since the last query"""
    if enable is not None:
        _check(fn(handle, 1 if enable else -1, None, None))
        return None
    ms, n = C.c_double(), C.c_uint64()
    _check(fn(handle, 0, C.byref(ms), C.byref(n)))
    return ms.value, n.value


def _ptr(p):
    """an optional device pointer or stream as a call's argument"""
    return None if p is None else C.c_void_p(int(p))


def _rows_arg(rows):
    """a stage object's rows argument (None: all): (n, pointer, the array the pointer reads)"""
    if rows is None:
        return 0, None, None
    r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    return len(r), r.ctypes.data, r


def _counts_arg(counts, n_rows):
    """a stage object's counts argument (None: every row whole): (pointer, the array it reads)"""
    if counts is None:
        return None, None
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(c) != n_rows:
        raise ValueError(f"{len(c)} counts for {n_rows} rows")
    return c.ctypes.data, c


def limiter_oversample(rate_hz):
    """the oversampling factor of a limiter's true-peak detector for a rate, as true_peak_oversample:
    4 below 96 kHz, 2 below 192 kHz; at or above 192 kHz there is nothing to interpolate"""
    f = true_peak_oversample(rate_hz)
    if f == 1:
        raise ValueError(f"no true-peak detector at {rate_hz} Hz: at or above 192 kHz use the plain limiter (oversample=None)")
    return f


class Limiter:
    """A bus limiter (Engine.limiter): n_rows rows of look-ahead peak limiting behind any two
    device planes; its state belongs to it, not to the engine's instances.  oversample is None for
    the plain kind, 2 or 4 for one with a true-peak detector."""

    def __init__(self, eng, handle, n_rows, cfg, oversample=None):
        self._eng, self._lib, self._h = eng, eng._lib, handle
        self.n_rows, self.ceiling, self.ahead, self.hold = n_rows, cfg.ceiling, cfg.ahead, cfg.hold
        self.oversample = oversample

    @property
    def latency(self):
        """tbf_limiter_latency: the frames by which the output trails the input (ahead - 1, with a
        true-peak detector ahead + 5)"""
        d = C.c_uint32()
        _check(self._lib.tbf_limiter_latency(self._h, C.byref(d)))
        return d.value

    @property
    def history(self):
        """the frames of input a row keeps per channel (2 * ahead + hold - 2, with a true-peak
        detector 11 more)"""
        return 2 * self.ahead + self.hold - 2 + (11 if self.oversample else 0)

    def process_device(self, L_ptr, R_ptr, in_stride, frames, outL_ptr, outR_ptr, out_stride, counts=None, meters_ptr=None,
                       stream=None):
        """tbf_limit_device: the limiter's rows of the device planes L_ptr / R_ptr (row r at
        r * in_stride floats; L_ptr == R_ptr: mono), `frames` frames per row or counts[r] (host
        array) of them, into outL_ptr / outR_ptr, out_stride floats apart; meters_ptr None or
        device memory of one tbf_limit_meter (12 B) per row."""
        cp, _c = _counts_arg(counts, self.n_rows)
        lo = LimitOut(_ptr(outL_ptr), _ptr(outR_ptr), int(out_stride), _ptr(meters_ptr))
        _check(self._lib.tbf_limit_device(self._h, _ptr(L_ptr), _ptr(R_ptr), int(in_stride), int(frames), cp, C.byref(lo),
                                          _ptr(stream)))

    def reset(self, rows=None, stream=None):
        """tbf_limiter_reset: the rows (None: all) start anew, ordered on the stream"""
        n, rp, _r = _rows_arg(rows)
        _check(self._lib.tbf_limiter_reset(self._h, n, rp, _ptr(stream)))

    def time(self, enable=None):
        """tbf_debug_limit_time: enable True / False switches the event pair around every call's
        launches on / off; None returns (milliseconds, launch sets) since the last query."""
        return _stage_time(self._lib.tbf_debug_limit_time, self._h, enable)

    def close(self):
        """tbf_limiter_destroy (the engine does it for the limiters still alive when it closes)"""
        if self._h and getattr(self._eng, "_h", None):
            _check(self._lib.tbf_limiter_destroy(self._h))
        self._h = None


class Loudness:
    """A loudness meter (Engine.loudness): n_rows rows of BS.1770 K-weighted hop energies beside any
    two device planes, and their gated loudness; its state belongs to it, not to the engine's
    instances."""

    def __init__(self, eng, handle, n_rows, cfg):
        self._eng, self._lib, self._h = eng, eng._lib, handle
        self.n_rows, self.rate_hz, self.max_hops = n_rows, cfg.rate_hz, cfg.max_hops

    def measure_device(self, L_ptr, R_ptr, in_stride, frames, counts=None, stream=None):
        """tbf_loudness_device: the meter's rows of the device planes L_ptr / R_ptr (row r at
        r * in_stride floats; L_ptr == R_ptr: a pair of equal channels) take `frames` frames, or
        counts[r] (host array) of them; the planes are only read."""
        cp, _c = _counts_arg(counts, self.n_rows)
        _check(self._lib.tbf_loudness_device(self._h, _ptr(L_ptr), _ptr(R_ptr), int(in_stride), int(frames), cp, _ptr(stream)))

    def read(self, rows=None):
        """tbf_loudness_read: LOUDNESS_RESULT_DTYPE records of the rows (None: all), after the
        meter's last call has passed its stream"""
        from .params import LOUDNESS_RESULT_DTYPE
        n, rp, _r = _rows_arg(rows)
        out = np.zeros(self.n_rows if rows is None else n, LOUDNESS_RESULT_DTYPE)
        _check(self._lib.tbf_loudness_read(self._h, n, rp, out.ctypes.data))
        return out

    def hops(self, row):
        """tbf_loudness_hops: the energies of the row's complete hops, [hops, 2] float64 (EL, ER)"""
        n = C.c_uint32()
        rc = self._lib.tbf_loudness_hops(self._h, int(row), None, 0, C.byref(n))
        if rc not in (0, -28):
            _check(rc)
        e = np.zeros((n.value, 2), np.float64)
        _check(self._lib.tbf_loudness_hops(self._h, int(row), e.ctypes.data, n.value, C.byref(n)))
        return e

    def gains(self, target_lufs):
        """per row the float32 gain 10**((target_lufs - integrated) / 20) that brings it to the
        target, computed in double and then rounded; 1.0 for a row with no gated block"""
        res = self.read()
        g = np.ones(self.n_rows, np.float64)
        ok = res["gated"] > 0
        g[ok] = 10.0 ** ((float(target_lufs) - res["integrated"][ok]) / 20.0)
        return g.astype(np.float32)

    def reset(self, rows=None, stream=None):
        """tbf_loudness_reset: the rows (None: all) start anew, ordered on the stream"""
        n, rp, _r = _rows_arg(rows)
        _check(self._lib.tbf_loudness_reset(self._h, n, rp, _ptr(stream)))

    def timing(self, enable=None):
        """tbf_debug_loudness_time: enable True / False switches the event pair around every call's
        launch on / off; None returns (milliseconds, launch sets) since the last query."""
        return _stage_time(self._lib.tbf_debug_loudness_time, self._h, enable)

    def range(self, rows=None):
        """tbf_loudness_range: (loudness range in LU [k] float64, the short-term windows behind it [k]
        uint32) of the rows (None: all), after the meter's last call has passed its stream"""
        n, rp, _r = _rows_arg(rows)
        k = self.n_rows if rows is None else n
        lra, win = np.zeros(k, np.float64), np.zeros(k, np.uint32)
        _check(self._lib.tbf_loudness_range(self._h, n, rp, lra.ctypes.data, win.ctypes.data))
        return lra, win

    def close(self):
        """tbf_loudness_destroy (the engine does it for the meters still alive when it closes)"""
        if self._h and getattr(self._eng, "_h", None):
            _check(self._lib.tbf_loudness_destroy(self._h))
        self._h = None


def _eq_band_lists(bands, n):
    """Equalizer.set's bands for n rows as (packed EQ_BAND_DTYPE records, uint32 counts): one list of
    records for all the rows, or one list per row"""
    from .params import EQ_BAND_DTYPE
    bands = list(bands)
    rowwise = bool(bands) and all(isinstance(r, (list, tuple)) or (isinstance(r, np.ndarray) and r.ndim == 1) for r in bands)
    per_row = [list(r) for r in bands] if rowwise else [bands] * n
    if len(per_row) != n:
        raise ValueError(f"{len(per_row)} band lists for {n} rows")
    flat = np.array([b for r in per_row for b in r], dtype=EQ_BAND_DTYPE).reshape(-1)
    return flat, np.array([len(r) for r in per_row], dtype=np.uint32)


class Equalizer:
    """A bus equaliser (Engine.equalizer): n_rows rows, each with its own list of up to max_bands
    biquad bands (params.eq_band), between two pairs of device planes; its state belongs to it, not
    to the engine's instances."""

    def __init__(self, eng, handle, n_rows, cfg):
        self._eng, self._lib, self._h = eng, eng._lib, handle
        self.n_rows, self.rate_hz, self.max_bands = n_rows, cfg.rate_hz, cfg.max_bands

    def set(self, bands, rows=None, stream=None):
        """tbf_eq_set: new bands for the rows (None: all): `bands` is one list of params.eq_band
        records for all of them, or one list per row; from the next process_device on, state kept"""
        n, rp, _r = _rows_arg(rows)
        flat, nb = _eq_band_lists(bands, self.n_rows if rows is None else n)
        _check(self._lib.tbf_eq_set(self._h, n, rp, flat.ctypes.data if len(flat) else None, nb.ctypes.data, _ptr(stream)))

    def bands(self, row):
        """tbf_eq_bands: the coefficients of the row's bands in use, [nb, 5] float64 (b0, b1, b2, a1, a2)"""
        n = C.c_uint32()
        c = np.zeros((self.max_bands, 5), np.float64)
        _check(self._lib.tbf_eq_bands(self._h, int(row), c.ctypes.data, self.max_bands, C.byref(n)))
        return c[:n.value].copy()

    def process_device(self, L_ptr, R_ptr, in_stride, frames, outL_ptr, outR_ptr, out_stride, counts=None, stream=None):
        """tbf_eq_device: the equaliser's rows of the device planes L_ptr / R_ptr (row r at
        r * in_stride floats; L_ptr == R_ptr: mono), `frames` frames per row or counts[r] (host
        array) of them, into outL_ptr / outR_ptr, out_stride floats apart."""
        cp, _c = _counts_arg(counts, self.n_rows)
        _check(self._lib.tbf_eq_device(self._h, _ptr(L_ptr), _ptr(R_ptr), int(in_stride), int(frames), _ptr(outL_ptr),
                                       _ptr(outR_ptr), int(out_stride), cp, _ptr(stream)))

    def reset(self, rows=None, stream=None):
        """tbf_eq_reset: the state of the rows (None: all) is zero again, ordered on the stream"""
        n, rp, _r = _rows_arg(rows)
        _check(self._lib.tbf_eq_reset(self._h, n, rp, _ptr(stream)))

    def timing(self, enable=None):
        """tbf_debug_eq_time: enable True / False switches the event pair around every call's
        launch on / off; None returns (milliseconds, launch sets) since the last query."""
        return _stage_time(self._lib.tbf_debug_eq_time, self._h, enable)

    def close(self):
        """tbf_eq_destroy (the engine does it for the equalisers still alive when it closes)"""
        if self._h and getattr(self._eng, "_h", None):
            _check(self._lib.tbf_eq_destroy(self._h))
        self._h = None


class Compressor:
    """A bus compressor (Engine.compressor): n_rows rows, each with a gain curve (one of n_curves,
    769 points each: params.comp_curve), an attack and a release coefficient and a make-up
    (params.comp_row), between two pairs of device planes, with an optional key pair; its state, one
    gain per row, belongs to it, not to the engine's instances."""

    def __init__(self, eng, handle, n_rows, cfg):
        self._eng, self._lib, self._h = eng, eng._lib, handle
        self.n_rows, self.n_curves = n_rows, cfg.n_curves

    def set_curve(self, i, pts, stream=None):
        """tbf_comp_curve_set: the 769 points of curve i; from the next process_device on, every g kept"""
        from .params import COMP_POINTS
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1)
        if len(p) != COMP_POINTS:
            raise ValueError(f"{len(p)} points: want {COMP_POINTS}")
        _check(self._lib.tbf_comp_curve_set(self._h, int(i), p.ctypes.data, _ptr(stream)))

    def set_rows(self, params, rows=None, stream=None):
        """tbf_comp_rows_set: new parameters for the rows (None: all): one params.comp_row record for
        all of them, or one per row; from the next process_device on, every g kept"""
        from .params import COMP_ROW_DTYPE
        n, rp, _r = _rows_arg(rows)
        want = self.n_rows if rows is None else n
        p = np.atleast_1d(np.asarray(params, dtype=COMP_ROW_DTYPE)).reshape(-1)
        if len(p) == 1:
            p = np.repeat(p, want)
        if len(p) != want:
            raise ValueError(f"{len(p)} parameter records for {want} rows")
        p = np.ascontiguousarray(p)
        _check(self._lib.tbf_comp_rows_set(self._h, n, rp, p.ctypes.data, _ptr(stream)))

    def curve(self, i):
        """tbf_comp_curve_get: the 769 points of curve i, float32"""
        from .params import COMP_POINTS
        p = np.zeros(COMP_POINTS, np.float32)
        _check(self._lib.tbf_comp_curve_get(self._h, int(i), p.ctypes.data))
        return p

    def row(self, r):
        """tbf_comp_row_get: row r's parameters, one params.COMP_ROW_DTYPE record"""
        from .params import COMP_ROW_DTYPE
        p = np.zeros(1, COMP_ROW_DTYPE)
        _check(self._lib.tbf_comp_row_get(self._h, int(r), p.ctypes.data))
        return p[0]

    def process_device(self, L_ptr, R_ptr, in_stride, frames, outL_ptr, outR_ptr, out_stride, counts=None, key=None,
                       meters_ptr=None, stream=None):
        """tbf_comp_device: the compressor's rows of the device planes L_ptr / R_ptr (row r at
        r * in_stride floats; L_ptr == R_ptr: mono), `frames` frames per row or counts[r] (host
        array) of them, into outL_ptr / outR_ptr, out_stride floats apart; key (kL_ptr, kR_ptr,
        stride): the planes the gain follows in place of the input; meters_ptr: device memory for one
        params.COMP_METER_DTYPE record per row."""
        cp, _c = _counts_arg(counts, self.n_rows)
        kl, kr, ks = (None, None, 0) if key is None else key
        _check(self._lib.tbf_comp_device(self._h, _ptr(L_ptr), _ptr(R_ptr), int(in_stride), int(frames), _ptr(kl), _ptr(kr),
                                         int(ks), _ptr(outL_ptr), _ptr(outR_ptr), int(out_stride), cp, _ptr(meters_ptr),
                                         _ptr(stream)))

    def reset(self, rows=None, stream=None):
        """tbf_comp_reset: the gain of the rows (None: all) is 1 again, ordered on the stream"""
        n, rp, _r = _rows_arg(rows)
        _check(self._lib.tbf_comp_reset(self._h, n, rp, _ptr(stream)))

    def timing(self, enable=None):
        """tbf_debug_comp_time: enable True / False switches the event pair around every call's
        launch on / off; None returns (milliseconds, launch sets) since the last query."""
        return _stage_time(self._lib.tbf_debug_comp_time, self._h, enable)

    def close(self):
        """tbf_comp_destroy (the engine does it for the compressors still alive when it closes)"""
        if self._h and getattr(self._eng, "_h", None):
            _check(self._lib.tbf_comp_destroy(self._h))
        self._h = None


def true_peak_oversample(rate_hz):
    """the oversampling factor of BS.1770-4 Annex 2 for a rate: 4 below 96 kHz, 2 below 192 kHz, else 1"""
    return 4 if rate_hz < 96000 else 2 if rate_hz < 192000 else 1


class TruePeak:
    """A true-peak meter (Engine.true_peak): n_rows rows of sample peaks and of the peaks of the
    BS.1770-4 Annex 2 interpolator beside any two device planes; its state belongs to it, not to the
    engine's instances."""

    def __init__(self, eng, handle, n_rows, cfg):
        self._eng, self._lib, self._h = eng, eng._lib, handle
        self.n_rows, self.oversample = n_rows, cfg.oversample

    def measure_device(self, L_ptr, R_ptr, in_stride, frames, counts=None, stream=None):
        """tbf_true_peak_device: the meter's rows of the device planes L_ptr / R_ptr (row r at
        r * in_stride floats; L_ptr == R_ptr: a pair of equal channels) take `frames` frames, or
        counts[r] (host array) of them; the planes are only read."""
        cp, _c = _counts_arg(counts, self.n_rows)
        _check(self._lib.tbf_true_peak_device(self._h, _ptr(L_ptr), _ptr(R_ptr), int(in_stride), int(frames), cp, _ptr(stream)))

    def read(self, rows=None):
        """tbf_true_peak_read: TRUE_PEAK_RESULT_DTYPE records of the rows (None: all), after the
        meter's last call has passed its stream"""
        from .params import TRUE_PEAK_RESULT_DTYPE
        n, rp, _r = _rows_arg(rows)
        out = np.zeros(self.n_rows if rows is None else n, TRUE_PEAK_RESULT_DTYPE)
        _check(self._lib.tbf_true_peak_read(self._h, n, rp, out.ctypes.data))
        return out

    def gains(self, ceiling_dbtp):
        """per row the float32 gain 10**((ceiling_dbtp - dbtp) / 20) that brings its true peak down to
        the ceiling, computed in double, capped at 1.0 and then rounded; 1.0 for a silent row (and
        for a row whose peak is a NaN, which no gain mends)"""
        d = self.read()["dbtp"]
        g = np.ones(self.n_rows, np.float64)
        ok = np.isfinite(d)
        g[ok] = np.minimum(10.0 ** ((float(ceiling_dbtp) - d[ok]) / 20.0), 1.0)
        g[np.isposinf(d)] = 0.0
        return g.astype(np.float32)

    def reset(self, rows=None, stream=None):
        """tbf_true_peak_reset: the rows (None: all) start anew, ordered on the stream"""
        n, rp, _r = _rows_arg(rows)
        _check(self._lib.tbf_true_peak_reset(self._h, n, rp, _ptr(stream)))

    def timing(self, enable=None):
        """tbf_debug_true_peak_time: enable True / False switches the event pair around every call's
        launch on / off; None returns (milliseconds, launches) since the last query."""
        return _stage_time(self._lib.tbf_debug_true_peak_time, self._h, enable)

    def close(self):
        """tbf_true_peak_destroy (the engine does it for the meters still alive when it closes)"""
        if self._h and getattr(self._eng, "_h", None):
            _check(self._lib.tbf_true_peak_destroy(self._h))
        self._h = None


class Engine:
    """A batch of organ instances on one GPU (one engine per device / rank)."""

    def __init__(self, sample_rate=48000.0, device=0, chain=0, debug_flags=0, whirl_out=WHIRL_OUT_MIC):
        lib = load_library()
        cfg = _Config(float(sample_rate), int(device), int(chain), int(debug_flags), int(whirl_out))
        h = C.c_void_p()
        _check(lib.tbf_engine_create(C.byref(cfg), C.byref(h)))
        self._lib, self._h = lib, h
        self.sample_rate, self.device = sample_rate, device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tbf_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def config_set(self, key, value):
        """One cfg key (tbf_config_set): 0 applied, 1 not a key of this path."""
        return _check(self._lib.tbf_config_set(self._h, str(key).encode(), str(value).encode()))

    def config(self, items):
        """Several cfg keys, a dict or (key, value) pairs, in order."""
        for k, v in (items.items() if isinstance(items, dict) else items):
            self.config_set(k, v)

    def config_parse(self, text):
        """A cfg file's text; returns the number of keys applied."""
        return _check(self._lib.tbf_config_parse(self._h, text.encode()))

    def layout(self):
        """The cfg-derived layout (tbf_debug_layout): compact whirl ring window, the
        geometry's largest write-ahead, reverb slab length; and (tbf_debug_whirl_lead) its
        smallest write-ahead with the bound under which a whirl chain is refused."""
        f = self._lib.tbf_debug_layout
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, _u32p, _fp, _u32p]
        w, a, s = C.c_uint32(), C.c_float(), C.c_uint32()
        _check(f(self._h, C.byref(w), C.byref(a), C.byref(s)))
        g = self._lib.tbf_debug_whirl_lead
        g.restype = C.c_int
        g.argtypes = [C.c_void_p, _fp, _fp]
        m, b = C.c_float(), C.c_float()
        _check(g(self._h, C.byref(m), C.byref(b)))
        return {"wring_len": w.value, "max_ahead": a.value, "slab_len": s.value, "min_ahead": m.value,
                "min_ahead_bound": b.value}

    def front_chunks(self):
        """tbf_debug_front_chunks: chunks with events stepped by (the device's, the host's) front end"""
        f = self._lib.tbf_debug_front_chunks
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]
        d, h = C.c_uint64(), C.c_uint64()
        _check(f(self._h, C.byref(d), C.byref(h)))
        return d.value, h.value

    def launches(self):
        """tbf_debug_launches: launches of each kernel variant since the engine was created,
        keyed by LAUNCH_KINDS ("k_tonegen": one block range per instance, "k_tonegen_ranges":
        several); a host engine reports zeros."""
        f = self._lib.tbf_debug_launches
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]
        cnt = np.zeros(len(LAUNCH_KINDS), np.uint64)
        assert _check(f(self._h, cnt.ctypes.data, len(cnt))) == len(LAUNCH_KINDS)
        return {k: int(c) for k, c in zip(LAUNCH_KINDS, cnt)}

    def pre_ahead(self):
        """tbf_debug_pre_ahead: k_rv_pre launches that ran ahead, beside the previous chunk's
        k_rv_post (TBF_PRE_AHEAD=1)."""
        f = self._lib.tbf_debug_pre_ahead
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        n = C.c_uint64()
        _check(f(self._h, C.byref(n)))
        return n.value

    def set_steady_chunk(self, blocks):
        """tbf_set_steady_chunk: the longest chunk without control deltas (64..2048 blocks),
        which bounds the stage buffers; returns the value in effect."""
        return _check(self._lib.tbf_set_steady_chunk(self._h, int(blocks)))

    def chunks(self):
        """Blocks per render chunk (tbf_debug_chunks): (with control deltas, without)."""
        f = self._lib.tbf_debug_chunks
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, _u32p, _u32p]
        d, s = C.c_uint32(), C.c_uint32()
        _check(f(self._h, C.byref(d), C.byref(s)))
        return d.value, s.value

    def template(self, mts128=None, ratio9=None, seed=1):
        m = None if mts128 is None else np.ascontiguousarray(mts128, dtype=np.float64)
        r = None if ratio9 is None else np.ascontiguousarray(ratio9, dtype=np.float64)
        out = C.c_uint32()
        _check(self._lib.tbf_template_create(self._h, None if m is None else m.ctypes.data,
                                             None if r is None else r.ctypes.data, int(seed), C.byref(out)))
        return out.value

    def templates(self, seeds, mts128=None, ratio9=None):
        """n templates built on the device (tbf_templates_create): mts128 (n, 128) or
        None, ratio9 (n, 9) or None; returns the template ids."""
        sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        n = len(sd)
        m = None if mts128 is None else np.ascontiguousarray(mts128, dtype=np.float64).reshape(n, 128)
        r = None if ratio9 is None else np.ascontiguousarray(ratio9, dtype=np.float64).reshape(n, 9)
        ids = np.zeros(n, np.uint32)
        _check(self._lib.tbf_templates_create(self._h, n, None if m is None else m.ctypes.data,
                                              None if r is None else r.ctypes.data,
                                              sd.ctypes.data_as(_u32p), ids.ctypes.data_as(_u32p)))
        return [int(x) for x in ids]

    def template_bank(self, tpl):
        lens = np.zeros(256, np.uint32)
        n = _check(self._lib.tbf_template_bank(self._h, int(tpl), None, 0, lens.ctypes.data_as(_u32p)))
        out = np.zeros(n, np.float32)
        _check(self._lib.tbf_template_bank(self._h, int(tpl), out.ctypes.data_as(_fp), n, None))
        return out, lens

    def retune(self, inst, tpl_id):
        """tbf_instance_retune: the CLAP reinitToneGen on another template, from the next block"""
        _check(self._lib.tbf_instance_retune(self._h, int(inst), int(tpl_id)))

    def add_instances(self, tpl_ids, seeds):
        t = np.ascontiguousarray(tpl_ids, dtype=np.uint32)
        s = np.ascontiguousarray(seeds, dtype=np.uint32)
        assert t.shape == s.shape
        first = C.c_uint32()
        _check(self._lib.tbf_instances_add(self._h, len(t), t.ctypes.data_as(_u32p), s.ctypes.data_as(_u32p),
                                           C.byref(first)))
        return first.value

    def clone(self, src):
        """tbf_instances_clone: append exact copies of the instances src (an index or a list,
        repeats allowed), device and host state, pending events included; returns the first
        new index."""
        a = np.ascontiguousarray(np.atleast_1d(src), dtype=np.uint32)
        first = C.c_uint32()
        _check(self._lib.tbf_instances_clone(self._h, len(a), a.ctypes.data_as(_u32p), C.byref(first)))
        return first.value

    def save(self, inst):
        """tbf_instances_save: the instances' full state as an opaque uint8 blob (valid for
        this build of the library only)."""
        a = np.ascontiguousarray(np.atleast_1d(inst), dtype=np.uint32)
        size = C.c_uint64()
        _check(self._lib.tbf_instances_save(self._h, len(a), a.ctypes.data_as(_u32p), None, 0, C.byref(size)))
        blob = np.zeros(size.value, np.uint8)
        _check(self._lib.tbf_instances_save(self._h, len(a), a.ctypes.data_as(_u32p), blob.ctypes.data, blob.nbytes,
                                            C.byref(size)))
        assert size.value == blob.nbytes
        return blob

    def load(self, inst, blob):
        """tbf_instances_load: overwrite the instances inst with the blob's records, in order."""
        a = np.ascontiguousarray(np.atleast_1d(inst), dtype=np.uint32)
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        _check(self._lib.tbf_instances_load(self._h, len(a), a.ctypes.data_as(_u32p), b.ctypes.data, b.nbytes))

    def remove(self, inst):
        """tbf_instances_remove: remove the instances inst (an index or a list of distinct
        indices); the survivors keep their order and are renumbered densely.  Returns the map
        old index -> new index as an int64 array, -1 for a removed instance."""
        a = np.ascontiguousarray(np.atleast_1d(inst), dtype=np.uint32)
        old = self.n_instances
        m = np.zeros(old + 1, np.uint32)
        _check(self._lib.tbf_instances_remove(self._h, len(a), a.ctypes.data_as(_u32p), m.ctypes.data_as(_u32p)))
        out = m[:old].astype(np.int64)
        out[out == 0xFFFFFFFF] = -1
        return out

    def device_bytes(self):
        """tbf_debug_device_bytes: (instance_bytes, stage_bytes) of device memory held now --
        the arrays sized by the instance count alone, and the stage buffers."""
        f = self._lib.tbf_debug_device_bytes
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        ib, sb = C.c_uint64(), C.c_uint64()
        _check(f(self._h, C.byref(ib), C.byref(sb)))
        return ib.value, sb.value

    @property
    def n_instances(self):
        return self._lib.tbf_instance_count(self._h)

    def note(self, inst, key, on):
        _check(self._lib.tbf_note(self._h, int(inst), int(key), int(on)))

    def set_param(self, inst, pid, value):
        _check(self._lib.tbf_set_param(self._h, int(inst), int(pid), float(value)))

    def render(self, nblocks):
        """Synchronous render into host arrays, shape [n_instances, nblocks*128]."""
        n = self.n_instances
        L = np.zeros((n, nblocks * 128), np.float32)
        R = np.zeros((n, nblocks * 128), np.float32)
        _check(self._lib.tbf_render(self._h, int(nblocks), L.ctypes.data_as(_fp), R.ctypes.data_as(_fp),
                                    nblocks * 128))
        return L, R

    def render_device(self, nblocks, outL_ptr, outR_ptr, stride, stream=None):
        """Enqueue a render into device memory (e.g. torch tensor data_ptr())."""
        _check(self._lib.tbf_render_device(self._h, int(nblocks), C.c_void_p(int(outL_ptr)),
                                           C.c_void_p(int(outR_ptr)), int(stride),
                                           None if stream is None else C.c_void_p(int(stream))))

    def synth_sound(self, nframes):
        n = self.n_instances
        L = np.zeros((n, nframes), np.float32)
        R = np.zeros((n, nframes), np.float32)
        _check(self._lib.tbf_synth_sound(self._h, int(nframes), L.ctypes.data_as(_fp), R.ctypes.data_as(_fp),
                                         nframes))
        return L, R

    def midi_control(self, inst, fn, value):
        """callMIDIControlFunction (src/midi.cpp:535): True if the name is a hot-path control."""
        return _check(self._lib.tbf_midi_control(self._h, int(inst), fn.encode(), int(value))) == 0

    def program_parse(self, text):
        """Load programme definitions in the reference's .pgm syntax; returns programmes in use."""
        return _check(self._lib.tbf_program_parse(self._h, text.encode()))

    def program_install(self, inst, pc):
        """installProgram (src/program.cpp:735) for MIDI program change pc on one instance."""
        _check(self._lib.tbf_program_install(self._h, int(inst), int(pc)))

    def program_name(self, pc):
        buf = C.create_string_buffer(64)
        return buf.value.decode() if _check(self._lib.tbf_program_name(self._h, int(pc), buf, 64)) else None

    def control_id(self, fn):
        return self._lib.tbf_midi_control_id(fn.encode())

    def events(self, rows):
        """Pack (block, inst, kind, id, value) rows into the tbf_event array, stably sorted
        by block."""
        a = np.array([tuple(r) for r in rows], dtype=EVENT_DTYPE)
        return a[np.argsort(a["block"], kind="stable")] if len(a) else a

    def render_events_device(self, nblocks, events, outL_ptr, outR_ptr, stride, stream=None):
        """tbf_render_events: enqueue a render of nblocks with scheduled events into device
        memory (e.g. torch tensor data_ptr())."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
        _check(self._lib.tbf_render_events(self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev),
                                           C.c_void_p(int(outL_ptr)), C.c_void_p(int(outR_ptr)), int(stride),
                                           None if stream is None else C.c_void_p(int(stream))))

    def process(self, x):
        """Effects-only engines (chain=CHAIN_FX*): x [n_instances, nblocks*128] float32 through
        overdrive -> reverb -> whirl; synchronous, returns (L, R) of the same shape."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.n_instances
        if x.ndim != 2 or x.shape[0] != n or x.shape[1] % 128:
            raise ValueError(f"input shape {x.shape}: want ({n}, nblocks*128)")
        L = np.zeros_like(x)
        R = np.zeros_like(x)
        _check(self._lib.tbf_process(self._h, x.shape[1] // 128, x.ctypes.data_as(_fp), x.shape[1],
                                     L.ctypes.data_as(_fp), R.ctypes.data_as(_fp), x.shape[1]))
        return L, R

    def process_device(self, nblocks, in_ptr, in_stride, outL_ptr, outR_ptr, stride, stream=None):
        """tbf_process_device: enqueue nblocks of device-resident input rows (e.g. a torch
        tensor's data_ptr()) through the effects into device memory.  The input must be
        complete where `stream` reaches the call and may be overwritten behind it."""
        _check(self._lib.tbf_process_device(self._h, int(nblocks), C.c_void_p(int(in_ptr)), int(in_stride),
                                            C.c_void_p(int(outL_ptr)), C.c_void_p(int(outR_ptr)), int(stride),
                                            None if stream is None else C.c_void_p(int(stream))))

    def process_events_device(self, nblocks, events, in_ptr, in_stride, outL_ptr, outR_ptr, stride, stream=None):
        """tbf_process_events: process_device with scheduled events (Engine.events)."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
        _check(self._lib.tbf_process_events(self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev),
                                            C.c_void_p(int(in_ptr)), int(in_stride), C.c_void_p(int(outL_ptr)),
                                            C.c_void_p(int(outR_ptr)), int(stride),
                                            None if stream is None else C.c_void_p(int(stream))))

    def _rotor_host(self, nblocks, lr, call):
        """four zeroed host planes (and L / R when lr), handed to call (L ptr, R ptr, RotorOut)"""
        shape = (self.n_instances, nblocks * 128)
        planes = [np.zeros(shape, np.float32) for _ in range(4)]
        L, R = (np.zeros(shape, np.float32), np.zeros(shape, np.float32)) if lr else (None, None)
        ro = RotorOut(*[p.ctypes.data for p in planes], nblocks * 128)
        _check(call(None if L is None else L.ctypes.data, None if R is None else R.ctypes.data, C.byref(ro)))
        return (L, R, *planes)

    def render_rotors(self, nblocks, lr=True):
        """tbf_render_rotors: one synchronous render with whirlProc2's horn and drum pairs;
        returns (L, R, hornL, hornR, drumL, drumR), each [n_instances, nblocks*128] (L and R
        None with lr=False: the call's NULL outL / outR)."""
        return self._rotor_host(nblocks, lr, lambda l, r, ro: self._lib.tbf_render_rotors(
            self._h, int(nblocks), l, r, nblocks * 128, ro))

    def process_rotors(self, x, lr=True):
        """tbf_process_rotors: Engine.process with the rotor planes; returns (L, R, hornL, hornR,
        drumL, drumR)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.n_instances
        if x.ndim != 2 or x.shape[0] != n or x.shape[1] % 128:
            raise ValueError(f"input shape {x.shape}: want ({n}, nblocks*128)")
        nb = x.shape[1] // 128
        return self._rotor_host(nb, lr, lambda l, r, ro: self._lib.tbf_process_rotors(
            self._h, nb, x.ctypes.data, x.shape[1], l, r, x.shape[1], ro))

    @staticmethod
    def _rotor_out(rotor_ptrs, rotor_stride):
        hl, hr, dl, dr = (None if p is None else int(p) for p in rotor_ptrs)
        return RotorOut(hl, hr, dl, dr, int(rotor_stride))

    def render_rotors_device(self, nblocks, outL_ptr, outR_ptr, stride, rotor_ptrs, rotor_stride, events=(),
                             stream=None):
        """tbf_render_rotors_device: enqueue a render into device memory; rotor_ptrs = (hornL,
        hornR, drumL, drumR) raw pointers of rotor_stride floats per instance, outL_ptr /
        outR_ptr raw pointers or both None, events as Engine.events."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        ro = self._rotor_out(rotor_ptrs, rotor_stride)
        _check(self._lib.tbf_render_rotors_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev),
            None if outL_ptr is None else C.c_void_p(int(outL_ptr)),
            None if outR_ptr is None else C.c_void_p(int(outR_ptr)), int(stride), C.byref(ro),
            None if stream is None else C.c_void_p(int(stream))))

    def process_rotors_device(self, nblocks, in_ptr, in_stride, outL_ptr, outR_ptr, stride, rotor_ptrs,
                              rotor_stride, events=(), stream=None):
        """tbf_process_rotors_device: render_rotors_device for an effects-only engine's
        device-resident input rows."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        ro = self._rotor_out(rotor_ptrs, rotor_stride)
        _check(self._lib.tbf_process_rotors_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev), C.c_void_p(int(in_ptr)),
            int(in_stride), None if outL_ptr is None else C.c_void_p(int(outL_ptr)),
            None if outR_ptr is None else C.c_void_p(int(outR_ptr)), int(stride), C.byref(ro),
            None if stream is None else C.c_void_p(int(stream))))

    def set_cabinet(self, irL, irR=None):
        """tbf_cabinet_set: the engine-wide cabinet response (irR None: irL for both channels;
        an empty irL: no cabinet).  Before the first add_instances."""
        l = np.ascontiguousarray(irL, dtype=np.float32).ravel()
        r = l if irR is None else np.ascontiguousarray(irR, dtype=np.float32).ravel()
        if len(l) != len(r):
            raise ValueError(f"irL has {len(l)} taps, irR {len(r)}")
        _check(self._lib.tbf_cabinet_set(self._h, l.ctypes.data if len(l) else None, r.ctypes.data if len(r) else None,
                                         len(l)))

    def cabinet_info(self, inst=0):
        """tbf_debug_cabinet: dict of taps, partitions, the history bytes per instance, the
        k_cabinet launches so far and instance inst's mix (None when it does not exist)"""
        f = self._lib.tbf_debug_cabinet
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, _u32p, _u32p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _fp]
        taps, parts, nb, nl, wet = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_float()
        has = inst < self.n_instances
        _check(f(self._h, int(inst), C.byref(taps), C.byref(parts), C.byref(nb), C.byref(nl), C.byref(wet) if has else None))
        return {"taps": taps.value, "partitions": parts.value, "instance_bytes": nb.value, "launches": nl.value,
                "wet": wet.value if has else None}

    def cabinet_time(self, enable=None):
        """tbf_debug_cabinet_time: enable True / False switches the event pair around every
        k_cabinet launch on / off; None returns (milliseconds, launches) since the last query."""
        return _stage_time(self._lib.tbf_debug_cabinet_time, self._h, enable)

    def _cabinet_host(self, nblocks, wet, rotors, call):
        shape = (self.n_instances, nblocks * 128)
        planes = [np.zeros(shape, np.float32) for _ in range(2 + (2 if wet else 0) + (4 if rotors else 0))]
        co = CabinetOut(planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data if wet else None,
                        planes[3].ctypes.data if wet else None, nblocks * 128)
        ro = RotorOut(*[p.ctypes.data for p in planes[-4:]], nblocks * 128) if rotors else None
        _check(call(C.byref(co), None if ro is None else C.byref(ro)))
        return tuple(planes)

    def render_cabinet(self, nblocks, wet=False, rotors=False):
        """tbf_render_cabinet: one synchronous render through the cabinet convolver; returns (L, R),
        then (wetL, wetR) with wet, then (hornL, hornR, drumL, drumR) with rotors, each
        [n_instances, nblocks*128]."""
        return self._cabinet_host(nblocks, wet, rotors, lambda co, ro: self._lib.tbf_render_cabinet(
            self._h, int(nblocks), co, ro))

    def process_cabinet(self, x, wet=False, rotors=False):
        """tbf_process_cabinet: render_cabinet for an effects-only engine's input x
        [n_instances, nblocks*128]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.n_instances
        if x.ndim != 2 or x.shape[0] != n or x.shape[1] % 128:
            raise ValueError(f"input shape {x.shape}: want ({n}, nblocks*128)")
        nb = x.shape[1] // 128
        return self._cabinet_host(nb, wet, rotors, lambda co, ro: self._lib.tbf_process_cabinet(
            self._h, nb, x.ctypes.data, x.shape[1], co, ro))

    @staticmethod
    def _cabinet_out(cab_ptrs, cab_stride):
        ptrs = [None if p is None else int(p) for p in cab_ptrs]
        ptrs += [None] * (4 - len(ptrs))
        return CabinetOut(*ptrs, int(cab_stride))

    def render_cabinet_device(self, nblocks, cab_ptrs, cab_stride, rotor_ptrs=None, rotor_stride=0, events=(),
                              stream=None):
        """tbf_render_cabinet_device: enqueue a render through the cabinet convolver into device
        memory; cab_ptrs = (L, R) or (L, R, wetL, wetR) raw pointers of cab_stride floats per
        instance, rotor_ptrs None or (hornL, hornR, drumL, drumR), events as Engine.events."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        co = self._cabinet_out(cab_ptrs, cab_stride)
        ro = None if rotor_ptrs is None else self._rotor_out(rotor_ptrs, rotor_stride)
        _check(self._lib.tbf_render_cabinet_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev), C.byref(co),
            None if ro is None else C.byref(ro), None if stream is None else C.c_void_p(int(stream))))

    def process_cabinet_device(self, nblocks, in_ptr, in_stride, cab_ptrs, cab_stride, rotor_ptrs=None, rotor_stride=0,
                               events=(), stream=None):
        """tbf_process_cabinet_device: render_cabinet_device for an effects-only engine's
        device-resident input rows."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        co = self._cabinet_out(cab_ptrs, cab_stride)
        ro = None if rotor_ptrs is None else self._rotor_out(rotor_ptrs, rotor_stride)
        _check(self._lib.tbf_process_cabinet_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev), C.c_void_p(int(in_ptr)),
            int(in_stride), C.byref(co), None if ro is None else C.byref(ro),
            None if stream is None else C.c_void_p(int(stream))))

    def set_output_rate(self, hz):
        """tbf_resampler_set: the engine-wide output rate of the *_resampled calls (0: none).
        Before the first add_instances."""
        _check(self._lib.tbf_resampler_set(self._h, int(hz)))

    def resampler_info(self, table=True):
        """tbf_debug_resampler: dict of L, M, T, the latency in engine-rate samples and (with
        table) the float32 prototype g[k] in k order"""
        f = self._lib.tbf_debug_resampler
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_void_p, C.c_uint64, _dp]
        L, M, T, lat = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_double()
        _check(f(self._h, C.byref(L), C.byref(M), C.byref(T), None, 0, C.byref(lat)))
        info = {"L": L.value, "M": M.value, "T": T.value, "latency": lat.value}
        if table:
            g = np.zeros(L.value * T.value, np.float32)
            _check(f(self._h, None, None, None, g.ctypes.data, len(g), None))
            info["table"] = g
        return info

    def resampled_frames(self, nblocks):
        """tbf_resampled_frames: the bound on any instance's count for a call of nblocks, and the
        least output stride"""
        m = C.c_uint64()
        _check(self._lib.tbf_resampled_frames(self._h, int(nblocks), C.byref(m)))
        return m.value

    def resample_ref(self, x, hist=None, pos0=0):
        """tbf_debug_resample_ref: the host restatement on one row: x the samples pos0 .., hist
        the T - 1 samples before them (None: zeros); returns the outputs the row gains"""
        f = self._lib.tbf_debug_resample_ref
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                      C.POINTER(C.c_uint64)]
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        h = None if hist is None else np.ascontiguousarray(hist, dtype=np.float32).ravel()
        n = C.c_uint64()
        y = np.zeros(self.resampled_frames((len(x) + 127) // 128) + 1, np.float32)
        _check(f(self._h, x.ctypes.data if len(x) else None, len(x), None if h is None else h.ctypes.data, int(pos0),
                 y.ctypes.data, len(y), C.byref(n)))
        return y[:n.value].copy()

    def resampler_pos(self, inst, pos):
        """tbf_debug_resampler_pos: set instance inst's position P; the history stays"""
        f = self._lib.tbf_debug_resampler_pos
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64]
        _check(f(self._h, int(inst), int(pos)))

    def resample_time(self, enable=None):
        """tbf_debug_resample_time: enable True / False switches the event pair around every
        k_resample launch on / off; None returns (milliseconds, launches) since the last query."""
        return _stage_time(self._lib.tbf_debug_resample_time, self._h, enable)

    def _resampled_host(self, nblocks, raw, call):
        n, frames = self.n_instances, self.resampled_frames(nblocks)
        planes = [np.zeros((n, frames), np.float32) for _ in range(2)]
        planes += [np.zeros((n, nblocks * 128), np.float32) for _ in range(2 if raw else 0)]
        counts = np.zeros(n, np.uint32)
        ro = ResampledOut(planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data if raw else None,
                          planes[3].ctypes.data if raw else None, frames, nblocks * 128, counts.ctypes.data)
        _check(call(C.byref(ro)))
        return tuple(planes) + (counts,)

    def render_resampled(self, nblocks, raw=False):
        """tbf_render_resampled: one synchronous render at the output rate; returns (L, R), then
        (rawL, rawR) with raw, then counts: L / R are [n_instances, resampled_frames(nblocks)] of
        which instance i's first counts[i] are its samples (the rest zeros)."""
        return self._resampled_host(nblocks, raw, lambda ro: self._lib.tbf_render_resampled(self._h, int(nblocks), ro))

    def process_resampled(self, x, raw=False):
        """tbf_process_resampled: render_resampled for an effects-only engine's input x
        [n_instances, nblocks*128]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.n_instances
        if x.ndim != 2 or x.shape[0] != n or x.shape[1] % 128:
            raise ValueError(f"input shape {x.shape}: want ({n}, nblocks*128)")
        nb = x.shape[1] // 128
        return self._resampled_host(nb, raw, lambda ro: self._lib.tbf_process_resampled(
            self._h, nb, x.ctypes.data, x.shape[1], ro))

    def _resampled_out(self, out_ptrs, stride, raw_ptrs, raw_stride):
        counts = np.zeros(self.n_instances, np.uint32)
        raw = (None, None) if raw_ptrs is None else raw_ptrs
        ptrs = [None if p is None else int(p) for p in tuple(out_ptrs) + tuple(raw)]
        return ResampledOut(*ptrs, int(stride), int(raw_stride), counts.ctypes.data), counts

    def render_resampled_device(self, nblocks, out_ptrs, stride, raw_ptrs=None, raw_stride=0, events=(), stream=None):
        """tbf_render_resampled_device: enqueue a render at the output rate into device memory;
        out_ptrs = (L, R) raw pointers of stride floats per instance, raw_ptrs None or (rawL,
        rawR) of raw_stride floats, events as Engine.events.  Returns the counts (host)."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        ro, counts = self._resampled_out(out_ptrs, stride, raw_ptrs, raw_stride)
        _check(self._lib.tbf_render_resampled_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev), C.byref(ro),
            None if stream is None else C.c_void_p(int(stream))))
        return counts

    def process_resampled_device(self, nblocks, in_ptr, in_stride, out_ptrs, stride, raw_ptrs=None, raw_stride=0,
                                 events=(), stream=None):
        """tbf_process_resampled_device: render_resampled_device for an effects-only engine's
        device-resident input rows."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        ro, counts = self._resampled_out(out_ptrs, stride, raw_ptrs, raw_stride)
        _check(self._lib.tbf_process_resampled_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev),
            None if in_ptr is None else C.c_void_p(int(in_ptr)), int(in_stride), C.byref(ro),
            None if stream is None else C.c_void_p(int(stream))))
        return counts

    @staticmethod
    def _pcm_array(fmt, n, frames):
        """the host array of n rows of frames frames: int16 [n, frames, 2], uint8 [n, frames * 6]
        or float32 [n, frames, 2]"""
        if fmt == PCM_S24_3LE:
            return np.zeros((n, frames * 6), np.uint8)
        return np.zeros((n, frames, 2), np.int16 if fmt == PCM_S16 else np.float32)

    @staticmethod
    def pcm_ref(fmt, L, R, flags=0, seed=0, row=0, frame0=0):
        """tbf_debug_pcm_ref: the host restatement of the PCM stage on one row (no device
        needed): returns (frames, meter): int16 [n, 2], uint8 [n * 6] or float32 [n, 2], and a
        METER_DTYPE scalar."""
        f = load_library().tbf_debug_pcm_ref
        f.restype = C.c_int
        f.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                      C.c_void_p, C.c_void_p]
        L = np.ascontiguousarray(L, dtype=np.float32).ravel()
        R = np.ascontiguousarray(R, dtype=np.float32).ravel()
        if len(L) != len(R):
            raise ValueError("L and R differ in length")
        out = Engine._pcm_array(int(fmt), 1, len(L))[0]
        meter = np.zeros(1, METER_DTYPE)
        _check(f(int(fmt), int(flags), int(seed), int(row), int(frame0), L.ctypes.data, R.ctypes.data, len(L),
                 out.ctypes.data, meter.ctypes.data))
        return out, meter[0]

    def pcm_time(self, enable=None):
        """tbf_debug_pcm_time: enable True / False switches the event pair around every k_pcm
        launch on / off; None returns (milliseconds, launches) since the last query."""
        return _stage_time(self._lib.tbf_debug_pcm_time, self._h, enable)

    @staticmethod
    def _pcm_out(out_ptr, out_stride_bytes, fmt, flags, seed, frame0, row_frame0, meters_ptr):
        """a PcmOut and the row_frame0 array it points to (keep it alive over the call)"""
        rf = None if row_frame0 is None else np.ascontiguousarray(row_frame0, dtype=np.uint64)
        po = PcmOut(None if out_ptr is None else int(out_ptr), int(out_stride_bytes),
                    None if meters_ptr is None else int(meters_ptr), int(fmt), int(flags), int(seed), int(frame0),
                    None if rf is None else rf.ctypes.data)
        return po, rf

    def _pcm_host(self, nblocks, fmt, flags, seed, frame0, row_frame0, meters, call):
        n, frames = self.n_instances, nblocks * 128
        out = self._pcm_array(int(fmt), n, frames)
        m = np.zeros(n, METER_DTYPE)
        po, _rf = self._pcm_out(out.ctypes.data, frames * PCM_FRAME_BYTES[int(fmt)], fmt, flags, seed, frame0, row_frame0,
                                m.ctypes.data if meters else None)
        _check(call(C.byref(po)))
        return (out, m) if meters else out

    def render_pcm(self, nblocks, fmt=PCM_S16, flags=0, seed=0, frame0=0, row_frame0=None, meters=False):
        """tbf_render_pcm: one synchronous render delivered as interleaved frames: int16
        [n_instances, frames, 2], uint8 [n_instances, frames * 6] (packed 24-bit) or float32
        [n_instances, frames, 2], frames = nblocks * 128; with meters, (frames, METER_DTYPE [n])."""
        return self._pcm_host(nblocks, fmt, flags, seed, frame0, row_frame0, meters,
                              lambda po: self._lib.tbf_render_pcm(self._h, int(nblocks), po))

    def process_pcm(self, x, fmt=PCM_S16, flags=0, seed=0, frame0=0, row_frame0=None, meters=False):
        """tbf_process_pcm: render_pcm for an effects-only engine's input x [n_instances, nblocks*128]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.n_instances
        if x.ndim != 2 or x.shape[0] != n or x.shape[1] % 128:
            raise ValueError(f"input shape {x.shape}: want ({n}, nblocks*128)")
        nb = x.shape[1] // 128
        return self._pcm_host(nb, fmt, flags, seed, frame0, row_frame0, meters,
                              lambda po: self._lib.tbf_process_pcm(self._h, nb, x.ctypes.data, x.shape[1], po))

    def render_pcm_device(self, nblocks, out_ptr, out_stride_bytes, fmt=PCM_S16, flags=0, seed=0, frame0=0, row_frame0=None,
                          meters_ptr=None, events=(), stream=None):
        """tbf_render_pcm_device: enqueue a render delivered as interleaved frames into device
        memory: row i from out_ptr + i * out_stride_bytes, meters_ptr None or device memory of one
        tbf_pcm_meter (16 B) per instance, events as Engine.events."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        po, _rf = self._pcm_out(out_ptr, out_stride_bytes, fmt, flags, seed, frame0, row_frame0, meters_ptr)
        _check(self._lib.tbf_render_pcm_device(self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev),
                                               C.byref(po), None if stream is None else C.c_void_p(int(stream))))

    def process_pcm_device(self, nblocks, in_ptr, in_stride, out_ptr, out_stride_bytes, fmt=PCM_S16, flags=0, seed=0,
                           frame0=0, row_frame0=None, meters_ptr=None, events=(), stream=None):
        """tbf_process_pcm_device: render_pcm_device for an effects-only engine's device-resident
        input rows."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        po, _rf = self._pcm_out(out_ptr, out_stride_bytes, fmt, flags, seed, frame0, row_frame0, meters_ptr)
        _check(self._lib.tbf_process_pcm_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev),
            None if in_ptr is None else C.c_void_p(int(in_ptr)), int(in_stride), C.byref(po),
            None if stream is None else C.c_void_p(int(stream))))

    def pcm_convert_device(self, n_rows, L_ptr, R_ptr, in_stride, frames, out_ptr, out_stride_bytes, fmt=PCM_S16, counts=None,
                           flags=0, seed=0, frame0=0, row_frame0=None, meters_ptr=None, stream=None):
        """tbf_pcm_convert_device: the PCM stage alone over any two device planes of n_rows rows
        (row r at r * in_stride floats): `frames` frames per row, or counts[r] (host array) of them."""
        c = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        po, _rf = self._pcm_out(out_ptr, out_stride_bytes, fmt, flags, seed, frame0, row_frame0, meters_ptr)
        _check(self._lib.tbf_pcm_convert_device(
            self._h, int(n_rows), C.c_void_p(int(L_ptr)), C.c_void_p(int(R_ptr)), int(in_stride), int(frames),
            None if c is None else c.ctypes.data, C.byref(po), None if stream is None else C.c_void_p(int(stream))))

    @staticmethod
    def _mix_rows(rows, n=None):
        """the rows as a contiguous MIX_ROW_DTYPE array (keep it alive over the call)"""
        r = np.ascontiguousarray(rows, dtype=MIX_ROW_DTYPE).reshape(-1)
        if n is not None and len(r) != n:
            raise ValueError(f"{len(r)} mix rows for {n} rows")
        return r

    @staticmethod
    def mix_ref(L, R, rows, n_buses, counts=None):
        """tbf_debug_mix_ref: the host restatement of the mixdown stage on host arrays (no device
        needed): L, R [n_rows, frames] float32 (the same array twice: mono planes), rows
        MIX_ROW_DTYPE [n_rows], counts None or [n_rows]; returns (busL, busR) [n_buses, frames]."""
        f = load_library().tbf_debug_mix_ref
        f.restype = C.c_int
        f.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                      C.POINTER(MixOut)]
        mono = L is R
        L = np.ascontiguousarray(L, dtype=np.float32)
        R = L if mono else np.ascontiguousarray(R, dtype=np.float32)
        if L.ndim != 2 or L.shape != R.shape:
            raise ValueError(f"planes of shape {L.shape} and {R.shape}: want two of [n_rows, frames]")
        n, frames = L.shape
        r = Engine._mix_rows(rows, n)
        c = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        oL, oR = np.full((int(n_buses), frames), np.nan, np.float32), np.full((int(n_buses), frames), np.nan, np.float32)
        mo = MixOut(oL.ctypes.data, oR.ctypes.data, frames)
        _check(f(n, L.ctypes.data, R.ctypes.data, frames, frames, None if c is None else c.ctypes.data,
                 r.ctypes.data if n else None, int(n_buses), C.byref(mo)))
        return oL, oR

    @staticmethod
    def mix_grid(frames, n_buses):
        """tbf_debug_mix_grid: (frames per lane, frames per workgroup tile, buses per launch) of a
        k_mix call of `frames` frames and n_buses buses"""
        f = load_library().tbf_debug_mix_grid
        f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p]
        g, t, sl = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(f(int(frames), int(n_buses), C.byref(g), C.byref(t), C.byref(sl)))
        return g.value, t.value, sl.value

    def mix_time(self, enable=None):
        """tbf_debug_mix_time: enable True / False switches the event pair around every k_mix
        launch on / off; None returns (milliseconds, launches) since the last query."""
        return _stage_time(self._lib.tbf_debug_mix_time, self._h, enable)

    def mix_device(self, n_rows, L_ptr, R_ptr, in_stride, frames, rows, n_buses, outL_ptr, outR_ptr, out_stride, counts=None,
                   stream=None):
        """tbf_mix_device: the mixdown stage alone over any two device planes of n_rows rows (row r
        at r * in_stride floats; L_ptr == R_ptr: mono): rows MIX_ROW_DTYPE [n_rows] (params.mix_rows),
        `frames` frames per row or counts[r] (host array) of them, into n_buses rows of `frames`
        frames at outL_ptr / outR_ptr, out_stride floats apart."""
        r = self._mix_rows(rows, int(n_rows))
        c = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        mo = MixOut(int(outL_ptr), int(outR_ptr), int(out_stride))
        _check(self._lib.tbf_mix_device(
            self._h, int(n_rows), C.c_void_p(int(L_ptr)), C.c_void_p(int(R_ptr)), int(in_stride), int(frames),
            None if c is None else c.ctypes.data, r.ctypes.data if len(r) else None, int(n_buses), C.byref(mo),
            None if stream is None else C.c_void_p(int(stream))))

    def _mix_host(self, nblocks, rows, n_buses, call):
        r = self._mix_rows(rows, self.n_instances)
        L, R = np.zeros((int(n_buses), nblocks * 128), np.float32), np.zeros((int(n_buses), nblocks * 128), np.float32)
        mo = MixOut(L.ctypes.data, R.ctypes.data, nblocks * 128)
        _check(call(r.ctypes.data if len(r) else None, C.byref(mo)))
        return L, R

    def render_mix(self, nblocks, rows, n_buses):
        """tbf_render_mix: one synchronous render summed into n_buses stereo buses: rows
        MIX_ROW_DTYPE [n_instances] (params.mix_rows), row r = instance r; returns (L, R), each
        [n_buses, nblocks*128]."""
        return self._mix_host(nblocks, rows, n_buses, lambda r, mo: self._lib.tbf_render_mix(
            self._h, int(nblocks), r, int(n_buses), mo))

    def process_mix(self, x, rows, n_buses):
        """tbf_process_mix: render_mix for an effects-only engine's input x [n_instances, nblocks*128]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = self.n_instances
        if x.ndim != 2 or x.shape[0] != n or x.shape[1] % 128:
            raise ValueError(f"input shape {x.shape}: want ({n}, nblocks*128)")
        nb = x.shape[1] // 128
        return self._mix_host(nb, rows, n_buses, lambda r, mo: self._lib.tbf_process_mix(
            self._h, nb, x.ctypes.data, x.shape[1], r, int(n_buses), mo))

    def render_mix_device(self, nblocks, rows, n_buses, outL_ptr, outR_ptr, out_stride, events=(), stream=None):
        """tbf_render_mix_device: enqueue a render summed into n_buses stereo buses in device
        memory: bus b from outL_ptr / outR_ptr + b * out_stride floats, events as Engine.events."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        r = self._mix_rows(rows, self.n_instances)
        mo = MixOut(int(outL_ptr), int(outR_ptr), int(out_stride))
        _check(self._lib.tbf_render_mix_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev), r.ctypes.data if len(r) else None,
            int(n_buses), C.byref(mo), None if stream is None else C.c_void_p(int(stream))))

    def process_mix_device(self, nblocks, in_ptr, in_stride, rows, n_buses, outL_ptr, outR_ptr, out_stride, events=(),
                           stream=None):
        """tbf_process_mix_device: render_mix_device for an effects-only engine's device-resident
        input rows."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE) if len(events) else np.zeros(0, EVENT_DTYPE)
        r = self._mix_rows(rows, self.n_instances)
        mo = MixOut(int(outL_ptr), int(outR_ptr), int(out_stride))
        _check(self._lib.tbf_process_mix_device(
            self._h, int(nblocks), ev.ctypes.data if len(ev) else None, len(ev),
            None if in_ptr is None else C.c_void_p(int(in_ptr)), int(in_stride), r.ctypes.data if len(r) else None,
            int(n_buses), C.byref(mo), None if stream is None else C.c_void_p(int(stream))))

    def limiter(self, n_rows, ceiling, ahead=64, hold=0, oversample=None):
        """tbf_limiter_create: a look-ahead peak limiter of n_rows rows on this engine's device
        (ceiling in float32; ahead a power of two in [2, LIMIT_MAX_AHEAD]; hold in
        [0, LIMIT_MAX_HOLD] frames); the engine releases it when it closes.  oversample 2 or 4
        (limiter_oversample(rate) picks one): tbf_limiter_create_tp, the same limiter with a
        true-peak detector, 6 frames more latency and 11 more of history."""
        cfg = LimiterConfig(float(ceiling), int(ahead), int(hold))
        h = C.c_void_p()
        if oversample is None:
            _check(self._lib.tbf_limiter_create(self._h, int(n_rows), C.byref(cfg), C.byref(h)))
            return Limiter(self, h, int(n_rows), cfg)
        det = LimiterDetect(int(oversample), 0)
        _check(self._lib.tbf_limiter_create_tp(self._h, int(n_rows), C.byref(cfg), C.byref(det), C.byref(h)))
        return Limiter(self, h, int(n_rows), cfg, int(oversample))

    @staticmethod
    def limit_ref(L, R, ceiling, ahead=64, hold=0, hist=None, oversample=None):
        """tbf_debug_limit_ref: the host restatement of the limiter on one row (no device needed):
        L, R [n] float32 (the same array twice: mono), hist None (a new row) or the (histL, histR)
        an earlier call returned; returns (outL, outR, LIMIT_METER_DTYPE record, (histL, histR)).
        oversample 2 or 4: tbf_debug_limit_tp_ref, the limiter with a true-peak detector, whose
        histories are 11 frames longer."""
        tp = oversample is not None
        f = load_library().tbf_debug_limit_tp_ref if tp else load_library().tbf_debug_limit_ref
        f.restype = C.c_int
        f.argtypes = [C.POINTER(LimiterConfig)] + ([C.POINTER(LimiterDetect)] if tp else []) + \
            [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        head = (C.byref(LimiterDetect(int(oversample), 0)),) if tp else ()
        mono = L is R
        L = np.ascontiguousarray(L, dtype=np.float32)
        R = L if mono else np.ascontiguousarray(R, dtype=np.float32)
        if L.ndim != 1 or L.shape != R.shape:
            raise ValueError(f"rows of shape {L.shape} and {R.shape}: want two of [n]")
        cfg = LimiterConfig(float(ceiling), int(ahead), int(hold))
        hn = max(2 * int(ahead) + int(hold) - 2, 0) + (11 if tp else 0)
        hL, hR = (np.zeros(hn, np.float32), np.zeros(hn, np.float32)) if hist is None else \
            (np.array(hist[0], np.float32), np.array(hist[1], np.float32))
        oL, oR = np.full(len(L), np.nan, np.float32), np.full(len(L), np.nan, np.float32)
        m = np.zeros(1, LIMIT_METER_DTYPE)
        _check(f(C.byref(cfg), *head, L.ctypes.data, R.ctypes.data, len(L), hL.ctypes.data, hR.ctypes.data, oL.ctypes.data,
                 oR.ctypes.data, m.ctypes.data))
        return oL, oR, m[0], (hL, hR)

    @staticmethod
    def limit_grid(ceiling, ahead=64, hold=0, oversample=None):
        """tbf_debug_limit_grid: (frames per lane, frames per workgroup tile, history frames Hn, LDS
        bytes per workgroup) of k_limit under a configuration; oversample 2 or 4:
        tbf_debug_limit_tp_grid, the same of k_limit_tp"""
        tp = oversample is not None
        f = load_library().tbf_debug_limit_tp_grid if tp else load_library().tbf_debug_limit_grid
        f.restype = C.c_int
        f.argtypes = [C.POINTER(LimiterConfig)] + ([C.POINTER(LimiterDetect)] if tp else []) + [_u32p, _u32p, _u32p, _u32p]
        head = (C.byref(LimiterDetect(int(oversample), 0)),) if tp else ()
        cfg = LimiterConfig(float(ceiling), int(ahead), int(hold))
        g, t, h, b = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(f(C.byref(cfg), *head, C.byref(g), C.byref(t), C.byref(h), C.byref(b)))
        return g.value, t.value, h.value, b.value

    def loudness(self, n_rows, rate_hz=None, max_hops=6000):
        """tbf_loudness_create: a BS.1770 loudness meter of n_rows rows on this engine's device, at
        rate_hz (None: the engine's rate), each row holding up to max_hops 100 ms hops between
        resets (16 B each); the engine releases it when it closes"""
        cfg = LoudnessConfig(int(round(self.sample_rate)) if rate_hz is None else int(rate_hz), int(max_hops))
        h = C.c_void_p()
        _check(self._lib.tbf_loudness_create(self._h, int(n_rows), C.byref(cfg), C.byref(h)))
        return Loudness(self, h, int(n_rows), cfg)

    @staticmethod
    def loudness_coeffs(rate_hz):
        """tbf_debug_loudness_coeffs: b0, b1, b2, a1, a2 of the shelf and c1, c2 of the high-pass"""
        f = load_library().tbf_debug_loudness_coeffs
        f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_void_p]
        c = np.zeros(7, np.float64)
        _check(f(int(rate_hz), c.ctypes.data))
        return c

    @staticmethod
    def loudness_ref(L, R, rate_hz, state=None, cap_hops=None):
        """tbf_debug_loudness_ref: the host restatement of the meter's recurrence on one row (no
        device needed): L, R [n] float32 (the same array twice: equal channels), state None (a new
        row) or the 12 doubles an earlier call returned; returns (energies [hops, 2] of the hops
        these frames complete, state).  cap_hops None: as many as are needed."""
        f = load_library().tbf_debug_loudness_ref
        f.restype = C.c_int
        f.argtypes = [C.POINTER(LoudnessConfig), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, _u32p]
        same = L is R
        L = np.ascontiguousarray(L, dtype=np.float32)
        R = L if same else np.ascontiguousarray(R, dtype=np.float32)
        if L.ndim != 1 or L.shape != R.shape:
            raise ValueError(f"rows of shape {L.shape} and {R.shape}: want two of [n]")
        cfg = LoudnessConfig(int(rate_hz), 1)
        st = np.zeros(12, np.float64) if state is None else np.array(state, np.float64)
        if st.shape != (12,):
            raise ValueError("state: want 12 doubles")
        cap = len(L) // max(int(rate_hz) // 10, 1) + 1 if cap_hops is None else int(cap_hops)
        e = np.zeros((cap, 2), np.float64)
        n = C.c_uint32()
        _check(f(C.byref(cfg), L.ctypes.data, R.ctypes.data, len(L), st.ctypes.data, e.ctypes.data, cap, C.byref(n)))
        return e[:n.value].copy(), st

    @staticmethod
    def loudness_result(rate_hz, energies):
        """tbf_debug_loudness_result: the gating alone on [hops, 2] energies; one
        LOUDNESS_RESULT_DTYPE record"""
        from .params import LOUDNESS_RESULT_DTYPE
        f = load_library().tbf_debug_loudness_result
        f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        e = np.ascontiguousarray(energies, dtype=np.float64).reshape(-1, 2)
        out = np.zeros(1, LOUDNESS_RESULT_DTYPE)
        _check(f(int(rate_hz), e.ctypes.data if len(e) else None, len(e), out.ctypes.data))
        return out[0]

    @staticmethod
    def loudness_grid(n_rows=1):
        """tbf_debug_loudness_grid: (rows per workgroup, frames per LDS tile, LDS bytes per
        workgroup) of k_loud"""
        f = load_library().tbf_debug_loudness_grid
        f.restype, f.argtypes = C.c_int, [C.c_uint32, _u32p, _u32p, _u32p]
        g, t, b = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(f(int(n_rows), C.byref(g), C.byref(t), C.byref(b)))
        return g.value, t.value, b.value

    @staticmethod
    def loudness_range(rate_hz, energies):
        """tbf_debug_loudness_range: the loudness range alone on [hops, 2] energies; (LRA in LU, the
        short-term windows behind it)"""
        f = load_library().tbf_debug_loudness_range
        f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_void_p, C.c_uint32, _dp, _u32p]
        e = np.ascontiguousarray(energies, dtype=np.float64).reshape(-1, 2)
        lra, win = C.c_double(), C.c_uint32()
        _check(f(int(rate_hz), e.ctypes.data if len(e) else None, len(e), C.byref(lra), C.byref(win)))
        return lra.value, win.value

    def equalizer(self, n_rows, max_bands=8, rate_hz=None):
        """tbf_eq_create: a bus equaliser of n_rows rows of up to max_bands (1 .. 8) bands each on this
        engine's device, designed at rate_hz (None: the engine's rate); no row has a band until
        Equalizer.set; the engine releases it when it closes"""
        cfg = EqConfig(int(round(self.sample_rate)) if rate_hz is None else int(rate_hz), int(max_bands))
        h = C.c_void_p()
        _check(self._lib.tbf_eq_create(self._h, int(n_rows), C.byref(cfg), C.byref(h)))
        return Equalizer(self, h, int(n_rows), cfg)

    @staticmethod
    def eq_coeffs(band, rate_hz):
        """tbf_debug_eq_coeffs: b0, b1, b2, a1, a2 of one params.eq_band record at a rate"""
        from .params import EQ_BAND_DTYPE
        f = load_library().tbf_debug_eq_coeffs
        f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p]
        b = np.array(band, dtype=EQ_BAND_DTYPE).reshape(1)
        c = np.zeros(5, np.float64)
        _check(f(int(rate_hz), b.ctypes.data, c.ctypes.data))
        return c

    @staticmethod
    def eq_ref(L, R, coeffs, state=None):
        """tbf_debug_eq_ref: the host restatement of the equaliser on one row (no device needed):
        L, R [n] float32 (the same array twice: mono) through the bands coeffs [nb, 5], state None
        (a new row) or the [2, nb, 2] doubles an earlier call returned; returns (outL, outR, state)."""
        f = load_library().tbf_debug_eq_ref
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        mono = L is R
        L = np.ascontiguousarray(L, dtype=np.float32)
        R = L if mono else np.ascontiguousarray(R, dtype=np.float32)
        if L.ndim != 1 or L.shape != R.shape:
            raise ValueError(f"rows of shape {L.shape} and {R.shape}: want two of [n]")
        c = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1, 5)
        st = np.zeros((2, len(c), 2), np.float64) if state is None else np.array(state, np.float64)
        if st.shape != (2, len(c), 2):
            raise ValueError(f"state of shape {st.shape}: want [2, {len(c)}, 2]")
        oL, oR = np.full(len(L), np.nan, np.float32), np.full(len(L), np.nan, np.float32)
        _check(f(c.ctypes.data if len(c) else None, len(c), L.ctypes.data, R.ctypes.data, len(L),
                 st.ctypes.data if len(c) else None, oL.ctypes.data, oR.ctypes.data))
        return oL, oR, st

    @staticmethod
    def eq_grid(max_bands):
        """tbf_debug_eq_grid: (P lanes per row and channel, rows per wave, frames per LDS tile, LDS
        bytes per workgroup) of k_eq for an equaliser of max_bands"""
        f = load_library().tbf_debug_eq_grid
        f.restype, f.argtypes = C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, _u32p]
        p, r, t, b = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(f(int(max_bands), C.byref(p), C.byref(r), C.byref(t), C.byref(b)))
        return p.value, r.value, t.value, b.value

    def compressor(self, n_rows, n_curves=1):
        """tbf_comp_create: a bus compressor of n_rows rows and n_curves (1 .. 8) gain curves on this
        engine's device; every curve is flat and every row at its defaults until Compressor.set_curve
        and .set_rows; the engine releases it when it closes"""
        cfg = CompConfig(int(n_curves))
        h = C.c_void_p()
        _check(self._lib.tbf_comp_create(self._h, int(n_rows), C.byref(cfg), C.byref(h)))
        return Compressor(self, h, int(n_rows), cfg)

    @staticmethod
    def comp_ref(L, R, pts, attack=0.0, release=0.0, makeup=1.0, g=1.0, key=None):
        """tbf_debug_comp_ref: the host restatement of the compressor on one row (no device needed):
        L, R [n] float32 (the same array twice: mono) through the curve pts [769] with the float32
        coefficients and make-up, behind the gain g, keyed by key = (kL, kR) or by themselves;
        returns (outL, outR, g behind the last frame, gains [n])."""
        f = load_library().tbf_debug_comp_ref
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        mono = L is R
        L = np.ascontiguousarray(L, dtype=np.float32)
        R = L if mono else np.ascontiguousarray(R, dtype=np.float32)
        if L.ndim != 1 or L.shape != R.shape:
            raise ValueError(f"rows of shape {L.shape} and {R.shape}: want two of [n]")
        kl = kr = None
        if key is not None:
            kl = np.ascontiguousarray(key[0], dtype=np.float32)
            kr = kl if key[1] is key[0] else np.ascontiguousarray(key[1], dtype=np.float32)
            if kl.shape != L.shape or kr.shape != L.shape:
                raise ValueError(f"key rows of shape {kl.shape} and {kr.shape}: want {L.shape}")
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1)
        if len(p) != 769:
            raise ValueError(f"{len(p)} points: want 769")
        gs = np.array([g], np.float32)
        oL, oR = np.full(len(L), np.nan, np.float32), np.full(len(L), np.nan, np.float32)
        gains = np.full(len(L), np.nan, np.float32)
        _check(f(p.ctypes.data, float(np.float32(attack)), float(np.float32(release)), float(np.float32(makeup)), L.ctypes.data,
                 R.ctypes.data, None if kl is None else kl.ctypes.data, None if kr is None else kr.ctypes.data, len(L),
                 gs.ctypes.data, oL.ctypes.data, oR.ctypes.data, gains.ctypes.data))
        return oL, oR, gs[0], gains

    @staticmethod
    def comp_lookup(pts, levels):
        """tbf_debug_comp_lookup: the curve pts [769] at the levels (float32, >= 0), float32"""
        f = load_library().tbf_debug_comp_lookup
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1)
        if len(p) != 769:
            raise ValueError(f"{len(p)} points: want 769")
        lv = np.ascontiguousarray(levels, dtype=np.float32).reshape(-1)
        t = np.full(len(lv), np.nan, np.float32)
        _check(f(p.ctypes.data, lv.ctypes.data, len(lv), t.ctypes.data))
        return t

    @staticmethod
    def comp_grid(n_rows, n_curves=1):
        """tbf_debug_comp_grid: (rows per wave, frames per LDS tile, LDS bytes per workgroup) of k_comp
        for a compressor of n_rows rows and n_curves curves"""
        f = load_library().tbf_debug_comp_grid
        f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p]
        r, t, b = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(f(int(n_rows), int(n_curves), C.byref(r), C.byref(t), C.byref(b)))
        return r.value, t.value, b.value

    def true_peak(self, n_rows, rate_hz=None, oversample=None):
        """tbf_true_peak_create: a true-peak meter of n_rows rows on this engine's device, at the
        oversampling factor `oversample` (1, 2 or 4) or the one of rate_hz (None: the engine's rate):
        4 below 96 kHz, 2 below 192 kHz, else 1; the engine releases it when it closes"""
        if oversample is None:
            oversample = true_peak_oversample(self.sample_rate if rate_hz is None else rate_hz)
        cfg = TruePeakConfig(int(oversample), 0)
        h = C.c_void_p()
        _check(self._lib.tbf_true_peak_create(self._h, int(n_rows), C.byref(cfg), C.byref(h)))
        return TruePeak(self, h, int(n_rows), cfg)

    @staticmethod
    def true_peak_table():
        """tbf_debug_true_peak_table: h[p][j], [4, 12] float32"""
        f = load_library().tbf_debug_true_peak_table
        f.restype, f.argtypes = C.c_int, [C.c_void_p]
        h = np.zeros((4, 12), np.float32)
        _check(f(h.ctypes.data))
        return h

    @staticmethod
    def true_peak_ref(L, R, oversample=4, hist=None, peaks=None, want_y=False):
        """tbf_debug_true_peak_ref: the host restatement of the meter on one row (no device needed):
        L, R [n] float32 (the same array twice: equal channels), hist None (a new row) or the 22
        floats and peaks None or the 4 words an earlier call returned.  Returns (peaks [4] uint32:
        the bit patterns of sample L, sample R, inter L, inter R; hist [22] float32), and with
        want_y also y [2, n, phases] float32."""
        f = load_library().tbf_debug_true_peak_ref
        f.restype = C.c_int
        f.argtypes = [C.POINTER(TruePeakConfig), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        same = L is R
        L = np.ascontiguousarray(L, dtype=np.float32)
        R = L if same else np.ascontiguousarray(R, dtype=np.float32)
        if L.ndim != 1 or L.shape != R.shape:
            raise ValueError(f"rows of shape {L.shape} and {R.shape}: want two of [n]")
        cfg = TruePeakConfig(int(oversample), 0)
        h = np.zeros(22, np.float32) if hist is None else np.array(hist, np.float32)
        p = np.zeros(4, np.uint32) if peaks is None else np.array(peaks, np.uint32)
        if h.shape != (22,) or p.shape != (4,):
            raise ValueError("hist: want 22 floats; peaks: want 4 words")
        ph = {4: 4, 2: 2}.get(int(oversample), 0)
        y = np.full((2, len(L), ph), np.nan, np.float32) if want_y else None
        _check(f(C.byref(cfg), L.ctypes.data, R.ctypes.data, len(L), h.ctypes.data, p.ctypes.data,
                 None if y is None else y.ctypes.data))
        return (p, h, y) if want_y else (p, h)

    @staticmethod
    def true_peak_dbtp(peaks):
        """tbf_debug_true_peak_dbtp: the read-out's dbtp of four peak words"""
        f = load_library().tbf_debug_true_peak_dbtp
        f.restype, f.argtypes = C.c_int, [C.c_void_p, _dp]
        p = np.ascontiguousarray(peaks, dtype=np.uint32).reshape(4)
        d = C.c_double()
        _check(f(p.ctypes.data, C.byref(d)))
        return d.value

    @staticmethod
    def true_peak_grid(n_rows=1, frames=0):
        """tbf_debug_true_peak_grid: (frames of a row per workgroup, frames per lane, workgroups of a
        call of `frames` frames on n_rows rows, LDS bytes per workgroup) of k_tpeak"""
        f = load_library().tbf_debug_true_peak_grid
        f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_uint32, _u32p, _u32p, C.POINTER(C.c_uint64), _u32p]
        t, g, n, b = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
        _check(f(int(n_rows), int(frames), C.byref(t), C.byref(g), C.byref(n), C.byref(b)))
        return t.value, g.value, n.value, b.value

    def synchronize(self):
        _check(self._lib.tbf_synchronize(self._h))

    def kernel_times(self, enable=None):
        """Per-stage HIP-event timing (tbf_debug_kernel_times): enable=True/False switches
        recording ("serial": with cross-chunk pipelining off, each kernel alone); with no
        argument returns {stage: (ms_total, launches)} since the last call."""
        fn = self._lib.tbf_debug_kernel_times
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        if enable is not None:
            _check(fn(self._h, -1 if not enable else (2 if enable == "serial" else 1), None, None))
            return None
        ms = np.zeros(8, np.float64)  # room for any build's stage count (A/B against older builds)
        cnt = np.zeros(8, np.uint32)
        _check(fn(self._h, 0, ms.ctypes.data, cnt.ctypes.data))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(STAGES)}

    def host_time(self, reset=True):
        """tbf_debug_host_time: (ms of host control stepping, blocks) since the last reset"""
        fn = self._lib.tbf_debug_host_time
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        ms, nb = C.c_double(), C.c_uint64()
        _check(fn(self._h, 1 if reset else 0, C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    def debug_reverb_phase(self, inst, ch, line, value):
        """test hook (tbf_debug_reverb_phase): set a reverb vibrato phase, from the next block"""
        fn = self._lib.tbf_debug_reverb_phase
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_double]
        _check(fn(self._h, int(inst), int(ch), int(line), float(value)))

    def error_flags(self):
        f = C.c_uint32()
        _check(self._lib.tbf_error_flags(self._h, C.byref(f)))
        return f.value
