"""Parameter ids of include/tbf.h: the CLAP ids of src/clap.cpp:31-48 plus the
setters the LV2/JACK hosts reach through MIDI CCs."""
import numpy as np

DRAWBAR_MIN, DRAWBAR_MAX = 0, 8
VIBRATO, VIBRATO_TYPE = 9, 10
DRUM, HORN = 11, 12
OVERDRIVE, CHARACTER, REVERB = 13, 14, 15
PERCUSSION, PERCUSSION_VOLUME, PERCUSSION_DECAY, PERCUSSION_HARMONIC = 16, 17, 18, 19
BUS_DRAWBAR_BASE = 100
VIBRATO_LOWER, SWELL, WHIRL_BYPASS = 130, 131, 132

CHAIN_FULL, CHAIN_TONEGEN = 0, 1
CHAIN_TAP_PREAMP, CHAIN_TAP_REVERB = 2, 3
# effects-only chains: the caller's audio through overdrive -> reverb -> whirl (Engine.process*)
CHAIN_FX, CHAIN_FX_TAP_PREAMP, CHAIN_FX_TAP_REVERB = 4, 5, 6

# tbf_engine_config.whirl_out: what L / R carry -- whirlProc3's microphone mix (the LV2 and CLAP
# shells) or whirlProc's direct sum (the JACK host's plain build); Engine(..., whirl_out=)
WHIRL_OUT_MIC, WHIRL_OUT_DIRECT = 0, 1

# the cabinet convolver (Engine.set_cabinet): the longest impulse response, in taps (TBF_CAB_MAX_TAPS)
CAB_MAX_TAPS = 8192

# the PCM output stage (Engine.render_pcm, .process_pcm, .pcm_convert_device): tbf_pcm_out.format
# (TBF_PCM_*: int16, packed 3-byte little-endian int24, float32 frames of L then R), the bytes per
# frame of each, and tbf_pcm_out.flags (TPDF dither, int16 only)
PCM_S16, PCM_S24_3LE, PCM_F32 = 0, 1, 2
PCM_FRAME_BYTES = (4, 6, 8)
PCM_DITHER = 1

# the mixdown stage (Engine.mix_device, .render_mix, .process_mix): tbf_mix_row.bus of a row that is
# in no bus (TBF_MIX_NONE), and the rows as a numpy record (20 B, as the C struct)
MIX_NONE = 0xFFFFFFFF
MIX_ROW_DTYPE = np.dtype([("bus", "<u4"), ("ll", "<f4"), ("lr", "<f4"), ("rl", "<f4"), ("rr", "<f4")])

# the bus limiter (Engine.limiter): the largest look-ahead (a power of two from 2) and hold in
# frames (TBF_LIMIT_MAX_*), and tbf_limit_meter as a numpy record (12 B, as the C struct)
LIMIT_MAX_AHEAD, LIMIT_MAX_HOLD = 512, 4096
LIMIT_METER_DTYPE = np.dtype([("min_gain", "<f4"), ("reduced", "<u4"), ("clamped", "<u4")])

# the loudness meter (Engine.loudness): tbf_loudness_result as a numpy record (40 B, as the C struct)
LOUDNESS_RESULT_DTYPE = np.dtype([("integrated", "<f8"), ("momentary_max", "<f8"), ("short_term_max", "<f8"),
                                  ("hops", "<u4"), ("blocks", "<u4"), ("gated", "<u4"), ("reserved", "<u4")])

# the true-peak meter (Engine.true_peak): tbf_true_peak_result as a numpy record (32 B, as the C struct)
TRUE_PEAK_RESULT_DTYPE = np.dtype([("sample_peak", "<f4", (2,)), ("inter_peak", "<f4", (2,)), ("frames", "<u8"),
                                   ("dbtp", "<f8")])

# the bus equaliser (Engine.equalizer): the band types (TBF_EQ_*, the RBJ designer's nine), the most
# bands of a row (TBF_EQ_MAX_BANDS), and tbf_eq_band as a numpy record (32 B, as the C struct)
EQ_LPF, EQ_HPF, EQ_BPF0, EQ_BPF1, EQ_NOTCH, EQ_APF, EQ_PEQ, EQ_LOW, EQ_HIGH = range(9)
EQ_MAX_BANDS = 8
EQ_BAND_DTYPE = np.dtype([("type", "<i4"), ("reserved", "<i4"), ("hz", "<f8"), ("q", "<f8"), ("gain_db", "<f8")])

# the bus compressor (Engine.compressor): the most curves (TBF_COMP_MAX_CURVES), the points of a curve
# (TBF_COMP_POINTS: 32 segments an octave from 2^-16 to 2^8), the largest make-up, and tbf_comp_row and
# tbf_comp_meter as numpy records (16 B and 8 B, as the C structs)
COMP_MAX_CURVES, COMP_SEG, COMP_POINTS, COMP_MAX_MAKEUP = 8, 32, 769, 256.0
COMP_ROW_DTYPE = np.dtype([("curve", "<u4"), ("attack", "<f4"), ("release", "<f4"), ("makeup", "<f4")])
COMP_METER_DTYPE = np.dtype([("min_gain", "<f4"), ("frames", "<u4")])


def comp_levels():
    """the levels of a compressor curve's 769 points, float64: point i at 2^(-16 + i // 32) (1 + (i % 32) / 32)"""
    i = np.arange(COMP_POINTS)
    return np.ldexp(1.0 + (i % COMP_SEG) / COMP_SEG, i // COMP_SEG - 16)


def comp_curve(threshold_db, ratio, knee_db=0.0):
    """tbf_comp_curve_design: the 769 float32 points of a compressor curve with the threshold in dB
    (-90 .. 0), the ratio (1 .. inf) and the soft knee's width in dB (0 .. 40), for
    Compressor.set_curve; the library refuses what lies outside."""
    from .engine import _check, load_library
    pts = np.zeros(COMP_POINTS, np.float32)
    _check(load_library().tbf_comp_curve_design(float(threshold_db), float(ratio), float(knee_db), pts.ctypes.data))
    return pts


def comp_row(curve=0, attack_ms=0.0, release_ms=0.0, makeup_db=0.0, rate=48000):
    """one tbf_comp_row record for Compressor.set_rows: the curve's index, the attack and release
    times as float32 coefficients exp(-1 / (ms * 1e-3 * rate)) computed in float64 (0 ms: 0), and
    the make-up 10^(dB / 20) as float32.  Nothing is checked here: the library refuses what lies
    outside its ranges."""
    def coef(ms):
        return 0.0 if ms == 0 else float(np.exp(-1.0 / (float(ms) * 1e-3 * float(rate))))
    r = np.zeros((), COMP_ROW_DTYPE)
    r["curve"], r["attack"], r["release"], r["makeup"] = int(curve), coef(attack_ms), coef(release_ms), 10.0 ** (float(makeup_db) / 20.0)
    return r


def eq_band(kind, hz, q=0.7071, gain_db=0.0):
    """one tbf_eq_band record for Equalizer.set / Engine.eq_coeffs: kind one of EQ_LPF .. EQ_HIGH,
    the frequency in Hz, the Q, and the gain in dB (PEQ and the shelves).  Nothing is checked here:
    the library refuses what lies outside its ranges."""
    b = np.zeros((), EQ_BAND_DTYPE)
    b["type"], b["hz"], b["q"], b["gain_db"] = int(kind), float(hz), float(q), float(gain_db)
    return b


def mix_rows(bus, gain=1.0, pan=0.0):
    """tbf_mix_row records for Engine.mix_device / .render_mix / .process_mix: row r goes to bus
    bus[r] (MIX_NONE: to none) at gain[r] and pan[r] in [-1, 1] (scalars apply to every row), by a
    constant-power law with unity at centre: ll = sqrt(2) g cos((pan + 1) pi / 4),
    rr = sqrt(2) g sin((pan + 1) pi / 4), lr = rl = 0, computed in float64 and rounded to float32.
    A convenience: the ABI knows only the four numbers, which a caller may set as it likes."""
    bus = np.atleast_1d(np.asarray(bus, dtype=np.int64))
    g = np.broadcast_to(np.asarray(gain, dtype=np.float64), bus.shape)
    p = np.broadcast_to(np.asarray(pan, dtype=np.float64), bus.shape)
    if np.any(np.abs(p) > 1.0):
        raise ValueError("pan outside [-1, 1]")
    a = (p + 1.0) * (np.pi / 4.0)
    rows = np.zeros(bus.shape, MIX_ROW_DTYPE)
    rows["bus"] = np.where(bus < 0, MIX_NONE, bus).astype(np.uint32)
    rows["ll"] = (np.sqrt(2.0) * g * np.cos(a)).astype(np.float32)
    rows["rr"] = (np.sqrt(2.0) * g * np.sin(a)).astype(np.float32)
    return rows


def gain_rows(gains):
    """tbf_mix_row records that apply a gain per row through Engine.mix_device: one bus per row
    (row r to bus r) with ll = rr = gains[r] as float32 and lr = rl = 0, so bus r is gains[r] times
    row r (Loudness.gains gives the gains that bring every row to a target loudness)."""
    g = np.atleast_1d(np.asarray(gains, dtype=np.float32))
    rows = np.zeros(g.shape, MIX_ROW_DTYPE)
    rows["bus"] = np.arange(len(g), dtype=np.uint32)
    rows["ll"] = rows["rr"] = g
    return rows
