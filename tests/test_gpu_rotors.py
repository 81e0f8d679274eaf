"""Whirl outputs beyond the mic mix, on the GPU: whirlProc's direct sum as the engine's L / R
(whirl_out = TBF_WHIRL_OUT_DIRECT) and whirlProc2's horn and drum pairs out of one render
(tbf_*_rotors*), bit for bit against the reference's own six whirlProc2 outputs
(tests/golden/rotor_vectors.npz) and against identities that tie them to what the rest of the
suite pins (the mic-mix engine, the CPU oracle, the reverb tap).  No tolerance anywhere; only
test_gpu_identity_drum_pair_is_the_oracle_without_horn compares values instead of bits (the
sign of a zero)."""
import functools
import json
import os

import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits, oracle_run
from test_rotors_cpu import bits, load_rotor_vectors, mic_mix

pytestmark = pytest.mark.gpu

MIC, DIRECT = 0, 1
FULL, TAP_REVERB, FX = 0, 3, 4
N = 3
SIX = ("L", "R", "HL", "HR", "DL", "DR")
WIDTHS = {"whirl.horn.width": 0.4, "whirl.drum.width": -0.3}


# ---------------------------------------------------------------- helpers
def _engine(sr=48000.0, chain=FULL, whirl_out=MIC, split=None, dbg=0, cfg=None):
    import tunebfree_amd as T
    if split is not None:
        os.environ["TBF_WHIRL_SPLIT"] = split
    try:
        eng = T.Engine(sample_rate=sr, device=0, chain=chain, debug_flags=dbg, whirl_out=whirl_out)
    finally:
        os.environ.pop("TBF_WHIRL_SPLIT", None)
    eng.config(cfg or {})
    return eng


def _organ(seeds, tpl_seed=7, mts=None, **kw):
    eng = _engine(**kw)
    tid = eng.template(mts128=mts, seed=tpl_seed)
    eng.add_instances([tid] * len(seeds), seeds)
    return eng


def _apply(eng, scens, s):
    for i, sc in enumerate(scens):
        for (b, kind, a, v) in sc:
            if b != s:
                continue
            if kind == "note":
                eng.note(i, a, v)
            elif kind == "control":
                assert eng.midi_control(i, a, v)
            else:
                eng.set_param(i, a, v)


def _bounds(scens, b0, nb):
    bounds = {b0, nb}
    for sc in scens:
        bounds.update(b for (b, *_r) in sc if b0 < b < nb)
    return sorted(bounds)


def _run(eng, scens, nb, how="rotors", b0=0):
    """The scripts from block b0 on as one host call per stretch between events (tbf_render /
    tbf_render_rotors with or without L / R); returns the call's arrays joined, [n, samples]."""
    call = {"render": lambda k: eng.render(k), "rotors": lambda k: eng.render_rotors(k),
            "rotors_nolr": lambda k: eng.render_rotors(k, lr=False)}[how]
    bounds = _bounds(scens, b0, nb)
    parts = []
    for s, e in zip(bounds[:-1], bounds[1:]):
        _apply(eng, scens, s)
        parts.append(call(e - s))
    return [None if p[0] is None else np.concatenate(p, axis=1) for p in zip(*parts)]


def _rows(eng, scens, nb):
    rows = []
    for i, sc in enumerate(scens):
        for (b, kind, a, v) in sc:
            if b >= nb:
                continue
            rows.append((b, i, 0, a, float(v)) if kind == "note" else
                        (b, i, 2, eng.control_id(a), float(v)) if kind == "control" else (b, i, 1, a, float(v)))
    rows.sort(key=lambda r: r[0])
    return eng.events(rows)


def _one_call(eng, scens, nb, lr=True, stride=None, lead=0, fill=0.0):
    """One tbf_render_rotors_device call with the scripts as events, into torch buffers of row
    stride `stride` floats that start `lead` floats into their allocation and are filled with
    `fill` first; returns the six whole buffers [n, stride] as numpy (L, R None without lr)."""
    import torch
    n = eng.n_instances
    stride = stride or nb * 128
    flat = [torch.full((lead + n * stride,), fill, dtype=torch.float32, device="cuda") for _ in range(6)]
    ptr = [t.data_ptr() + 4 * lead for t in flat]
    eng.render_rotors_device(nb, ptr[0] if lr else None, ptr[1] if lr else None, stride, ptr[2:], stride,
                             events=_rows(eng, scens, nb))
    eng.synchronize()
    out = [t.cpu().numpy()[lead:].reshape(n, stride) for t in flat]
    return ([None, None] if not lr else out[:2]) + out[2:]


def _only(eng, split):
    la = eng.launches()
    ran, other = ("k_whirl_split", "k_whirl") if split == "1" else ("k_whirl", "k_whirl_split")
    assert la[ran] > 0 and la[other] == 0, (split, la)


def _mic_of(hw, dw):
    """the microphone mix whirlProc3 applies for the two widths (src/whirl.cpp whirlConfig /
    computeOffsets: clamp, then square roots in float): hll hlr dll dlr hrl hrr drl drr"""
    f = np.float32
    hwP, hwN = f(min(max(hw, 0.0), 1.0)), f(min(max(-hw, 0.0), 1.0))
    dwP, dwN = f(min(max(dw, 0.0), 1.0)), f(min(max(-dw, 0.0), 1.0))
    return np.array([np.sqrt(f(1) - hwP), np.sqrt(f(0) + hwP), np.sqrt(f(1) - dwP), np.sqrt(f(0) + dwP),
                     np.sqrt(f(0) + hwN), np.sqrt(f(1) - hwN), np.sqrt(f(0) + dwN), np.sqrt(f(1) - dwN)], np.float32)


def _distinct_and_finite(arrs, what):
    for a in arrs:
        assert np.isfinite(a).all() and float(np.abs(a).max()) > 1e-3, what
        for i in range(len(a)):
            for j in range(i):
                assert not np.array_equal(bits(a[i]), bits(a[j])), f"{what}: instances {j} and {i} are the same"


@functools.lru_cache(None)
def _gold():
    from golden.make_ref_vectors import load_vectors
    from pathlib import Path
    vec, cases = load_rotor_vectors()
    ref = load_vectors()
    table = {t["name"]: t for t in json.loads(str(ref["cases"]))}
    tunings = json.loads((Path(__file__).resolve().parent / "golden" / "tunings.json").read_text())
    return vec, {c["name"]: c for c in cases}, table, tunings


def _case(name):
    """the case's streams (instance 0 plays it), its scripts for N instances, and an engine maker"""
    from golden.make_ref_vectors import scenario
    vec, cases, table, tunings = _gold()
    c, base = cases[name], table[cases[name]["base"]]
    want = {k: vec[f"{name}/{k}"] for k in SIX}
    want["micL"], want["micR"] = mic_mix(c["mic"], *[want[k] for k in SIX[2:]])
    scens = [scenario(*base["scenario"])] * N
    mts = None if base["tuning"] is None else np.array(tunings[base["tuning"]], np.float64)
    seeds = [base["inst_seed"] + 101 * i for i in range(N)]

    def make(**kw):
        return _organ(seeds, tpl_seed=base["tpl_seed"], mts=mts, sr=base["sr"], cfg=c["cfg"], **kw)
    return want, scens, base["nblocks"], make, c


def _check_six(got, want, whirl_out, what):
    """instance 0's streams against the archive (L / R: the direct sum or the mic mix); the other
    instances finite and distinct"""
    for k, a in zip(SIX, got):
        if a is None:
            continue
        ref = want[k] if whirl_out == DIRECT or k not in "LR" else want["mic" + k]
        assert_bits(a[0], ref, f"{what} {k}")
    _distinct_and_finite([a for a in got if a is not None], what)


# ---------------------------------------------------------------- 1. the fixture cases
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("name", ["sweep48_3", "bench96_p4", "events192_p4", "levels48"])
def test_gpu_rotor_fixtures(name, split):
    """One tbf_render_rotors_device call with the case's script as events (72-block cases cross
    the 64-block event chunk: outOffset on the new planes): all six streams are the reference's,
    on a mic-mix engine (L / R = the committed whirlProc3 output), on a direct engine, and
    without L / R."""
    want, scens, nb, make, c = _case(name)
    for whirl_out, lr in ((MIC, True), (DIRECT, True), (MIC, False)):
        eng = make(whirl_out=whirl_out, split=split)
        assert eng.layout()["wring_len"] == c["window"]
        got = _one_call(eng, scens, nb, lr=lr)
        _only(eng, split)
        eng.close()
        _check_six(got, want, whirl_out, f"{name} split={split} whirl_out={whirl_out} lr={lr}")


@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_rotor_fixture_host_calls_forced_serial(split):
    """tbf_render_rotors (host buffers, one call per stretch between events) under
    TBF_DEBUG_FORCE_SERIAL, with and without L / R on a direct engine."""
    want, scens, nb, make, _c = _case("sweep48_3")
    for how in ("rotors", "rotors_nolr"):
        eng = make(whirl_out=DIRECT, split=split, dbg=1)
        got = _run(eng, scens, nb, how)
        _only(eng, split)
        eng.close()
        _check_six(got, want, DIRECT, f"sweep48_3 forced serial split={split} {how}")


# ---------------------------------------------------------------- 2. DIRECT through the old calls
@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_direct_through_render_calls(split):
    """A direct engine's tbf_render, tbf_render_device and tbf_render_events deliver whirlProc's
    outL / outR in the usual two buffers."""
    import torch
    want, scens, nb, make, _c = _case("sweep48_3")
    eng = make(whirl_out=DIRECT, split=split)
    L, R = _run(eng, scens, nb, "render")
    eng.close()
    _check_six([L, R], want, DIRECT, f"tbf_render split={split}")

    eng = make(whirl_out=DIRECT, split=split)
    dL = torch.zeros((N, nb * 128), dtype=torch.float32, device="cuda")
    dR = torch.zeros_like(dL)
    bounds = _bounds(scens, 0, nb)
    for s, e in zip(bounds[:-1], bounds[1:]):
        _apply(eng, scens, s)
        eng.render_device(e - s, dL[:, s * 128:].data_ptr(), dR[:, s * 128:].data_ptr(), nb * 128)
    eng.synchronize()
    _only(eng, split)
    eng.close()
    _check_six([dL.cpu().numpy(), dR.cpu().numpy()], want, DIRECT, f"tbf_render_device split={split}")

    eng = make(whirl_out=DIRECT, split=split)
    dL.zero_()
    dR.zero_()
    eng.render_events_device(nb, _rows(eng, scens, nb), dL.data_ptr(), dR.data_ptr(), nb * 128)
    eng.synchronize()
    eng.close()
    _check_six([dL.cpu().numpy(), dR.cpu().numpy()], want, DIRECT, f"tbf_render_events split={split}")


@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_direct_through_synth_sound(split):
    """tbf_synth_sound on a direct engine, irregular frame counts through its FIFO (the 1024
    window; the case's events all land before the first block)."""
    want, scens, nb, make, _c = _case("bench96_p4")
    assert all(b == 0 for sc in scens for (b, *_r) in sc)
    eng = make(whirl_out=DIRECT, split=split)
    _apply(eng, scens, 0)
    frames, left, parts = [100, 37, 256, 1, 511, 128, 1000, 129], nb * 128, []
    while left:
        k = min(frames[len(parts) % len(frames)], left)
        parts.append(eng.synth_sound(k))
        left -= k
    eng.close()
    L, R = (np.concatenate(p, axis=1) for p in zip(*parts))
    _check_six([L, R], want, DIRECT, f"tbf_synth_sound split={split}")


# ---------------------------------------------------------------- 3. oracle identities
NB3 = 66  # cfg_scenario: rotors stop 6, fast 9, stop 26, slow 48, stop 60
SEEDS3 = [7100 + 13 * i for i in range(N)]


def _scens3():
    return [S.cfg_scenario(i) for i in range(N)]


@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_identity_mic_mix_of_rotor_streams(split):
    """(a) With both microphone widths off their defaults, whirlProc3's mix of the four rotor
    streams, in float32, is a mic-mix engine's L / R: those of the same call, those of a plain
    tbf_render on another engine, and the mix of a direct engine's rotor streams."""
    m = _mic_of(WIDTHS["whirl.horn.width"], WIDTHS["whirl.drum.width"])
    assert (m > 0).sum() == 6
    eng = _organ(SEEDS3, cfg=WIDTHS, split=split)
    plain = _run(eng, _scens3(), NB3, "render")
    eng.close()
    _distinct_and_finite(plain, "mic-mix engine")
    for whirl_out in (MIC, DIRECT):
        eng = _organ(SEEDS3, cfg=WIDTHS, split=split, whirl_out=whirl_out)
        L, R, HL, HR, DL, DR = _run(eng, _scens3(), NB3, "rotors")
        eng.close()
        mL, mR = mic_mix(m, HL, HR, DL, DR)
        assert_bits(mL, plain[0], f"mix of the rotor streams (whirl_out={whirl_out}) vs tbf_render, L")
        assert_bits(mR, plain[1], f"mix of the rotor streams (whirl_out={whirl_out}) vs tbf_render, R")
        if whirl_out == MIC:
            assert_bits(L, plain[0], "L of the rotor call vs tbf_render")
            assert_bits(R, plain[1], "R of the rotor call vs tbf_render")
        else:
            assert (bits(L) != bits(plain[0])).mean() > 0.1


@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_identity_drum_pair_is_the_oracle_without_horn(oracle, split):
    """(b) drumL / drumR are the oracle's whirlProc3 L / R of the same scripts with
    whirl.horn.level = 0 and whirl.horn.leak = 0 at the default widths (L = 0*1 + 0*0 + DL*1 +
    DR*0): equal as values, the sign of a zero aside."""
    from orc_bind import Cfg, Template
    tpl = Template(oracle, sr=48000.0, seed=7, cfg=Cfg(oracle, {"whirl.horn.level": 0, "whirl.horn.leak": 0}))
    oL, oR = oracle_run(oracle, tpl, SEEDS3, _scens3(), NB3)[:2]
    assert float(np.abs(oL).max()) > 1e-3 and float(np.abs(oR).max()) > 1e-3
    eng = _organ(SEEDS3, split=split)
    _L, _R, _HL, _HR, DL, DR = _run(eng, _scens3(), NB3, "rotors_nolr")
    eng.close()
    assert _L is None and _R is None
    for got, ref, k in ((DL, oL, "drumL"), (DR, oR, "drumR")):
        bad = got != ref
        assert not bad.any(), f"{k}: {int(bad.sum())} of {bad.size} samples differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_identity_direct_sum_without_leak(split):
    """(c) With whirl.horn.leak = 0 the direct sum (y + hornLevel*H) + 0 is float32 (drumL +
    hornL), hornL being hornLevel*H + 0."""
    eng = _organ(SEEDS3, cfg={"whirl.horn.leak": 0}, split=split, whirl_out=DIRECT)
    L, R, HL, HR, DL, DR = _run(eng, _scens3(), NB3, "rotors")
    eng.close()
    _distinct_and_finite([L, R, HL, HR, DL, DR], "leak 0")
    assert_bits(L, (DL + HL).astype(np.float32), "direct L vs drumL + hornL")
    assert_bits(R, (DR + HR).astype(np.float32), "direct R vs drumR + hornR")


# ---------------------------------------------------------------- 4. bypass mid-render
@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_bypass_toggled_mid_render(split):
    """P_WHIRL_BYPASS on and off inside one 70-block call (two event chunks) of a direct engine:
    in the bypassed blocks horn, L and R are the input, i.e. the reverb tap engine's output, and
    the drum pair is 0; on every block identity (a) holds against a mic-mix engine."""
    nb, spans = 70, ((5, 9), (30, 31), (62, 66))
    scens = []
    for i in range(N):
        sc = S.cfg_scenario(i)
        for (a, b) in spans:
            sc += [(a + i, "param", S.P_WHIRL_BYPASS, 1), (b + i, "param", S.P_WHIRL_BYPASS, 0)]
        scens.append(sorted(sc, key=lambda r: r[0]))
    m = _mic_of(WIDTHS["whirl.horn.width"], WIDTHS["whirl.drum.width"])
    eng = _organ(SEEDS3, cfg=WIDTHS, chain=TAP_REVERB)
    tap = _run(eng, scens, nb, "render")[0]
    eng.close()
    eng = _organ(SEEDS3, cfg=WIDTHS, split=split)
    plain = _run(eng, scens, nb, "render")
    eng.close()
    eng = _organ(SEEDS3, cfg=WIDTHS, split=split, whirl_out=DIRECT)
    L, R, HL, HR, DL, DR = _one_call(eng, scens, nb)
    _only(eng, split)
    eng.close()
    mL, mR = mic_mix(m, HL, HR, DL, DR)
    assert_bits(mL, plain[0], "mix of the rotor streams vs the mic-mix engine, L")
    assert_bits(mR, plain[1], "mix of the rotor streams vs the mic-mix engine, R")
    for i in range(N):
        by = np.zeros(nb * 128, bool)
        for (a, b) in spans:
            by[(a + i) * 128:(b + i) * 128] = True
        for k, a in (("L", L), ("R", R), ("hornL", HL), ("hornR", HR)):
            assert_bits(a[i][by], tap[i][by], f"bypassed blocks of instance {i}: {k} vs the reverb tap")
            assert (bits(a[i][~by]) != bits(tap[i][~by])).mean() > 0.5
        for k, a in (("drumL", DL), ("drumR", DR)):
            assert_bits(a[i][by], np.zeros(int(by.sum()), np.float32), f"bypassed blocks of instance {i}: {k}")
            assert float(np.abs(a[i][~by]).max()) > 1e-3


# ---------------------------------------------------------------- 5. effects-only chain
@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_fx_process_rotors(split):
    """tbf_process_rotors on caller audio: identities (a) and (c); an input that overlaps a rotor
    plane is refused."""
    import torch
    import tunebfree_amd as T
    nb = 24
    x = (np.random.default_rng(5).standard_normal((N, nb * 128)) * 0.2).astype(np.float32)
    m = _mic_of(WIDTHS["whirl.horn.width"], WIDTHS["whirl.drum.width"])

    def fx(**kw):
        eng = _organ(SEEDS3, chain=FX, split=split, **kw)
        for i in range(N):
            eng.set_param(i, S.P_HORN, 2 - i % 2)
            eng.set_param(i, S.P_DRUM, 2)
        return eng
    eng = fx(cfg=WIDTHS)
    plain = eng.process(x)
    eng.close()
    eng = fx(cfg=WIDTHS)
    L, R, HL, HR, DL, DR = eng.process_rotors(x)
    _only(eng, split)
    eng.close()
    _distinct_and_finite([L, R, HL, HR, DL, DR], "fx")
    mL, mR = mic_mix(m, HL, HR, DL, DR)
    for got, k in ((mL, 0), (mR, 1), (L, 0), (R, 1)):
        assert_bits(got, plain[k], f"fx: mix of the rotor streams / rotor call vs tbf_process, {'LR'[k]}")
    eng = fx(cfg={"whirl.horn.leak": 0}, whirl_out=DIRECT)
    L, R, HL, HR, DL, DR = eng.process_rotors(x)
    assert_bits(L, (DL + HL).astype(np.float32), "fx: direct L vs drumL + hornL")
    assert_bits(R, (DR + HR).astype(np.float32), "fx: direct R vs drumR + hornR")
    nl = eng.process_rotors(x, lr=False)
    assert nl[0] is None and nl[1] is None
    d = [torch.zeros((N, nb * 128), dtype=torch.float32, device="cuda") for _ in range(7)]
    p = [t.data_ptr() for t in d]
    for k in range(2, 6):
        with pytest.raises(T.TbfError, match="-22.*overlap"):
            eng.process_rotors_device(nb, p[k] + 4 * (nb * 128 - 1), nb * 128, p[0], p[1], nb * 128, p[2:6], nb * 128)
    eng.close()


# ---------------------------------------------------------------- 6. odd strides
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("whirl_out", [MIC, DIRECT])
def test_gpu_rotor_rows_odd_stride_sentinels(whirl_out, split):
    """Rows of an odd stride starting one float into their allocation: the six rows hold what
    an even-stride render holds, and nothing outside [0, nblocks*128) of a row changes."""
    nb, pad, sentinel = 5, 131, np.float32(-777.25)
    scens = [S.event_scenario(i) for i in range(N)]
    eng = _organ(SEEDS3, split=split, whirl_out=whirl_out)
    even = _one_call(eng, scens, nb)
    eng.close()
    for lr in (True, False):
        eng = _organ(SEEDS3, split=split, whirl_out=whirl_out)
        odd = _one_call(eng, scens, nb, lr=lr, stride=nb * 128 + pad, lead=1, fill=float(sentinel))
        eng.close()
        for k, a, b in zip(SIX, odd, even):
            if a is None:
                continue
            assert_bits(a[:, :nb * 128], b, f"odd stride lr={lr}: {k}")
            assert (a[:, nb * 128:] == sentinel).all(), f"odd stride lr={lr}: {k} wrote past its rows"


# ---------------------------------------------------------------- 7. save and load across modes
def test_gpu_save_on_mic_load_on_direct():
    """A blob saved on a mic-mix engine mid-script loads into a direct engine of otherwise equal
    configuration, whose rotor renders continue an uninterrupted run bit for bit."""
    nb, cut = 40, 17
    scens = [S.cfg_scenario(i) for i in range(N)]
    eng = _organ(SEEDS3, whirl_out=DIRECT)
    whole = _run(eng, scens, nb, "rotors")
    eng.close()
    src = _organ(SEEDS3, whirl_out=MIC)
    _run(src, scens, cut, "render")
    blob = src.save(list(range(N)))
    src.close()
    dst = _organ(SEEDS3, whirl_out=DIRECT)
    dst.load(list(range(N)), blob)
    rest = _run(dst, scens, nb, "rotors_nolr", b0=cut)
    dst.load(list(range(N)), blob)
    rest_lr = _run(dst, scens, nb, "rotors", b0=cut)
    dst.close()
    for k, a, b, w in zip(SIX, rest, rest_lr, whole):
        if a is not None:
            assert_bits(a, w[:, cut * 128:], f"after save / load, without L / R: {k}")
        assert_bits(b, w[:, cut * 128:], f"after save / load: {k}")
