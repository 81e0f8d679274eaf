"""The edges of what the engine accepts: whatever it accepts, it renders bit for bit.

A chain that runs the whirl is refused when the geometry's smallest write-ahead is under one
64-sample sub-block (TBF_WH_MIN_LEAD, buildShared in csrc/tbf_engine.cpp) or its largest
passes the reference's 2048-sample ring.  The tests here find the edges by asking host-only
engines, not from constants, and render at them: the lowest accepted rate, the nearest
accepted microphone, 192 kHz with the ring all but full; every stage tap at rates the rest
of the suite never runs; and the chains without the whirl at the low rates they keep.  Every
comparison is enginerun.assert_bits against the CPU oracle (itself bit-identical to the
reference at these rates: test_oracle_cpu.py)."""
import functools
import math
import os

import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits, engine_run, oracle_run
from test_gpu_parity import DISPATCH, TAPS, _all_taps, _organ, _ran, _ref_once, _setup

pytestmark = pytest.mark.gpu

S_FX = 4  # TBF_CHAIN_FX
SECONDS = 0.45  # of both rotors fast: more than two horn turns at 7.06 turns per second


def _accepted(rate, cfg=None, chain=0):
    """whether a host-only engine of the chain takes the rate and the cfg keys; a refusal
    must be the write-ahead one"""
    import tunebfree_amd as T
    try:
        eng = T.Engine(sample_rate=rate, device=-1, chain=chain)
        try:
            eng.config(cfg or {})
        finally:
            eng.close()
    except T.TbfError as e:
        assert "whirl write-ahead" in str(e) and "-22" in str(e), e
        return False
    return True


@functools.lru_cache(None)
def _r0():
    """the lowest rate a full-chain engine accepts, from 35000 Hz upward in 100 Hz steps"""
    r0 = next((float(r) for r in range(35000, 44101, 100) if _accepted(float(r))), None)
    assert r0 is not None, "no rate up to 44100 Hz is accepted"
    assert not _accepted(r0 - 100.0) and _accepted(r0, chain=S_FX) and not _accepted(r0 - 100.0, chain=S_FX)
    return r0


@functools.lru_cache(None)
def _d0(rate):
    """the nearest microphone (whole centimetres from 20) a full-chain engine accepts"""
    d0 = next((d for d in range(20, 43) if _accepted(rate, {"whirl.mic.distance": d})), None)
    assert d0 is not None and d0 > 20, d0
    assert not _accepted(rate, {"whirl.mic.distance": d0 - 1})
    return d0


def _render(scens, calls, rate, cfg=None, dbg=0, split="0"):
    """The scripts as consecutive tbf_render_events calls [(first block, blocks)] on a fresh
    engine under TBF_WHIRL_SPLIT=split; returns (L, R), its launches and its layout."""
    import torch
    import tunebfree_amd as T
    n = len(scens)
    nb = calls[-1][0] + calls[-1][1]
    os.environ["TBF_WHIRL_SPLIT"] = split
    try:
        eng = T.Engine(sample_rate=rate, device=0, debug_flags=dbg)
    finally:
        os.environ.pop("TBF_WHIRL_SPLIT", None)
    eng.config(cfg or {})
    lay = eng.layout()
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, [6300 + i for i in range(n)])
    L = torch.zeros((n, nb * 128), dtype=torch.float32, device="cuda")
    R = torch.zeros_like(L)
    for (s, k) in calls:
        rows = []
        for i, sc in enumerate(scens):
            for (b, kind, a, v) in sc:
                if not s <= b < s + k:
                    continue
                if kind == "note":
                    rows.append((b - s, i, 0, a, float(v)))
                elif kind == "control":
                    rows.append((b - s, i, 2, eng.control_id(a), float(v)))
                else:
                    rows.append((b - s, i, 1, a, float(v)))
        rows.sort(key=lambda r: r[0])
        eng.render_events_device(k, eng.events(rows), L[:, s * 128:].data_ptr(), R[:, s * 128:].data_ptr(), nb * 128)
    eng.synchronize()
    out = (L.cpu().numpy(), R.cpu().numpy())
    la = eng.launches()
    eng.close()
    return out, la, lay


def _fast_ref(oracle, n, nb, rate, cfg=None):
    from orc_bind import Cfg, Template
    tpl = Template(oracle, sr=rate, seed=7, cfg=None if cfg is None else Cfg(oracle, cfg))
    return oracle_run(oracle, tpl, [6300 + i for i in range(n)], S.fast_scens(n), nb)[:2]


def _four_renders(oracle, what, rate, cfg, n, calls_of):
    """k_whirl and k_whirl_split, each on its fast paths and forced serial: each against the
    oracle's L and R (so all four equal each other), each having launched its kernel only"""
    nb = int(math.ceil(SECONDS * rate / 128))
    ref = _fast_ref(oracle, n, nb, rate, cfg)
    assert all(np.isfinite(a).all() and float(np.abs(a).max()) > 1e-3 for a in ref)
    scens = S.fast_scens(n)
    lay = None
    for split, ran, other in (("0", "k_whirl", "k_whirl_split"), ("1", "k_whirl_split", "k_whirl")):
        for dbg in (0, 1):
            out, la, lay = _render(scens, calls_of(nb), rate, cfg, dbg, split)
            assert la[ran] > 0 and la[other] == 0, (split, la)
            for ch in (0, 1):
                assert_bits(out[ch], ref[ch], f"{what}: {ran}{' forced serial' if dbg else ''} vs oracle, {'LR'[ch]}")
    return lay


# ---------------------------------------------------------------- lower edges
def test_gpu_lowest_accepted_rate(oracle):
    """r0, the lowest rate a full-chain engine accepts (it exists at or below 44100 Hz):
    the smallest write-ahead is just over a sub-block, and two horn turns pass through it."""
    r0 = _r0()
    assert r0 <= 44100.0
    lay = _four_renders(oracle, f"{r0:g} Hz", r0, None, 6, lambda nb: [(0, nb)])
    print(f"r0 = {r0:g} Hz: write-ahead {lay['min_ahead']:.3f} .. {lay['max_ahead']:.3f}, bound {lay['min_ahead_bound']:.4f}")
    assert lay["min_ahead_bound"] <= lay["min_ahead"] < lay["min_ahead_bound"] + 0.25 and lay["wring_len"] == 512


@pytest.mark.parametrize("rate", [48000.0, 44100.0])
def test_gpu_nearest_accepted_microphone(oracle, rate):
    """d0, the nearest whirl.mic.distance (whole centimetres) a full-chain engine accepts."""
    d0 = _d0(rate)
    cfg = {"whirl.mic.distance": d0}
    lay = _four_renders(oracle, f"mic at {d0} cm, {rate:g} Hz", rate, cfg, 6, lambda nb: [(0, nb)])
    print(f"d0 = {d0} cm at {rate:g} Hz: write-ahead {lay['min_ahead']:.3f} .. {lay['max_ahead']:.3f}")
    assert lay["min_ahead_bound"] <= lay["min_ahead"] < lay["min_ahead_bound"] + 1.5
    if rate == 48000.0:
        assert S.CFG_SETS["geometry_near"] == cfg  # test_gpu_cfg_keys runs every tap at d0


# ---------------------------------------------------------------- upper edge
@pytest.mark.parametrize("geo", ["default", "geometry_wide"])
def test_gpu_192k_ring_2048(oracle, geo):
    """192 kHz: the 2048-sample ring (k_whirl<2048>, k_whirl_split<2048>), with geometry_wide
    all but full (write-ahead 1968.8 + 68 of 2048 slots); 4 instances over 680 blocks, as one
    call and as calls of 64 and 616 blocks."""
    cfg = None if geo == "default" else S.CFG_SETS[geo]
    rate, n, nb = 192000.0, 4, 680
    assert nb >= SECONDS * rate / 128
    ref = _fast_ref(oracle, n, nb, rate, cfg)
    assert all(np.isfinite(a).all() and float(np.abs(a).max()) > 1e-3 for a in ref)
    scens = S.fast_scens(n)
    for split, ran, other in (("0", "k_whirl", "k_whirl_split"), ("1", "k_whirl_split", "k_whirl")):
        for calls in ([(0, nb)], [(0, 64), (64, 616)]):
            out, la, lay = _render(scens, calls, rate, cfg, 0, split)
            assert lay["wring_len"] == 2048, lay
            assert (lay["max_ahead"] > 1960.0) == (geo == "geometry_wide"), lay
            assert la[ran] > 0 and la[other] == 0, (split, la)
            for ch in (0, 1):
                assert_bits(out[ch], ref[ch], f"192 kHz {geo}: {ran}<2048> in {len(calls)} call(s) vs oracle, {'LR'[ch]}")


# ---------------------------------------------------------------- every tap across the rates
@pytest.mark.parametrize("dispatch", list(DISPATCH))
@pytest.mark.parametrize("rate", ["r0", 88200.0, 176400.0, 192000.0])
def test_gpu_every_tap_at_rate(oracle, rate, dispatch):
    """The event script through the tone-generator, preamp and reverb taps and the outputs."""
    sr = _r0() if rate == "r0" else rate
    n, nb = 4, 72
    kw = dict(sr=sr, env=DISPATCH[dispatch])
    eng, tpl, seeds, scens = _setup(oracle, n, S.event_scenario, chain=1, **kw)
    ref = _ref_once(("rates", sr), lambda: oracle_run(oracle, tpl, seeds, scens, nb))
    assert all(np.isfinite(a).all() and float(np.abs(a).max()) > 1e-3 for a in ref)
    _all_taps(f"events at {sr:g} Hz", dispatch, ref, lambda chain: eng if chain == 1 else _organ(n, chain=chain, **kw),
              lambda e: engine_run(e, scens, nb))


# ---------------------------------------------------------------- low rates, chains without the whirl
@pytest.mark.parametrize("scen", ["events", "sweep"])
@pytest.mark.parametrize("rate", [8000.0, 22050.0])
def test_gpu_low_rate_taps(oracle, rate, scen):
    """8000 and 22050 Hz, refused on a chain with the whirl: the tone-generator, preamp and
    reverb chains against the oracle's stage outputs (attack envelopes of 2-15 samples, the
    scanner's stator step six times the usual one, the preamp's overallscale 0.18 at 8 kHz)."""
    assert not _accepted(rate) and not _accepted(rate, chain=S_FX)
    n, nb = 4, 72
    fn = S.event_scenario if scen == "events" else S.sweep_scenario
    eng, tpl, seeds, scens = _setup(oracle, n, fn, chain=1, sr=rate)
    ref = oracle_run(oracle, tpl, seeds, scens, nb)
    for chain, idx, tap in TAPS:
        assert np.isfinite(ref[idx]).all() and float(np.abs(ref[idx]).max()) > 1e-3, tap
        e = eng if chain == 1 else _organ(n, chain=chain, sr=rate)
        L, R = engine_run(e, scens, nb)
        assert_bits(L, ref[idx], f"{scen} at {rate:g} Hz: {tap} tap")
        assert np.array_equal(L.view(np.uint32), R.view(np.uint32))
        _ran(e, "small", chain)
        e.close()


# ---------------------------------------------------------------- effects-only chain
@pytest.mark.parametrize("whirl", ["split", "whirl"])
@pytest.mark.parametrize("rate", ["r0", 192000.0])
def test_gpu_fx_arbitrary_input_at_rate(oracle, rate, whirl):
    """test_gpu_fx_chain's arbitrary-input case at the lowest accepted rate and at 192 kHz:
    Gaussian and full-scale noise rows through the three effects-only modes."""
    from fx_oracle import fx_run
    from test_gpu_fx_chain import MODES, SEEDS, WHIRL, _compare, _process_script, fx_input, fx_settings
    from test_gpu_fx_chain import _ran as fx_ran
    sr = _r0() if rate == "r0" else rate
    nb = 9 if sr < 100000.0 else 36  # past the largest write-ahead (1555 samples at 192 kHz)
    g = np.random.default_rng(int(sr))
    x = np.stack([fx_input(i, nb * 128, g, sr) for i in (0, 3)])
    scens = [fx_settings(i) for i in (8, 4)]  # both rotors fast; both slow
    ref = fx_run(oracle, SEEDS[:2], x, scens, sr)
    assert all(np.isfinite(a).all() and float(np.abs(a).max()) > 1e-3 for a in ref)
    for chain, idx, tap in MODES:
        eng = _setup(None, 2, None, chain=chain, sr=sr, env=WHIRL[whirl])
        L, R = _process_script(eng, x, scens)
        _compare(f"arbitrary input at {sr:g} Hz [{whirl}] {tap}", chain, idx, L, R, ref)
        fx_ran(eng, chain, whirl)
        eng.close()
