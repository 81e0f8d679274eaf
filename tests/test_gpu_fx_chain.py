"""Effects-only chains (TBF_CHAIN_FX, TBF_CHAIN_FX_TAP_PREAMP, TBF_CHAIN_FX_TAP_REVERB): the
caller's audio through preamp -> reverb -> whirl, bit for bit the reference's
preamp -> b_reverb::reverb -> whirlProc3 on that input (enginerun.assert_bits at every
comparison).

Two references.  fx_oracle runs the CPU oracle's own effect stages on arbitrary input (it is
pinned against the chain oracle in test_fx_cpu.py).  The loop-back tests feed the full chain
oracle's tone-generator tap into effects-only engines of the same seeds and compare with that
oracle's preamp, reverb and L / R taps, which also reaches what fx_oracle cannot: whirl cfg
keys, the whirl's MIDI control functions and bypass.

Every case checks through Engine.launches() that no k_tonegen ran and that the whirl kernel
its environment names did: k_whirl_split is the engine's choice at these sizes,
TBF_WHIRL_SPLIT=0 forces k_whirl, what a full batch runs.
"""
import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits, oracle_run
from fx_oracle import effect_events, fx_run
from test_gpu_parity import _engine, _script_events, _setup

pytestmark = pytest.mark.gpu

FX, FX_PRE, FX_REV = 4, 5, 6
# (chain mode, index into [preamp, reverb, L, R] of the reference it ends at, name)
MODES = ((FX_PRE, 0, "preamp tap"), (FX_REV, 1, "reverb tap"), (FX, 2, "L / R"))
WHIRL = {"split": {}, "whirl": {"TBF_WHIRL_SPLIT": "0"}}
SEEDS = [1000 + 17 * i for i in range(64)]  # test_gpu_parity._setup's


def _ran(eng, chain, whirl, **more):
    """no k_tonegen; the whirl kernel of the environment on the full effects chain, none on a
    tap; the reverb network past the preamp tap; more: kernel names that must (not) have run"""
    c = eng.launches()
    assert c["k_tonegen"] == 0 and c["k_tonegen_ranges"] == 0, c
    ran, other = ("k_whirl", "k_whirl_split") if whirl == "whirl" else ("k_whirl_split", "k_whirl")
    assert c[other] == 0 and (c[ran] > 0) == (chain == FX), (chain, whirl, c)
    assert (c["k_rv_core"] + c["k_rv_core_lds"] > 0) == (chain != FX_PRE), (chain, c)
    for k, want in more.items():
        assert (c[k] > 0) == want, (k, want, c)
    return c


def _apply(eng, i, ev):
    (b, kind, a, v) = ev
    if kind == "note":
        eng.note(i, a, v)
    elif kind == "control":
        assert eng.midi_control(i, a, v)
    else:
        eng.set_param(i, a, v)


def _process_script(eng, x, scens):
    """x [n, nblocks*128] through Engine.process, in calls that end where the scripts have
    events (applied between the calls, as enginerun.engine_run does for renders)"""
    nb = x.shape[1] // 128
    bounds = sorted({0, nb} | {e[0] for sc in scens for e in sc if e[0] < nb})
    Ls, Rs = [], []
    for s, e in zip(bounds[:-1], bounds[1:]):
        for i, sc in enumerate(scens):
            for ev in sc:
                if ev[0] == s:
                    _apply(eng, i, ev)
        L, R = eng.process(x[:, s * 128:e * 128])
        Ls.append(L)
        Rs.append(R)
    return np.concatenate(Ls, axis=1), np.concatenate(Rs, axis=1)


def _compare(what, chain, idx, L, R, ref):
    if chain == FX:
        assert_bits(L, ref[2], f"{what} L")
        assert_bits(R, ref[3], f"{what} R")
    else:
        assert_bits(L, ref[idx], what)
        assert np.array_equal(L.view(np.uint32), R.view(np.uint32)), what


# ------------------------------------------------------------------ loop-back
_LOOP = {}
LOOP_CASES = {
    # name: (instances, scenario, sample rate, cfg set)
    "sweep": (6, S.sweep_scenario, 48000.0, None),
    "sr96k": (2, S.sweep_scenario, 96000.0, None),          # W = 1024 whirl ring, the preamp's overallscale
    "cfg_mix": (2, S.cfg_scenario, 48000.0, "mix"),         # mic widths, horn level and leak, reverb.mix
    "whirl_controls": (2, S.whirl_control_scenario, 48000.0, None),  # filter setters, brake, bypass
}


def _loop_ref(oracle, name):
    """the chain oracle's [preamp, reverb, L, R] taps and its tone-generator tap, once per case"""
    if name not in _LOOP:
        from orc_bind import Cfg, Template
        n, scen, sr, cfg = LOOP_CASES[name]
        tpl = Template(oracle, sr=sr, seed=7, cfg=None if cfg is None else Cfg(oracle, S.CFG_SETS[cfg]))
        scens = [scen(i) for i in range(n)]
        L, R, A, B, Cc = oracle_run(oracle, tpl, SEEDS[:n], scens, 64)
        for a in (L, R, A, B, Cc):
            a.setflags(write=False)
        _LOOP[name] = ((B, Cc, L, R), A, scens)
    return _LOOP[name]


@pytest.mark.parametrize("whirl", list(WHIRL))
@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_gpu_fx_loopback(oracle, name, whirl):
    """64 blocks of a full-chain script through the chain oracle; its tone-generator tap goes
    into effects-only engines of the same seeds that carry the script's effect events only, and
    the three modes give the oracle's preamp tap, reverb tap and L / R.  The tap holds the
    silences and release tails that reach the preamp's denormal guard."""
    n, scen, sr, cfg = LOOP_CASES[name]
    ref, A, scens = _loop_ref(oracle, name)
    assert float(np.abs(A).max()) > 1e-3
    if name == "sweep":  # the silences: exact zeros, which the guard (|x| < 1.18e-23) replaces
        assert (A == 0).any()
    fx = [effect_events(sc) for sc in scens]
    for chain, idx, tap in MODES:
        eng = _setup(None, n, None, chain=chain, sr=sr, cfg=None if cfg is None else S.CFG_SETS[cfg],
                     env=WHIRL[whirl])
        L, R = _process_script(eng, A, fx)
        _compare(f"loop-back {name} [{whirl}] {tap}", chain, idx, L, R, ref)
        _ran(eng, chain, whirl)
        eng.close()


# ------------------------------------------------------------------ arbitrary input
def fx_input(i, ns, g, sr=48000.0):
    """input kinds by i % 6: Gaussian noise at 0.25, two unit impulses, half a row of silence
    then a 20 Hz - 12 kHz sweep at 0.9, uniform full-scale noise, 1e-30-scale noise with -0.f
    and 1e-41 subnormals mixed in, a +-1 square wave"""
    k = i % 6
    x = np.zeros(ns, np.float32)
    if k == 0:
        x = (g.standard_normal(ns) * 0.25).clip(-1, 1).astype(np.float32)
    elif k == 1:
        x[5] = 1.0
        x[700] = -1.0
    elif k == 2:
        m = ns - ns // 2
        x[ns // 2:] = (0.9 * np.sin(2 * np.pi * np.cumsum(np.linspace(20, 12000, m)) / sr)).astype(np.float32)
    elif k == 3:
        x = g.uniform(-1, 1, ns).astype(np.float32)
    elif k == 4:
        x = (g.standard_normal(ns) * 1e-30).astype(np.float32)
        x[::7] = -0.0
        x[3::11] = np.float32(1e-41)
    else:
        x = np.where(np.arange(ns) % 256 < 128, 1.0, -1.0).astype(np.float32)
    return x


def fx_settings(i):
    """per instance, at block 0: overdrive, character, reverb mix, drum and horn speed"""
    return [(0, "param", S.P_OVERDRIVE, 1 if i % 3 else 0), (0, "param", S.P_CHARACTER, S.SWEEP_CHARACTER[i % 4]),
            (0, "param", S.P_REVERB, S.SWEEP_REVERB[i % 3]), (0, "param", S.P_DRUM, i % 3),
            (0, "param", S.P_HORN, (i // 3) % 3)]


_ARB = {}


def _arb_ref(oracle):
    """37 instances (28 + 9: a full and a partial chain-block workgroup) x 9 blocks (>= 8:
    k_rv_core_lds; 18 tiles and 3 more iterations: the pipeline's odd tail)"""
    if not _ARB:
        n, nb = 37, 9
        g = np.random.default_rng(5)
        x = np.stack([fx_input(i, nb * 128, g) for i in range(n)])
        scens = [fx_settings(i) for i in range(n)]
        ref = fx_run(oracle, SEEDS[:n], x, scens)
        for a in ref + [x]:
            a.setflags(write=False)
        assert all(np.isfinite(a).all() for a in ref) and float(np.abs(ref[2]).max()) > 0.1
        assert np.signbit(x[4][x[4] == 0]).any() and (np.abs(x[4][x[4] != 0]) < 1.2e-38).any()
        _ARB.update(x=x, scens=scens, ref=ref)
    return _ARB["x"], _ARB["scens"], _ARB["ref"]


def _arb_engine(chain, env, debug_flags=0):
    eng = _engine(chain, env=env, debug_flags=debug_flags)
    tid = eng.template(seed=7)
    eng.add_instances([tid] * 37, SEEDS[:37])
    return eng


@pytest.mark.parametrize("whirl", list(WHIRL))
def test_gpu_fx_arbitrary_input(oracle, whirl):
    """Noise, impulses, silence and a sweep, full-scale noise, denormal-scale noise with -0.f
    and subnormals, a square wave; overdrive on and off, four characters, three mixes, every
    rotor option: the three modes against fx_oracle."""
    x, scens, ref = _arb_ref(oracle)
    for chain, idx, tap in MODES:
        eng = _arb_engine(chain, WHIRL[whirl])
        L, R = _process_script(eng, x, scens)
        _compare(f"arbitrary input [{whirl}] {tap}", chain, idx, L, R, ref)
        _ran(eng, chain, whirl, **({} if chain == FX_PRE else {"k_rv_core_lds": True, "k_rv_core": False}))
        eng.close()


@pytest.mark.parametrize("case", ["force_serial", "no_rv_lds"])
def test_gpu_fx_arbitrary_input_other_paths(oracle, case):
    """The same input with every fast-path vote failed (TBF_DEBUG_FORCE_SERIAL: the exact serial
    replays of reverb and whirl) and with the streaming reverb network (TBF_RV_LDS=0)."""
    x, scens, ref = _arb_ref(oracle)
    env, dbg = ({}, 1) if case == "force_serial" else ({"TBF_RV_LDS": "0"}, 0)
    eng = _arb_engine(FX, env, dbg)
    L, R = _process_script(eng, x, scens)
    _compare(f"arbitrary input {case}", FX, 2, L, R, ref)
    _ran(eng, FX, "split", k_rv_core_lds=case != "no_rv_lds", k_rv_core=case == "no_rv_lds")
    if case == "force_serial":  # the whirl's and the reverb's replays ran (no scanner vibrato here)
        import tunebfree_amd as T
        want = T.engine.PATH_WH_ANGLE | T.engine.PATH_WH_MOTION | T.engine.PATH_RV_PHASE
        assert eng.error_flags() & want == want, hex(eng.error_flags())
    eng.close()


# ------------------------------------------------------------------ rows, strides, call splits
def test_gpu_fx_rows_strides_call_splits(oracle):
    """Device buffers with in_stride = nblocks*128 + 37, the input pointer one float into its
    allocation, NaN in the input padding (nothing outside [0, nblocks*128) of a row is read: a
    NaN read would spread through the reverb) and a sentinel in the output padding, which
    survives; calls of 5 + 3 + 16 blocks (the 3- and 5-block calls take the streaming
    k_rv_core) against one 24-block oracle run.  Input overlapping an output is -22."""
    import torch
    import tunebfree_amd as T
    n, nb = 5, 24
    ns, stride, ostride = nb * 128, nb * 128 + 37, nb * 128 + 11
    g = np.random.default_rng(11)
    x = np.stack([fx_input(i, ns, g) for i in (0, 3, 2, 0, 5)])
    scens = [fx_settings(i + 1) for i in range(n)]
    ref = fx_run(oracle, SEEDS[:n], x, scens)
    eng = _engine(FX)
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, SEEDS[:n])
    for i, sc in enumerate(scens):
        for ev in sc:
            _apply(eng, i, ev)
    hin = np.full(1 + n * stride, np.nan, np.float32)
    rows = hin[1:].reshape(n, stride)
    rows[:, :ns] = x
    din = torch.from_numpy(hin).cuda()
    SENT = -12345.0
    dL = torch.full((n * ostride + 1,), SENT, dtype=torch.float32, device="cuda")
    dR = torch.full((n * ostride + 1,), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b0 = 0
    for m in (5, 3, 16):
        eng.process_device(m, din.data_ptr() + 4 * (1 + b0 * 128), stride, dL.data_ptr() + 4 * (1 + b0 * 128),
                           dR.data_ptr() + 4 * (1 + b0 * 128), ostride)
        b0 += m
    eng.synchronize()
    hL, hR = dL.cpu().numpy(), dR.cpu().numpy()
    L, R = hL[1:].reshape(n, ostride), hR[1:].reshape(n, ostride)
    assert_bits(L[:, :ns], ref[2], "strides and call splits L")
    assert_bits(R[:, :ns], ref[3], "strides and call splits R")
    assert hL[0] == SENT and hR[0] == SENT and (L[:, ns:] == SENT).all() and (R[:, ns:] == SENT).all()
    _ran(eng, FX, "split", k_rv_core=True, k_rv_core_lds=True)
    # a host-side pointer check (nothing is launched): the one-block input range from din + 4 against
    # an outL that starts inside it, and an outR whose last ten floats reach into it
    extent = (n - 1) * ostride + 128
    for oL, oR in ((din.data_ptr() + 4 * ns, dR.data_ptr()), (dL.data_ptr(), din.data_ptr() + 4 - 4 * (extent - 10))):
        with pytest.raises(T.TbfError, match="-22.*overlap"):
            eng.process_device(1, din.data_ptr() + 4, stride, oL, oR, ostride)
    eng.close()


# ------------------------------------------------------------------ events
def test_gpu_fx_process_events(oracle):
    """tbf_process_events, 5 instances x 48 blocks in one call: overdrive, character, reverb-mix
    and rotor events on consecutive blocks and on shared blocks (a delta chunk with an index
    table), and a burst of note and drawbar events on instance 0, which changes nothing."""
    import torch
    n, nb = 5, 48
    g = np.random.default_rng(23)
    x = np.stack([fx_input(i, nb * 128, g) for i in (0, 3, 5, 2, 0)])

    def scen(i):
        ev = fx_settings(i + 1)
        b = 3 + i  # consecutive blocks, a different phase per instance
        ev += [(b, "param", S.P_OVERDRIVE, 0 if (i + 1) % 3 else 1), (b + 1, "param", S.P_CHARACTER, 0.45),
               (b + 2, "param", S.P_REVERB, 0.25), (b + 3, "param", S.P_DRUM, 2), (b + 4, "param", S.P_HORN, 0)]
        # shared blocks: every instance, all four at once
        ev += [(20, "param", S.P_OVERDRIVE, 1), (20, "param", S.P_CHARACTER, S.SWEEP_CHARACTER[(i + 2) % 4]),
               (20, "param", S.P_REVERB, S.SWEEP_REVERB[(i + 1) % 3]), (20, "param", S.P_DRUM, (i + 1) % 3),
               (20, "param", S.P_HORN, 2), (33, "param", S.P_OVERDRIVE, i & 1), (33, "param", S.P_HORN, 1),
               (47, "param", S.P_REVERB, 0.5)]
        if i == 0:
            for b in (0, 1, 2, 9, 20, 21, 40):
                ev += [(b, "note", 48 + b % 12, 1), (b, "note", 60 + b % 7, b & 1),
                       (b, "param", S.P_DRAWBAR + b % 9, b % 9), (b, "param", S.P_VIBRATO, b & 1),
                       (b, "param", S.P_PERC, 1 - (b & 1))]
        return sorted(ev, key=lambda r: r[0])
    scens = [scen(i) for i in range(n)]
    ref = fx_run(oracle, SEEDS[:n], x, scens)
    eng = _engine(FX)
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, SEEDS[:n])
    din = torch.from_numpy(x).cuda()
    dL = torch.zeros((n, nb * 128), dtype=torch.float32, device="cuda")
    dR = torch.zeros_like(dL)
    torch.cuda.synchronize()
    eng.process_events_device(nb, _script_events(eng, scens), din.data_ptr(), nb * 128, dL.data_ptr(), dR.data_ptr(),
                              nb * 128)
    eng.synchronize()
    assert_bits(dL.cpu().numpy(), ref[2], "process_events L")
    assert_bits(dR.cpu().numpy(), ref[3], "process_events R")
    _ran(eng, FX, "split")
    eng.close()


# ------------------------------------------------------------------ pipelining, input ordering
def test_gpu_fx_pipelined_calls_reuse_the_input(oracle):
    """TBF_CHAIN_FX pipelines across chunks like the full chain.  set_steady_chunk (64), 3
    instances: one call of 200 blocks (chunks 64 / 64 / 64 / 8) from a device tensor; then,
    with no synchronisation, a torch op on the same stream overwrites that tensor with new
    audio and a second call of 72 blocks reads it.  Both calls equal the oracle's 272-block run.

    Two orderings are at stake: the first call's stage-1 launches must all have read the tensor
    before the stream reaches the overwrite (the call's end-of-call join), and the second
    call's first stage must wait for the stream although the stage streams are busy (the
    input-side wait renderBody makes on every call).  A missing wait is a race and need not
    show on every run: the engine code is the proof, this test is the tripwire."""
    import torch
    n, nb1, nb2 = 3, 200, 72
    g = np.random.default_rng(31)
    x1 = np.stack([fx_input(i, nb1 * 128, g) for i in (0, 3, 5)])
    x2 = np.stack([fx_input(i, nb2 * 128, g) for i in (3, 0, 0)])
    scens = [fx_settings(i + 4) for i in range(n)]
    ref = fx_run(oracle, SEEDS[:n], np.concatenate([x1, x2], axis=1), scens)
    eng = _engine(FX, env={"TBF_WHIRL_SPLIT": "0"})
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, SEEDS[:n])
    assert eng.set_steady_chunk(64) == 64
    for i, sc in enumerate(scens):
        for ev in sc:
            _apply(eng, i, ev)
    st = torch.cuda.Stream()
    din = torch.from_numpy(x1).cuda()
    new = torch.from_numpy(x2).cuda()
    dL = torch.zeros((n, (nb1 + nb2) * 128), dtype=torch.float32, device="cuda")
    dR = torch.zeros_like(dL)
    torch.cuda.synchronize()
    stride, ostride = nb1 * 128, (nb1 + nb2) * 128
    with torch.cuda.stream(st):
        eng.process_device(nb1, din.data_ptr(), stride, dL.data_ptr(), dR.data_ptr(), ostride, st.cuda_stream)
        din[:, :nb2 * 128].copy_(new)
        eng.process_device(nb2, din.data_ptr(), stride, dL.data_ptr() + 4 * nb1 * 128, dR.data_ptr() + 4 * nb1 * 128,
                           ostride, st.cuda_stream)
        hL, hR = dL.to("cpu", non_blocking=True), dR.to("cpu", non_blocking=True)
    st.synchronize()
    assert_bits(hL.numpy(), ref[2], "pipelined calls L")
    assert_bits(hR.numpy(), ref[3], "pipelined calls R")
    c = _ran(eng, FX, "whirl")
    assert c["k_whirl"] == 4 + 2 and c["k_rv_core_lds"] == 4 + 2 and c["k_rv_core"] == 0, c
    eng.close()
