"""The cabinet convolver on the GPU (tbf_render_cabinet* / tbf_process_cabinet*, k_cabinet):
accuracy against a float64 direct sum of the call's own horn plane, the chain undisturbed, the
mix law bit for bit from the call's own planes, cut invariance bit for bit, known answers, the
history through clone / save / load / remove / add, and the device-memory contract.

The convolver has no reference implementation to restate: its accuracy
bound is 4 x the error of the numpy model of the same scheme (tests/cab_model.py) on the same
plane; everything else here is an identity in bits."""
import numpy as np
import pytest

import cab_model as M
import scenarios as S

pytestmark = pytest.mark.gpu

FULL, FX = 0, 4
N = 3
SEEDS = [4100 + 37 * i for i in range(N)]
PLANES = ("L", "R", "wetL", "wetR", "hornL", "hornR", "drumL", "drumR")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} of {a.size} differ, first at {tuple(bad[0])}")


def responses(taps, seed=0):
    """two different seeded decaying-noise responses of `taps` taps"""
    return M.decaying_noise(taps, 2 * taps + seed), M.decaying_noise(taps, 2 * taps + seed + 1)


def scen(i, nb):
    """a held chord plus rotor speed changes (block 3; in a long run block 40 too)"""
    ev = S.bench_scenario(i) + [(3, "param", S.P_DRUM, 2), (3, "param", S.P_HORN, 2)]
    if nb > 40:
        ev += [(40, "param", S.P_HORN, 0), (40, "param", S.P_DRUM, 1)]
    return ev


def scens(nb, n=N):
    return [scen(i, nb) for i in range(n)]


def noise(nb, n=N, seed=11):
    return (np.random.default_rng(seed).standard_normal((n, nb * 128)) * 0.1).astype(np.float32)


def engine(chain=FULL, ir=None, n=N, cfg=None, seeds=None):
    import tunebfree_amd as T
    eng = T.Engine(sample_rate=48000.0, device=0, chain=chain)
    eng.config(cfg or {})
    if ir is not None:
        eng.set_cabinet(*ir)
    tid = eng.template(seed=7)
    if n:
        eng.add_instances([tid] * n, (seeds or SEEDS)[:n])
    return eng


def apply(eng, sc, s, insts=None):
    for i, script in enumerate(sc):
        for (b, kind, a, v) in script:
            if b != s:
                continue
            k = i if insts is None else insts[i]
            if kind == "note":
                eng.note(k, a, v)
            elif kind == "control":
                assert eng.midi_control(k, a, v)
            else:
                eng.set_param(k, a, v)


def run_calls(eng, sc, b0, b1, cuts=None, x=None, insts=None, call=None):
    """blocks [b0, b1) as host calls: one per stretch between the scripts' events and the cut
    points, controls by direct call in between; returns the eight planes joined, by name"""
    bounds = {b0, b1}
    for script in sc:
        bounds.update(b for (b, *_r) in script if b0 < b < b1)
    at = b0
    for c in cuts or []:
        at += c
        if at < b1:
            bounds.add(at)
    bounds = sorted(bounds)
    parts = []
    for s, e in zip(bounds[:-1], bounds[1:]):
        apply(eng, sc, s, insts)
        if call is not None:
            parts.append(call(s, e))
        elif x is None:
            parts.append(eng.render_cabinet(e - s, wet=True, rotors=True))
        else:
            parts.append(eng.process_cabinet(x[:, s * 128:e * 128], wet=True, rotors=True))
    return dict(zip(PLANES, (np.concatenate(p, axis=1) for p in zip(*parts))))


def event_rows(eng, sc, b0, b1):
    """the scripts' events of blocks [b0, b1) as tbf_event rows, blocks counted from b0"""
    rows = []
    for i, script in enumerate(sc):
        for (b, kind, a, v) in script:
            if not b0 <= b < b1:
                continue
            rows.append((b - b0, i, 0, a, float(v)) if kind == "note" else
                        (b - b0, i, 2, eng.control_id(a), float(v)) if kind == "control" else (b - b0, i, 1, a, float(v)))
    rows.sort(key=lambda r: r[0])
    return eng.events(rows)


def one_call(eng, sc, nb, b0=0, wet=True, rotors=True, stride=None, lead=0, fill=0.0, x=None, ev_upto=None):
    """One device call with the scripts' events of [b0, b0 + nb) (or up to block ev_upto: events at
    or beyond the call's end apply after it), into torch buffers of row stride
    `stride` that start `lead` floats into their allocation and are filled with `fill`.  Returns
    the planes by name as whole rows [n, stride], and the raw allocations."""
    import torch
    n = eng.n_instances
    stride = stride or nb * 128
    names = PLANES[:2] + (PLANES[2:4] if wet else ()) + (PLANES[4:] if rotors else ())
    flat = {k: torch.full((lead + n * stride,), fill, dtype=torch.float32, device="cuda") for k in names}
    ptr = {k: t.data_ptr() + 4 * lead for k, t in flat.items()}
    cab = [ptr[k] for k in names if k in PLANES[:4]]
    rot = [ptr[k] for k in PLANES[4:]] if rotors else None
    ev = event_rows(eng, sc, b0, ev_upto or b0 + nb)
    if x is None:
        eng.render_cabinet_device(nb, cab, stride, rot, stride, events=ev)
    else:
        xt = torch.from_numpy(np.ascontiguousarray(x[:, b0 * 128:(b0 + nb) * 128])).cuda()
        torch.cuda.synchronize()
        eng.process_cabinet_device(nb, xt.data_ptr(), xt.shape[1], cab, stride, rot, stride, events=ev)
    eng.synchronize()
    raw = {k: t.cpu().numpy() for k, t in flat.items()}
    return {k: r[lead:].reshape(n, stride) for k, r in raw.items()}, raw


def law(horn, wet, drum, mix):
    """(dry * horn + mix * wet) + drum, every operation in float32; mix a scalar or per sample"""
    f = np.float32
    mix = np.asarray(mix, f)
    dry = f(1.0) - mix
    return ((dry * horn.astype(f)).astype(f) + (mix * wet.astype(f)).astype(f)).astype(f) + drum.astype(f)


def check_law(p, mix, what):
    same(p["L"], law(p["hornL"], p["wetL"], p["drumL"], mix), what + " L")
    same(p["R"], law(p["hornR"], p["wetR"], p["drumR"], mix), what + " R")


def check_accuracy(p, ir, what, nb=None, floor=1e-4):
    """each wet plane against direct64 of the call's own horn plane: err_gpu <= 4 err_model"""
    ratios = []
    for ch, h in zip("LR", ir):
        for i in range(len(p["horn" + ch])):
            horn, wet = p["horn" + ch][i], p["wet" + ch][i]
            if nb:
                horn, wet = horn[:nb * 128], wet[:nb * 128]
            assert float(np.abs(horn).max()) > floor, f"{what}: silent horn plane"
            eg, em = M.err(wet, horn, h), M.err(M.convolve(horn, h), horn, h)
            print(f"{what} {ch}[{i}]: err_gpu {eg / M.EPS:.3f} err_model {em / M.EPS:.3f} (x 2^-24) ratio {eg / em:.2f}")
            ratios.append((eg, em))
    for eg, em in ratios:
        assert eg <= 4 * em, (what, eg / M.EPS, em / M.EPS)


# ---------------------------------------------------------------- 1. accuracy
@pytest.mark.parametrize("chain", [FULL, FX])
@pytest.mark.parametrize("taps,nb", [(1, 12), (128, 12), (129, 12), (300, 12), (8192, 70)])
def test_gpu_cabinet_accuracy(taps, nb, chain):
    ir = responses(taps)
    eng = engine(chain, ir)
    info = eng.cabinet_info()
    assert (info["taps"], info["partitions"]) == (taps, (taps + 127) // 128)
    x = noise(nb) if chain == FX else None
    p = run_calls(eng, scens(nb), 0, nb, x=x)
    assert eng.cabinet_info()["launches"] > 0
    eng.close()
    check_accuracy(p, ir, f"taps {taps} chain {chain}")
    # each channel went through its own response: against the other one the planes are far off
    if taps > 1:
        for ch, other in zip("LR", ir[::-1]):
            assert M.err(p["wet" + ch][0], p["horn" + ch][0], other) > 1e-3


# ---------------------------------------------------------------- 2. the chain is undisturbed
@pytest.mark.parametrize("chain", [FULL, FX])
def test_gpu_cabinet_leaves_the_rotor_planes_alone(chain):
    nb = 12
    x = noise(nb) if chain == FX else None
    sc = scens(nb)
    eng = engine(chain, responses(300))
    p = run_calls(eng, sc, 0, nb, x=x)
    eng.close()
    twin = engine(chain)

    def rotors(s, e):
        six = twin.render_rotors(e - s) if x is None else twin.process_rotors(x[:, s * 128:e * 128])
        return (six[0], six[1]) * 2 + tuple(six[2:])
    q = run_calls(twin, sc, 0, nb, call=rotors)
    twin.close()
    for k in PLANES[4:]:
        same(p[k], q[k], f"chain {chain} {k} against the engine without a cabinet")
        assert float(np.abs(p[k]).max()) > 1e-4


# ---------------------------------------------------------------- 3. the mix law
@pytest.mark.parametrize("chain", [FULL, FX])
def test_gpu_cabinet_mix_law(chain):
    f = np.float32
    nb = 12
    x = noise(3 * nb + 24) if chain == FX else None
    sc = scens(nb)
    eng = engine(chain, responses(300))
    p = run_calls(eng, sc, 0, nb, x=x)            # the default: mix 1
    check_law(p, f(1.0), "default mix")
    assert float(np.abs(p["wetL"]).max()) > 1e-4 and float(np.abs(p["drumL"]).max()) > 1e-5
    at = nb
    for v in (0, 40, 127):                        # by tbf_midi_control between calls, per instance
        eng.midi_control(1, "convolution.mix", v)
        assert eng.cabinet_info(1)["wet"] == f(v / 127.0)
        p = run_calls(eng, [[]] * N, at, at + 4, x=x)
        at += 4
        mix = np.array([1.0, v / 127.0, 1.0], f)[:, None]
        check_law(p, mix, f"mix {v} by control")
        if v == 0:                                # wet 0: the horn and the drum alone
            assert np.array_equal(p["L"][1], p["hornL"][1] + p["drumL"][1])
            assert np.array_equal(p["R"][1], p["hornR"][1] + p["drumR"][1])
    # by event at block 5 of a 12-block call: the old value before it, the new one from it on
    eng.midi_control(1, "convolution.mix", 127)
    eng.midi_control(2, "convolution.mix", 100)
    cid = eng.control_id("convolution.mix")
    sc_ev = [[], [(5, "control", "convolution.mix", 40)], [(5, "control", "convolution.mix", 0),
                                                           (12, "control", "convolution.mix", 90)]]
    assert cid >= 0
    p, _raw = one_call(eng, sc_ev, 12, x=None if x is None else x[:, at * 128:], ev_upto=13)
    at += 12
    mix = np.ones((N, 12 * 128), f)
    mix[1, 5 * 128:] = f(40 / 127.0)
    mix[2, :5 * 128] = f(100 / 127.0)
    mix[2, 5 * 128:] = f(0.0)
    check_law(p, mix, "mix by event at block 5")
    assert eng.cabinet_info(1)["wet"] == f(40 / 127.0)
    assert eng.cabinet_info(2)["wet"] == f(90 / 127.0)   # the event at the call's end applies after it
    # under whirl.bypass the horn pair is the whirl's input and the drum pair 0
    for i in range(N):
        eng.set_param(i, S.P_WHIRL_BYPASS, 1)
        eng.midi_control(i, "convolution.mix", 64)
    p = run_calls(eng, [[]] * N, at, at + 4, x=x)
    assert not p["drumL"].any() and not p["drumR"].any()
    same(p["hornL"], p["hornR"], "bypass: the horn pair is the input")
    assert float(np.abs(p["hornL"]).max()) > 1e-4
    check_law(p, f(64 / 127.0), "bypass")
    eng.close()


# ---------------------------------------------------------------- 4. cut invariance
@pytest.mark.parametrize("chain", [FULL, FX])
@pytest.mark.parametrize("taps", [300, 8192])
def test_gpu_cabinet_cut_invariance(taps, chain):
    nb = 70
    ir = responses(taps)
    x = noise(nb) if chain == FX else None
    sc = scens(nb)
    for s in sc:                                   # a mix change rides along
        s.append((20, "control", "convolution.mix", 50))

    def variant(how):
        eng = engine(chain, ir)
        if how == "one call":
            p, _ = one_call(eng, sc, nb, x=x)
        elif how == "one call, steady chunk 64":
            assert eng.set_steady_chunk(64) == 64
            p, _ = one_call(eng, sc, nb, x=x)
        elif how == "one call, engine scratch":
            p, _ = one_call(eng, sc, nb, x=x, rotors=False)
        elif how == "70 calls":
            p = run_calls(eng, sc, 0, nb, cuts=[1] * nb, x=x)
        else:
            p = run_calls(eng, sc, 0, nb, cuts=[1, 5, 64], x=x)
        eng.close()
        return p
    ref = variant("one call")
    assert float(np.abs(ref["wetL"]).max()) > 1e-4
    for how in ("70 calls", "1 + 5 + 64", "one call, steady chunk 64", "one call, engine scratch"):
        got = variant(how)
        for k in got:
            same(got[k], ref[k], f"taps {taps} chain {chain}: {how} against one call, {k}")


def test_gpu_cabinet_pieces_of_a_long_call():
    """a call without rotor planes longer than a scratch piece (256 blocks), with a rotor and a mix
    event inside the second piece, against the same call with the caller's rotor planes"""
    nb = 260
    ir = responses(300)
    sc = scens(nb)
    sc[1] += [(257, "param", S.P_HORN, 1), (258, "control", "convolution.mix", 30)]
    out = []
    for rotors in (True, False):
        eng = engine(FULL, ir)
        p, _ = one_call(eng, sc, nb, rotors=rotors)
        assert eng.cabinet_info(1)["wet"] == np.float32(30 / 127.0)
        assert eng.cabinet_info()["launches"] == (1 if rotors else 2)
        eng.close()
        out.append(p)
    for k in PLANES[:4]:
        same(out[1][k], out[0][k], f"pieces against one piece, {k}")
    assert not np.array_equal(bits(out[0]["L"][1, 258 * 128:]), bits(out[0]["wetL"][1, 258 * 128:] + out[0]["drumL"][1, 258 * 128:]))


# ---------------------------------------------------------------- 5. known answers
def test_gpu_cabinet_known_answers():
    nb = 12
    sc = scens(nb)
    one = np.ones(1, np.float32)
    d200 = np.zeros(201, np.float32)
    d200[200] = 1.0
    for ir, delay, what in (((one, one), 0, "unit impulse"), ((d200, d200), 200, "impulse at tap 200")):
        eng = engine(FULL, ir)
        p = run_calls(eng, sc, 0, nb)
        eng.close()
        check_accuracy(p, ir, what)
        for ch in "LR":
            horn, wet = p["horn" + ch], p["wet" + ch]
            want = np.zeros_like(horn)
            want[:, delay:] = horn[:, :horn.shape[1] - delay]
            assert np.abs(wet - want).max() <= 16 * M.EPS * np.abs(horn).max(), what


def test_gpu_cabinet_silence():
    """A silent effects-only input with the rotors stopped: the convolver adds nothing of its own.
    The horn pair of such a run is not zero: like the reference, the reverb replaces silence by
    its dither noise (src/reverb.cpp), 1.9e-8 at most here.  So the wet planes cannot be zero either;
    what holds is that they are that noise through the response, to the accuracy bound at that
    level (nothing at an absolute level is added), and exactly zero wherever the horn history is
    exactly zero."""
    nb = 12
    ir = responses(300)
    eng = engine(FX, ir)
    for i in range(N):
        eng.set_param(i, S.P_HORN, 0)
        eng.set_param(i, S.P_DRUM, 0)
    p = dict(zip(PLANES, eng.process_cabinet(np.zeros((N, nb * 128), np.float32), wet=True, rotors=True)))
    eng.close()
    level = max(float(np.abs(p["hornL"]).max()), float(np.abs(p["hornR"]).max()))
    print(f"silent input: max |horn| = {level:.3e}, max |wet| = {float(np.abs(p['wetL']).max()):.3e}")
    assert level < 1e-6   # silence as the chain renders it, far below any signal
    for ch in "LR":
        horn, wet = p["horn" + ch], p["wet" + ch]
        for i in range(N):
            nz = np.flatnonzero(horn[i])
            first = len(horn[i]) if len(nz) == 0 else nz[0] // 128 * 128   # the first block with a sample
            assert not wet[i, :first].any(), "wet before the first horn sample"
    if level > 0.0:
        check_accuracy(p, ir, "silence", floor=0.0)


# ---------------------------------------------------------------- 6. state
def test_gpu_cabinet_state_clone_and_rewind():
    ir = responses(300)
    sc = scens(18)
    eng = engine(FULL, ir)
    run_calls(eng, sc, 0, 9)
    blob = eng.save(list(range(N)))
    assert eng.clone(1) == N
    a = run_calls(eng, sc + [sc[1]], 9, 18)
    for k in PLANES:
        same(a[k][N], a[k][1], f"the clone's next 9 blocks, {k}")
        assert not np.array_equal(bits(a[k][0]), bits(a[k][1]))
    eng.remove([N])
    eng.load(list(range(N)), blob)
    b = run_calls(eng, sc, 9, 18)
    eng.close()
    for k in PLANES:
        same(b[k], a[k][:N], f"rewind: blocks 9..18 again, {k}")


def test_gpu_cabinet_state_remove_memory_and_fresh_instance():
    ir = responses(300)
    sc = scens(18)
    eng, twin, plain = engine(FULL, ir), engine(FULL, ir), engine(FULL)
    run_calls(eng, sc, 0, 9)
    run_calls(twin, sc, 0, 9)
    plain.render(1)
    share = eng.cabinet_info()["instance_bytes"]
    assert share >= 2 * 2 * 128 * 4
    assert eng.device_bytes()[0] - plain.device_bytes()[0] == N * share
    assert eng.remove([1]).tolist() == [0, -1, 1]
    plain.remove([1])
    assert eng.device_bytes()[0] - plain.device_bytes()[0] == (N - 1) * share
    plain.close()
    keep = [sc[0], sc[2]]
    a = run_calls(eng, keep, 9, 18)
    b = run_calls(twin, sc, 9, 18)
    twin.close()
    for k in PLANES:
        same(a[k], b[k][[0, 2]], f"the survivors' next 9 blocks, {k}")
    # a fresh instance starts from zero history whatever the memory held before
    tid = 0
    assert eng.add_instances([tid], [SEEDS[1] + 5]) == 2
    late = [[], [], [(18 + b, kind, a_, v) for (b, kind, a_, v) in scen(1, 12)]]
    p = run_calls(eng, late, 18, 30)
    eng.close()
    fresh = {k: v[2:3] for k, v in p.items()}
    check_accuracy(fresh, ir, "a fresh instance's first blocks")
    check_accuracy(fresh, ir, "a fresh instance's first block", nb=1)


# ---------------------------------------------------------------- 7. the memory contract
@pytest.mark.parametrize("chain", [FULL, FX])
def test_gpu_cabinet_memory_contract(chain):
    nb = 12
    per = nb * 128
    ir = responses(300)
    x = noise(nb) if chain == FX else None
    sc = scens(nb)
    eng = engine(chain, ir)
    ref, _ = one_call(eng, sc, nb, x=x)
    eng.close()
    fill = 12345.5
    for wet, rotors in ((True, True), (False, False), (True, False), (False, True)):
        eng = engine(chain, ir)
        got, raw = one_call(eng, sc, nb, x=x, wet=wet, rotors=rotors, stride=per + 131, lead=1, fill=fill)
        eng.close()
        assert set(got) == {"L", "R"} | ({"wetL", "wetR"} if wet else set()) | (set(PLANES[4:]) if rotors else set())
        for k, rows in got.items():
            same(rows[:, :per], ref[k], f"chain {chain} wet {wet} rotors {rotors}: odd stride rows, {k}")
            assert (rows[:, per:] == fill).all() and raw[k][0] == fill, f"{k}: sentinel overwritten"


# ---------------------------------------------------------------- 8. timing
def test_gpu_cabinet_time():
    """cabinet_time counts k_cabinet's launches while it is on, hands them out once, and counts
    nothing while it is off: one instance, one block, the one-tap response"""
    eng = engine(FULL, responses(1), n=1)
    eng.cabinet_time(True)
    for _ in range(2):
        eng.render_cabinet(1)
    ms, n = eng.cabinet_time()
    assert n == 2 and ms > 0.0
    assert eng.cabinet_time() == (0.0, 0)
    eng.cabinet_time(False)
    eng.render_cabinet(1)
    assert eng.cabinet_time() == (0.0, 0)
    eng.close()
