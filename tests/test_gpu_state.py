"""GPU tests of tbf_instances_clone / tbf_instances_save / tbf_instances_load: forked,
saved and restored instances against the CPU oracle, bit for bit (enginerun.assert_bits).

A clone of instance s must render what the oracle renders for an organ of s's SEED that had
s's history and then the clone's own events.  Every rendered history is >= 24 blocks (3072
samples: past the longest reverb line, the predelay history and every whirl ring window, so
every ring has wrapped) with overdrive on, percussion decaying, vibrato routed, a random
programme change (the control rand() stream has advanced), a rotor speed change 6 blocks
before the fork (the fork lands mid-ramp) and a key released in the last block before it (a
release envelope / steadyPending in flight).
"""
import ctypes as C

import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits, oracle_run
from fx_oracle import fx_run
from test_gpu_parity import DISPATCH, _engine, _ran, _setup

pytestmark = pytest.mark.gpu

H = 24                                    # blocks of history before a fork
PGM = '5 { name="any bars", drawbars=random }\n'
PC_RANDOM = 4                             # program change 4 -> programme 5 (offset 1)
_REFS = {}


def _ref(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
        for a in _REFS[key]:
            a.setflags(write=False)
    return _REFS[key]


# ------------------------------------------------------------------ scripts
def history(i):
    ev = S.bench_scenario(i)                               # overdrive, percussion, vibrato C3, chord at 0
    ev += [(2, "program", PC_RANDOM, 0)]
    ev += [(10, "note", 72 + i % 5, 1), (10, "param", S.P_DRAWBAR + 4, 5)]
    ev += [(H - 6, "param", S.P_DRUM, 2), (H - 6, "param", S.P_HORN, 2)]
    ev += [(H - 1, "note", S.chord_for(i)[1], 0)]
    return ev


def cont_same(i, at=H):
    """the source's continuation; its first events sit at block `at`"""
    c = S.chord_for(i + 7)
    return [(at, "note", c[0], 1), (at, "note", c[2], 1), (at + 5, "param", S.P_DRAWBAR + 2, 3),
            (at + 9, "note", S.chord_for(i)[0], 0), (at + 14, "param", S.P_DRUM, 1), (at + 14, "param", S.P_HORN, 1),
            (at + 20, "note", c[0], 0)]


def cont_other(i, at=H):
    """a different one: reverb mix, rotor stop, character, a new chord, a drawbar move, a
    programme change with random drawbars"""
    c = S.chord_for(i + 11)
    return [(at, "param", S.P_REVERB, 0.6), (at, "param", S.P_DRUM, 0), (at, "param", S.P_HORN, 0),
            (at, "param", S.P_CHARACTER, 0.9)] + [(at, "note", k, 1) for k in c] + \
           [(at + 2, "param", S.P_DRAWBAR + 1, 2), (at + 3, "program", PC_RANDOM, 0), (at + 12, "note", c[1], 0),
            (at + 13, "param", S.P_VIBRATO_TYPE, 1)]


def for_oracle(scen, seed):
    """the script as the oracle takes it: a random-drawbar programme change becomes the
    drawbar parameters of the instance's control rand() stream (seed ^ 0x5bd1e995)"""
    g = S.GlibcRand((seed ^ 0x5bd1e995) & 0xFFFFFFFF)
    out = []
    for ev in sorted(scen, key=lambda e: e[0]):
        if ev[1] == "program":
            out += [(ev[0], "param", S.P_DRAWBAR + j, g.next() % 9) for j in range(9)]
        else:
            out.append(ev)
    return out


def _apply(eng, i, ev, tids=None):
    (_, kind, a, v) = ev
    if kind == "note":
        eng.note(i, a, v)
    elif kind == "program":
        eng.program_install(i, a)
    elif kind == "control":
        assert eng.midi_control(i, a, v)
    elif kind == "retune":
        eng.retune(i, tids[a])
    else:
        eng.set_param(i, a, v)


def queue(eng, scens, b, tids=None):
    """the scripts' events of block b, through the API, not rendered yet"""
    for i, sc in enumerate(scens):
        for ev in sc:
            if ev[0] == b:
                _apply(eng, i, ev, tids)


def run_span(eng, scens, b0, b1, tids=None, queued=False):
    """blocks [b0, b1) with the scripts' events at their blocks (queued: block b0's are
    already in), one tbf_render per stretch between events"""
    bounds = sorted({b0, b1} | {e[0] for sc in scens for e in sc if b0 < e[0] < b1})
    Ls, Rs = [], []
    for s, e in zip(bounds[:-1], bounds[1:]):
        if not (queued and s == b0):
            queue(eng, scens, s, tids)
        L, R = eng.render(e - s)
        Ls.append(L)
        Rs.append(R)
    return np.concatenate(Ls, axis=1), np.concatenate(Rs, axis=1)


def run_events(eng, scens, b0, b1):
    """the same in ONE tbf_render_events call (note / param / program events)"""
    import torch
    kinds = {"note": 0, "param": 1, "program": 3}
    rows = [(e[0] - b0, i, kinds[e[1]], e[2], float(e[3])) for i, sc in enumerate(scens) for e in sc if b0 <= e[0] < b1]
    n, nb = eng.n_instances, b1 - b0
    L = torch.zeros((n, nb * 128), dtype=torch.float32, device="cuda")
    R = torch.zeros_like(L)
    eng.render_events_device(nb, eng.events(rows), L.data_ptr(), R.data_ptr(), nb * 128)
    eng.synchronize()
    return L.cpu().numpy(), R.cpu().numpy()


def oracle_rows(oracle, tpl, seeds, scens, nb, **kw):
    return oracle_run(oracle, tpl, seeds, [for_oracle(sc, sd) for sc, sd in zip(scens, seeds)], nb, **kw)[:2]


def check_rows(what, got, ref, rows=None, b0=0, b1=None):
    for name, g, r in zip("LR", got, ref):
        r = r[:, b0 * 128:None if b1 is None else b1 * 128]
        assert_bits(g if rows is None else g[rows], r, f"{what} {name}")


# ------------------------------------------------------------------ 1. fork against the oracle
FORK_CASES = {
    # name: (sample rate, cfg set, debug flags, engine environment)
    "48k": (48000.0, None, 0, {}),
    "48k_host_front": (48000.0, None, 0, {"TBF_DEVICE_FRONT": "0"}),
    "48k_host_control": (48000.0, None, 0, {"TBF_HOST_CONTROL": "1"}),
    "96k": (96000.0, None, 0, {}),                      # W = 1024
    "96k_wide": (96000.0, "geometry_wide", 0, {}),      # W = 2048
    "48k_force_serial": (48000.0, None, 1, {}),         # TBF_DEBUG_FORCE_SERIAL
}
FORK_WRING = {"48k": 512, "96k": 1024, "96k_wide": 2048}


def _fork_scripts(seeds3):
    """rows 0-2: the sources; 3, 5: clones of 0, 1 with their source's continuation; 4: a
    clone of 1 with the source's queued block-H events and then another continuation"""
    src = [history(i) + cont_same(i) for i in range(3)]
    other = history(1) + [e for e in cont_same(1) if e[0] == H] + cont_other(1)
    return src + [src[0], other, src[1]], list(seeds3) + [seeds3[0], seeds3[1], seeds3[1]]


@pytest.mark.parametrize("dispatch", list(DISPATCH))
@pytest.mark.parametrize("case", list(FORK_CASES))
def test_gpu_fork_same_and_divergent_continuations(oracle, case, dispatch):
    sr, cfg, dbg, env = FORK_CASES[case]
    nb = H + 40
    eng, tpl, seeds, _ = _setup(oracle, 3, history, sr=sr, debug_flags=dbg, cfg=None if cfg is None else S.CFG_SETS[cfg],
                                env={**DISPATCH[dispatch], **env})
    if case in FORK_WRING:
        assert eng.layout()["wring_len"] == FORK_WRING[case]
    eng.program_parse(PGM)
    scens, seeds6 = _fork_scripts(seeds)
    ref = _ref(("fork", sr, cfg), lambda: oracle_rows(oracle, tpl, seeds6, scens, nb))
    head = run_span(eng, scens[:3], 0, H)
    check_rows(f"fork {case} [{dispatch}] history", head, [r[:3] for r in ref], b1=H)
    queue(eng, scens[:3], H)                       # un-rendered events: the clones inherit them
    assert eng.clone([0, 1, 1]) == 3 and eng.n_instances == 6
    for ev in cont_other(1):
        if ev[0] == H:
            _apply(eng, 4, ev)
    tail = run_span(eng, scens, H, nb, queued=True)
    check_rows(f"fork {case} [{dispatch}] blocks {H}..{nb}", tail, ref, b0=H)
    assert not np.array_equal(tail[0][4], tail[0][1]) and float(np.abs(tail[0][4]).max()) > 1e-3
    _ran(eng, dispatch)                            # the kernels the case's name says
    eng.close()


# ------------------------------------------------------------------ 2. persistent-slot rotation
@pytest.mark.parametrize("calls", [1, 2, 3])
def test_gpu_fork_persistent_slot_rotation(oracle, calls):
    """The history as 1, 2 and 3 tbf_render_events calls, each with a key event (blocks 0, 10,
    23), so each is one chunk that steps the sources' programs and rotates their persistent
    program slot: 1, 2, 0 at the fork."""
    nb = H + 40
    eng, tpl, seeds, _ = _setup(oracle, 3, history)
    eng.program_parse(PGM)
    scens, seeds6 = _fork_scripts(seeds)
    ref = _ref(("fork", 48000.0, None), lambda: oracle_rows(oracle, tpl, seeds6, scens, nb))
    cuts = {1: [0, H], 2: [0, 12, H], 3: [0, 8, 16, H]}[calls]
    for a, b in zip(cuts[:-1], cuts[1:]):
        run_events(eng, scens[:3], a, b)
    queue(eng, scens[:3], H)
    assert eng.clone([0, 1, 1]) == 3
    for ev in cont_other(1):
        if ev[0] == H:
            _apply(eng, 4, ev)
    tail = run_span(eng, scens, H, nb, queued=True)
    check_rows(f"fork after {calls} event calls", tail, ref, b0=H)
    eng.close()


def test_gpu_fork_after_long_steady_chunk(oracle):
    """A 130-block history that ends in one steady chunk longer than 64 blocks (104: the two
    blocks before it settle the release that block 23 started)."""
    h2, nb = 130, 130 + 24
    eng, tpl, seeds, _ = _setup(oracle, 2, history)
    eng.program_parse(PGM)
    assert eng.set_steady_chunk(128) == 128
    src = [history(i) + cont_same(i, h2) for i in range(2)]
    scens = src + [src[1], history(0) + [e for e in cont_same(0, h2) if e[0] == h2] + cont_other(0, h2)]
    seeds4 = seeds + [seeds[1], seeds[0]]
    ref = oracle_rows(oracle, tpl, seeds4, scens, nb)
    run_span(eng, scens[:2], 0, H)
    eng.render(2)
    L, R = eng.render(h2 - H - 2)                  # 104 blocks, nothing pending: one chunk
    assert eng.chunks()[1] == 128
    assert_bits(L, ref[0][:2, (H + 2) * 128:h2 * 128], "steady chunk L")
    queue(eng, scens[:2], h2)
    assert eng.clone([1, 0]) == 2
    for ev in cont_other(0, h2):
        if ev[0] == h2:
            _apply(eng, 3, ev)
    tail = run_span(eng, scens, h2, nb, queued=True)
    check_rows("fork after a steady chunk", tail, ref, b0=h2)
    eng.close()


@pytest.mark.parametrize("ctl", ["device_control", "host_control"])
def test_gpu_clone_stays_put_while_source_moves(oracle, ctl):
    """A settled clone (nothing pending at the fork, no event after it) keeps playing its own
    copy of the program while its source steps four times -- more often than there are
    persistent slots -- so a clone whose program offset still pointed into the source's slots
    would play the source's new chords."""
    env = {} if ctl == "device_control" else {"TBF_HOST_CONTROL": "1"}
    f, nb = H + 2, H + 2 + 16
    eng, tpl, seeds, _ = _setup(oracle, 2, history, env=env)
    eng.program_parse(PGM)
    moves = [[(f + 2 * k, "note", 50 + 3 * k + i, 1) for k in range(4)] + [(f + 9, "note", 50 + i, 0)] for i in range(2)]
    scens = [history(i) + moves[i] for i in range(2)] + [history(1), history(0)]
    run_span(eng, scens[:2], 0, f)                 # two blocks past the release: settled
    assert eng.clone([1, 0]) == 2
    tail = run_span(eng, scens, f, nb)
    check_rows(f"settled clone [{ctl}]", tail, oracle_rows(oracle, tpl, seeds + [seeds[1], seeds[0]], scens, nb), b0=f)
    assert not np.array_equal(tail[0][2], tail[0][1])
    eng.close()


# ------------------------------------------------------------------ 3. pending state
def test_gpu_clone_before_any_render(oracle):
    """Notes, parameters, a MIDI control function and a programme install, then the clone,
    then the first render: both rows equal the oracle from time zero."""
    nb = 24
    eng, tpl, seeds, _ = _setup(oracle, 2, history)
    eng.program_parse(PGM)
    first = [S.bench_scenario(i) + [(0, "control", "whirl.horn.brakepos", 40 + i), (0, "program", PC_RANDOM, 0),
                                    (0, "param", S.P_DRUM, 2), (0, "param", S.P_HORN, 0)] for i in range(2)]
    later = [[(6, "note", 70 + i, 1), (9, "param", S.P_DRUM, 0), (15, "note", S.chord_for(i)[0], 0)] for i in range(2)]
    scens = [first[0] + later[0], first[1] + later[1], first[1] + later[0], first[0] + later[1]]
    seeds4 = seeds + [seeds[1], seeds[0]]
    queue(eng, first, 0)
    assert eng.clone([1, 0]) == 2
    got = run_span(eng, scens, 0, nb, queued=True)
    check_rows("clone before the first render", got, oracle_rows(oracle, tpl, seeds4, scens, nb))
    eng.close()


def test_gpu_clone_retune_pending_and_rendered(oracle, tunings):
    """Instance 0 was retuned at block 12 and rendered on; instance 1's retune is pending (called
    at the fork, not rendered).  Their clones continue like them."""
    from orc_bind import Template
    m19 = np.asarray(tunings["19TET"], np.float64)
    nb = H + 24
    eng = _engine()
    tids = [eng.template(seed=7), eng.template(mts128=m19, seed=8)]
    seeds = [1000, 1017]
    eng.add_instances([tids[0]] * 2, seeds)
    eng.program_parse(PGM)
    # (no programme change here: a retune restores the drawbars from the CLAP parameters,
    # which a programme does not set)
    hist = [[e for e in history(i) if e[1] != "program"] for i in range(2)]
    src = [hist[0] + [(12, "retune", 1, 0), (12, "note", 60, 1), (14, "note", 64, 1)] + cont_same(0),
           hist[1] + [(H, "retune", 1, 0)] + cont_same(1)]
    scens = src + [src[0], src[1]]
    t12, t19 = Template(oracle, seed=7), Template(oracle, mts128=m19, seed=8)
    ref = oracle_rows(oracle, t12, seeds + seeds, scens, nb, templates=[t12, t19])
    run_span(eng, src, 0, H, tids=tids)
    queue(eng, src, H, tids=tids)
    assert eng.clone([0, 1]) == 2
    tail = run_span(eng, scens, H, nb, tids=tids, queued=True)
    check_rows("clone around a retune", tail, ref, b0=H)
    eng.close()


# ------------------------------------------------------------------ 4. shapes of the mover
def test_gpu_clone_shapes_27_to_57(oracle):
    """27 instances cloned 30 times with repeats (instance 5 eight times) to 57: across the 28-
    and 56-instance workgroups of the chain blocks, an odd reverb pair count, a partial last
    workgroup.  Every clone row equals its source row; four rows equal the oracle."""
    n, nb = 27, H + 16
    eng, tpl, seeds, _ = _setup(oracle, n, history)
    eng.program_parse(PGM)
    scens = [history(i) + cont_same(i) for i in range(n)]
    run_span(eng, scens, 0, H)
    queue(eng, scens, H)
    src = [5] * 8 + [0, 26, 13, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19, 20, 26]
    assert len(src) == 30 and eng.clone(src) == n and eng.n_instances == 57
    L, R = run_span(eng, scens + [scens[s] for s in src], H, nb, queued=True)
    for k, s in enumerate(src):
        assert np.array_equal(L[n + k].view(np.uint32), L[s].view(np.uint32)), (k, s)
        assert np.array_equal(R[n + k].view(np.uint32), R[s].view(np.uint32)), (k, s)
    rows = [5, n + 7, n + 8, 56]
    pick = [5, 5, 0, 26]
    ref = oracle_rows(oracle, tpl, [seeds[i] for i in pick], [scens[i] for i in pick], nb)
    check_rows("27 -> 57", (L[rows], R[rows]), ref, b0=H)
    eng.close()


def test_gpu_clone_single_instance(oracle):
    nb = H + 16
    eng, tpl, seeds, _ = _setup(oracle, 1, history)
    eng.program_parse(PGM)
    sc = history(0) + cont_same(0)
    run_span(eng, [sc], 0, H)
    assert eng.clone(0) == 1
    got = run_span(eng, [sc, sc], H, nb)
    check_rows("n = 1 cloned once", got, oracle_rows(oracle, tpl, seeds * 2, [sc, sc], nb), b0=H)
    eng.close()


# ------------------------------------------------------------------ 5. effects-only chain
def test_gpu_clone_fx_chain(oracle):
    import tunebfree_amd as T
    from test_gpu_fx_chain import fx_input, fx_settings
    n, nb = 3, 2 * H
    g = np.random.default_rng(77)
    x = np.stack([fx_input(i, nb * 128, g) for i in (0, 3, 5)])
    xo = fx_input(0, nb * 128, g)                                  # another input for the divergent clone
    scens = [fx_settings(i + 1) + [(H - 6, "param", S.P_DRUM, 2), (H - 6, "param", S.P_HORN, 2),
                                   (H + 4, "param", S.P_REVERB, 0.45)] for i in range(n)]
    eng = _engine(chain=T.engine.CHAIN_FX)
    seeds = [1000 + 17 * i for i in range(n)]
    eng.add_instances([eng.template(seed=7)] * n, seeds)
    for b0, b1 in ((0, H - 6), (H - 6, H)):
        queue(eng, scens, b0)
        eng.process(x[:, b0 * 128:b1 * 128])
    assert eng.clone([0, 1, 1]) == 3
    x6 = np.concatenate([x, x[[0]], np.concatenate([x[1, :H * 128], xo[H * 128:]])[None], x[[1]]])
    sc6, seeds6 = scens + [scens[0], scens[1], scens[1]], seeds + [seeds[0], seeds[1], seeds[1]]
    Ls, Rs = [], []
    for b0, b1 in ((H, H + 4), (H + 4, nb)):
        if b0 > H:
            queue(eng, sc6, b0)
        L, R = eng.process(x6[:, b0 * 128:b1 * 128])
        Ls.append(L)
        Rs.append(R)
    L, R = np.concatenate(Ls, axis=1), np.concatenate(Rs, axis=1)
    ref = fx_run(oracle, seeds6, x6, sc6)
    assert_bits(L, ref[2][:, H * 128:], "fx clone L")
    assert_bits(R, ref[3][:, H * 128:], "fx clone R")
    assert np.array_equal(L[3], L[0]) and np.array_equal(L[5], L[1]) and not np.array_equal(L[4], L[1])
    c = eng.launches()
    assert c["k_tonegen"] == 0 and c["k_tonegen_ranges"] == 0, c
    eng.close()


# ------------------------------------------------------------------ 6. tbf_synth_sound
def test_gpu_clone_synth_sound_fifo(oracle):
    """A clone made with 56 frames of a block still in the FIFO serves those frames too."""
    eng, tpl, seeds, _ = _setup(oracle, 2, history)
    queue(eng, [S.bench_scenario(i) for i in range(2)], 0)
    L0, R0 = eng.synth_sound(200)
    assert eng.clone([0, 1]) == 2
    with pytest.raises(Exception, match="tbf error -16"):
        eng.save([0])
    rng = np.random.default_rng(9)
    outs, consumed, oscen = [], 200, [S.bench_scenario(i) for i in range(2)]
    for c, nf in enumerate([56] + [int(v) for v in rng.integers(1, 301, 9)]):
        if c in (3, 6):
            blk = -(-consumed // 128)
            for i in range(2):
                ev = (blk, "note", 65 + c + i, 1)
                oscen[i].append(ev)
                _apply(eng, i, ev)
                _apply(eng, 2 + i, ev)
        outs.append(eng.synth_sound(nf))
        consumed += nf
    L = np.concatenate([o[0] for o in outs], axis=1)
    R = np.concatenate([o[1] for o in outs], axis=1)
    assert_bits(L[2:], L[:2], "synth_sound: the clones' frames against the sources' L")
    assert_bits(R[2:], R[:2], "synth_sound R")
    oL, oR = oracle_rows(oracle, tpl, seeds, oscen, -(-consumed // 128))
    assert_bits(np.concatenate([L0[:2], L[:2]], axis=1), oL[:, :consumed], "synth_sound against the oracle L")
    assert L[2, :56].any()  # (the frames the FIFO held at the clone)
    eng.close()


# ------------------------------------------------------------------ 7. save / load, migrate
def other_history(i):
    ev = S.event_scenario(i + 3)
    return [e for e in ev if e[0] < H]


@pytest.mark.parametrize("ctl", ["device_control", "host_control"])
def test_gpu_save_load_migrate(oracle, ctl):
    env = {} if ctl == "device_control" else {"TBF_HOST_CONTROL": "1"}
    nb = H + 32
    a, tpl, seedsA, _ = _setup(oracle, 4, history, env=env)
    a.program_parse(PGM)
    scA = [history(i) + cont_same(i) for i in range(4)]
    run_span(a, scA, 0, H)
    blob = a.save([1, 3])
    b = _engine(env=env)
    seedsB = [77, 78, 79]
    b.add_instances([b.template(seed=7)] * 3, seedsB)
    b.program_parse(PGM)
    scB = [other_history(i) + cont_same(i + 2) for i in range(3)]
    run_span(b, scB, 0, H)
    b.load([2, 0], blob)
    rowsB = [scA[3], scB[1], scA[1]]
    gotA = run_span(a, scA, H, nb)
    gotB = run_span(b, rowsB, H, nb)
    ref = _ref(("migrate",), lambda: oracle_rows(oracle, tpl, seedsA + [seedsB[1]], scA + [scB[1]], nb))
    check_rows(f"migrate [{ctl}] engine A", gotA, [r[:4] for r in ref], b0=H)
    check_rows(f"migrate [{ctl}] engine B", gotB, [r[[3, 4, 1]] for r in ref], b0=H)
    a.close()
    b.close()


# ------------------------------------------------------------------ 8. rewind
def test_gpu_rewind(oracle):
    nb = H + 16
    eng, tpl, seeds, _ = _setup(oracle, 3, history)
    eng.program_parse(PGM)
    scens = [history(i) + cont_same(i) for i in range(3)]
    run_span(eng, scens, 0, H)
    blob = eng.save([0, 1, 2])
    X = run_span(eng, scens, H, nb)
    eng.load([0, 1, 2], blob)
    Y = run_span(eng, scens, H, nb)
    assert_bits(Y[0], X[0], "rewind L")
    assert_bits(Y[1], X[1], "rewind R")
    eng.load([0, 1, 2], blob)
    alt = [history(i) + [(H, "param", S.P_CHARACTER, 0.2 + 0.3 * i), (H + 3, "param", S.P_DRUM, 0)] for i in range(3)]
    Z = run_span(eng, alt, H, nb)
    check_rows("rewind, then another parameter", Z, oracle_rows(oracle, tpl, seeds, alt, nb), b0=H)
    eng.close()


# ------------------------------------------------------------------ 9. refusals
def test_gpu_refusals_change_nothing(oracle):
    import tunebfree_amd as T
    lib = T.load_library()
    nb = H + 8
    eng, tpl, seeds, _ = _setup(oracle, 2, history)
    eng.program_parse(PGM)
    scens = [history(i) + cont_same(i) for i in range(2)]
    run_span(eng, scens, 0, H)
    good = eng.save([0, 1])

    def organ(sr=48000.0, chain=0, cfg=None, tpl_seed=7):
        o = _engine(chain=chain, sr=sr)
        if cfg:
            o.config(cfg)
        o.add_instances([o.template(seed=tpl_seed)] * 2, seeds)
        o.render(2) if chain == 0 else None
        return o
    for kw, word in (({"sr": 96000.0}, "sample rate"), ({"chain": T.engine.CHAIN_FX}, "chain"),
                     ({"cfg": S.CFG_SETS["geometry"]}, "(fingerprint|wringLen)"), ({"tpl_seed": 8}, "template")):
        o = organ(**kw)
        with pytest.raises(T.TbfError, match="tbf error -22.*" + word):
            eng.load([0, 1], o.save([0, 1]))
        o.close()
    with pytest.raises(T.TbfError, match="tbf error -22.*count"):
        eng.load([0], good)
    size, inst = C.c_uint64(), np.array([0, 1], np.uint32)
    buf = np.zeros(len(good), np.uint8)
    u32p = C.POINTER(C.c_uint32)
    assert lib.tbf_instances_save(eng._h, 2, inst.ctypes.data_as(u32p), buf.ctypes.data, len(good) - 16, C.byref(size)) == -22
    assert size.value == len(good) and not buf.any()
    with pytest.raises(T.TbfError, match="tbf error -22"):
        eng.clone([0, 2])
    assert eng.n_instances == 2
    got = run_span(eng, scens, H, nb)
    check_rows("after the refusals", got, oracle_rows(oracle, tpl, seeds, scens, nb), b0=H)
    # frames pending in the tbf_synth_sound FIFO: -16 for save and load, and nothing changes
    eng.synth_sound(100)
    for call in (lambda: eng.save([0]), lambda: eng.load([0, 1], good)):
        with pytest.raises(T.TbfError, match="tbf error -16"):
            call()
    eng.close()


# ------------------------------------------------------------------ 10. the caller's stream
def test_gpu_clone_between_renders_on_a_caller_stream(oracle):
    import torch
    nb = H + 16
    eng, tpl, seeds, _ = _setup(oracle, 3, history)
    eng.program_parse(PGM)
    scens, seeds6 = _fork_scripts(seeds)
    st = torch.cuda.Stream()
    L = torch.zeros((3, H * 128), dtype=torch.float32, device="cuda")
    R = torch.zeros_like(L)
    done = 0
    for b in sorted({e[0] for sc in scens[:3] for e in sc if e[0] < H} | {H}):
        if b > done:
            eng.render_device(b - done, L[:, done * 128:].data_ptr(), R[:, done * 128:].data_ptr(), H * 128, st.cuda_stream)
            done = b
        if b < H:
            queue(eng, scens[:3], b)
    st.synchronize()
    queue(eng, scens[:3], H)
    assert eng.clone([0, 1, 1]) == 3
    for ev in cont_other(1):
        if ev[0] == H:
            _apply(eng, 4, ev)
    L2 = torch.zeros((6, (nb - H) * 128), dtype=torch.float32, device="cuda")
    R2 = torch.zeros_like(L2)
    done = H
    for b in sorted({e[0] for sc in scens for e in sc if H < e[0] < nb} | {nb}):
        eng.render_device(b - done, L2[:, (done - H) * 128:].data_ptr(), R2[:, (done - H) * 128:].data_ptr(),
                          (nb - H) * 128, st.cuda_stream)
        done = b
        if b < nb:
            queue(eng, scens, b)
    st.synchronize()
    ref = _ref(("fork", 48000.0, None), lambda: oracle_rows(oracle, tpl, seeds6, scens, H + 40))
    check_rows("caller stream, history", (L.cpu().numpy(), R.cpu().numpy()), [r[:3] for r in ref], b1=H)
    check_rows("caller stream, after the clone", (L2.cpu().numpy(), R2.cpu().numpy()), ref, b0=H, b1=nb)
    eng.close()
