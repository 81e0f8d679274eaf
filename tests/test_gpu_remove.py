"""GPU tests of tbf_instances_remove: the survivors of a removal against the CPU oracle and
against a twin engine that held only them from the start, bit for bit (enginerun.assert_bits).

A survivor must render what the oracle renders for an organ of its SEED with its own script,
whatever index it had before and has now.  The histories are test_gpu_state's (H = 24 blocks:
every ring has wrapped, a rotor ramp and a release are in flight, the control rand() stream
has advanced), and block H's events are queued, not rendered, when the removal is made.
"""
import ctypes as C

import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits
from fx_oracle import fx_run
from test_gpu_parity import DISPATCH, _engine, _ran, _setup
from test_gpu_state import (FORK_CASES, FORK_WRING, H, PGM, _apply, check_rows, cont_other, cont_same, history,
                            oracle_rows, queue, run_span)

pytestmark = pytest.mark.gpu

_REFS = {}


def _ref(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
        for a in _REFS[key]:
            a.setflags(write=False)
    return _REFS[key]


def script(i, at=H):
    """organ i's whole script: the history, then a continuation of its own (odd organs: the
    one with a reverb, rotor and character change and a random-drawbar programme).  Organs
    with i % 3 = 1, 2 step their program once and twice more than the others in the history
    (blocks 5 and 7), so neighbours differ in their persistent program slot rotation."""
    more = [(5, "note", 84 + i % 3, 1)] * (i % 3 >= 1) + [(7, "note", 84 + i % 3, 0)] * (i % 3 == 2)
    return history(i) + more + (cont_other(i, at) if i % 2 else cont_same(i, at))


def seed_of(i):
    return 1000 + 17 * i          # _setup's seeds


def organs(ids, **kw):
    """an engine whose instance k is organ ids[k] (_setup's template; seed and script by id)"""
    eng = _engine(**kw)
    eng.add_instances([eng.template(seed=7)] * len(ids), [seed_of(i) for i in ids])
    eng.program_parse(PGM)
    return eng


def ref6(oracle, tpl, sr=48000.0, cfg=None):
    """organs 0 .. 5 with their scripts, H + 40 blocks: the reference most tests share"""
    return _ref(("six", sr, cfg), lambda: oracle_rows(oracle, tpl, [seed_of(i) for i in range(6)],
                                                      [script(i) for i in range(6)], H + 40))


def rows_of(ref, ids):
    return [r[ids] for r in ref]


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("dispatch", list(DISPATCH))
@pytest.mark.parametrize("case", list(FORK_CASES))
def test_gpu_remove_against_the_oracle(oracle, case, dispatch):
    sr, cfg, dbg, env = FORK_CASES[case]
    nb, gone, keep = H + 40, [1, 4], [0, 2, 3, 5]
    eng, tpl, seeds, _ = _setup(oracle, 6, history, sr=sr, debug_flags=dbg, cfg=None if cfg is None else S.CFG_SETS[cfg],
                                env={**DISPATCH[dispatch], **env})
    if case in FORK_WRING:
        assert eng.layout()["wring_len"] == FORK_WRING[case]
    eng.program_parse(PGM)
    scens = [script(i) for i in range(6)]
    ref = ref6(oracle, tpl, sr, cfg)
    head = run_span(eng, scens, 0, H)
    check_rows(f"remove {case} [{dispatch}] history", head, ref, b1=H)
    queue(eng, scens, H)                           # un-rendered events: the survivors keep theirs
    assert eng.remove(gone).tolist() == [0, -1, 1, 2, -1, 3] and eng.n_instances == 4
    tail = run_span(eng, [scens[i] for i in keep], H, nb, queued=True)
    check_rows(f"remove {case} [{dispatch}] blocks {H}..{nb}", tail, rows_of(ref, keep), b0=H)
    assert float(np.abs(tail[0]).max()) > 1e-3
    _ran(eng, dispatch)                            # the kernels the case's name says
    eng.close()


# ------------------------------------------------------------------ 2. shapes of the mover
GONE_57 = sorted([0, 56] + list(range(24, 33)) + [2, 5, 7, 11, 13, 17, 19, 22, 34, 37, 40, 41, 43, 46, 47, 50, 52, 53, 55])


def test_gpu_remove_shapes_57_to_27(oracle):
    """57 instances, 30 removed (the first, the last, a run of 9 across index 28, scattered
    single ones) to 27: from beyond the 56-instance workgroup boundary to below the
    28-instance one, an odd count.  Every row equals the row of a twin that held the 27 from
    the start with the same render calls; four rows equal the oracle; the device memory held
    is the twin's."""
    n, nb = 57, H + 16
    assert len(GONE_57) == 30 and len(set(GONE_57)) == 30
    keep = [i for i in range(n) if i not in GONE_57]
    a, tpl, _, _ = _setup(oracle, n, history)
    a.program_parse(PGM)
    c = organs(keep)
    sa, sc = [script(i) for i in range(n)], [script(i) for i in keep]
    run_span(a, sa, 0, H)
    run_span(c, sc, 0, H)
    queue(a, sa, H)
    queue(c, sc, H)
    big = a.device_bytes()
    m = a.remove(GONE_57)
    assert a.n_instances == 27
    assert [int(m[i]) for i in keep] == list(range(27)) and all(m[i] == -1 for i in GONE_57)
    assert a.device_bytes()[0] == c.device_bytes()[0] > 0   # before the next render already
    La, Ra = run_span(a, sc, H, nb, queued=True)
    Lc, Rc = run_span(c, sc, H, nb, queued=True)
    assert_bits(La, Lc, "57 -> 27 against the twin L")
    assert_bits(Ra, Rc, "57 -> 27 against the twin R")
    rows = [0, 14, 15, 26]                                   # organs 1, 23, 33 (either side of the run), 54
    pick = [keep[r] for r in rows]
    assert pick == [1, 23, 33, 54]
    ref = oracle_rows(oracle, tpl, [seed_of(i) for i in pick], [script(i) for i in pick], nb)
    check_rows("57 -> 27", (La[rows], Ra[rows]), ref, b0=H)
    small = c.device_bytes()
    assert a.device_bytes() == small and small[0] > 0 and small[1] > 0
    assert big[0] > small[0] and big[1] > small[1], (big, small)   # (the hook reports no constant)
    a.close()
    c.close()


# ------------------------------------------------------------------ 3. edges
def test_gpu_remove_the_only_instance_then_add(oracle):
    """1 -> 0 -> 1: the engine renders nothing in between, holds no instance memory, and the
    new instance equals the oracle from time zero of its seed."""
    nb = 24
    eng, tpl, seeds, _ = _setup(oracle, 1, history)
    eng.program_parse(PGM)
    run_span(eng, [script(0)], 0, H)
    queue(eng, [script(0)], H)
    assert eng.remove(0).tolist() == [-1] and eng.n_instances == 0
    assert eng.device_bytes() == (0, 0)
    fp, row = C.POINTER(C.c_float), np.full(384, 7.0, np.float32)
    assert eng._lib.tbf_render(eng._h, 3, row.ctypes.data_as(fp), row.ctypes.data_as(fp), 384) == 0
    assert (row == 7.0).all() and eng.device_bytes() == (0, 0)
    assert eng.add_instances([0], [seed_of(3)]) == 0          # the template id is still valid
    got = run_span(eng, [script(3)], 0, nb)
    check_rows("1 -> 0 -> 1", got, rows_of(ref6(oracle, tpl), [3]), b1=nb)
    eng.close()


@pytest.mark.parametrize("which", ["last", "first"])
def test_gpu_remove_last_or_first(oracle, which):
    """The removed instance has a retune pending (and block H's events): nothing of it may
    reach the instance that takes its index."""
    nb = H + 16
    eng, tpl, seeds, _ = _setup(oracle, 3, history)
    eng.program_parse(PGM)
    other = eng.template(seed=8)
    scens = [script(i) for i in range(3)]
    run_span(eng, scens, 0, H)
    queue(eng, scens, H)
    gone, keep, want = (2, [0, 1], [0, 1, -1]) if which == "last" else (0, [1, 2], [-1, 0, 1])
    eng.retune(gone, other)
    assert eng.remove(gone).tolist() == want
    tail = run_span(eng, [scens[i] for i in keep], H, nb, queued=True)
    check_rows(f"remove the {which}", tail, rows_of(ref6(oracle, tpl), keep), b0=H, b1=nb)
    eng.close()


def test_gpu_remove_before_any_render(oracle):
    eng, tpl, seeds, _ = _setup(oracle, 3, history)
    eng.program_parse(PGM)
    scens = [script(i) for i in range(3)]
    queue(eng, scens, 0)
    assert eng.remove(1).tolist() == [0, -1, 1]
    got = run_span(eng, [scens[0], scens[2]], 0, H, queued=True)
    check_rows("remove before the first render", got, rows_of(ref6(oracle, tpl), [0, 2]), b1=H)
    eng.close()


def test_gpu_remove_keeps_a_pending_retune(oracle, tunings):
    """Organ 1 was retuned at block 12 and rendered on; organ 2's retune is pending at the
    removal of organ 0.  Both move down one index and continue like the oracle's."""
    from orc_bind import Template
    m19 = np.asarray(tunings["19TET"], np.float64)
    nb = H + 16
    eng = _engine()
    tids = [eng.template(seed=7), eng.template(mts128=m19, seed=8)]
    eng.add_instances([tids[0]] * 3, [seed_of(i) for i in range(3)])
    hist = [[e for e in history(i) if e[1] != "program"] for i in range(3)]   # (as test_gpu_clone_retune_*)
    scens = [hist[0] + cont_same(0),
             hist[1] + [(12, "retune", 1, 0), (12, "note", 60, 1), (14, "note", 64, 1)] + cont_same(1),
             hist[2] + [(H, "retune", 1, 0)] + cont_same(2)]
    t12, t19 = Template(oracle, seed=7), Template(oracle, mts128=m19, seed=8)
    ref = oracle_rows(oracle, t12, [seed_of(1), seed_of(2)], scens[1:], nb, templates=[t12, t19])
    run_span(eng, scens, 0, H, tids=tids)
    queue(eng, scens, H, tids=tids)
    assert eng.remove(0).tolist() == [-1, 0, 1]
    tail = run_span(eng, scens[1:], H, nb, tids=tids, queued=True)
    check_rows("remove around a retune", tail, ref, b0=H)
    eng.close()


# ------------------------------------------------------------------ 4. remove, then grow again
@pytest.mark.parametrize("ctl", ["device_control", "host_control"])
def test_gpu_remove_then_add_and_clone(oracle, ctl):
    """4 organs, organ 1 removed; a new organ 9 added (it starts at its time zero, the engine's
    block H); organ 2, renumbered to index 1, cloned with block H's events queued, the clone
    then takes another continuation.  Survivors, new instance and clone equal the oracle."""
    env = {} if ctl == "device_control" else {"TBF_HOST_CONTROL": "1"}
    nb = H + 24
    eng, tpl, seeds, _ = _setup(oracle, 4, history, env=env)
    eng.program_parse(PGM)
    scens = [script(i) for i in range(4)]
    run_span(eng, scens, 0, H)
    queue(eng, scens, H)
    assert eng.remove(1).tolist() == [0, -1, 1, 2]
    fresh = script(9, at=12)                                   # organ 9's own time
    late = [(b + H, k, a, v) for (b, k, a, v) in fresh if b + H < nb]
    assert eng.add_instances([eng.template(seed=7)], [seed_of(9)]) == 3
    assert eng.clone(1) == 4 and eng.n_instances == 5
    forked = [e for e in script(2) if e[0] <= H] + cont_other(2)
    for inst, evs in ((3, late), (4, cont_other(2))):
        for ev in evs:
            if ev[0] == H:
                _apply(eng, inst, ev)
    got = run_span(eng, [scens[0], scens[2], scens[3], late, forked], H, nb, queued=True)
    ref = ref6(oracle, tpl)
    check_rows(f"remove, add, clone [{ctl}]: survivors", (got[0][:3], got[1][:3]), rows_of(ref, [0, 2, 3]), b0=H, b1=nb)
    more = _ref(("grow",), lambda: oracle_rows(oracle, tpl, [seed_of(9), seed_of(2)], [fresh, forked], nb))
    assert_bits(got[0][3], more[0][0, :(nb - H) * 128], "the new instance L")
    assert_bits(got[1][3], more[1][0, :(nb - H) * 128], "the new instance R")
    assert_bits(got[0][4], more[0][1, H * 128:], "the clone of a renumbered survivor L")
    assert_bits(got[1][4], more[1][1, H * 128:], "the clone of a renumbered survivor R")
    assert not np.array_equal(got[0][4], got[0][1])
    eng.close()


# ------------------------------------------------------------------ 5. effects-only chain
def test_gpu_remove_fx_chain(oracle):
    import tunebfree_amd as T
    from test_gpu_fx_chain import fx_input, fx_settings
    n, nb, gone, keep = 6, H + 40, [1, 4], [0, 2, 3, 5]
    g = np.random.default_rng(78)
    x = np.stack([fx_input(i, nb * 128, g) for i in range(n)])
    scens = [fx_settings(i + 1) + [(H - 6, "param", S.P_DRUM, 2), (H - 6, "param", S.P_HORN, 2),
                                   (H, "param", S.P_CHARACTER, 0.3 + 0.1 * i), (H + 4, "param", S.P_REVERB, 0.45)]
             for i in range(n)]
    eng = _engine(chain=T.engine.CHAIN_FX)
    seeds = [seed_of(i) for i in range(n)]
    eng.add_instances([eng.template(seed=7)] * n, seeds)
    for b0, b1 in ((0, H - 6), (H - 6, H)):
        queue(eng, scens, b0)
        eng.process(x[:, b0 * 128:b1 * 128])
    queue(eng, scens, H)
    assert eng.remove(gone).tolist() == [0, -1, 1, 2, -1, 3]
    sk, xk = [scens[i] for i in keep], x[keep]
    Ls, Rs = [], []
    for b0, b1 in ((H, H + 4), (H + 4, nb)):
        if b0 > H:
            queue(eng, sk, b0)
        L, R = eng.process(xk[:, b0 * 128:b1 * 128])
        Ls.append(L)
        Rs.append(R)
    ref = fx_run(oracle, [seeds[i] for i in keep], xk, sk)
    assert_bits(np.concatenate(Ls, axis=1), ref[2][:, H * 128:], "fx remove L")
    assert_bits(np.concatenate(Rs, axis=1), ref[3][:, H * 128:], "fx remove R")
    c = eng.launches()
    assert c["k_tonegen"] == 0 and c["k_tonegen_ranges"] == 0, c
    eng.close()


# ------------------------------------------------------------------ 6. tbf_synth_sound
def test_gpu_remove_synth_sound_fifo(oracle):
    """A removal made with 56 frames of a block still in the FIFO: the survivors serve those
    frames from their own rows, then irregular periods."""
    eng, tpl, seeds, _ = _setup(oracle, 3, history)
    oscen = [S.bench_scenario(i) for i in range(3)]
    queue(eng, oscen, 0)
    L0, R0 = eng.synth_sound(200)
    assert eng.remove(1).tolist() == [0, -1, 1]
    keep = [0, 2]
    rng = np.random.default_rng(10)
    outs, consumed = [], 200
    for c, nf in enumerate([56] + [int(v) for v in rng.integers(1, 301, 9)]):
        if c in (3, 6):
            blk = -(-consumed // 128)
            for k, i in enumerate(keep):
                ev = (blk, "note", 65 + c + i, 1)
                oscen[i].append(ev)
                _apply(eng, k, ev)
        outs.append(eng.synth_sound(nf))
        consumed += nf
    L = np.concatenate([o[0] for o in outs], axis=1)
    R = np.concatenate([o[1] for o in outs], axis=1)
    oL, oR = oracle_rows(oracle, tpl, [seeds[i] for i in keep], [oscen[i] for i in keep], -(-consumed // 128))
    assert_bits(np.concatenate([L0[keep], L], axis=1), oL[:, :consumed], "synth_sound after a removal L")
    assert_bits(np.concatenate([R0[keep], R], axis=1), oR[:, :consumed], "synth_sound after a removal R")
    assert L[1, :56].any() and not np.array_equal(L[0, :56], L[1, :56])   # (the frames the FIFO held)
    eng.close()


# ------------------------------------------------------------------ 7. long steady chunk
def test_gpu_remove_after_long_steady_chunk(oracle):
    """A 130-block history that ends in one 104-block steady chunk (stage buffers of 128
    blocks), then the removal of the first of three."""
    h2, nb = 130, 130 + 24
    eng, tpl, seeds, _ = _setup(oracle, 3, history)
    eng.program_parse(PGM)
    assert eng.set_steady_chunk(128) == 128
    scens = [history(i) + cont_same(i, h2) for i in range(3)]
    ref = oracle_rows(oracle, tpl, seeds[1:], scens[1:], nb)
    run_span(eng, scens, 0, H)
    eng.render(2)
    L, R = eng.render(h2 - H - 2)                  # 104 blocks, nothing pending: one chunk
    assert eng.chunks()[1] == 128
    assert_bits(L[1:], ref[0][:, (H + 2) * 128:h2 * 128], "steady chunk L")
    queue(eng, scens, h2)
    assert eng.remove(0).tolist() == [-1, 0, 1]
    tail = run_span(eng, scens[1:], h2, nb, queued=True)
    check_rows("remove after a steady chunk", tail, ref, b0=h2)
    eng.close()


# ------------------------------------------------------------------ 8. the caller's stream
def test_gpu_remove_between_renders_on_a_caller_stream(oracle):
    import torch
    nb, keep = H + 16, [0, 2, 3, 5]
    eng, tpl, seeds, _ = _setup(oracle, 6, history)
    eng.program_parse(PGM)
    scens = [script(i) for i in range(6)]
    st = torch.cuda.Stream()
    L = torch.zeros((6, H * 128), dtype=torch.float32, device="cuda")
    R = torch.zeros_like(L)
    done = 0
    for b in sorted({e[0] for sc in scens for e in sc if e[0] < H} | {H}):
        if b > done:
            eng.render_device(b - done, L[:, done * 128:].data_ptr(), R[:, done * 128:].data_ptr(), H * 128, st.cuda_stream)
            done = b
        if b < H:
            queue(eng, scens, b)
    st.synchronize()
    queue(eng, scens, H)
    assert eng.remove([4, 1]).tolist() == [0, -1, 1, 2, -1, 3]
    sk = [scens[i] for i in keep]
    L2 = torch.zeros((4, (nb - H) * 128), dtype=torch.float32, device="cuda")
    R2 = torch.zeros_like(L2)
    done = H
    for b in sorted({e[0] for sc in sk for e in sc if H < e[0] < nb} | {nb}):
        eng.render_device(b - done, L2[:, (done - H) * 128:].data_ptr(), R2[:, (done - H) * 128:].data_ptr(),
                          (nb - H) * 128, st.cuda_stream)
        done = b
        if b < nb:
            queue(eng, sk, b)
    st.synchronize()
    ref = ref6(oracle, tpl)
    check_rows("caller stream, history", (L.cpu().numpy(), R.cpu().numpy()), ref, b1=H)
    check_rows("caller stream, after the removal", (L2.cpu().numpy(), R2.cpu().numpy()), rows_of(ref, keep), b0=H, b1=nb)
    eng.close()


# ------------------------------------------------------------------ 9. refusals
def test_gpu_remove_refusals_change_nothing(oracle):
    import tunebfree_amd as T
    lib = T.load_library()
    u32p = C.POINTER(C.c_uint32)
    nb = H + 8
    eng, tpl, seeds, _ = _setup(oracle, 3, history)
    eng.program_parse(PGM)
    scens = [script(i) for i in range(3)]
    run_span(eng, scens, 0, H)
    queue(eng, scens, H)
    held = eng.device_bytes()
    m = np.full(3, 77, np.uint32)
    for lst in ([0, 3], [2, 1, 2]):
        with pytest.raises(T.TbfError, match="tbf error -22"):
            eng.remove(lst)
        arr = np.array(lst, np.uint32)
        assert lib.tbf_instances_remove(eng._h, len(arr), arr.ctypes.data_as(u32p), m.ctypes.data_as(u32p)) == -22
    assert lib.tbf_instances_remove(eng._h, 1, None, m.ctypes.data_as(u32p)) == -22
    assert (m == 77).all() and eng.n_instances == 3 and eng.device_bytes() == held
    assert eng.remove([]).tolist() == [0, 1, 2] and eng.device_bytes() == held
    got = run_span(eng, scens, H, nb, queued=True)
    check_rows("after the refused removals", got, rows_of(ref6(oracle, tpl), [0, 1, 2]), b0=H, b1=nb)
    eng.close()
