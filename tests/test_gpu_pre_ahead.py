"""k_rv_pre ahead (TBF_PRE_AHEAD=1): chunk c + 1's k_rv_pre runs on the k_whirl stream in
front of k_whirl (c), in its own launch shape (24 instances and 8 waves a workgroup), and
k_whirl (c)'s launch is held back until chunk c + 1 has issued it, or until anything else
needs the streams complete.

Every test renders one script with the switch on and off through engines of chain 1, 2, 3
and 0, and compares bit for bit (enginerun.assert_bits): the switched-on render's stage taps
and outputs against the oracle, and the switched-off render against the switched-on one.
Engine.launches() and Engine.pre_ahead() say which launches ran: the switch changes none of
launches(), and pre_ahead() counts exactly the chunks the schedule can run ahead: a chunk
without control deltas, of at least 8 blocks (k_rv_core_lds), behind a chunk without control
deltas of the same call.

All engines run TBF_WHIRL_SPLIT=0 (k_whirl, the kernel the ahead launch shares its stream
with) and TBF_STEADY_CHUNK=64 (the shortest chunks: several per call at test sizes).  A
chunk with control deltas ends with new control entries, which the next two chunks (one per
control region) upload before they run, so neither of those runs ahead or holds a launch
back.  Every script therefore starts with a preamble of PRE blocks in renders of its own:
block 0 (the scripts' first events) and three 64-block chunks (the first still has deltas: the
controls settle over some blocks after an event; the other two upload), and the calls under
test start with a chunk that has neither deltas nor uploads.
"""
import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits, engine_run, oracle_run
from test_gpu_parity import TAPS, _engine, _script_events

pytestmark = pytest.mark.gpu

ENV = {"TBF_WHIRL_SPLIT": "0", "TBF_STEADY_CHUNK": "64"}
PRE = 1 + 192  # the preamble's blocks; its launches: k_rv_core 1, k_rv_core_lds 3, k_whirl 4


def _preamble(eng, scens):
    """the scripts' block-0 events and block 0, then 192 blocks (three chunks): L, R"""
    L0, R0 = engine_run(eng, [[e for e in sc if e[0] == 0] for sc in scens], 1)
    L1, R1 = eng.render(PRE - 1)
    return np.concatenate([L0, L1], axis=1), np.concatenate([R0, R1], axis=1)


def _after(scens):
    """the scripts as the oracle plays them: events past block 0 are given relative to the
    call under test, PRE blocks later"""
    return [[(b + PRE if b else 0, k, a, v) for (b, k, a, v) in sc] for sc in scens]


def _organ(n, chain, ahead, env=None, tpl_seed=7):
    eng = _engine(chain, env={**ENV, **(env or {}), "TBF_PRE_AHEAD": "1" if ahead else "0"})
    tid = eng.template(seed=tpl_seed)
    eng.add_instances([tid] * n, [1000 + 17 * i for i in range(n)])
    return eng


def _oracle(oracle, n, scens, nblocks, tpl_seed=7):
    from orc_bind import Template
    return oracle_run(oracle, Template(oracle, seed=tpl_seed), [1000 + 17 * i for i in range(n)], scens, nblocks)


def _one_call(eng, n, scens, nb, ev=None):
    """The preamble, then one call of nb blocks into device buffers, with the events ev
    (blocks relative to the call) if any."""
    import torch
    L0, R0 = _preamble(eng, scens)
    L = torch.zeros((n, nb * 128), dtype=torch.float32, device="cuda")
    R = torch.zeros_like(L)
    if ev is None:
        eng.render_device(nb, L.data_ptr(), R.data_ptr(), nb * 128)
    else:
        eng.render_events_device(nb, ev, L.data_ptr(), R.data_ptr(), nb * 128)
    eng.synchronize()
    return np.concatenate([L0, L.cpu().numpy()], axis=1), np.concatenate([R0, R.cpu().numpy()], axis=1)


def _check(what, ref, n, run, want_ahead, chains=(1, 2, 3, 0), env=None, counts=None):
    """run(engine) -> L, R for engines of every chain in `chains` with the switch on and off.
    On: taps and outputs against the oracle (ref = oracle_run's [L, R, A, B, C]), pre_ahead()
    == want_ahead on the full chain and 0 on the taps.  Off: the same bits, the same
    launches(), pre_ahead() == 0.  counts(c): further assertions on the full chain's launches()."""
    tap = {c: (i, name) for c, i, name in TAPS}
    for chain in chains:
        got = {}
        for ahead in (True, False):
            eng = _organ(n, chain, ahead, env)
            L, R = run(eng)
            got[ahead] = (L, R, eng.launches(), eng.pre_ahead())
            eng.close()
        L, R, c, na = got[True]
        print(f"{what} chain {chain}: launches {c}, ahead {na} (off: {got[False][3]})")
        if chain == 0:
            assert_bits(L, ref[0], f"{what} ahead L")
            assert_bits(R, ref[1], f"{what} ahead R")
        else:
            assert_bits(L, ref[tap[chain][0]], f"{what} ahead {tap[chain][1]} tap")
        assert_bits(got[False][0], L, f"{what} chain {chain} switch off against on, L")
        assert_bits(got[False][1], R, f"{what} chain {chain} switch off against on, R")
        assert got[False][2] == c, (what, chain, got[False][2], c)
        assert got[False][3] == 0, (what, chain, got[False][3])
        assert na == (want_ahead if chain == 0 else 0), (what, chain, na, want_ahead)
        assert c["k_whirl_split"] == 0 and (c["k_whirl"] > 0) == (chain == 0), (what, chain, c)
        if chain == 0 and counts:
            counts(c)


def test_gpu_pre_ahead_partial_workgroups(oracle):
    """37 instances with neighbouring scripts that differ (events at blocks 32..56, silent
    instances, reverb-heavy ones): the default shape's workgroups hold 28 + 9 instances, the
    ahead shape's 24 + 13, k_rv_post's 16 + 16 + 5.  One call of 320 blocks with the events:
    its first chunk has deltas, the next two upload the control it ended with, the fourth
    runs as before and holds its k_whirl back, the fifth runs ahead."""
    n, nb = 37, 320

    def scen(i):
        if i in (2, 33):
            return []
        return S.event_scenario(i) if i % 2 else S.bench_scenario(i)
    scens = [scen(i) for i in range(n)]
    ref = _oracle(oracle, n, _after(scens), PRE + nb)

    def run(eng):
        ev = _script_events(eng, [[(b, k, a, v) for (b, k, a, v) in sc if b] for sc in scens])
        return _one_call(eng, n, scens, nb, ev)

    def counts(c):  # the preamble and five 64-block chunks
        assert c["k_rv_core"] == 1 and c["k_rv_core_lds"] == 3 + 5 and c["k_whirl"] == 4 + 5, c
    _check("partial workgroups", ref, n, run, 1, counts=counts)
    assert float(np.abs(ref[0][1]).max()) > 1e-3 and float(np.abs(ref[0][3]).max()) > 1e-3


def test_gpu_pre_ahead_197_blocks_one_call(oracle):
    """One call of 197 blocks: chunks of 64, 64, 64 and 5.  The second and third run ahead,
    the last takes k_rv_core and runs as before, behind the third chunk's held-back k_whirl;
    the predelay history (delayM samples back) crosses every chunk boundary."""
    n, nb = 5, 197
    scens = [S.bench_scenario(i) for i in range(n)]
    ref = _oracle(oracle, n, scens, PRE + nb)

    def counts(c):
        assert c["k_rv_core"] == 1 + 1 and c["k_rv_core_lds"] == 3 + 3 and c["k_whirl"] == 4 + 4, c
    _check("197 blocks", ref, n, lambda eng: _one_call(eng, n, scens, nb), 2, counts=counts)


def test_gpu_pre_ahead_calls_back_to_back(oracle):
    """Two calls of 130 blocks back to back on one caller stream, a third on another, no host
    synchronisation between the first two: each call's held-back k_whirl is issued at the
    call's end (its last chunk, 2 blocks, follows the one that ran ahead), the outputs are
    complete where the caller's stream continues, and a call's first chunk never runs ahead
    (one ahead launch per call)."""
    n, nb = 5, 130
    scens = [S.bench_scenario(i) for i in range(n)]
    ref = _oracle(oracle, n, scens, PRE + 3 * nb)

    def run(eng):
        import torch
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        L0, R0 = _preamble(eng, scens)
        L = torch.zeros((n, 3 * nb * 128), dtype=torch.float32, device="cuda")
        R = torch.zeros_like(L)
        torch.cuda.synchronize()
        for c, st in enumerate((s1, s1, s2)):
            if c == 2:  # the caller orders its own streams (the tap chains render on them)
                s2.wait_stream(s1)
            eng.render_device(nb, L[:, c * nb * 128:].data_ptr(), R[:, c * nb * 128:].data_ptr(), 3 * nb * 128,
                              st.cuda_stream)
        with torch.cuda.stream(s1):
            h1 = [x[:, :2 * nb * 128].to("cpu", non_blocking=True) for x in (L, R)]
        with torch.cuda.stream(s2):
            h2 = [x[:, 2 * nb * 128:].to("cpu", non_blocking=True) for x in (L, R)]
        s1.synchronize()
        s2.synchronize()
        return (np.concatenate([L0, h1[0].numpy(), h2[0].numpy()], axis=1),
                np.concatenate([R0, h1[1].numpy(), h2[1].numpy()], axis=1))

    def counts(c):
        assert c["k_rv_core"] == 1 + 3 and c["k_rv_core_lds"] == 3 + 6 and c["k_whirl"] == 4 + 9, c
    _check("three calls", ref, n, run, 3, counts=counts)


def test_gpu_pre_ahead_events_between_steady_chunks(oracle):
    """One call of 458 blocks with events at its blocks 70 and 140 (chord and drawbar change
    and rotary fast -> slow; note-offs, percussion off and swell): chunk 0 has no deltas and
    holds its k_whirl back, which then goes out in front of a delta chunk; chunks 1 and 2 have
    deltas, chunks 3 and 4 upload the control they ended with, chunk 5 runs as before, chunks
    6 and 7 (10 blocks) run ahead."""
    n, nb = 6, 7 * 64 + 10

    def scen(i):
        c0, c1 = S.chord_for(i), S.chord_for(i + 5)
        ev = S.bench_scenario(i) + [(0, "param", S.P_DRUM, 2), (0, "param", S.P_HORN, 2)]
        ev += [(70, "note", k, 0) for k in c0[:2]] + [(70, "note", k, 1) for k in c1[:3]]
        ev += [(70, "param", S.P_DRAWBAR + 3, 6), (70, "param", S.P_DRUM, 1), (70, "param", S.P_HORN, 1)]
        ev += [(140, "note", k, 0) for k in set(c0[2:] + c1[:3])]
        ev += [(140, "param", S.P_PERC, 0), (140, "param", S.P_SWELL, 0.5), (140, "note", 60 + (i % 7), 1)]
        return ev
    scens = [scen(i) for i in range(n)]
    ref = _oracle(oracle, n, _after(scens), PRE + nb)

    def run(eng):
        ev = _script_events(eng, [[e for e in sc if e[0]] for sc in scens])
        return _one_call(eng, n, scens, nb, ev)

    def counts(c):
        assert c["k_rv_core"] == 1 and c["k_rv_core_lds"] == 3 + 8 and c["k_whirl"] == 4 + 8, c
    _check("events at 70 and 140", ref, n, run, 2, counts=counts)


def test_gpu_pre_ahead_set_steady_chunk_between_calls(oracle):
    """tbf_set_steady_chunk 64 -> 128 between a call of 130 blocks and one of 260: the second
    call's chunks are 128, 128 and 4 blocks, so the stage buffers are reallocated right after
    a call that held a launch back.  One chunk runs ahead in each call."""
    n, nb1, nb2 = 5, 130, 260
    scens = [S.bench_scenario(i) for i in range(n)]
    ref = _oracle(oracle, n, scens, PRE + nb1 + nb2)

    def run(eng):
        import torch
        L0, R0 = _preamble(eng, scens)
        L = torch.zeros((n, (nb1 + nb2) * 128), dtype=torch.float32, device="cuda")
        R = torch.zeros_like(L)
        eng.render_device(nb1, L.data_ptr(), R.data_ptr(), (nb1 + nb2) * 128)
        assert eng.set_steady_chunk(128) == 128
        eng.render_device(nb2, L[:, nb1 * 128:].data_ptr(), R[:, nb1 * 128:].data_ptr(), (nb1 + nb2) * 128)
        eng.synchronize()
        return np.concatenate([L0, L.cpu().numpy()], axis=1), np.concatenate([R0, R.cpu().numpy()], axis=1)

    def counts(c):
        assert c["k_rv_core"] == 1 + 2 and c["k_rv_core_lds"] == 3 + 4 and c["k_whirl"] == 4 + 6, c
    _check("set_steady_chunk", ref, n, run, 2, counts=counts)


_SHORT = {}


@pytest.mark.parametrize("chain,env", [(1, {}), (2, {}), (3, {}), (0, {"TBF_PIPELINE": "0"}),
                                       (0, {"TBF_PIPE_GROUPS": "0,0,1,1,2,2"}), (0, {"TBF_RV_LDS": "0"})],
                         ids=["tonegen", "preamp", "reverb_tap", "no_pipeline", "other_groups", "no_rv_lds"])
def test_gpu_pre_ahead_keeps_other_paths(oracle, chain, env):
    """Chain modes that end before k_whirl, TBF_PIPELINE=0, stage groups other than the
    default and TBF_RV_LDS=0 (every chunk takes k_rv_core) keep their schedule: 197 blocks in
    one call give the oracle's bits, and the same bits, launches() and no ahead launch with
    the switch on and off."""
    n, nb = 5, 197
    scens = [S.bench_scenario(i) for i in range(n)]
    if "ref" not in _SHORT:
        _SHORT["ref"] = _oracle(oracle, n, scens, PRE + nb)
    _check(f"chain {chain} {env}", _SHORT["ref"], n, lambda eng: _one_call(eng, n, scens, nb), 0,
           chains=(chain,), env=env)
