"""k_rv_post's wave roles: one serial wave runs both biquads (lanes 0-31 the biquadB chains
of tile it - 1, lanes 32-63 the biquadC chains of tile it - 3), one wave the dither streams,
and the helper waves take the workgroup's 16 instance tasks by a table, one or two a wave.

Every test is bit for bit against the CPU oracle (enginerun.oracle_run, assert_bits) on the
reverb tap (chain 3) and on L / R of the full chain (chain 0):
  - partial workgroups: last workgroups of 1 and 15 instances, so both halves of the serial
    wave have lanes without a chain and helper tasks fall past the workgroup's instances;
  - launches of 1 block (4 tiles: the halves' active windows overlap in two iterations) and
    the same blocks as 1 + 2 + 5 calls and as one call (the biquads' and the dither streams'
    state goes through memory between launches);
  - reverb mix 0.0, 0.7, 1.0 (no dry path) and the bench's 0.1;
  - one launch of more than 64 blocks (blocks past lane 63's control entry);
  - the k_rv_pre ahead shape (TBF_PRE_AHEAD=1) beside the workgroup.
"""
import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits, engine_run, oracle_run
from test_gpu_parity import TAPS, _engine

pytestmark = pytest.mark.gpu

REVERB_TAP = next(idx for chain, idx, _ in TAPS if chain == 3)


def _seeds(n):
    return [1000 + 17 * i for i in range(n)]


def _organ(n, chain, env=None):
    eng = _engine(chain, env=env)
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, _seeds(n))
    return eng


def _oracle(oracle, scens, nblocks):
    from orc_bind import Template
    return oracle_run(oracle, Template(oracle, seed=7), _seeds(len(scens)), scens, nblocks)


def _registration(i, reverb):
    """the bench registration and instance i's chord with another reverb mix"""
    return [(0, k, a, v) for (k, a, v) in S.jazz1_params(reverb=reverb)] + [(0, "note", k, 1) for k in S.chord_for(i)]


def _against_oracle(what, ref, run, n, env=None):
    """run(engine) -> L, R through engines of chain 3 and 0: the reverb tap and L / R"""
    eng = _organ(n, 3, env)
    L, _ = run(eng)
    eng.close()
    assert_bits(L, ref[REVERB_TAP], f"{what}: reverb tap")
    eng = _organ(n, 0, env)
    L, R = run(eng)
    eng.close()
    assert_bits(L, ref[0], f"{what}: L")
    assert_bits(R, ref[1], f"{what}: R")


def _mixed(i):
    """neighbours play different scripts, every third instance is silent"""
    if i % 3 == 1:
        return []
    if i % 3 == 2:
        return _registration(i, S.SWEEP_REVERB[(i // 3) % 3])
    return S.bench_scenario(i)


@pytest.mark.parametrize("n", [1, 15, 17, 33])
def test_gpu_rv_post_partial_workgroups(oracle, n):
    """Batches of 1, 15, 17 and 33 instances: last workgroups of 1, 15, 1 and 1."""
    nb = 6
    scens = [_mixed(i) for i in range(n)]
    ref = _oracle(oracle, scens, nb)
    _against_oracle(f"{n} instances", ref, lambda eng: engine_run(eng, scens, nb), n)
    assert float(np.abs(ref[REVERB_TAP]).max()) > 1e-4


_CARRIED = {}


def _carried_ref(oracle):
    if not _CARRIED:
        n = 3
        scens = [S.bench_scenario(0), [], _registration(2, 0.7)]
        _CARRIED["n"], _CARRIED["scens"] = n, scens
        _CARRIED["ref"] = _oracle(oracle, scens, 8)
    return _CARRIED["n"], _CARRIED["scens"], _CARRIED["ref"]


def test_gpu_rv_post_one_block_launch(oracle):
    """One call of 1 block: 4 tiles, 8 iterations, of which 4 have one half of the serial
    wave without a tile."""
    n, scens, ref = _carried_ref(oracle)
    _against_oracle("1 block", [r[:, :128] for r in ref], lambda eng: engine_run(eng, scens, 1), n)


@pytest.mark.parametrize("calls", [(1, 2, 5), (8,)], ids=["1+2+5", "8"])
def test_gpu_rv_post_state_carried_between_launches(oracle, calls):
    """8 blocks as calls of 1 + 2 + 5 blocks and as one call."""
    n, scens, ref = _carried_ref(oracle)

    def run(eng):
        Ls, Rs = zip(*([engine_run(eng, scens, calls[0])] + [eng.render(k) for k in calls[1:]]))
        return np.concatenate(Ls, axis=1), np.concatenate(Rs, axis=1)
    _against_oracle(f"calls of {calls} blocks", ref, run, n)


def test_gpu_rv_post_reverb_mix(oracle):
    """Reverb mix 0.0, 0.7, 1.0 (the branch without the dry path) and the bench's 0.1, as
    neighbours of one workgroup."""
    mixes = S.SWEEP_REVERB + (0.1,)
    n, nb = len(mixes), 6
    scens = [_registration(i, m) for i, m in enumerate(mixes)]
    ref = _oracle(oracle, scens, nb)
    _against_oracle("reverb mixes", ref, lambda eng: engine_run(eng, scens, nb), n)


PRE = 1 + 192  # block 0 with the events, then three 64-block chunks in which the controls settle


def _long(eng, scens, nb, want_launches):
    """the preamble, then one call of nb blocks; the call's reverb launches are counted"""
    L0, R0 = engine_run(eng, scens, 1)
    L1, R1 = eng.render(PRE - 1)
    before = eng.launches()
    L2, R2 = eng.render(nb)
    after = eng.launches()
    ran = sum(after[k] - before[k] for k in ("k_rv_core", "k_rv_core_lds"))
    assert ran == want_launches, (before, after)
    return np.concatenate([L0, L1, L2], axis=1), np.concatenate([R0, R1, R2], axis=1)


def test_gpu_rv_post_launch_of_more_than_64_blocks(oracle):
    """One launch of 80 blocks behind the preamble: the blocks past 63 read lane 63's wet level."""
    n, nb = 3, 80
    scens = [S.bench_scenario(0), _registration(1, 1.0), _registration(2, 0.7)]
    ref = _oracle(oracle, scens, PRE + nb)
    _against_oracle("80-block launch", ref, lambda eng: _long(eng, scens, nb, 1), n)


def test_gpu_rv_post_beside_the_ahead_shape(oracle):
    """TBF_PRE_AHEAD=1 with 64-block chunks: in a call of 192 blocks the second and third
    chunks' k_rv_pre run in the ahead shape beside the chunk before's k_rv_post."""
    n, nb = 5, 192
    env ={"TBF_PRE_AHEAD": "1", "TBF_WHIRL_SPLIT": "0", "TBF_STEADY_CHUNK": "64"}
    scens = [_mixed(i) for i in range(n)]
    ref = _oracle(oracle, scens, PRE + nb)
    eng = _organ(n, 3, env)
    L, _ = _long(eng, scens, nb, 3)
    eng.close()
    assert_bits(L, ref[REVERB_TAP], "ahead shape: reverb tap")
    eng = _organ(n, 0, env)
    L, R = _long(eng, scens, nb, 3)
    ahead = eng.pre_ahead()
    eng.close()
    assert_bits(L, ref[0], "ahead shape: L")
    assert_bits(R, ref[1], "ahead shape: R")
    assert ahead == 2, ahead
