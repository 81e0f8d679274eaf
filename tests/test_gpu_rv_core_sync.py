"""k_rv_core_lds orders the read and write phases of its groups of eleven 64-sample sub-blocks by
per-wave counters in LDS (readDone, writeDone, planDone) instead of workgroup barriers: a worker
waits for the reads of the two sub-blocks before its own before it writes, and for the writes up
to its own sub-block of the group before, and the plan, before it reads.

Every test is bit for bit (assert_bits) on the reverb tap (chain 3) and on L / R (chain 0),
against the CPU oracle or, where said, an engine on the streaming kernel (TBF_RV_LDS=0).  One
oracle run (5 instances, 1 + 64 blocks) serves every test: block 0 carries the scripts' events
(k_rv_core), then the calls under test follow, each of >= 8 blocks and so one k_rv_core_lds launch
of 2 x blocks sub-blocks:
  - 8, 11, 12, 17 blocks: 16 = 11 + 5 sub-blocks (six workers only publish), 22 = 2 x 11,
    24 = 22 + 2, 34 = 33 + 1 (worker 0 alone; its waits wrap to workers 10 and 9 of the group before);
  - 64 blocks: 11 groups + 7 sub-blocks, every ring wraps at least four times;
  - 8 + 9 + 11 blocks as three calls against one of 28: the state between launches;
  - TBF_RV_PERSIST=2 with 5 instances: five pairs in a row per workgroup, the counters start again;
  - forced serial replays: the planner's sub-block walk under the handshakes;
  - 64 instances x 64 blocks against TBF_RV_LDS=0, GPU against GPU: a race net without oracle cost.
In every test the engine's path flags have PATH_RV_SYNC clear: no wait gave up.
"""
import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits, engine_run, oracle_run
from test_gpu_parity import TAPS, _engine

pytestmark = pytest.mark.gpu

REVERB_TAP = next(idx for chain, idx, _ in TAPS if chain == 3)
LONG = 64  # blocks after block 0 in the shared oracle run


def _seeds(n):
    return [1000 + 17 * i for i in range(n)]


def _registration(i, reverb):
    """the bench registration and instance i's chord with another reverb mix"""
    return [(0, k, a, v) for (k, a, v) in S.jazz1_params(reverb=reverb)] + [(0, "note", k, 1) for k in S.chord_for(i)]


# the bench scenario, a silent instance, reverb 0.7; then two more for the five-instance test
SCENS = [S.bench_scenario(0), [], _registration(2, 0.7), S.bench_scenario(3), _registration(4, 1.0)]
_REF = {}


def _ref(oracle, n, nblocks):
    """rows [:n] and blocks [:1 + nblocks] of the one oracle run: (reverb tap, L, R)"""
    if not _REF:
        from orc_bind import Template
        _REF["ref"] = oracle_run(oracle, Template(oracle, seed=7), _seeds(len(SCENS)), SCENS, 1 + LONG)
        for r in _REF["ref"]:
            r.setflags(write=False)
    k = (1 + nblocks) * 128
    r = _REF["ref"]
    return r[REVERB_TAP][:n, :k], r[0][:n, :k], r[1][:n, :k]


def _render(n, chain, calls, env=None, debug_flags=0, scens=None):
    """an engine of n instances: block 0, then one render call per entry of calls; every call took
    k_rv_core_lds once (or k_rv_core with TBF_RV_LDS=0) and no wait of it gave up"""
    import tunebfree_amd as T
    eng = _engine(chain, debug_flags=debug_flags, env=env)
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, _seeds(n))
    parts = [engine_run(eng, (scens or SCENS)[:n], 1)] + [eng.render(k) for k in calls]
    c, flags = eng.launches(), eng.error_flags()
    eng.close()
    lds = (env or {}).get("TBF_RV_LDS") != "0"
    want = (1, len(calls)) if lds else (1 + len(calls), 0)
    assert (c["k_rv_core"], c["k_rv_core_lds"]) == want, (env, calls, c)
    assert not flags & T.engine.PATH_RV_SYNC, hex(flags)
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1), flags


def _against_oracle(what, oracle, n, calls, **kw):
    tap, oL, oR = _ref(oracle, n, sum(calls))
    L, _, f3 = _render(n, 3, calls, **kw)
    assert_bits(L, tap, f"{what}: reverb tap")
    L, R, f0 = _render(n, 0, calls, **kw)
    assert_bits(L, oL, f"{what}: L")
    assert_bits(R, oR, f"{what}: R")
    return L, R, f3, f0


@pytest.mark.parametrize("nb", [8, 11, 12, 17])
def test_gpu_rv_core_sync_group_boundaries(oracle, nb):
    """One launch of 16, 22, 24 and 34 sub-blocks: a partial group of 5, none, one of 2 and one of 1."""
    _against_oracle(f"{nb} blocks", oracle, 3, [nb])
    assert float(np.abs(_ref(oracle, 3, nb)[0]).max()) > 1e-4


def test_gpu_rv_core_sync_ring_wraps(oracle):
    """One 64-block launch: 11 full groups and 7 sub-blocks, 8192 samples through rings of at most
    1928 slots, so every ring wraps at least four times and every mirror slot is written."""
    _against_oracle("64 blocks", oracle, 3, [64])


def test_gpu_rv_core_sync_state_between_launches(oracle):
    """8 + 9 + 11 blocks as three calls and as one call of 28, both against the oracle."""
    a = _against_oracle("8 + 9 + 11 blocks", oracle, 3, [8, 9, 11])
    b = _against_oracle("28 blocks", oracle, 3, [28])
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_gpu_rv_core_sync_pairs_in_a_row(oracle):
    """TBF_RV_PERSIST=2, 5 instances, 12 blocks: each of the two workgroups runs five pairs in a
    row, every pair on counters that start again; the default grid gives the same bits."""
    a = _against_oracle("two workgroups", oracle, 5, [12], env={"TBF_RV_PERSIST": "2"})
    b = _against_oracle("default grid", oracle, 5, [12])
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_gpu_rv_core_sync_forced_serial(oracle):
    """TBF_DEBUG_FORCE_SERIAL, 12 blocks: the planner walks every group sub-block by sub-block while
    the workers wait for its plan.  The path flags are the forced-serial ones, without PATH_RV_SYNC."""
    import tunebfree_amd as T
    _, _, f3, f0 = _against_oracle("forced serial", oracle, 3, [12], debug_flags=T.engine.DEBUG_FORCE_SERIAL)
    assert f3 & T.engine.PATH_RV_PHASE, hex(f3)
    want = T.engine.PATH_WH_ANGLE | T.engine.PATH_WH_MOTION | T.engine.PATH_RV_PHASE
    assert f0 & want == want, hex(f0)


def test_gpu_rv_core_sync_against_streaming_kernel():
    """64 instances x 64 blocks on the reverb tap: 128 workgroups of k_rv_core_lds at once against
    an engine that runs k_rv_core (TBF_RV_LDS=0), GPU against GPU."""
    n = 64
    scens = [[] if i % 3 == 1 else _registration(i, S.SWEEP_REVERB[(i // 3) % 3]) if i % 3 == 2 else S.bench_scenario(i)
             for i in range(n)]
    a, _, _ = _render(n, 3, [64], scens=scens)
    b, _, _ = _render(n, 3, [64], scens=scens, env={"TBF_RV_LDS": "0"})
    assert_bits(a, b, "k_rv_core_lds against k_rv_core: reverb tap")
    assert float(np.abs(b).max()) > 1e-4
