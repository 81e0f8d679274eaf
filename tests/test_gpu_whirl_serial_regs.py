"""The serial DF2 pass of k_whirl and k_whirl_split fed from registers (one chain per DPP
row, its state in lanes 0, 16, 32, 48: wh_serial_regs) against the CPU oracle, bit for bit,
on L, R and the three stage taps.

Every case renders three instances: a plain one, one whose rotary is bypassed for some
blocks (horn A's run-ahead stops and restarts: the catch-up pass) and one that gets a new
horn-filter parameter set mid-render (the block before it has no next sub-block for horn A,
the block itself starts with horn A not ahead).  The render lengths put the launch's last
sub-block (no next: horn A's chain inactive), a second block, a bypass inside the launch and
a 65th block (past lane 63's control entry) into one call; the 1 + 1 + 2 + 3 calls send the
state of lanes 16 f through tbf_wh_state.fz in memory and back.

The engine chooses its whirl kernel when it is created and exports no state, so one stream
cannot alternate between the kernels: each is checked against the oracle over the same
calls instead, which pins what either leaves in memory after every call to the one layout.

Not reachable from inputs, checked by reading: horn A's NaN scrub
(finite inputs keep the states finite) and a wrapped drum window (the ring position advances
by whole sub-blocks from 0, so a window never wraps)."""
import os

import pytest

import scenarios as S
from enginerun import assert_bits, oracle_run

pytestmark = pytest.mark.gpu

N = 3
SEEDS = [7700 + i for i in range(N)]
TAPS = ((1, 2, "tonegen"), (2, 3, "preamp"), (3, 4, "reverb"))
LONG = {48000.0: 65, 96000.0: 5}  # the longest render at each rate: one oracle run serves every length


def _c(b, name, v):
    return (b, "control", name, v)


def _scens():
    plain = S.bench_scenario(0)
    byp = S.bench_scenario(5) + [(1, "param", S.P_WHIRL_BYPASS, 1), (3, "param", S.P_WHIRL_BYPASS, 0),
                                 (34, "param", S.P_WHIRL_BYPASS, 1), (36, "param", S.P_WHIRL_BYPASS, 0)]
    prm = S.bench_scenario(9) + [_c(2, "whirl.horn.filter.a.hz", 37), _c(4, "whirl.horn.filter.b.q", 41),
                                 _c(40, "whirl.horn.filter.a.gain", 55), _c(64, "whirl.horn.filter.b.hz", 83)]
    return [sorted(s, key=lambda r: r[0]) for s in (plain, byp, prm)]


SCENS = _scens()
_REFS = {}


def _ref(oracle, rate):
    """the oracle's [L, R, A, B, C] over the longest render at this rate, computed once and
    never modified; a shorter render is its prefix"""
    if rate not in _REFS:
        from orc_bind import Template
        _REFS[rate] = oracle_run(oracle, Template(oracle, sr=rate, seed=7), SEEDS, SCENS, LONG[rate])
        for a in _REFS[rate]:
            a.setflags(write=False)
    return _REFS[rate]


def _render(calls, rate, split, chain=0):
    """The scripts as consecutive render calls [(first block, blocks)], each carrying the
    events that land inside it; returns L, R and the engine's launch counts."""
    import torch
    import tunebfree_amd as T
    nb = calls[-1][0] + calls[-1][1]
    os.environ["TBF_WHIRL_SPLIT"] = split
    try:
        eng = T.Engine(sample_rate=rate, device=0, chain=chain)
    finally:
        os.environ.pop("TBF_WHIRL_SPLIT", None)
    tid = eng.template(seed=7)
    eng.add_instances([tid] * N, SEEDS)
    L = torch.zeros((N, nb * 128), dtype=torch.float32, device="cuda")
    R = torch.zeros_like(L)
    for (s, k) in calls:
        rows = []
        for i, sc in enumerate(SCENS):
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
    out = (L.cpu().numpy(), R.cpu().numpy(), eng.launches())
    eng.close()
    return out


def _check(oracle, calls, rate, split, what):
    """L, R and the three stage taps of the calls against the oracle; the whirl kernel that
    ran is the one the case names"""
    nb = calls[-1][0] + calls[-1][1]
    ref = [a[:, :nb * 128] for a in _ref(oracle, rate)]
    for chain, idx, tap in TAPS:
        L, _, _ = _render(calls, rate, split, chain)
        assert_bits(L, ref[idx], f"{what}: {tap} tap")
    L, R, c = _render(calls, rate, split)
    assert (c["k_whirl_split"] > 0) == (split == "1") and (c["k_whirl"] > 0) == (split == "0"), (split, c)
    assert_bits(L, ref[0], f"{what}: L")
    assert_bits(R, ref[1], f"{what}: R")
    return L, R


@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("nb", [1, 2, 5, 65])
def test_gpu_whirl_serial_regs_lengths(oracle, nb, split):
    _check(oracle, [(0, nb)], 48000.0, split, f"{nb} blocks in one call, TBF_WHIRL_SPLIT={split}")


@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_whirl_serial_regs_calls(oracle, split):
    """7 blocks as calls of 1 + 1 + 2 + 3 and as one call: equal, and equal to the oracle"""
    what = f"TBF_WHIRL_SPLIT={split}"
    a = _check(oracle, [(0, 1), (1, 1), (2, 2), (4, 3)], 48000.0, split, f"calls of 1 + 1 + 2 + 3 blocks, {what}")
    b = _check(oracle, [(0, 7)], 48000.0, split, f"7 blocks in one call, {what}")
    for ch in (0, 1):
        assert_bits(a[ch], b[ch], f"calls of 1 + 1 + 2 + 3 blocks vs one call, {what}: {'LR'[ch]}")


@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_whirl_serial_regs_96k(oracle, split):
    """5 blocks at 96 kHz: k_whirl<1024> and the split kernel at the 1024-sample ring"""
    _check(oracle, [(0, 5)], 96000.0, split, f"5 blocks at 96 kHz, TBF_WHIRL_SPLIT={split}")


def test_gpu_whirl_serial_regs_kernels_agree():
    """The two kernels over the same calls, call by call the same bits: each leaves, after
    every call, the state (tbf_wh_state.fz among it) that the other leaves."""
    calls = [(0, 1), (1, 1), (2, 2), (4, 3)]
    a = _render(calls, 48000.0, "0")
    b = _render(calls, 48000.0, "1")
    for ch in (0, 1):
        assert_bits(b[ch], a[ch], f"k_whirl_split vs k_whirl over calls of 1 + 1 + 2 + 3 blocks: {'LR'[ch]}")
