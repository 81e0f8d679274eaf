"""k_whirl's launch-long register state (rotor angles and increments, ring position, filter
states and carries, horn A's run-ahead flags, the history rows' heads) against the CPU
oracle and the forced-serial render, bit for bit.

Small batches pick k_whirl_split by themselves, so every engine here is created under
TBF_WHIRL_SPLIT=0 (k_whirl, the kernel a full batch runs) unless a case asks for the other.
The state lives in registers between a launch's first and last block, so the cases put
launch edges, bypassed blocks, new parameter sets and rotor selections where that state is
loaded, written back or bypassed."""
import os

import pytest

import scenarios as S
from enginerun import assert_bits, oracle_run

pytestmark = pytest.mark.gpu

SAMPLE = (0, 3, 6, 11)  # instances compared with the oracle (both brake scripts of the scenario: i & 1)


def _render(scens, calls, rate=48000.0, dbg=0, split="0", steady=None):
    """Render the scripts as consecutive tbf_render_events calls [(first block, blocks)],
    each call carrying the events that land inside it."""
    import torch
    import tunebfree_amd as T
    n = len(scens)
    nb = calls[-1][0] + calls[-1][1]
    os.environ["TBF_WHIRL_SPLIT"] = split
    if steady is not None:
        os.environ["TBF_STEADY_CHUNK"] = steady
    try:
        eng = T.Engine(sample_rate=rate, device=0, debug_flags=dbg)
    finally:
        os.environ.pop("TBF_WHIRL_SPLIT", None)
        os.environ.pop("TBF_STEADY_CHUNK", None)
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
    eng.close()
    return out


def _same(a, b, what):
    for ch in (0, 1):
        assert_bits(a[ch], b[ch], f"{what}: {'LR'[ch]}")


def _oracle(oracle, scens, nb, rate=48000.0):
    from orc_bind import Template
    tpl = Template(oracle, sr=rate, seed=7)
    oL, oR, *_ = oracle_run(oracle, tpl, [6300 + i for i in SAMPLE], [scens[i] for i in SAMPLE], nb)
    return oL, oR


def _vs_oracle(out, ref, what):
    _same((out[0][list(SAMPLE)], out[1][list(SAMPLE)]), ref, what)


def _c(b, name, v):
    return (b, "control", name, v)


def _bypass(on, off):
    return [(on, "param", S.P_WHIRL_BYPASS, 1), (off, "param", S.P_WHIRL_BYPASS, 0)]


# ---------------------------------------------------------------- 1. launch edges
EDGE_CALLS = []
for _k in (1, 2, 3, 63, 64, 65, 150):
    EDGE_CALLS.append((sum(k for _, k in EDGE_CALLS), _k))
EDGE_NB = EDGE_CALLS[-1][0] + EDGE_CALLS[-1][1]  # 348


def _edge_scens(n):
    """The whirl-control script (its events on blocks 3..6 land on the 1-, 2- and 3-block
    calls' edges) and, later, events on both sides of the long calls' edges: a parameter set
    on a call's last and first block, a bypass over an edge, rotor selections at an edge."""
    scens = []
    for i in range(n):
        e = S.whirl_control_scenario(i)
        e += [_c(68, "whirl.horn.filter.a.hz", 30 + i), _c(69, "whirl.horn.filter.b.hz", 90 - i)]
        e += [(70, "param", S.P_HORN, 2), (70, "param", S.P_DRUM, 2)]
        e += _bypass(132, 134) if i % 3 == 0 else _bypass(133, 135)
        e += [_c(197, "whirl.horn.filter.a.q", 40 + i), _c(198, "whirl.horn.brakepos", 10 + 7 * i)]
        e += [(198, "param", S.P_HORN, 0), (198, "param", S.P_DRUM, 0), (260, "param", S.P_HORN, 1), (261, "param", S.P_DRUM, 1)]
        e += _bypass(340, 344)
        scens.append(sorted(e, key=lambda r: r[0]))
    return scens


def test_gpu_whirl_launch_edges(oracle):
    """One stream as calls of 1, 2, 3, 63, 64, 65 and 150 blocks, as one call, and as one
    call in 64-block chunks: the three equal, and equal to the oracle and the forced-serial
    render.  Every launch edge writes the register state back and reads it again (the
    st.adx layout included) and restarts horn A's run-ahead."""
    n = 12
    scens = _edge_scens(n)
    split = _render(scens, EDGE_CALLS)
    one = _render(scens, [(0, EDGE_NB)])
    s64 = _render(scens, [(0, EDGE_NB)], steady="64")
    ser = _render(scens, [(0, EDGE_NB)], dbg=1)
    _same(split, one, "calls of 1, 2, 3, 63, 64, 65, 150 blocks vs one call")
    _same(s64, one, "64-block chunks vs one call")
    _same(ser, one, "forced serial vs one call")
    _vs_oracle(one, _oracle(oracle, scens, EDGE_NB), "one call vs oracle")


# ---------------------------------------------------------------- 2. run-ahead breakers
BRK_CALLS = [(0, 20), (20, 20), (40, 24), (64, 8)]
BRK_NB = 72


def _breaker_scens(n):
    """On the whirl-control script (rotor stop 6, fast 9, stop 26 with brake positions set,
    slow 48, stop 60): a bypass on and off on consecutive blocks and on a call's last block,
    a horn-filter change on a call's first, second and last block, and a rotor selection on
    every block of the last call.  A brake position is non-zero from block 2 on."""
    scens = []
    for i in range(n):
        e = S.whirl_control_scenario(i)
        e += [_c(2, "whirl.horn.brakepos", 64 + i), _c(2, "whirl.drum.brakepos", 32 + i)]
        e += _bypass(10, 11) + _bypass(12, 13) + _bypass(14, 16)
        e += _bypass(19, 20) if i & 1 else _bypass(19, 21)       # on a call's last block
        e += [_c(20, "whirl.horn.filter.a.hz", 20 + 3 * i),      # a call's first block
              _c(21, "whirl.horn.filter.b.q", 30 + 2 * i),       # its second
              _c(39, "whirl.horn.filter.a.gain", 50 + i),        # its last
              _c(63, "whirl.horn.filter.b.hz", 70 + i)]          # the next call's last
        e += _bypass(39, 40) if i % 3 == 0 else []
        for k in range(8):
            e += [(64 + k, "param", S.P_HORN, (2, 1, 0, 2, 0, 1, 2, 0)[(k + i) % 8]),
                  (64 + k, "param", S.P_DRUM, (1, 2, 2, 0, 1, 0, 0, 2)[(k + i) % 8])]
        scens.append(sorted(e, key=lambda r: r[0]))
    return scens


@pytest.fixture(scope="module")
def breaker_render():
    scens = _breaker_scens(16)
    return scens, _render(scens, BRK_CALLS)


def test_gpu_whirl_run_ahead_breakers(oracle, breaker_render):
    scens, out = breaker_render
    _same(_render(scens, BRK_CALLS, dbg=1), out, "forced serial vs fast paths")
    _same(_render(scens, [(0, BRK_NB)]), out, "one call vs four")
    _vs_oracle(out, _oracle(oracle, scens, BRK_NB), "k_whirl vs oracle")


def test_gpu_whirl_split_equals_k_whirl_on_breakers(breaker_render):
    """k_whirl_split shares k_whirl's helpers (motion_pass, the serial filter passes)."""
    scens, out = breaker_render
    _same(_render(scens, BRK_CALLS, split="1"), out, "k_whirl_split vs k_whirl")
    _same(_render(scens, BRK_CALLS, split="1", dbg=1), out, "k_whirl_split forced serial vs k_whirl")


# ---------------------------------------------------------------- 3. rotor at fast speed
_fast_scens = S.fast_scens  # shared with test_gpu_rates.py and test_oracle_cpu.py


@pytest.mark.parametrize("rate", [48000.0, 44100.0, 96000.0])
def test_gpu_whirl_fast_rotor(oracle, rate):
    """48 kHz and 44.1 kHz (write-ahead 79) run k_whirl<512>, 96 kHz k_whirl<1024>; 150
    blocks hold two horn turns at the first two rates, 300 at 96 kHz."""
    n, nb = 12, 300 if rate > 48000.0 else 150
    scens = _fast_scens(n)
    out = _render(scens, [(0, 64), (64, nb - 64)], rate=rate)
    _same(_render(scens, [(0, nb)], rate=rate, dbg=1), out, f"forced serial vs fast paths at {rate:g} Hz")
    _vs_oracle(out, _oracle(oracle, scens, nb, rate), f"k_whirl vs oracle at {rate:g} Hz")
