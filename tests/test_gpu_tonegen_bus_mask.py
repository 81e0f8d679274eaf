"""k_tonegen's live-bus mask: the interpreter leaves out the buses that no
entry of the block's program feeds (all of the entries' gains for the bus are zero) or
that the block's routing does not read, and gives a skipped bus the zero, sign included,
that the full loop would have summed.

Every case renders a script through engines of chain 1 (tonegen only), 2, 3 and 0 and
compares the three stage taps and the outputs bit for bit with the oracle
(test_gpu_parity._all_taps, enginerun.assert_bits).  The batches are small (3-6
instances), so a call without control deltas of 8 blocks or more splits each instance's
blocks into ranges (k_tonegen_ranges: the warm-up block goes through the same variant);
TBF_TG_SPLIT=0 runs one range.

The masks a registration reaches are taken from the host control plane's programs
(tbf_debug_render_program on a host-only engine) and asserted, so a case keeps testing
the mask its name says.  Bit 0 is the swell bus, bit 1 percussion, bit 2 vibrato.

Programs of more than TG_PCAP = 128 entries (the loop that keeps all three buses) come
from key clusters released and pressed again: released wheels stay in the program, up to
147 entries here, and 129 remain when the last cluster is held
(test_gpu_bus_mask_programs_past_tg_pcap).  Keys that are only held stop at 102 entries
(all 27 drawbars out, keys on all three manuals: test_gpu_bus_mask_long_programs).

What the control plane cannot reach: a gain of -0.f or NaN (the gains are products and
sums of non-negative tapers and drawbar levels).  An idle bus whose
samples are negative for a whole block: the shortest program that leaves a routed bus
idle (one pedal or lower-manual key, the crosstalk models off) still has 7 entries up to
wheel 37 (about 262 Hz), whose half period is 91 samples; such programs give runs of
samples where every entry is negative between runs of mixed signs, which is what
test_gpu_bus_mask_zero_rule plays.
"""
import ctypes as C

import numpy as np
import pytest

import scenarios as S
from enginerun import assert_bits, engine_run, oracle_run
from test_gpu_parity import _all_taps, _organ, _script_events, _setup

pytestmark = pytest.mark.gpu

SW, PC, VB = 1, 2, 4
PARAMS = [(0, k, a, v) for (k, a, v) in S.jazz1_params()]  # Jazz 1: percussion on, vibrato on the upper manual
LOWER, PEDAL = 128, 256  # key offsets of the lower manual and the pedals
NO_CROSSTALK = {"osc.compartment-crosstalk": 0, "osc.transformer-crosstalk": 0, "osc.terminalstrip-crosstalk": 0,
                "osc.wiring-crosstalk": 0}


def _keys(keys, block=0, on=1):
    return [(block, "note", k, on) for k in keys]


def _gain_masks(scen, nblocks, cfg=None):
    """Per block of one instance playing `scen` on the host control plane: (entries,
    envelope entries, the mask of the buses some entry feeds -- by the gains alone --, the
    mask after the gate of the block's routing word: what the kernel computes)."""
    import tunebfree_amd as T
    lib = T.load_library()
    lib.tbf_debug_render_program.restype = C.c_int
    lib.tbf_debug_render_program.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.tbf_debug_control.restype = C.c_int
    lib.tbf_debug_control.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    eng = T.Engine(device=-1)
    for k, v in (cfg or {}).items():
        eng.config_set(k, v)
    eng.add_instances([eng.template(seed=7)], [1000])
    buf, ctl, out = np.zeros(9 * 600, np.float32), np.zeros(64, np.float64), []
    for b in range(nblocks):
        for (bb, kind, a, v) in scen:
            if bb == b:
                eng.note(0, a, v) if kind == "note" else eng.set_param(0, a, v)
        n = lib.tbf_debug_render_program(eng._h, 0, buf.ctypes.data, 600)
        assert n >= 0
        bits = buf[:9 * n].view(np.uint32).reshape(n, 9)
        env = buf[:9 * n].reshape(n, 9)[:, 1] != 0
        m = 0
        for bit, col in ((SW, 3), (PC, 4), (VB, 5)):
            if (((bits[:, col] << 1) != 0) | (env & ((bits[:, col + 3] << 1) != 0))).any():
                m |= bit
        # the routing word the block's control carries (a routing event takes effect on its
        # own block; the held wheels' sums follow on the next one)
        assert lib.tbf_debug_control(eng._h, 0, ctl.ctypes.data, 64) > 7
        routing = int(ctl[7])
        gated = m & ~((0 if routing & 0x0C else PC) | (0 if routing & 0x03 else VB))
        out.append((n, int(env.sum()), m, gated))
    eng.close()
    return out


def _play(what, oracle, scen_fn, n, nb, tail=0, env=None, cfg=None, one_call=False, check=None):
    """n instances play scen_fn(i) for nb blocks (a render per stretch between events, or
    one tbf_render_events call), then `tail` blocks in a call of their own (no control
    deltas: block ranges): every tap and the outputs against the oracle."""
    eng, tpl, seeds, scens = _setup(oracle, n, scen_fn, chain=1, cfg=cfg, env=env)
    ref = oracle_run(oracle, tpl, seeds, scens, nb + tail)

    def run(e):
        if one_call:
            import torch
            L = torch.zeros((n, nb * 128), dtype=torch.float32, device="cuda")
            R = torch.zeros_like(L)
            e.render_events_device(nb, _script_events(e, scens), L.data_ptr(), R.data_ptr(), nb * 128)
            e.synchronize()
            L, R = L.cpu().numpy(), R.cpu().numpy()
        else:
            L, R = engine_run(e, scens, nb)
        if tail:
            L2, R2 = e.render(tail)
            L, R = np.concatenate([L, L2], axis=1), np.concatenate([R, R2], axis=1)
        return L, R
    c = _all_taps(what, "small", ref, lambda chain: eng if chain == 1 else _organ(n, chain=chain, cfg=cfg, env=env),
                  run, check=check)
    print(f"{what}: launches {c}")
    return ref, c


# name: (events after Jazz 1's parameters, the program's mask).  A registration set before
# the keys go down never has a gain on a bus its routing leaves out, so the routing gate
# changes nothing here; a switch thrown while keys are held does
# (test_gpu_bus_mask_changes_inside_a_call).
REGISTRATIONS = {
    "jazz1_swell_idle": ([], PC | VB),  # the bench
    "vibrato_off_upper_only": ([(0, "param", S.P_VIBRATO, 0)], SW | PC),
    "percussion_off_lower_key": ([(0, "param", S.P_PERC, 0)] + _keys([LOWER + 40]), SW | VB),
    "lower_key_all_live": (_keys([LOWER + 40]), SW | PC | VB),
    "pedal_key_all_live": (_keys([PEDAL + 30]), SW | PC | VB),
    "percussion_off_vibrato_only": ([(0, "param", S.P_PERC, 0)], VB),
    "vibrato_and_percussion_off_swell_only": ([(0, "param", S.P_VIBRATO, 0), (0, "param", S.P_PERC, 0)], SW),
}


@pytest.mark.parametrize("name", list(REGISTRATIONS))
def test_gpu_bus_mask_registrations(oracle, name):
    """One registration per mask the control plane reaches, three chords each: 4 blocks from
    creation (the attack's envelope entries, then plain ones), then a call of 8 blocks
    without deltas, which runs as two block ranges."""
    extra, mask = REGISTRATIONS[name]

    def scen(i):
        return PARAMS + _keys(S.chord_for(5 * i)) + extra
    progs = _gain_masks(scen(0), 3)
    assert progs[0][1] == progs[0][0] > 0 and progs[2][1] == 0, progs  # attack entries, then none
    assert [p[2:] for p in progs] == [(mask, mask)] * 3, (name, progs)  # by the gains, and after the routing gate
    _, c = _play(name, oracle, scen, 3, 4, tail=8)
    assert c["k_tonegen_ranges"] > 0, c


@pytest.mark.parametrize("name", ["jazz1_swell_idle", "percussion_off_lower_key"])
def test_gpu_bus_mask_one_block_range(oracle, name):
    """TBF_TG_SPLIT=0: every call's blocks in one range per instance."""
    extra = REGISTRATIONS[name][0]
    _, c = _play(name + " TBF_TG_SPLIT=0", oracle, lambda i: PARAMS + _keys(S.chord_for(5 * i)) + extra, 3, 4, tail=8,
                 env={"TBF_TG_SPLIT": "0"})
    assert c["k_tonegen_ranges"] == 0, c


def _changing(i):
    """the mask and the routing change on different blocks, differently per instance"""
    o = i % 3
    return (PARAMS + _keys(S.chord_for(i)) +
            [(2 + o, "param", S.P_VIBRATO, 0), (4 + o, "param", S.P_PERC, 0), (5, "param", S.P_VIBRATO, 1)] +
            _keys([LOWER + 36 + i], 6 + o) + [(8, "param", S.P_PERC, 1), (9 + o, "param", S.P_VIB_LOWER, 1)] +
            _keys([LOWER + 36 + i], 10, 0) + [(11, "param", S.P_VIBRATO, 0)])


def test_gpu_bus_mask_changes_inside_a_call(oracle):
    """One tbf_render_events call (a chunk with control deltas: the per-block prologue forms
    the mask under that block's routing): the vibrato routing flips, percussion goes off
    and on, a lower-manual key comes and goes and the lower manual joins the vibrato, on
    blocks that differ between the instances.  On the block of a switch the routing word
    has changed and the held wheels still carry the old sums: the entries have vibrato gains
    with the scanner routed out (block 2 of instance 0), and percussion gains with the
    percussion routed out (block 4), so the mask is what the routing gate leaves."""
    progs = _gain_masks(_changing(0), 12)
    assert len({p[3] for p in progs}) >= 4, progs  # the script walks through four masks or more
    assert progs[2][2:] == (PC | VB, PC) and progs[4][2:] == (SW | PC, SW), progs  # gated by the routing
    _play("masks change in a call", oracle, _changing, 4, 12, one_call=True)
    _play("masks change between calls", oracle, _changing, 4, 12)


def _pressed_and_released(i):
    c = S.chord_for(i)
    return (PARAMS + ([(0, "param", S.P_PERC, 0)] if i % 2 else []) + _keys(c) + _keys(c[:2], 3, 0) + _keys(c[2:], 5 + i % 2, 0) +
            _keys([c[0] + 2], 5) + _keys([c[0] + 2, c[1] + 1], 8) + _keys([c[0] + 2], 9, 0))


def test_gpu_bus_mask_envelope_entries(oracle):
    """Keys pressed and released so that attack and release entries (their next gains count
    for the mask) stand beside plain ones with the swell bus idle, and with the percussion
    bus idle too on the odd instances; blocks whose program has envelope entries alternate
    with blocks that have none (on instance 0 anyEnv turns false after blocks 0, 3, 5 and
    9), in one call and as a render per stretch."""
    progs = _gain_masks(_pressed_and_released(0), 12)
    mixed = [p for p in progs if 0 < p[1] < p[0]]
    assert mixed and any(p[1] == 0 and p[0] > 0 for p in progs), progs
    assert all(not (p[2] & SW) for p in progs), progs
    _play("envelopes in a call", oracle, _pressed_and_released, 4, 12, one_call=True)
    _play("envelopes between calls", oracle, _pressed_and_released, 4, 12)


def _zero_rule(i):
    """0: no key down, ever (np == 0: every bus +0).  1: a pedal key alone (8 entries, all
    on the swell bus: the percussion and vibrato buses are routed and idle, and see every
    sign pattern of a few low wheels).  2: a low upper key (the swell bus idle under 9
    entries).  3: no key for two blocks, then a pedal key.
    4, 5: every upper drawbar pushed in, vibrato and percussion off, one key held (54 / 60:
    the wheels start in phase, and these keys' first samples with every entry negative come
    in blocks 2 to 4): a program whose entries all have zero gains, so the tonegen tap is the
    skipped swell bus itself times the gains -- the zero's sign sample by sample, with
    nothing added that could hide it.  (Wherever the scanner or a live bus adds to a skipped
    one the sum swallows the zero's sign: -0 + v is v, and the scanner's ring never holds
    -0.  A build that gave every skipped bus +0.f failed this case alone.)"""
    bars = [(0, "param", S.P_BUS_DRAWBAR + 18, 8)]
    mute = [(0, "param", S.P_DRAWBAR + j, 0) for j in range(9)] + [(0, "param", S.P_VIBRATO, 0), (0, "param", S.P_PERC, 0)]
    return [[], PARAMS + bars + _keys([PEDAL]), PARAMS + _keys([36]),
            PARAMS + bars + _keys([PEDAL + 2], 2), PARAMS + mute + _keys([54]), PARAMS + mute + _keys([60])][i]


def test_gpu_bus_mask_zero_rule(oracle):
    """The value of a skipped bus is -0.f where every entry's sample is negative and +0.f
    otherwise (and +0.f without a program).  Crosstalk models off: the shortest programs.
    The oracle's tonegen tap of the muted instances has both zeros, so the case compares
    what it is about."""
    p = _gain_masks(_zero_rule(1), 3, NO_CROSSTALK)
    assert 0 < p[2][0] <= 9 and p[2][2] == SW, p
    assert _gain_masks(_zero_rule(2), 3, NO_CROSSTALK)[2][2] == (PC | VB)
    for i in (4, 5):
        p = _gain_masks(_zero_rule(i), 3, NO_CROSSTALK)
        assert p[2][0] > 0 and p[2][2] == 0, p
    ref, _ = _play("zero rule", oracle, _zero_rule, 6, 4, tail=8, cfg=NO_CROSSTALK)
    for i in (4, 5):  # both zeros, in the calls with events and in the block ranges' call
        tap = ref[2][i].view(np.uint32)
        assert set(np.unique(tap)) == {0, 0x80000000}, (i, np.unique(tap))
        assert (tap[:4 * 128] != 0).any() and (tap[4 * 128:] != 0).any(), i
    assert not ref[2][0].view(np.uint32).any()
    _play("zero rule, blocks one by one", oracle, lambda i: _zero_rule(i) + [(b, "param", S.P_REVERB, 0.1) for b in range(12)],
          6, 12, cfg=NO_CROSSTALK)


def _full_organ(i):
    bars = [(0, "param", S.P_BUS_DRAWBAR + j, 8) for j in range(27)]
    if i == 0:  # every wheel sounding: 102 entries, all buses live
        return (PARAMS + bars + _keys(range(0, 61, 2)) + _keys(range(LOWER + 1, LOWER + 61, 2)) +
                _keys(range(PEDAL, PEDAL + 25, 3)))
    if i == 1:  # the upper manual alone, all drawbars: the swell bus idle over more than 64 entries
        return PARAMS + bars + _keys(range(0, 61, 3))
    return S.bench_scenario(i)  # a plain one


def test_gpu_bus_mask_long_programs(oracle):
    """The longest program the control plane makes (102 entries: the prologue's second pass
    and 25 groups of four and a remainder in the loop) with all buses live, a program past
    64 entries with the swell bus idle, and the bench's."""
    p0, p1 = _gain_masks(_full_organ(0), 3), _gain_masks(_full_organ(1), 3)
    assert p0[2][0] > 96 and p0[2][2] == (SW | PC | VB), p0
    assert p1[2][0] > 64 and p1[2][2] == (PC | VB), p1
    _play("long programs", oracle, _full_organ, 3, 4, tail=8)


def _cluster(i, t):
    base = 36 + (3 * i + 5 * t) % 40
    return [base + 2 * k for k in range(12)]


def _clusters(i):
    """Jazz 1, a 12-key cluster released and another pressed on every block up to block 6
    (test_gpu_device_control_large_clusters' clusters): the released wheels stay in the
    program, which grows past TG_PCAP.  Instances 0, 1: the last cluster is held (129
    entries from block 7 on, none with an envelope); 2: the same, 126 entries; 3: every key
    released on block 8 and a chord pressed on block 9 (back to a short program)."""
    i3 = i == 3
    ev, cur = PARAMS + _keys(_cluster(i, 0)), _cluster(i, 0)
    for b in range(1, 7):
        ev += _keys(cur, b, 0) + _keys(_cluster(i, b), b)
        cur = _cluster(i, b)
    if i3:
        ev += _keys(cur, 8, 0) + _keys(S.chord_for(i), 9)
    return ev


def test_gpu_bus_mask_programs_past_tg_pcap(oracle):
    """np passes TG_PCAP = 128 inside one tbf_render_events call and comes back (a delta
    chunk whose blocks switch between the swell-idle variant and the loop with all buses,
    which reads the entries from HBM), then a call without deltas starts while np is 129
    (no position cache, tc.on false: the per-block prologue in a steady chunk, two block
    ranges with a warm-up block) next to instances at 126 and below; the swell bus is idle
    throughout.  np and the mask are asserted from the host's programs."""
    progs = [_gain_masks(_clusters(i), 12) for i in range(4)]
    for i, p in enumerate(progs):
        assert p[0][0] <= 128 < max(q[0] for q in p) and all(q[3] == (PC | VB) for q in p if q[0]), (i, p)
    assert progs[0][11][:2] == (129, 0) and progs[1][11][:2] == (129, 0) and progs[2][11][:2] == (126, 0), progs
    assert progs[2][6][0] > 128 and progs[3][6][0] > 128 and 0 < progs[3][11][0] < 64, (progs[2], progs[3])
    _, c = _play("past TG_PCAP in a call", oracle, _clusters, 4, 12, tail=8, one_call=True)
    assert c["k_tonegen_ranges"] > 0, c
    _play("past TG_PCAP between calls", oracle, _clusters, 4, 12, tail=8, env={"TBF_TG_SPLIT": "0"})


def test_gpu_bus_mask_steady_and_delta_agree(oracle):
    """The registrations as one call without deltas (the mask formed once per launch, in
    tg_cache_load) and as calls of one block each: identical bits, and the oracle's."""
    regs = list(REGISTRATIONS.values())

    def scen(i):
        return PARAMS + _keys(S.chord_for(i)) + regs[i][0]
    n, nb = 6, 10
    eng, tpl, seeds, scens = _setup(oracle, n, scen)
    ref = oracle_run(oracle, tpl, seeds, scens, 2 + nb)
    outs = []
    for step in (nb, 1):
        e = eng if step == nb else _organ(n)
        parts = [engine_run(e, scens, 2)] + [e.render(step) for _ in range(nb // step)]
        outs.append([np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1)])
        e.close()
    assert_bits(outs[0][0], ref[0], "steady call L")
    assert_bits(outs[0][1], ref[1], "steady call R")
    assert_bits(outs[1][0], outs[0][0], "one-block calls against the steady call, L")
    assert_bits(outs[1][1], outs[0][1], "one-block calls against the steady call, R")
