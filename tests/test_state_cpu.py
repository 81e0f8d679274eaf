"""CPU tests of tbf_instances_clone / tbf_instances_save / tbf_instances_load on host-only
engines (device = -1: the control plane alone, no GPU).

  - a clone's control state (tbf_debug_control) and per-block core programs (tbf_debug_step,
    and tbf_debug_render_program: the step a render makes) equal its source's block by block
    under a script, from a fork in the middle of it with key messages still queued; with
    other events it equals an engine that replays the source's history and then those events;
  - save -> load into a second host-only engine gives the same;
  - a blob cut at every word of its header and directory and at seeded random lengths, a cut
    blob whose stated size is patched to the cut, every header and directory word altered, and
    a device engine's header are all refused with -22 and leave the engine unchanged;
  - the size query (blob = NULL) reports the size the real call then fills exactly.
"""
import ctypes as C

import numpy as np
import pytest

import scenarios as S

T = pytest.importorskip("tunebfree_amd")

NB = 14        # blocks of the script
FORK = 7       # the fork lands here: keys released at block 6, new ones queued at 7


def _lib():
    lib = T.load_library()
    lib.tbf_debug_control.restype = C.c_int
    lib.tbf_debug_control.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    for f in (lib.tbf_debug_step, lib.tbf_debug_render_program):
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    return lib


def _ctl(eng, i):
    out = np.zeros(64, np.float64)
    n = _lib().tbf_debug_control(eng._h, i, out.ctypes.data, 64)
    assert n == 57
    return out[:n]


def _prog(eng, i, lazy):
    fn = _lib().tbf_debug_render_program if lazy else _lib().tbf_debug_step
    buf = np.zeros(9 * 600, np.float32)
    n = fn(eng._h, i, buf.ctypes.data, 600)
    assert n >= 0, T.load_library().tbf_last_error()
    return buf[: 9 * n].reshape(n, 9).copy()


def _script(i):
    """registration, chord, a rotor change, a drawbar move, the chord's release one block
    before the fork and a new chord queued at it, then a percussion retrigger and a swell"""
    ev = S.bench_scenario(i)
    ev += [(3, "param", S.P_DRUM, 2), (3, "param", S.P_HORN, 2), (4, "param", S.P_DRAWBAR + 3, 6)]
    ev += [(FORK - 1, "note", k, 0) for k in S.chord_for(i)]
    ev += [(FORK, "note", k, 1) for k in S.chord_for(i + 5)]
    ev += [(FORK + 2, "param", S.P_VIBRATO_TYPE, 2), (FORK + 3, "param", S.P_SWELL, 0.5),
           (FORK + 4, "note", S.chord_for(i + 5)[0], 0)]
    return ev


def _other(i):
    """a different continuation from the fork on"""
    return [(FORK, "note", 60 + i, 1), (FORK, "param", S.P_REVERB, 0.6), (FORK + 1, "param", S.P_DRAWBAR, 2),
            (FORK + 2, "param", S.P_CHARACTER, 0.9), (FORK + 3, "note", 60 + i, 0)]


def _apply(eng, i, script, b):
    for (blk, kind, a, v) in script:
        if blk != b:
            continue
        if kind == "note":
            eng.note(i, a, v)
        else:
            eng.set_param(i, a, v)


def _engine(n, sr=48000.0, chain=0, tpl_seed=7):
    eng = T.Engine(sample_rate=sr, device=-1, chain=chain)
    tid = eng.template(seed=tpl_seed)
    eng.add_instances([tid] * n, [1000 + 17 * i for i in range(n)])
    return eng


def _history(eng, n, lazy, upto=FORK):
    """the script's blocks [0, upto) stepped, and block upto's events queued, not stepped"""
    for b in range(upto + 1):
        for i in range(n):
            _apply(eng, i, _script(i), b)
        if b < upto:
            for i in range(n):
                _prog(eng, i, lazy)


def _continue_equal(eng, pairs, scripts, lazy, what):
    """from the fork on: instance b of each (a, b) gets scripts[b]; where a is an engine
    index pair ((ea, ia), (eb, ib)) the two rows' control and programs are compared"""
    for b in range(FORK, NB):
        for (e, i), sc in scripts.items():
            if b > FORK:  # block FORK's events were queued before the fork
                _apply(e, i, sc, b)
        for (ea, ia), (eb, ib) in pairs:
            assert np.array_equal(_ctl(ea, ia), _ctl(eb, ib)), (what, b, ia, ib)
        progs = {k: _prog(k[0], k[1], lazy) for k in scripts}
        for ka, kb in pairs:
            assert np.array_equal(progs[ka].view(np.uint32), progs[kb].view(np.uint32)), (what, b, ka[1], kb[1])


@pytest.mark.parametrize("lazy", [False, True])
def test_clone_equals_source_and_replay(lazy):
    n = 2
    eng = _engine(n)
    _history(eng, n, lazy)
    assert eng.clone([0, 1, 1]) == n and eng.n_instances == 5
    # a replay engine: instance 0 = instance 1's seed, history, then the other continuation
    rep = T.Engine(sample_rate=48000.0, device=-1)
    rep.add_instances([rep.template(seed=7)], [1000 + 17])
    for b in range(FORK + 1):
        _apply(rep, 0, _script(1), b)
        if b < FORK:
            _prog(rep, 0, lazy)
    for ev in _other(1):
        if ev[0] == FORK:
            _apply(eng, 3, [ev], FORK)
            _apply(rep, 0, [ev], FORK)
    scripts = {(eng, 0): _script(0), (eng, 1): _script(1), (eng, 2): _script(0), (eng, 4): _script(1),
               (eng, 3): _other(1), (rep, 0): _other(1)}
    pairs = [((eng, 0), (eng, 2)), ((eng, 1), (eng, 4)), ((rep, 0), (eng, 3))]
    _continue_equal(eng, pairs, scripts, lazy, "clone")
    assert not np.array_equal(_ctl(eng, 1), _ctl(eng, 3))
    eng.close()
    rep.close()


def test_clone_before_first_step_and_refusals():
    eng = _engine(2)
    _apply(eng, 1, _script(1), 0)  # pending notes and parameters, nothing stepped
    assert eng.clone(1) == 2
    assert np.array_equal(_ctl(eng, 1), _ctl(eng, 2))
    for _ in range(3):
        assert np.array_equal(_prog(eng, 1, False), _prog(eng, 2, False))
    with pytest.raises(T.TbfError, match="tbf error -22"):
        eng.clone([0, 3])  # 3 does not exist yet
    assert eng.n_instances == 3
    assert eng.clone([]) == 3 and eng.n_instances == 3
    eng.close()


@pytest.mark.parametrize("lazy", [False, True])
def test_save_load_into_second_engine(lazy):
    n = 3
    a = _engine(n)
    _history(a, n, lazy)
    blob = a.save([2, 0])
    b = _engine(4)
    for i in range(4):  # something else happened on b
        _apply(b, i, S.event_scenario(i), 0)
        _prog(b, i, lazy)
    before = _ctl(b, 2)
    b.load([1, 3], blob)
    assert np.array_equal(_ctl(b, 2), before)
    scripts = {(a, 2): _script(2), (a, 0): _script(0), (b, 1): _script(2), (b, 3): _script(0)}
    _continue_equal(a, [((a, 2), (b, 1)), ((a, 0), (b, 3))], scripts, lazy, "save/load")
    a.close()
    b.close()


def test_size_query_and_capacity():
    lib = _lib()
    eng = _engine(2)
    _history(eng, 2, False, upto=3)
    inst = np.array([1, 0, 1], np.uint32)
    size = C.c_uint64()
    u32p = C.POINTER(C.c_uint32)
    assert lib.tbf_instances_save(eng._h, 3, inst.ctypes.data_as(u32p), None, 0, C.byref(size)) == 0
    want = size.value
    assert want > 0
    buf = np.full(want + 64, 0xA5, np.uint8)
    size.value = 0
    assert lib.tbf_instances_save(eng._h, 3, inst.ctypes.data_as(u32p), buf.ctypes.data, want, C.byref(size)) == 0
    assert size.value == want
    assert (buf[want:] == 0xA5).all()  # filled exactly: nothing written past the size
    assert lib.tbf_instances_save(eng._h, 3, inst.ctypes.data_as(u32p), buf.ctypes.data, want - 1, C.byref(size)) == -22
    # the blob loads back where it came from (repeats in the saved list are fine, not in the target)
    eng2 = _engine(3)
    eng2.load([2, 0, 1], buf[:want])
    with pytest.raises(T.TbfError, match="tbf error -22.*twice"):
        eng2.load([2, 0, 2], buf[:want])
    eng.close()
    eng2.close()


def _refused(eng, inst, blob, what):
    with pytest.raises(T.TbfError, match="tbf error -22") as ei:
        eng.load(inst, blob)
    return str(ei.value)


def test_bad_blobs_are_refused_and_change_nothing():
    a = _engine(2)
    _history(a, 2, False)
    blob = a.save([0, 1])
    b = _engine(3)
    _history(b, 3, False, upto=2)
    state0 = b.save([0, 1, 2])
    hdr = int(blob[8:12].view(np.uint32)[0])       # the header's own size field
    head = hdr + 2 * 32                            # header + one 32-byte directory entry per record
    assert hdr % 8 == 0 and head < len(blob)
    rng = np.random.default_rng(20240611)
    cuts = list(range(0, head + 1, 4)) + [int(x) for x in rng.integers(head, len(blob), 5)] + [len(blob) - 1]
    for cut in cuts:
        _refused(b, [0, 2], blob[:cut], f"cut at {cut}")
    # a cut blob whose header states the cut size: the interior lengths are checked too
    for cut in [int(x) for x in rng.integers(head, len(blob), 5)]:
        c = blob[:cut].copy()
        c[hdr - 8:hdr].view(np.uint64)[0] = cut    # the header's last field: the total size
        _refused(b, [0, 2], c, f"cut at {cut}, size patched")
    # every word of the header and the directory altered
    for w in range(0, head, 4):
        c = blob.copy()
        c[w:w + 4].view(np.uint32)[0] ^= 0x00010001
        _refused(b, [0, 2], c, f"word at {w}")
    # wrong n, and an instance that does not exist
    _refused(b, [0], blob, "n = 1")
    _refused(b, [0, 1, 2], blob, "n = 3")
    _refused(b, [0, 3], blob, "instance 3")
    # other sample rate, other chain, other template at the same id, other cfg tables
    for kw, cfg, word in (({"sr": 96000.0}, None, "sample rate"), ({"chain": T.engine.CHAIN_FX}, None, "chain"),
                          ({"tpl_seed": 8}, None, "template"), ({}, {"scanner.hz": 6.5}, "fingerprint"),
                          ({}, S.CFG_SETS["geometry_wide"], "wringLen")):
        if cfg is None:
            o = _engine(2, **kw)
        else:
            o = T.Engine(sample_rate=48000.0, device=-1)
            o.config(cfg)
            o.add_instances([o.template(seed=7)] * 2, [1, 2])
        msg = _refused(o, [0, 1], blob, word)
        assert word in msg, (word, msg)
        o.close()
    # a device engine's blob: the same header with the device flag set
    words = blob[:hdr].view(np.uint32)
    flagged = [w for w in range(hdr // 4) if words[w] == 0]
    c = blob.copy()
    msg = None
    for w in flagged:  # one of the zero words is the device flag: find it by the message
        c = blob.copy()
        c[4 * w:4 * w + 4].view(np.uint32)[0] = 1
        m = _refused(b, [0, 2], c, "device flag")
        if "host-only" in m:
            msg = m
    assert msg is not None
    # nothing of all that changed the engine
    assert np.array_equal(b.save([0, 1, 2]), state0)
    b.load([0, 2], blob)  # and the blob itself is good
    assert not np.array_equal(b.save([0, 1, 2]), state0)
    a.close()
    b.close()
