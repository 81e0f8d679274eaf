"""CPU tests of tbf_instances_remove on host-only engines (device = -1: the control plane
alone, no GPU), compared through tbf_debug_control and the per-block core programs
(tbf_debug_step, and tbf_debug_render_program: the step a render makes) as test_state_cpu does.

  - the survivors of a removal equal, block by block, the instances of a twin engine that
    held only them from the start: with the next block's events queued and not stepped, a
    retune pending and a programme with random drawbars installed;
  - nothing of a removed instance is left behind at the index it had;
  - an instance added after a removal is a fresh one, a clone of a renumbered survivor
    equals it, and a blob saved before the removal loads into the survivor's new index;
  - the refusals change nothing; n = 0, remove all, add again, the table-shaping cfg keys.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import scenarios as S

T = pytest.importorskip("tunebfree_amd")

H = 24         # the removal lands here: blocks [0, H) stepped, block H's events queued
NB = H + 16    # blocks compared after it
PGM = '5 { name="any bars", drawbars=random }\n'
PC_RANDOM = 4  # program change 4 -> programme 5 (offset 1)
U32P = C.POINTER(C.c_uint32)


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
    """registration and chord, a programme with random drawbars (instance 4: twice, so its
    control rand() stream matters after the removal too), a rotor change, drawbar moves, a
    release one block before the removal, a new chord queued at it (instance 2: and a retune),
    then a percussion retrigger, a vibrato change and a swell"""
    ev = S.bench_scenario(i)
    ev += [(3, "param", S.P_DRUM, 2), (3, "param", S.P_HORN, 2), (4, "param", S.P_DRAWBAR + 3, 6)]
    ev += [(10, "note", 72 + i % 5, 1), (10, "param", S.P_DRAWBAR + 4, 5)]
    if i % 7 == 4:
        ev += [(2, "program", PC_RANDOM, 0), (H + 5, "program", PC_RANDOM, 0)]
    ev += [(H - 1, "note", k, 0) for k in S.chord_for(i)]
    if i % 7 in (2, 3):
        ev += [(H, "retune", 1, 0)]
    ev += [(H, "note", k, 1) for k in S.chord_for(i + 5)]
    ev += [(H, "param", S.P_REVERB, 0.2 + 0.05 * (i % 7)), (H, "param", S.P_DRAWBAR + 1, (3 + i) % 9)]
    ev += [(H + 2, "param", S.P_VIBRATO_TYPE, 2), (H + 3, "param", S.P_SWELL, 0.5),
           (H + 4, "note", S.chord_for(i + 5)[0], 0), (H + 9, "param", S.P_DRUM, 0), (H + 11, "note", 60 + i, 1)]
    return ev


def _apply(eng, i, script, b):
    for (blk, kind, a, v) in script:
        if blk != b:
            continue
        if kind == "note":
            eng.note(i, a, v)
        elif kind == "program":
            eng.program_install(i, a)
        elif kind == "retune":
            eng.retune(i, eng.tids[a])
        else:
            eng.set_param(i, a, v)


def _engine(ids):
    """a host-only engine whose instance k is organ ids[k]: seed and script by the organ's id"""
    eng = T.Engine(sample_rate=48000.0, device=-1)
    eng.tids = [eng.template(seed=7), eng.template(seed=8)]
    eng.program_parse(PGM)
    eng.add_instances([eng.tids[0]] * len(ids), [1000 + 17 * i for i in ids])
    return eng


def _history(eng, ids, lazy, upto=H):
    """the scripts' blocks [0, upto) stepped, and block upto's events queued, not stepped"""
    for b in range(upto + 1):
        for k, i in enumerate(ids):
            _apply(eng, k, _script(i), b)
        if b < upto:
            for k in range(len(ids)):
                _prog(eng, k, lazy)


def _state(eng, lazy=None):
    """every instance's control vector (and, with lazy given, a stepped program)"""
    n = eng.n_instances
    out = [_ctl(eng, k) for k in range(n)]
    if lazy is not None:
        out += [_prog(eng, k, lazy) for k in range(n)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _continue_equal(a, ids_a, b, ids_b, lazy, what, b0=H, b1=NB):
    """blocks [b0, b1): engine a's instance k is organ ids_a[k], b's likewise (block b0's
    events are queued already); every organ the two engines share is compared, control vector
    before the step and program of the step"""
    shared = [(ids_a.index(i), ids_b.index(i)) for i in ids_a if i in ids_b]
    assert shared
    for blk in range(b0, b1):
        if blk > b0:
            for eng, ids in ((a, ids_a), (b, ids_b)):
                for k, i in enumerate(ids):
                    _apply(eng, k, _script(i), blk)
        for ka, kb in shared:
            assert np.array_equal(_ctl(a, ka), _ctl(b, kb)), (what, blk, ka, kb)
        pa = [_prog(a, k, lazy) for k in range(len(ids_a))]
        pb = [_prog(b, k, lazy) for k in range(len(ids_b))]
        for ka, kb in shared:
            assert np.array_equal(pa[ka].view(np.uint32), pb[kb].view(np.uint32)), (what, blk, ka, kb)


# ------------------------------------------------------------------ 1. survivors equal a twin
@pytest.mark.parametrize("lazy", [False, True])
def test_survivors_equal_a_twin(lazy):
    ids, gone = list(range(7)), [0, 3, 6]
    keep = [i for i in ids if i not in gone]
    a, b = _engine(ids), _engine(keep)
    _history(a, ids, lazy)
    _history(b, keep, lazy)
    m = a.remove(gone)
    assert m.dtype == np.int64 and m.tolist() == [-1, 0, 1, -1, 2, 3, -1]
    assert a.n_instances == 4
    _continue_equal(a, keep, b, keep, lazy, "survivors")
    # the organs differ from each other, so a row that landed in another's place would show
    assert not np.array_equal(_ctl(a, 0), _ctl(a, 1)) and not np.array_equal(_ctl(a, 2), _ctl(a, 3))
    a.close()
    b.close()


# ------------------------------------------------------------------ 2. removed state does not leak
@pytest.mark.parametrize("lazy", [False, True])
def test_removed_state_does_not_leak(lazy):
    """Organ 3 (a retune and a chord pending at block H) is removed: organ 4 now sits at index
    3, plays its own program on its own template, and nothing of organ 3's is stepped."""
    ids, keep = [0, 1, 2, 3, 4], [0, 1, 2, 4]
    a, b = _engine(ids), _engine(keep)
    _history(a, ids, lazy)
    _history(b, keep, lazy)
    gone_ctl = _ctl(a, 3)
    assert a.remove(3).tolist() == [0, 1, 2, -1, 3]
    assert not np.array_equal(_ctl(a, 3), gone_ctl)
    with pytest.raises(T.TbfError, match="tbf error -22"):
        a.note(4, 60, 1)                               # the old last index is gone
    _continue_equal(a, keep, b, keep, lazy, "no leak")
    a.close()
    b.close()


# ------------------------------------------------------------------ 3. remove, then add and clone
@pytest.mark.parametrize("lazy", [False, True])
def test_remove_then_add_and_clone(lazy):
    ids = [0, 1, 2, 3, 4]
    a = _engine(ids)
    _history(a, ids, lazy)
    assert a.remove([1, 4]).tolist() == [0, -1, 1, 2, -1]
    # a new organ 9 from time zero, against a fresh engine that holds only it
    assert a.add_instances([a.tids[0]], [1000 + 17 * 9]) == 3
    f = _engine([9])
    for blk in range(6):
        _apply(a, 3, _script(9), blk)
        _apply(f, 0, _script(9), blk)
        assert np.array_equal(_ctl(a, 3), _ctl(f, 0)), blk
        assert np.array_equal(_prog(a, 3, lazy).view(np.uint32), _prog(f, 0, lazy).view(np.uint32)), blk
    # a clone of renumbered survivor organ 2 (index 1, a retune pending) equals its source,
    # and both equal the twin
    assert a.clone(1) == 4 and a.n_instances == 5
    assert np.array_equal(_ctl(a, 4), _ctl(a, 1))
    b = _engine([0, 2, 3])
    _history(b, [0, 2, 3], lazy)
    # (a's instances 3 and 4 are stepped along by _continue_equal with scripts of their own:
    # organ 9's is past its events, the clone takes organ 2's)
    ids_a = [0, 2, 3, 90, 2]
    for blk in range(H, NB):
        if blk > H:
            for k, i in enumerate(ids_a):
                if i != 90:
                    _apply(a, k, _script(i), blk)
            for k, i in enumerate([0, 2, 3]):
                _apply(b, k, _script(i), blk)
        pa = [_prog(a, k, lazy) for k in range(5)]
        pb = [_prog(b, k, lazy) for k in range(3)]
        for ka, kb in ((0, 0), (1, 1), (2, 2), (4, 1)):
            assert np.array_equal(pa[ka].view(np.uint32), pb[kb].view(np.uint32)), (blk, ka, kb)
            assert np.array_equal(_ctl(a, ka), _ctl(b, kb)), (blk, ka, kb)
    for e in (a, b, f):
        e.close()


# ------------------------------------------------------------------ 4. save, remove, load
@pytest.mark.parametrize("lazy", [False, True])
def test_save_remove_load_rewinds_into_the_new_index(lazy):
    ids, keep = [0, 1, 2, 3], [1, 3]
    a, b = _engine(ids), _engine(keep)
    _history(a, ids, lazy)
    _history(b, keep, lazy)
    blob = a.save([3, 1])
    assert a.remove([0, 2]).tolist() == [-1, 0, -1, 1]
    for blk in range(H, H + 5):                        # the survivors run on, away from the blob
        for k in range(2):
            _apply(a, k, _script(5 + k), blk)
            _prog(a, k, lazy)
    assert not np.array_equal(_ctl(a, 1), _ctl(b, 1))
    a.load([1, 0], blob)                               # organ 3 -> index 1, organ 1 -> index 0
    _continue_equal(a, keep, b, keep, lazy, "rewind after a removal")
    a.close()
    b.close()


# ------------------------------------------------------------------ 5. refusals and edges
def test_refusals_change_nothing():
    lib = _lib()
    ids = [0, 1, 2]
    a, b = _engine(ids), _engine(ids)
    _history(a, ids, True, upto=6)
    _history(b, ids, True, upto=6)
    before = _state(a)
    blob = a.save(ids)
    m = np.full(3, 77, np.uint32)
    for what, lst in (("unknown", [0, 3]), ("duplicate", [1, 2, 1])):
        arr = np.array(lst, np.uint32)
        assert lib.tbf_instances_remove(a._h, len(arr), arr.ctypes.data_as(U32P), m.ctypes.data_as(U32P)) == -22, what
        with pytest.raises(T.TbfError, match="tbf error -22"):
            a.remove(lst)
    assert lib.tbf_instances_remove(a._h, 2, None, m.ctypes.data_as(U32P)) == -22
    assert lib.tbf_instances_remove(None, 0, None, None) == -22
    assert (m == 77).all() and a.n_instances == 3
    assert _same(_state(a), before) and np.array_equal(a.save(ids), blob)
    # n == 0: the identity map (NULL list allowed), nothing changed; new_index may be NULL
    assert a.remove([]).tolist() == [0, 1, 2]
    assert lib.tbf_instances_remove(a._h, 0, None, None) == 0
    one = np.array([1], np.uint32)
    assert _same(_state(a), before) and np.array_equal(a.save(ids), blob)
    _continue_equal(a, ids, b, ids, True, "after the refusals", b0=6, b1=12)
    assert lib.tbf_instances_remove(a._h, 1, one.ctypes.data_as(U32P), None) == 0 and a.n_instances == 2
    a.close()
    b.close()


@pytest.mark.parametrize("lazy", [False, True])
def test_remove_all_then_add(lazy):
    ids = [0, 1, 2]
    a = _engine(ids)
    _history(a, ids, lazy, upto=6)
    assert a.remove([2, 0, 1]).tolist() == [-1, -1, -1]   # any order
    assert a.n_instances == 0 and a.remove([]).tolist() == []
    with pytest.raises(T.TbfError, match="tbf error -22"):
        a.remove(0)
    with pytest.raises(T.TbfError, match="tbf error -22"):
        a.note(0, 60, 1)
    # removal does not reopen the table-shaping keys
    for key, v in (("whirl.horn.radius", 25), ("scanner.hz", 6.5)):
        with pytest.raises(T.TbfError, match="tbf error -16"):
            a.config_set(key, v)
    # templates are untouched and their ids stay valid: a new organ on the second one
    assert a.add_instances([a.tids[1]], [1000 + 17 * 5]) == 0 and a.n_instances == 1
    f = T.Engine(sample_rate=48000.0, device=-1)
    f.tids = [f.template(seed=7), f.template(seed=8)]
    f.program_parse(PGM)
    f.add_instances([f.tids[1]], [1000 + 17 * 5])
    for blk in range(8):
        _apply(a, 0, _script(5), blk)
        _apply(f, 0, _script(5), blk)
        assert np.array_equal(_ctl(a, 0), _ctl(f, 0)), blk
        assert np.array_equal(_prog(a, 0, lazy).view(np.uint32), _prog(f, 0, lazy).view(np.uint32)), blk
    a.close()
    f.close()


def test_device_bytes_of_a_host_engine_are_zero():
    a = _engine([0, 1])
    assert a.device_bytes() == (0, 0)
    a.remove(0)
    assert a.device_bytes() == (0, 0)
    a.close()


# ------------------------------------------------------------------ 6. source pins
def test_abi_pins():
    hdr = (Path(T.__file__).resolve().parent.parent / "include" / "tbf.h").read_text()
    assert re.search(r"^#define TBF_ABI_VERSION 1$", hdr, re.M)
    assert T.load_library().tbf_abi_version() == 1
    assert re.search(r"^int tbf_instances_remove \(tbf_engine\* e, uint32_t n, const uint32_t\* inst, "
                     r"uint32_t\* new_index\);$", hdr, re.M)
    assert re.search(r"^int tbf_debug_device_bytes \(const tbf_engine\* e, uint64_t\* instance_bytes, "
                     r"uint64_t\* stage_bytes\);$", hdr, re.M)
    res, args = T.engine.SIGNATURES["tbf_instances_remove"]
    assert res is C.c_int and len(args) == 4
    assert callable(T.Engine.remove) and callable(T.Engine.device_bytes)
    assert hasattr(T.load_library(), "tbf_debug_device_bytes")
