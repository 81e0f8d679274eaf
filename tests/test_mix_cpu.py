"""The mixdown stage without a GPU: the host restatement of the definition (tbf_debug_mix_ref,
built from the header k_mix is built from) against the float64 model within the bound of a
sequential fma sum, the order of the sum made observable, the literal cases of the definition,
the refusals of the mix calls on host-only engines and the pan helper."""
import ctypes as C

import numpy as np
import pytest

import mix_model as M

T = pytest.importorskip("tunebfree_amd")
E = T.engine

FULL, TONEGEN, FX = 0, 1, 4
NONE = M.NONE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def order_case(seed=5, members=9, frames=257):
    """the inputs the issue sets for the order test: randn * 10^uniform (-3, 0), random
    coefficients, one bus of nine members"""
    rng = np.random.default_rng(seed)
    L = (rng.standard_normal((members, frames)) * 10.0 ** rng.uniform(-3, 0, (members, frames))).astype(np.float32)
    R = (rng.standard_normal((members, frames)) * 10.0 ** rng.uniform(-3, 0, (members, frames))).astype(np.float32)
    c = rng.uniform(-1.5, 1.5, (4, members)).astype(np.float32)
    return L, R, M.rows_of([0] * members, *c)


def _engine(chain=FULL, n=2):
    eng = T.Engine(sample_rate=48000.0, device=-1, chain=chain)
    if n:
        tid = eng.template(seed=7)
        eng.add_instances([tid] * n, [100 + i for i in range(n)])
    return eng


def _err(eng):
    return eng._lib.tbf_last_error().decode()


# ---------------------------------------------------------------- 1. the restatement against float64
def test_constants_mirror_the_header():
    assert T.params.MIX_NONE == E.MIX_NONE == NONE == 0xFFFFFFFF
    assert C.sizeof(E.MixRow) == T.params.MIX_ROW_DTYPE.itemsize == M.ROW_DTYPE.itemsize == 20
    assert T.params.MIX_ROW_DTYPE == M.ROW_DTYPE and C.sizeof(E.MixOut) == 24
    assert [f[0] for f in E.MixRow._fields_] == list(M.ROW_DTYPE.names)


def test_order_is_observable():
    """the ascending sum and the sum over the rows reversed differ in at least one sample, so a
    kernel that sums in another order cannot equal the restatement in bits by accident"""
    L, R, rows = order_case()
    upL, upR = T.Engine.mix_ref(L, R, rows, 1)
    dnL, dnR = T.Engine.mix_ref(L[::-1], R[::-1], rows[::-1], 1)
    nl, nr = int((bits(upL) != bits(dnL)).sum()), int((bits(upR) != bits(dnR)).sum())
    print(f"samples that differ between the two orders: L {nl}, R {nr} of {upL.size}")
    assert nl >= 1 and nr >= 1


def test_ref_against_float64_within_the_fma_bound():
    """every sample of the restatement within gamma_m sum |c x| of the float64 value, m = 2 x the
    members that reach the sample, gamma_m = m u / (1 - m u), u = 2^-24: the bound of a
    sequential fma sum, derived, not measured.  Buses of 0, 1, 2, 9, 17 and 33 members,
    interleaved, rows in no bus, counts of 0, 1, partial and full."""
    rng = np.random.default_rng(21)
    sizes = [0, 1, 2, 9, 17, 33]
    bus = np.concatenate([[b] * k for b, k in enumerate(sizes)] + [[-1] * 8])
    rng.shuffle(bus)
    n, frames = len(bus), 301
    L = (rng.standard_normal((n, frames)) * 10.0 ** rng.uniform(-3, 0, (n, frames))).astype(np.float32)
    R = (rng.standard_normal((n, frames)) * 10.0 ** rng.uniform(-3, 0, (n, frames))).astype(np.float32)
    rows = M.rows_of(bus, *rng.uniform(-1.5, 1.5, (4, n)).astype(np.float32))
    counts = rng.integers(0, frames + 1, n).astype(np.uint32)
    counts[:4] = [0, 1, frames, frames - 1]
    worst = 0.0
    for cnt in (None, counts):
        gotL, gotR = T.Engine.mix_ref(L, R, rows, len(sizes), counts=cnt)
        L64, R64, magL, magR, mem = M.mix64(L, R, rows, len(sizes), cnt)
        if cnt is None:
            assert mem[:, 0].tolist() == sizes
        bound = M.gamma(2 * mem)
        for got, want, mag in ((gotL, L64, magL), (gotR, R64, magR)):
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound * mag).all(), float((err - bound * mag).max())
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(mag > 0, err / (bound * mag), 0.0))))
            assert not got[mem == 0].any() and not np.signbit(got[mem == 0]).any()
    print(f"largest error over its bound: {worst:.3f}")
    assert 0.0 < worst <= 1.0


# ---------------------------------------------------------------- 2. the literal cases
def test_empty_bus_and_unreached_frames_are_plus_zero():
    L = np.full((2, 6), -1.0, np.float32)
    rows = M.rows_of([1, NONE], [1.0] * 2, [0.0] * 2, [0.0] * 2, [1.0] * 2)
    oL, oR = T.Engine.mix_ref(L, L.copy(), rows, 3, counts=[4, 6])
    for o in (oL, oR):
        assert bits(o[0]).tolist() == [0] * 6 and bits(o[2]).tolist() == [0] * 6  # +0.0f: the sign bit too
        assert o[1, :4].tolist() == [-1.0] * 4 and bits(o[1, 4:]).tolist() == [0, 0]
    oL, oR = T.Engine.mix_ref(np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, M.ROW_DTYPE), 2)
    assert oL.shape == (2, 5) and bits(oL).sum() == 0 and bits(oR).sum() == 0


def test_a_member_of_count_zero_adds_no_term():
    """its NaN never shows, and the sum is in bits that of the other member alone"""
    L = np.array([[np.nan, np.nan, np.nan], [-0.0, 3.0, -2.5]], np.float32)
    rows = M.rows_of([0, 0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0])
    oL, oR = T.Engine.mix_ref(L, L, rows, 1, counts=[0, 3])
    alone, _ = T.Engine.mix_ref(L[1:], L[1:], rows[1:], 1)
    assert bits(oL).tolist() == bits(alone).tolist() and bits(oR).tolist() == bits(alone).tolist()
    assert oL[0].tolist() == [0.0, 3.0, -2.5]


def test_nan_shows_only_through_a_term():
    x = np.ones((3, 4), np.float32)
    x[0, :] = np.nan          # a row in no bus
    x[1, 2:] = np.nan         # beyond the row's count
    rows = M.rows_of([NONE, 0, 0], [1.0] * 3, [1.0] * 3, [1.0] * 3, [1.0] * 3)
    oL, oR = T.Engine.mix_ref(x, x.copy(), rows, 1, counts=[4, 2, 4])
    assert oL.tolist() == [[4.0, 4.0, 2.0, 2.0]] and oR.tolist() == oL.tolist()
    # a member with all-zero coefficients still contributes its terms: 0 * NaN and 0 * Inf are NaN
    y = np.ones((2, 3), np.float32)
    y[1] = [np.nan, np.inf, 5.0]
    rows = M.rows_of([0, 0], [1.0, 0.0], [0.0, 0.0], [0.0, 0.0], [1.0, 0.0])
    oL, oR = T.Engine.mix_ref(y, y.copy(), rows, 1)
    assert np.isnan(oL[0, :2]).all() and np.isnan(oR[0, :2]).all() and oL[0, 2] == 1.0 and oR[0, 2] == 1.0
    # Inf propagates literally, Inf - Inf is NaN, and the zero coefficient on an Inf is NaN too
    z = np.array([[np.inf, np.inf], [1.0, -np.inf]], np.float32)
    rows = M.rows_of([0, 0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0])
    oL, oR = T.Engine.mix_ref(z, np.ones_like(z), rows, 1)
    assert oL[0, 0] == np.inf and np.isnan(oL[0, 1]) and np.isnan(oR[0]).all()


def test_signed_zeros_and_denormals_go_through_fmaf():
    """the sums start from +0.0f, so a product of -0 gives +0 under round to nearest; a negative
    product that underflows gives -0, and only -0 terms keep it.  Denormal inputs, products and
    sums are kept, not flushed."""
    x = np.array([[-0.0, 0.0, -0.0]], np.float32)
    rows = M.rows_of([0], [1.0], [0.0], [-1.0], [0.0])
    oL, oR = T.Engine.mix_ref(x, x, rows, 1)
    assert bits(oL).tolist() == [[0, 0, 0]] and bits(oR).tolist() == [[0, 0, 0]]
    tiny = float(np.float32(2.0 ** -149))
    m = np.array([[-tiny, -tiny]], np.float32)
    p = np.array([[-tiny, tiny]], np.float32)
    rows = M.rows_of([0], [0.25], [0.0], [-1.0], [0.0])
    oL, oR = T.Engine.mix_ref(m, p, rows, 1)
    # 0.25 * -2^-149 rounds to -0; then 0 * -2^-149 = -0 keeps it, 0 * +2^-149 = +0 makes it +0
    assert bits(oL).tolist() == [[0x80000000, 0]] and oR[0].tolist() == [tiny, tiny]
    d = np.array([[tiny, 3 * tiny, 2.0 ** -126], [tiny, -tiny, 2.0 ** -127]], np.float32)
    rows = M.rows_of([0, 0], [1.0, 1.0], [0.0, 0.0], [0.5, 0.5], [0.0, 0.0])
    oL, oR = T.Engine.mix_ref(d, d, rows, 1)
    assert oL[0].tolist() == [2 * tiny, 2 * tiny, 2.0 ** -126 + 2.0 ** -127]
    # halves of odd denormals are ties and round to even: 0.5 -> 0, 1.5 -> 2, then 2 - 0.5 -> 2;
    # 2^-127 and 2^-128 are exact
    assert oR[0].tolist() == [0.0, 2 * tiny, 2.0 ** -127 + 2.0 ** -128]


def test_mono_planes():
    """d_L is d_R: the four coefficients see the same sample twice"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 40)).astype(np.float32)
    rows = M.rows_of([0, 1, 0, 1, 0], *rng.uniform(-1, 1, (4, 5)).astype(np.float32))
    monoL, monoR = T.Engine.mix_ref(x, x, rows, 2)
    twoL, twoR = T.Engine.mix_ref(x, x.copy(), rows, 2)
    assert np.array_equal(bits(monoL), bits(twoL)) and np.array_equal(bits(monoR), bits(twoR))
    assert float(np.abs(monoL).max()) > 0.1


# ---------------------------------------------------------------- 3. refusals on host-only engines
def _out(n_buses, frames, slack=3):
    L, R = np.zeros((n_buses, frames + slack), np.float32), np.zeros((n_buses, frames + slack), np.float32)
    return E.MixOut(L.ctypes.data, R.ctypes.data, frames + slack), (L, R)


def _rows(n, bus=0):
    return T.params.mix_rows([bus] * n)


def test_mix_device_refused_on_host_engines():
    """every -22 of tbf_mix_device, each with an error that names the argument, then -19:
    validation comes first"""
    lib = T.load_library()
    eng = _engine(n=0)
    n, frames, nb = 3, 100, 2
    L = np.zeros((n, frames + 1), np.float32)
    R = np.zeros_like(L)
    counts = np.array([0, 1, 100], np.uint32)
    good = _rows(n)

    def call(mo, l=L.ctypes.data, r=R.ctypes.data, stride=frames + 1, cnt=counts.ctypes.data, fr=frames, rows=good, buses=nb):
        return lib.tbf_mix_device(eng._h, n, l, r, stride, fr, cnt, None if rows is None else rows.ctypes.data, buses,
                                  None if mo is None else C.byref(mo), None)
    mo, keep = _out(nb, frames)
    assert call(mo) == -19 and "host-only" in _err(eng)
    assert call(mo, cnt=None) == -19 and call(mo, r=L.ctypes.data) == -19  # mono planes
    none = T.params.mix_rows([-1] * n)
    assert call(mo, rows=none, buses=0) == -19                               # no bus named, none asked for
    for kw in (dict(l=None), dict(r=None), dict(rows=None)):
        assert call(mo, **kw) == -22 and "null" in _err(eng)
    assert call(None) == -22 and "null" in _err(eng)
    for field in ("L", "R"):
        mo2, keep2 = _out(nb, frames)
        setattr(mo2, field, None)
        assert call(mo2) == -22 and "null" in _err(eng)
    assert lib.tbf_mix_device(None, n, L.ctypes.data, R.ctypes.data, frames + 1, frames, None, good.ctypes.data, nb, C.byref(mo),
                              None) == -22
    assert call(mo, buses=0) == -22 and "n_buses is 0" in _err(eng) and "rows[0]" in _err(eng)
    bad = good.copy()
    bad["bus"][1] = 2
    assert call(mo, rows=bad) == -22 and "rows[1].bus" in _err(eng)
    for k, v in (("ll", np.nan), ("lr", np.inf), ("rl", -np.inf), ("rr", np.nan)):
        bad = good.copy()
        bad[k][2] = v
        assert call(mo, rows=bad) == -22 and "rows[2]" in _err(eng) and "non-finite" in _err(eng)
        bad["bus"][2] = NONE                                                 # a row in no bus carries no coefficient
        assert call(mo, rows=bad) == -19
    assert call(mo, stride=frames - 1) == -22 and "in_stride" in _err(eng)
    mo2, keep2 = _out(nb, frames, slack=-1)
    assert call(mo2) == -22 and "out stride" in _err(eng)
    assert call(mo, l=L.ctypes.data + 2) == -22 and "aligned" in _err(eng)
    assert call(mo, r=R.ctypes.data + 1) == -22 and "aligned" in _err(eng)
    for field in ("L", "R"):
        mo2, keep2 = _out(nb, frames)
        setattr(mo2, field, getattr(mo2, field) + 2)
        assert call(mo2) == -22 and "aligned" in _err(eng)
    assert call(mo, fr=99) == -22 and "counts[2]" in _err(eng)
    # overlaps: an output plane inside the input rows, the two output planes in each other
    mo2, keep2 = _out(nb, frames)
    mo2.L = L.ctypes.data + 4 * (frames + 1)
    assert call(mo2) == -22 and "overlap" in _err(eng)
    mo2, keep2 = _out(nb, frames)
    mo2.R = R.ctypes.data + 4 * (n * (frames + 1) - 2)  # the last valid input frame
    assert call(mo2) == -22 and "overlap" in _err(eng)
    mo2, keep2 = _out(nb, frames)
    mo2.R = mo2.L + 4 * (frames + 3)
    assert call(mo2) == -22 and "overlap" in _err(eng)
    eng.close()


def test_mix_calls_refused_on_host_engines():
    """the render and process families: the refusals above, the wrong family for the chain and
    events out of order; -19 last"""
    lib = T.load_library()
    nblk, n, nb = 2, 2, 2
    frames = nblk * 128
    x = np.zeros((n, frames), np.float32)
    for chain in (FULL, TONEGEN, FX):
        fx = chain == FX
        eng = _engine(chain, n)
        good = _rows(n, 1)

        def call(mo, rows=good, buses=nb, fx=fx, eng=eng):
            r = None if rows is None else rows.ctypes.data
            m = None if mo is None else C.byref(mo)
            if fx:
                return lib.tbf_process_mix(eng._h, nblk, x.ctypes.data, frames, r, buses, m)
            return lib.tbf_render_mix(eng._h, nblk, r, buses, m)

        def call_dev(mo, rows=good, buses=nb, ev=None, nev=0, fx=fx, eng=eng):
            r = None if rows is None else rows.ctypes.data
            if fx:
                return lib.tbf_process_mix_device(eng._h, nblk, ev, nev, x.ctypes.data, frames, r, buses, C.byref(mo), None)
            return lib.tbf_render_mix_device(eng._h, nblk, ev, nev, r, buses, C.byref(mo), None)
        mo, keep = _out(nb, frames)
        assert call(mo) == -19 and "host-only" in _err(eng)
        assert call_dev(mo) == -19
        if fx:
            assert lib.tbf_render_mix(eng._h, nblk, good.ctypes.data, nb, C.byref(mo)) == -22 and "tbf_process_mix" in _err(eng)
            assert lib.tbf_render_mix_device(eng._h, nblk, None, 0, good.ctypes.data, nb, C.byref(mo), None) == -22
            assert lib.tbf_process_mix(eng._h, nblk, None, frames, good.ctypes.data, nb, C.byref(mo)) == -22 and "null" in _err(eng)
            assert lib.tbf_process_mix(eng._h, nblk, x.ctypes.data, frames - 1, good.ctypes.data, nb, C.byref(mo)) == -22
            assert "in_stride" in _err(eng)
            assert lib.tbf_process_mix_device(eng._h, nblk, None, 0, x.ctypes.data + 2, frames, good.ctypes.data, nb, C.byref(mo),
                                              None) == -22 and "aligned" in _err(eng)
            mo2, keep2 = _out(nb, frames)
            mo2.R = x.ctypes.data + 8  # a bus plane inside the effects-only input
            assert call(mo2) == -22 and "overlap" in _err(eng)
        else:
            assert lib.tbf_process_mix(eng._h, nblk, x.ctypes.data, frames, good.ctypes.data, nb, C.byref(mo)) == -22
            assert "effects-only" in _err(eng)
            assert lib.tbf_process_mix_device(eng._h, nblk, None, 0, x.ctypes.data, frames, good.ctypes.data, nb, C.byref(mo),
                                              None) == -22
        assert call(None) == -22 and "null" in _err(eng) and call(mo, rows=None) == -22 and "null" in _err(eng)
        assert call(mo, buses=0) == -22 and "n_buses is 0" in _err(eng)
        assert call(mo, buses=1) == -22 and "rows[0].bus" in _err(eng)
        bad = good.copy()
        bad["rl"][1] = np.inf
        assert call(mo, rows=bad) == -22 and "non-finite" in _err(eng) and call_dev(mo, rows=bad) == -22
        mo2, keep2 = _out(nb, frames, slack=-4)
        assert call(mo2) == -22 and "out stride" in _err(eng) and call_dev(mo2) == -22
        mo2, keep2 = _out(nb, frames)
        mo2.R = mo2.L + 4 * frames
        assert call(mo2) == -22 and "overlap" in _err(eng) and call_dev(mo2) == -22
        mo2, keep2 = _out(nb, frames)
        mo2.L += 2
        assert call_dev(mo2) == -22 and "aligned" in _err(eng)  # device pointers are 4-byte aligned
        assert call(mo2) == -19                                   # a host buffer need not be
        ev = eng.events([(1, 0, 0, 60, 1.0), (0, 0, 0, 62, 1.0)])[::-1].copy()  # out of order
        assert call_dev(mo, ev=ev.ctypes.data, nev=len(ev)) == -22
        assert call_dev(mo, ev=None, nev=2) == -22 and "null" in _err(eng)
        assert not keep[0].any() and not keep[1].any()
        eng.close()


def test_ref_refuses_what_the_calls_refuse():
    x = np.zeros((2, 8), np.float32)
    with pytest.raises(T.TbfError, match="rows\\[1\\].bus"):
        T.Engine.mix_ref(x, x, M.rows_of([0, 1], [1, 1], [0, 0], [0, 0], [1, 1]), 1)
    with pytest.raises(T.TbfError, match="non-finite"):
        T.Engine.mix_ref(x, x, M.rows_of([0, 0], [1, np.nan], [0, 0], [0, 0], [1, 1]), 1)
    with pytest.raises(T.TbfError, match="counts\\[0\\]"):
        T.Engine.mix_ref(x, x, M.rows_of([0, 0], [1, 1], [0, 0], [0, 0], [1, 1]), 1, counts=[9, 8])
    with pytest.raises(T.TbfError, match="n_buses is 0"):
        T.Engine.mix_ref(x, x, M.rows_of([0, NONE], [1, 1], [0, 0], [0, 0], [1, 1]), 0)


# ---------------------------------------------------------------- 4. the pan helper
def test_mix_rows_against_its_formula():
    bus = [0, 3, -1, 2, 2]
    gain = np.array([1.0, 0.5, 1.0, 2.0, 0.25])
    pan = np.array([0.0, -1.0, 0.3, 1.0, -0.4])
    rows = T.params.mix_rows(bus, gain, pan)
    assert rows.dtype == T.params.MIX_ROW_DTYPE and rows["bus"].tolist() == [0, 3, NONE, 2, 2]
    a = (pan + 1.0) * np.pi / 4.0
    assert np.array_equal(rows["ll"], (np.sqrt(2.0) * gain * np.cos(a)).astype(np.float32))
    assert np.array_equal(rows["rr"], (np.sqrt(2.0) * gain * np.sin(a)).astype(np.float32))
    assert not rows["lr"].any() and not rows["rl"].any()
    assert rows["ll"][0] == rows["rr"][0] == np.float32(1.0)   # unity at centre
    assert rows["rr"][1] == 0.0 and rows["ll"][1] == np.float32(np.sqrt(2.0) * 0.5)
    # constant power: ll^2 + rr^2 = 2 g^2 at every pan
    assert np.allclose(rows["ll"].astype(np.float64) ** 2 + rows["rr"].astype(np.float64) ** 2, 2 * gain ** 2, rtol=1e-6)
    one = T.params.mix_rows([0, 1])                              # scalars apply to every row
    assert one["ll"].tolist() == [1.0, 1.0] and one["rr"].tolist() == [1.0, 1.0]
    with pytest.raises(ValueError):
        T.params.mix_rows([0], 1.0, 1.5)
