"""The true-peak meter and the loudness range without a GPU: the table against its 48 integers, the
host restatement (tbf_debug_true_peak_ref, built from the header k_tpeak is built from) against
exact arithmetic in bits and against float64 within the sequential sum's bound, the tap order made
observable, aimed bursts that put the maximum where a test wants it, cuts into calls, the shift of
the history, the literal -0.0 / subnormal / NaN / Inf cases, the refusals, the sines of the issue's
table, and tbf_debug_loudness_range against a numpy restatement and the EBU Tech 3342 sequences."""
import ctypes as C

import numpy as np
import pytest

import loudness_model as LM
import truepeak_model as M

T = pytest.importorskip("tunebfree_amd")
E = T.engine

bits, mag = M.bits, M.mag


def _err():
    return T.load_library().tbf_last_error().decode()


def ref(L, R, F=4, **kw):
    return T.Engine.true_peak_ref(L, R, F, **kw)


def same_words(got, want, what):
    """peak words in bits, a NaN as "is NaN" """
    for k, (g, w) in enumerate(zip(got, want)):
        if M.is_nan_word(w):
            assert M.is_nan_word(g), (what, k, hex(int(g)), hex(int(w)))
        else:
            assert int(g) == int(w), (what, k, hex(int(g)), hex(int(w)))


def words_of(x, y):
    """the peak words two channels' samples [2][n] and y [2, n, phases] give"""
    return np.array([mag(x[0]).max(), mag(x[1]).max(), mag(y[0]).max() if y[0].size else 0,
                     mag(y[1]).max() if y[1].size else 0], np.uint32)


# ---------------------------------------------------------------- 1. table and mirrors
def test_table_is_the_48_integers_over_8192_in_bits():
    h = T.Engine.true_peak_table()
    assert h.dtype == np.float32 and h.shape == (4, 12)
    assert np.array_equal(bits(h), bits(M.K.astype(np.float32) / np.float32(8192.0)))
    assert np.array_equal(h.astype(np.float64) * 8192.0, M.K)        # every coefficient exact
    assert np.array_equal(bits(h[2]), bits(h[1][::-1])) and np.array_equal(bits(h[3]), bits(h[0][::-1]))
    assert h[0][0] == np.float32(0.0017089843750) and h[0][6] == np.float32(0.9721679687500)
    sums = h.astype(np.float64).sum(axis=1)
    assert np.allclose(sums, [1.00158691, 0.97302246, 0.97302246, 1.00158691], atol=5e-9)


def test_structs_mirror_the_header():
    assert C.sizeof(E.TruePeakConfig) == 8 and C.sizeof(E.TruePeakResult) == 32
    assert T.params.TRUE_PEAK_RESULT_DTYPE.itemsize == 32 and T.params.TRUE_PEAK_RESULT_DTYPE == M.RESULT_DTYPE
    assert [f[0] for f in E.TruePeakResult._fields_] == list(M.RESULT_DTYPE.names)
    tile, per_lane, groups, lds = T.Engine.true_peak_grid(3, 2 * 1024 + 1)
    assert tile >= 1 and tile % per_lane == 0 and lds <= 160 * 1024
    assert groups == 3 * -(-(2 * 1024 + 1) // tile)
    assert [E.true_peak_oversample(r) for r in (8000, 48000, 95999, 96000, 191999, 192000, 384000)] == [4, 4, 4, 2, 2, 1, 1]


# ---------------------------------------------------------------- 2. the chains
@pytest.mark.parametrize("F", [4, 2])
def test_ref_is_exact_on_an_exact_grid(F):
    """x = k / 1024 with |k| <= 4: every product is an integer multiple of 2^-23 and every partial sum
    one below 2^-6, so float32 holds them all and the chain equals the float64 sum in bits"""
    rng = np.random.default_rng(11)
    L = (rng.integers(-4, 5, 700) / 1024.0).astype(np.float32)
    R = (rng.integers(-4, 5, 700) / 1024.0).astype(np.float32)
    p, h, y = ref(L, R, F, want_y=True)
    for ch, x in enumerate((L, R)):
        want = M.y64(x, F)
        assert np.abs(want).max() < 2.0 ** -6 and np.array_equal(want * 2.0 ** 23, np.round(want * 2.0 ** 23))
        assert np.array_equal(bits(y[ch]), bits(want.astype(np.float32))), (F, ch)
    same_words(p, words_of((L, R), y), "exact grid")
    assert np.array_equal(bits(h), bits(np.concatenate([L[-11:], R[-11:]])))


@pytest.mark.parametrize("F", [4, 2])
def test_ref_on_noise_is_within_the_sequential_bound_of_float64(F):
    L, R = M.noise(21, 4000), M.noise(22, 4000)
    _p, _h, y = ref(L, R, F, want_y=True)
    worst = 0.0
    for ch, x in enumerate((L, R)):
        err = np.abs(y[ch].astype(np.float64) - M.y64(x, F))
        for q, ph in enumerate(M.phases(F)):
            bound = 12.0 * 2.0 ** -24 * np.abs(M.H[ph]).sum() * float(np.abs(x).max())
            worst = max(worst, err[:, q].max() / (2.0 ** -24))
            assert err[:, q].max() <= bound, (F, ch, ph, err[:, q].max(), bound)
    print(f"F = {F}: worst error {worst:.2f} x 2^-24")
    assert worst > 0.0


def test_tap_order_is_observable_and_the_ref_keeps_it():
    """first: on this noise the model with the taps summed in descending order differs from the
    ascending one in some bit of y, so a chain in another order could not pass by accident; then the
    ref equals the ascending model in bits"""
    x = M.noise(31, 300)
    _p, _h, y = ref(x, x, 4, want_y=True)
    changed = 0
    for p in range(4):
        up, down = M.chain(x, p), M.chain(x, p, descending=True)
        changed += int((bits(up) != bits(down)).sum())
        assert np.array_equal(bits(y[0][:, p]), bits(up)), p
        assert np.array_equal(bits(y[1][:, p]), bits(up)), p
    print("y values the descending order changes:", changed, "of", 4 * len(x))
    assert changed >= 1


def test_history_enters_the_chain_in_the_model_too():
    x, hist = M.noise(32, 40), M.noise(33, 11)
    _p, _h, y = ref(x, x, 4, hist=np.concatenate([hist, hist]), want_y=True)
    for p in range(4):
        assert np.array_equal(bits(y[0][:, p]), bits(M.chain(x, p, hist=hist))), p


# ---------------------------------------------------------------- 3. aimed bursts
@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_aimed_burst_puts_the_one_maximum_where_it_is_aimed(p):
    for seed in range(12):
        n0 = 11 + 17 * seed
        x = M.aimed(100 + seed, 400, n0, p)
        w, _h, y = ref(x, x, 4, want_y=True)
        at, ph, ratio = M.argmax_y(y[0])
        assert (at, ph) == (n0, p) and ratio >= 1.06, (seed, p, at, ph, ratio)
        top = float(np.abs(y[0]).max())
        assert abs(top - (1.011 if p in (0, 3) else 1.179)) < 0.012 and top > float(np.abs(x).max()) == 1.0
        assert int(w[2]) == M.word(y[0][n0, p]) and int(w[0]) == M.word(1.0)
    # at F = 2 a burst aimed at phase 2 is seen, one aimed at phase 1 falls between the phases used
    x = M.aimed(7, 400, 200, 2)
    _w, _h, y = ref(x, x, 2, want_y=True)
    assert M.argmax_y(y[0])[:2] == (200, 1)


# ---------------------------------------------------------------- 4. cuts and the history
def _in_cuts(L, R, cuts, F=4):
    p, h = None, None
    at = [0] + list(cuts) + [len(L)]
    for a, b in zip(at[:-1], at[1:]):
        p, h = ref(L[a:b].copy(), R[a:b].copy(), F, hist=h, peaks=p)
    return p, h


@pytest.mark.parametrize("F", [4, 2, 1])
def test_cuts_give_the_same_bits(F):
    n0 = 300
    L, R = M.aimed(41, 700, n0, 1), M.aimed(42, 700, n0 + 5, 3)
    p, h = ref(L, R, F)
    for cuts in [(1,), (10,), (11,), (12,), (1, 2, 3), (10, 21, 33), (0, 0, 5, 5)] + [(c,) for c in range(n0 - 11, n0 + 2)]:
        pc, hc = _in_cuts(L, R, cuts, F)
        same_words(pc, p, cuts)
        assert np.array_equal(bits(hc), bits(h)), cuts
    if F == 1:
        assert p[2] == 0 and p[3] == 0


def test_counts_below_11_shift_the_history():
    L, R = M.noise(51, 30), M.noise(52, 30)
    _p, h = ref(L[:20], R[:20])
    assert np.array_equal(bits(h), bits(np.concatenate([L[9:20], R[9:20]])))
    for k in (0, 1, 5, 10):
        _p2, h2 = ref(L[20:20 + k], R[20:20 + k], hist=h)
        want = np.concatenate([np.concatenate([L[9:20], L[20:20 + k]])[-11:], np.concatenate([R[9:20], R[20:20 + k]])[-11:]])
        assert np.array_equal(bits(h2), bits(want)), k
    # a new row's history is +0.0f, and fewer than 11 frames leave zeros in front
    _p3, h3 = ref(L[:3], R[:3])
    assert np.array_equal(bits(h3[:8]), np.zeros(8, np.uint32)) and np.array_equal(bits(h3[8:11]), bits(L[:3]))


# ---------------------------------------------------------------- 5. literal values
def test_negative_zero_and_a_subnormal_are_literal():
    x = M.noise(61, 200, scale=0.5)
    x[40:60] = 0.0
    x[45], x[52] = -0.0, np.float32(1e-41)
    p, h, y = ref(x, x, 4, want_y=True)
    for ph in range(4):
        assert np.array_equal(bits(y[0][:, ph]), bits(M.chain(x, ph))), ph    # signs of zero included
    tiny = np.full(30, np.float32(1e-41))
    tiny[3] = -0.0
    p, _h, y = ref(tiny, tiny, 4, want_y=True)
    assert p[0] == M.word(1e-41) and 0 < p[2] < 0x00800000           # a subnormal peak: nothing flushed
    for ph in range(4):
        assert np.array_equal(bits(y[0][:, ph]), bits(M.chain(tiny, ph))), ph
    z = np.full(20, -0.0, np.float32)
    p, _h = ref(z, z)
    assert not p.any() and T.Engine.true_peak_dbtp(p) == -np.inf              # -0.0 has magnitude 0


def test_nan_and_inf_rows():
    L, R = M.noise(71, 100, scale=0.5), M.noise(72, 100, scale=0.5)
    clean, _h = ref(L, R)
    Ln = L.copy()
    Ln[50] = np.nan
    p, _h, y = ref(Ln, R, want_y=True)
    assert M.is_nan_word(p[0]) and M.is_nan_word(p[2]) and p[1] == clean[1] and p[3] == clean[3]
    assert np.isnan(y[0][50:62]).all() and not np.isnan(y[0][:50]).any() and not np.isnan(y[0][62:]).any()
    assert np.isnan(T.Engine.true_peak_dbtp(p))
    p2, _h2 = ref(L, R, peaks=p)            # poisoned until reset
    assert M.is_nan_word(p2[0]) and M.is_nan_word(p2[2])
    Li = L.copy()
    Li[50] = -np.inf
    p, _h = ref(Li, R)
    assert p[0] == 0x7F800000 and p[2] == 0x7F800000 and p[1] == clean[1] and p[3] == clean[3]   # Inf in bits
    assert T.Engine.true_peak_dbtp(p) == np.inf
    Li[51] = -np.inf        # neighbouring taps of opposite sign: Inf - Inf in the chain, a NaN above the Inf
    p, _h = ref(Li, R)
    assert p[0] == 0x7F800000 and M.is_nan_word(p[2]) and np.isnan(T.Engine.true_peak_dbtp(p))
    one = np.zeros(40, np.float32)
    one[5] = np.inf
    p, _h = ref(one, one, 1)
    assert p.tolist() == [0x7F800000, 0x7F800000, 0, 0] and T.Engine.true_peak_dbtp(p) == np.inf


def test_dbtp_rule():
    d = T.Engine.true_peak_dbtp
    one, half = M.word(1.0), M.word(0.5)
    assert d([0, 0, 0, 0]) == -np.inf and d([one, 0, 0, 0]) == 0.0
    assert abs(d([half, one, half, half]) - 0.0) == 0.0 and abs(d([half, 0, 0, 0]) + 6.020599913279624) < 1e-12
    assert np.isnan(d([one, 0x7FC00000, 0, 0])) and d([0x7F800000, 0, one, 0]) == np.inf
    for w in ([1, 2, 3, 4], [one, half, 5, 0x3F900000]):
        assert d(w) == M.dbtp(w) or abs(d(w) - M.dbtp(w)) < 1e-12


# ---------------------------------------------------------------- 6. sines
SINES = [  # cycles per frame, phase, sample peak dB or None, dBTP at F = 4, the same at F = 2
    (1 / 4, 45.0, -3.010, +0.045, True),
    (1 / 4, 0.0, None, -0.197, True),
    (1 / 8, 67.5, None, -0.007, True),
    (997.0 / 48000.0, 0.0, None, +0.009, False),
]


@pytest.mark.parametrize("cpf,phase,sample_db,want,same_at_2", SINES)
def test_sines_at_48k(cpf, phase, sample_db, want, same_at_2):
    """The table's figures are those of a running sine: the 4800 frames are measured behind the 11
    frames before them as the row's history, so that no onset from silence enters (an abrupt onset
    overshoots by itself: 0.7 dB at fs/8 and 67.5 degrees).  The F = 4 column is the largest
    interpolated value; the reported dbtp also takes the samples in and so is never below them."""
    x = M.sine(4811, cpf, phase - 360.0 * cpf * 11)
    hist, x = np.concatenate([x[:11], x[:11]]), x[11:]
    p, _h = ref(x, x, 4, hist=hist)
    f = p.view(np.float32)
    sp, ip, d = 20.0 * np.log10(float(f[0])), 20.0 * np.log10(float(f[2])), T.Engine.true_peak_dbtp(p)
    print(f"{cpf:.5f} cycles/frame at {phase} deg: sample peak {sp:+.3f} dB, F = 4 {ip:+.3f} dBTP, dbtp {d:+.3f}")
    assert abs(ip - want) <= 0.01
    if sample_db is not None:
        assert abs(sp - sample_db) <= 0.01
    assert d >= sp and abs(d - max(sp, ip)) < 1e-6          # never below the sample peak
    p2, _h = ref(x, x, 2, hist=hist)
    ip2, d2 = 20.0 * np.log10(float(p2.view(np.float32)[2])), T.Engine.true_peak_dbtp(p2)
    assert ip2 <= ip and sp <= d2 <= d
    if same_at_2:
        assert abs(ip2 - want) <= 0.01
    p1, _h = ref(x, x, 1, hist=hist)
    assert abs(T.Engine.true_peak_dbtp(p1) - sp) < 1e-6 and p1[2] == 0


# ---------------------------------------------------------------- 7. refusals
def _create(eng, n_rows, F, cfg_null=False, out_null=False):
    cfg, h = E.TruePeakConfig(F, 0), C.c_void_p()
    return eng._lib.tbf_true_peak_create(eng._h, n_rows, None if cfg_null else C.byref(cfg), None if out_null else C.byref(h))


def test_host_only_engine_validates_then_refuses():
    eng = T.Engine(sample_rate=48000.0, device=-1)
    assert _create(eng, 4, 4) == -19 and "host-only" in _err()
    with pytest.raises(T.TbfError, match="-19"):
        eng.true_peak(4)
    bad = [(dict(n_rows=4, F=0), "oversample"), (dict(n_rows=4, F=3), "oversample"), (dict(n_rows=4, F=8), "oversample"),
           (dict(n_rows=0, F=4), "n_rows"), (dict(n_rows=4, F=4, cfg_null=True), "cfg"), (dict(n_rows=4, F=4, out_null=True), "out")]
    for kw, word in bad:   # validation comes before the -19
        assert _create(eng, **kw) == -22, kw
        assert word in _err(), (kw, _err())
    cfg, h = E.TruePeakConfig(4, 0), C.c_void_p()
    assert eng._lib.tbf_true_peak_create(None, 4, C.byref(cfg), C.byref(h)) == -22 and "engine" in _err()
    eng.close()


def test_null_meter_and_hook_refusals():
    lib = T.load_library()
    res = np.zeros(1, M.RESULT_DTYPE)
    assert lib.tbf_true_peak_reset(None, 0, None, None) == -22 and "tp" in _err()
    assert lib.tbf_true_peak_device(None, None, None, 0, 0, None, None) == -22 and "tp" in _err()
    assert lib.tbf_true_peak_read(None, 0, None, res.ctypes.data) == -22 and "tp" in _err()
    assert lib.tbf_true_peak_destroy(None) == 0
    x = np.zeros(8, np.float32)
    for F in (0, 3, 5):
        with pytest.raises(T.TbfError, match="-22.*oversample"):
            ref(x, x, F)
    f = lib.tbf_debug_true_peak_ref
    f.restype = C.c_int
    f.argtypes = [C.POINTER(E.TruePeakConfig), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    cfg, h, p = E.TruePeakConfig(4, 0), np.full(22, 0.25, np.float32), np.full(4, 7, np.uint32)
    assert f(None, x.ctypes.data, x.ctypes.data, 8, h.ctypes.data, p.ctypes.data, None) == -22 and "cfg" in _err()
    assert f(C.byref(cfg), x.ctypes.data, x.ctypes.data, 8, None, p.ctypes.data, None) == -22 and "hist22" in _err()
    assert f(C.byref(cfg), x.ctypes.data, x.ctypes.data, 8, h.ctypes.data, None, None) == -22 and "peaks4" in _err()
    assert f(C.byref(cfg), None, x.ctypes.data, 8, h.ctypes.data, p.ctypes.data, None) == -22 and "L is NULL" in _err()
    assert f(C.byref(cfg), x.ctypes.data, None, 8, h.ctypes.data, p.ctypes.data, None) == -22 and "R is NULL" in _err()
    assert (h == 0.25).all() and (p == 7).all()            # a refused call moves nothing
    assert f(C.byref(cfg), None, None, 0, h.ctypes.data, p.ctypes.data, None) == 0 and (h == 0.25).all() and (p == 7).all()
    g = lib.tbf_debug_true_peak_table
    g.restype, g.argtypes = C.c_int, [C.c_void_p]
    assert g(None) == -22 and "h48" in _err()
    d = lib.tbf_debug_true_peak_dbtp
    d.restype, d.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    assert d(None, None) == -22 and "peaks4" in _err()
    r = lib.tbf_debug_loudness_range
    r.restype, r.argtypes = C.c_int, [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lra = C.c_double()
    assert r(48001, np.zeros(8).ctypes.data, 4, C.byref(lra), None) == -22 and "rate_hz" in _err()
    assert r(48000, np.zeros(8).ctypes.data, 4, None, None) == -22 and "lra" in _err()
    assert r(48000, None, 4, C.byref(lra), None) == -22 and "e is NULL" in _err()
    assert r(48000, None, 0, C.byref(lra), None) == 0 and lra.value == 0.0
    assert lib.tbf_loudness_range(None, 0, None, C.byref(lra), None) == -22 and "lm" in _err()


def test_ref_writes_y_inside_its_room_only():
    x = M.noise(81, 50)
    lib = T.load_library()
    f = lib.tbf_debug_true_peak_ref
    f.restype = C.c_int
    f.argtypes = [C.POINTER(E.TruePeakConfig), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    for F, ph in ((4, 4), (2, 2), (1, 0)):
        buf = np.full(2 * 50 * ph + 8, -5.0, np.float32)
        h, p = np.zeros(22, np.float32), np.zeros(4, np.uint32)
        assert f(C.byref(E.TruePeakConfig(F, 0)), x.ctypes.data, x.ctypes.data, 50, h.ctypes.data, p.ctypes.data, buf[4:].ctypes.data) == 0
        assert (buf[:4] == -5.0).all() and (buf[-4:] == -5.0).all() and not (buf[4:-4] == -5.0).any()


# ---------------------------------------------------------------- 8. loudness range
def _energies(seed, n, lo=-60.0, hi=-10.0):
    """hop energies of levels spread between lo and hi dB"""
    rng = np.random.default_rng(seed)
    return 4800.0 * 10.0 ** (rng.uniform(lo, hi, (n, 2)) / 10.0)


@pytest.mark.parametrize("seed,n", [(1, 30), (2, 31), (3, 100), (4, 400), (5, 777)])
def test_range_against_numpy(seed, n):
    e = _energies(seed, n)
    e[n // 3: n // 3 + 5] = 0.0                    # silence inside
    e[n // 2] = 1e-9                               # far below the absolute gate
    lra, win = T.Engine.loudness_range(48000, e)
    want, wwin = M.loudness_range(48000, e)
    print(f"{n} hops: LRA {lra:.6f} LU over {win} windows")
    assert win == wwin and abs(lra - want) <= 1e-9
    assert n < 60 or (win > 0 and lra > 0.0)


def test_range_edges():
    for n in (0, 1, 29):
        assert T.Engine.loudness_range(48000, _energies(6, n)) == (0.0, 0)
    assert T.Engine.loudness_range(48000, np.zeros((100, 2))) == (0.0, 0)                       # silence
    assert T.Engine.loudness_range(48000, np.full((100, 2), 4800.0 * 10.0 ** -7.5)) == (0.0, 0)  # -75 LUFS: under the absolute gate
    lra, win = T.Engine.loudness_range(48000, np.full((100, 2), 4800.0 * 0.01))
    assert lra == 0.0 and win == 71                                                             # a constant level: no range
    e = np.full((60, 2), 4800.0 * 0.01)
    e[10, 0] = np.nan                                                                           # windows over a NaN pass no gate
    lra, win = T.Engine.loudness_range(48000, e)
    assert lra == 0.0 and win == 31 - 11


@pytest.mark.parametrize("first,second,want", [(-20.0, -30.0, 10.0), (-20.0, -15.0, 5.0), (-40.0, -20.0, 20.0)])
def test_tech_3342_sequences(first, second, want):
    """EBU Tech 3342 test signals 1 to 3: a 1 kHz sine at two levels, 20 s each, in both channels;
    the expected range within that document's own tolerance of 1 LU"""
    x = LM.sine(48000, [(first, 20.0), (second, 20.0)])
    e, _st = T.Engine.loudness_ref(x, x, 48000)
    assert len(e) == 400
    lra, win = T.Engine.loudness_range(48000, e)
    m, mw = M.loudness_range(48000, e)
    print(f"{first} then {second} dBFS: LRA {lra:.4f} LU over {win} windows")
    assert abs(lra - want) <= 1.0 and win == mw and abs(lra - m) <= 1e-9
