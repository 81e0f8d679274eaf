"""The bus compressor on the GPU (tbf_comp_*, k_comp): identity in bits of every output frame, every
row's gain and every meter with the host restatement of the definition (tbf_debug_comp_ref, run per
row) at every layout the kernel takes, rows at their own counts, the key input, rows of one wave on
different curves, streaming with set and reset mid-stream, isolation, two compressors on one engine,
the refusals, the accounting, and the mix -> equalise -> compress -> limit -> PCM chain with ducking.

The stage is this project's own definition (include/tbf.h); the restatement
against the plain-Python model, the lookup, the designer and the order of the operations are checked
without a GPU (tests/test_comp_cpu.py).  The rate is 8000 wherever the stage stands alone."""
import numpy as np
import pytest

import comp_model as M
import scenarios as S

pytestmark = pytest.mark.gpu

TONEGEN = 1
FILL = 777.0
RATE = 8000
F32 = np.float32
bits = M.bits
LAYOUTS = (4,)   # every rows-per-wave the library can choose (asserted in test_gpu_comp_the_layouts_the_host_chooses)


def same(a, b, what):
    """equal in bits; a NaN equals any NaN: the definition says that a NaN stays one, not which"""
    both = np.isnan(np.asarray(a, F32)) & np.isnan(np.asarray(b, F32))
    a, b = np.where(both, 0, bits(a)), np.where(both, 0, bits(b))
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} of {a.size} differ, first at {tuple(bad[0])}")


def engine(n=0, chain=0):
    import tunebfree_amd as T
    eng = T.Engine(sample_rate=48000.0, device=0, chain=chain)
    if n:
        tid = eng.template(seed=7)
        eng.add_instances([tid] * n, [4100 + 37 * i for i in range(n)])
    return eng


def audio(seed, frames, rows):
    """noise whose level wanders over 14 octaves around the curves' thresholds, frame by frame"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, frames)) * np.exp2(rng.uniform(-12.0, 2.0, (rows, frames)))).astype(F32)


def curves(k):
    """k curves, all different, none flat"""
    import tunebfree_amd as T
    spec = [(-30.0, 4.0, 6.0), (-20.0, np.inf, 0.0), (-45.0, 2.0, 12.0), (-12.0, 8.0, 3.0), (-60.0, 3.0, 0.0), (-25.0, 20.0, 20.0),
            (-36.0, 1.5, 1.0), (-6.0, np.inf, 9.0)]
    return [T.params.comp_curve(*spec[i]) for i in range(k)]


def params_for(n, n_curves, seed):
    """per-row parameters: every curve in use, coefficients from 0 to close to 1, make-ups around 1"""
    import tunebfree_amd as T
    rng = np.random.default_rng(seed)
    p = np.zeros(n, T.params.COMP_ROW_DTYPE)
    p["curve"] = (np.arange(n) + seed) % n_curves
    p["attack"] = np.where(np.arange(n) % 5 == 0, 0.0, rng.uniform(0.0, 0.999, n)).astype(F32)
    p["release"] = np.where(np.arange(n) % 7 == 3, 0.0, 1.0 - np.exp2(rng.uniform(-12.0, -1.0, n))).astype(F32)
    p["makeup"] = np.exp2(rng.uniform(-1.0, 2.0, n)).astype(F32)
    return p


class Ref:
    """the rows of a compressor on the host: comp_ref per row, the curves, parameters and gains carried"""

    def __init__(self, n, n_curves=1):
        import tunebfree_amd as T
        self.n = n
        self.curves = [np.ones(M.POINTS, F32) for _ in range(n_curves)]
        self.p = np.zeros(n, T.params.COMP_ROW_DTYPE)
        self.p["makeup"] = 1.0
        self.g = np.ones(n, F32)

    def set_rows(self, p, rows=None):
        self.p[slice(None) if rows is None else list(rows)] = p

    def reset(self, rows=None):
        self.g[slice(None) if rows is None else list(rows)] = 1.0

    def call(self, L, R, counts=None, key=None):
        """the outputs and meters a call must give, FILL where it must write nothing"""
        import tunebfree_amd as T
        oL, oR = np.full(L.shape, FILL, F32), np.full(L.shape, FILL, F32)
        mt = np.zeros(self.n, T.params.COMP_METER_DTYPE)
        mt["min_gain"] = 1.0
        for r in range(self.n):
            c = L.shape[1] if counts is None else int(counts[r])
            mt["frames"][r] = c
            if c == 0:
                continue
            l = L[r, :c]
            k = None
            if key is not None:
                kl = key[0][r, :c]
                k = (kl, kl if key[1] is key[0] else key[1][r, :c])
            p = self.p[r]
            oL[r, :c], oR[r, :c], self.g[r], gains = T.Engine.comp_ref(l, l if R is L else R[r, :c], self.curves[p["curve"]], p["attack"],
                                                                       p["release"], p["makeup"], self.g[r], key=k)
            mt["min_gain"][r] = gains.min()
        return oL, oR, mt


def planes(srcs, n, frames, lead, stride):
    """the source rows in allocations of their own with FILL around: (host arrays, device tensors)"""
    import torch
    host, dev = [], []
    for src in srcs:
        a = np.full(lead + n * stride + 4, FILL, F32)
        a[lead:lead + n * stride].reshape(n, stride)[:, :frames] = src
        host.append(a)
        dev.append(torch.from_numpy(a).cuda())
    return host, dev


def run(comp, L, R, aligned=True, counts=None, key=None, meters=True):
    """one tbf_comp_device call in torch memory: aligned -- every row 16-byte aligned, even strides;
    otherwise everything one float into its allocation with odd strides (inputs, key and outputs with
    different ones).  R is L, and key[1] is key[0]: one plane passed twice.  Asserts that the call left
    the inputs and the key, pads included, as they were and the outputs' pads at their fill; returns
    (outL rows, outR rows, the meters or None)."""
    import torch
    import tunebfree_amd as T
    n, frames = L.shape
    lead = 0 if aligned else 1
    stride = (frames + 3) // 4 * 4 + (0 if aligned else 1)
    ostride, kstride = (stride, stride) if aligned else (stride + 2, stride + 4)
    host, dev = planes((L,) if R is L else (L, R), n, frames, lead, stride)
    kh, kd = planes(() if key is None else (key[0],) if key[1] is key[0] else key, n, frames, lead, kstride)
    out = [torch.full((lead + n * ostride + 4,), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    mt = torch.full((2 * n + 2,), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 for t in dev + kd + out)
    ptr = [t.data_ptr() + 4 * lead for t in dev]
    kp = [t.data_ptr() + 4 * lead for t in kd]
    comp.process_device(ptr[0], ptr[-1], stride, frames, out[0].data_ptr() + 4 * lead, out[1].data_ptr() + 4 * lead, ostride,
                        counts=counts, key=None if key is None else (kp[0], kp[-1], kstride),
                        meters_ptr=mt.data_ptr() if meters else None)
    torch.cuda.synchronize()
    for a, t in zip(host + kh, dev + kd):
        assert a.tobytes() == t.cpu().numpy().tobytes(), "the compressor wrote into its input or its key"
    res = []
    for t in out:
        o = t.cpu().numpy()
        body = o[lead:lead + n * ostride].reshape(n, ostride)
        assert (o[:lead] == FILL).all() and (o[lead + n * ostride:] == FILL).all() and (body[:, frames:] == FILL).all(), \
            "written outside the output rows"
        res.append(body[:, :frames].copy())
    m = mt.cpu().numpy()
    if not meters:
        assert (m == FILL).all(), "a NULL meter pointer and something was written"
        return res[0], res[1], None
    assert (m[2 * n:] == FILL).all(), "written behind the meters"
    return res[0], res[1], m[:2 * n].copy().view(T.params.COMP_METER_DTYPE)


def check_call(comp, ref, L, R, what, aligned=True, counts=None, key=None, meters=True):
    gL, gR, gm = run(comp, L, R, aligned, counts, key, meters)
    wL, wR, wm = ref.call(L, R, counts, key)
    same(gL, wL, what + ": L against comp_ref")
    same(gR, wR, what + ": R against comp_ref")
    if meters:
        assert np.array_equal(gm["frames"], wm["frames"]), what + ": the meters' frames"
        assert np.array_equal(bits(gm["min_gain"]), bits(wm["min_gain"])), what + ": the meters' min_gain"
    return gL, gR, gm


def make(eng, n, n_curves=1, layout=0, seed=1):
    """a compressor with n_curves curves loaded and per-row parameters, and its Ref"""
    import tunebfree_amd as T
    comp, ref = eng.compressor(n, n_curves), Ref(n, n_curves)
    assert layout in (0, T.Engine.comp_grid(n, n_curves)[0])   # the one the library takes for these rows
    for i, c in enumerate(curves(n_curves)):
        comp.set_curve(i, c)
        ref.curves[i] = c
    p = params_for(n, n_curves, seed)
    comp.set_rows(p)
    ref.set_rows(p)
    return comp, ref


def counts_for(n, frames, seed):
    """0, 1, half and full counts mixed across a wave's rows"""
    c = np.random.default_rng(seed).integers(0, frames + 1, n).astype(np.uint32)
    c[0::5] = frames
    c[1::5] = 0
    c[2::5] = min(1, frames)
    c[3::5] = frames // 2
    return c


def with_nan_beyond(x, counts):
    x = x.copy()
    for r, c in enumerate(counts):
        x[r, int(c):] = np.nan
    return x


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


# ---------------------------------------------------------------- 1. layouts
def test_gpu_comp_the_layouts_the_host_chooses():
    import tunebfree_amd as T
    seen = {T.Engine.comp_grid(n)[0] for n in (1, 2, 100, 4096, 8192, 8193, 20000, 70000, 300000, 2 ** 22)}
    assert seen == set(LAYOUTS)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("rows", ["1", "2", "R-1", "R", "R+1", "2R+3"])
@pytest.mark.parametrize("R", LAYOUTS)
def test_gpu_comp_layouts_against_ref(eng, R, rows, aligned):
    """row counts around a wave's rows for every R, frame counts around the group of four, the wave and
    the LDS tile, with and without counts (0, 1, half and full, NaN behind each), and one call with
    d_L == d_R; the calls follow each other on one compressor, so every one but the first starts from
    a gain"""
    import tunebfree_amd as T
    _, tile, lds = T.Engine.comp_grid(1, 3)
    assert tile >= 64 and lds <= 160 * 1024
    n = {"1": 1, "2": 2, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+3": 2 * R + 3}[rows]
    comp, ref = make(eng, n, 3, R, seed=R + n)
    assert comp.curve(2).tobytes() == ref.curves[2].tobytes() and comp.row(n - 1).tobytes() == ref.p[n - 1].tobytes()
    for k, frames in enumerate((1, 3, 4, tile - 1, tile, tile + 1, 2 * tile + 5)):
        L, Rr = audio(100 + k, frames, n), audio(200 + k, frames, n)
        what = f"R={R} rows={n} aligned={aligned} frames={frames}"
        check_call(comp, ref, L, Rr, what, aligned)
        c = counts_for(n, frames, 300 + k)
        g0 = ref.g.copy()
        check_call(comp, ref, with_nan_beyond(L, c), with_nan_beyond(Rr, c), what + " counts", aligned, c)
        assert np.array_equal(bits(ref.g[c == 0]), bits(g0[c == 0]))
        if frames == tile + 1:
            gL, gR, _ = check_call(comp, ref, L, L, what + " mono", aligned)
            same(gL, gR, "mono: outL against outR")
    assert np.isfinite(ref.g).all() and (ref.g < 1.0).any()
    comp.close()


def test_gpu_comp_count_zero_rows_keep_their_gain(eng):
    """rows pushed down, then a call in which some take nothing, then silence: the rows that took
    nothing release from the gain they had"""
    n, frames = 7, 200
    import tunebfree_amd as T
    comp, ref = make(eng, n, 1, seed=3)
    p = np.zeros(n, T.params.COMP_ROW_DTYPE)
    p["attack"], p["release"], p["makeup"] = 0.5, 0.99, 1.0
    comp.set_rows(p), ref.set_rows(p)
    loud = np.full((n, frames), 0.9, F32)
    check_call(comp, ref, loud, loud, "loud")
    assert (ref.g < 0.5).all()
    c = np.array([0, frames, 0, 1, frames // 2, 0, frames], np.uint32)
    g0 = ref.g.copy()
    _, _, mt = check_call(comp, ref, loud, loud, "some rows take nothing", counts=c)
    assert np.array_equal(bits(ref.g[c == 0]), bits(g0[c == 0]))
    assert (mt["min_gain"][c == 0] == 1.0).all() and (mt["frames"][c == 0] == 0).all()
    _, _, mt = check_call(comp, ref, loud, loud, "no row takes anything", counts=np.zeros(n, np.uint32))
    assert (mt["min_gain"] == 1.0).all() and (mt["frames"] == 0).all()
    quiet = np.zeros((n, 5), F32)
    _, _, mt = check_call(comp, ref, quiet, quiet, "silence behind it")
    assert np.array_equal(bits(mt["min_gain"][c == 0]), bits(np.array([M.step(g, 1.0, 0.0, r) for g, r in
                                                                       zip(g0[c == 0], ref.p["release"][c == 0])], F32)))
    comp.close()


# ---------------------------------------------------------------- 2. the key input
@pytest.mark.parametrize("R", LAYOUTS)
def test_gpu_comp_key_input(eng, R):
    """the gain follows the key pair, which has its own stride: a silent key under loud input leaves
    the input alone, a loud key ducks a quiet input, and one key plane may serve as both"""
    import tunebfree_amd as T
    n = R + 3
    tile = T.Engine.comp_grid(1)[1]
    frames = tile + 37
    comp, ref = make(eng, n, 2, R, seed=9)
    L, Rr, kL, kR = (audio(400 + i, frames, n) for i in range(4))
    for aligned in (True, False):
        check_call(comp, ref, L, Rr, f"key aligned={aligned}", aligned, key=(kL, kR))
        c = counts_for(n, frames, 17)
        check_call(comp, ref, L, Rr, f"key and counts aligned={aligned}", aligned, counts=c, key=(with_nan_beyond(kL, c), kR))
        check_call(comp, ref, L, Rr, f"one key plane aligned={aligned}", aligned, key=(kL, kL))
    p = np.zeros(n, T.params.COMP_ROW_DTYPE)
    p["makeup"] = 1.0   # attack and release 0: the gain is the target
    comp.set_rows(p), ref.set_rows(p), comp.reset(), ref.reset()
    loud, silent = np.full((n, frames), 0.8, F32), np.zeros((n, frames), F32)
    gL, _, mt = check_call(comp, ref, loud, loud, "a silent key under loud input", key=(silent, silent))
    same(gL, loud, "a silent key: the input as it was")
    assert (mt["min_gain"] == 1.0).all()
    quiet = np.full((n, frames), 1e-4, F32)
    gL, _, mt = check_call(comp, ref, quiet, quiet, "a loud key over quiet input", key=(loud, loud))
    assert (gL < quiet).all() and (mt["min_gain"] < 0.5).all()
    gL, _, _ = check_call(comp, ref, quiet, quiet, "the same input without the key")
    same(gL, quiet, "quiet input without a key")
    comp.close()


# ---------------------------------------------------------------- 3. mixed parameters
@pytest.mark.parametrize("R", LAYOUTS)
def test_gpu_comp_rows_of_one_wave_on_different_curves(eng, R):
    """8 curves loaded, the rows of every wave spread over them with their own attack, release and
    make-up; the rows on curve 0, which is made flat again, with make-up 1 come out as their own bits
    beside them, a NaN included"""
    n = 2 * R + 1
    comp, ref = make(eng, n, 8, R, seed=5)
    flat = np.ones(M.POINTS, F32)
    comp.set_curve(0, flat)
    ref.curves[0] = flat
    own = [r for r in range(n) if ref.p["curve"][r] == 0]
    assert len(own) >= 1 and len(set(ref.p["curve"])) == 8
    p = ref.p[own].copy()
    p["makeup"] = 1.0
    comp.set_rows(p, rows=own), ref.set_rows(p, rows=own)
    L, Rr = audio(31, 333, n), audio(32, 333, n)
    L[own[0], 40] = np.nan
    L[own[0], 41], L[own[0], 42], L[own[0], 43] = np.inf, -0.0, 1e-42
    gL, gR, mt = check_call(comp, ref, L, Rr, "8 curves")
    for r in own:
        same(gL[r], L[r], f"row {r} on the flat curve, L")
        same(gR[r], Rr[r], f"row {r} on the flat curve, R")
    assert (mt["min_gain"][own] == 1.0).all() and (np.delete(mt["min_gain"], own) < 1.0).all()
    assert all(not np.array_equal(bits(gL[r]), bits(L[r])) for r in range(n) if r not in own)
    comp.close()


# ---------------------------------------------------------------- 4. streaming
@pytest.mark.parametrize("R", LAYOUTS)
def test_gpu_comp_a_stream_in_cuts_equals_one_call(eng, R):
    """calls of 1, 5, TILE - 1 and 3 TILE + 2 frames against one call over the same frames, in bits,
    the meters' minimum included"""
    import tunebfree_amd as T
    tile = T.Engine.comp_grid(1)[1]
    cuts = (1, 5, tile - 1, 3 * tile + 2)
    n, frames = R + 1, sum(cuts)
    L, Rr = audio(51, frames, n), audio(52, frames, n)
    whole, ref = make(eng, n, 2, R, seed=6)
    wL, wR, wm = check_call(whole, ref, L, Rr, "one call")
    parts, _ = make(eng, n, 2, R, seed=6)
    pL, pR, lows, at = [], [], [], 0
    for c in cuts:
        a, b, m = run(parts, L[:, at:at + c], Rr[:, at:at + c], aligned=bool(c % 2))
        pL.append(a), pR.append(b), lows.append(m["min_gain"])
        at += c
    same(np.concatenate(pL, axis=1), wL, "the cuts against one call, L")
    same(np.concatenate(pR, axis=1), wR, "the cuts against one call, R")
    assert np.array_equal(bits(np.min(lows, axis=0)), bits(wm["min_gain"]))
    for c in (whole, parts):
        c.close()


def test_gpu_comp_set_curve_set_rows_and_reset_mid_stream(eng):
    """a new curve, new rows and a reset of some rows between calls: each takes effect from the next
    call, keeps every gain (a reset: of the other rows), and the read-back follows"""
    import tunebfree_amd as T
    n, frames = 9, 150
    comp, ref = make(eng, n, 2, seed=8)
    for k in range(6):
        L, Rr = audio(60 + k, frames, n), audio(70 + k, frames, n)
        if k == 1:
            c = T.params.comp_curve(-50.0, 10.0, 5.0)
            comp.set_curve(1, c)
            ref.curves[1] = c
            assert comp.curve(1).tobytes() == c.tobytes() and comp.curve(0).tobytes() == ref.curves[0].tobytes()
        if k == 2:
            p = params_for(2, 2, 99)
            comp.set_rows(p, rows=[1, 5]), ref.set_rows(p, rows=[1, 5])
            assert comp.row(5).tobytes() == p[1].tobytes() and comp.row(0).tobytes() == ref.p[0].tobytes()
        if k == 3:
            comp.reset([3, 4]), ref.reset([3, 4])
        if k == 5:
            comp.reset(), ref.reset()
        g0 = ref.g.copy()
        check_call(comp, ref, L, Rr, f"call {k}", aligned=bool(k % 2))
        if k in (1, 2, 3):
            assert (g0 < 1.0).sum() >= n - 2   # the calls started from gains that the changes had kept
    comp.close()


def test_gpu_comp_two_compressors_back_to_back_on_one_stream(eng):
    """set, process, set, process on two compressors with nothing waited for in between: the bits are
    the sequential ones"""
    import torch
    import tunebfree_amd as T
    n, frames = 21, 300
    a, ra = make(eng, n, 2, seed=11)
    b, rb = make(eng, n, 1, seed=12)
    x = [audio(80 + i, frames, n) for i in range(4)]
    d = [torch.from_numpy(v).cuda() for v in x]
    o = [torch.full((n, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    c2, p2 = T.params.comp_curve(-15.0, 3.0, 2.0), params_for(n, 2, 13)
    a.process_device(d[0].data_ptr(), d[1].data_ptr(), frames, frames, o[0].data_ptr(), o[1].data_ptr(), frames)
    b.process_device(o[0].data_ptr(), o[1].data_ptr(), frames, frames, o[2].data_ptr(), o[3].data_ptr(), frames)   # a's output
    a.set_curve(0, c2)
    a.set_rows(p2)
    a.process_device(d[2].data_ptr(), d[3].data_ptr(), frames, frames, o[4].data_ptr(), o[5].data_ptr(), frames)
    eng.synchronize()
    w1 = ra.call(x[0], x[1])
    w2 = rb.call(w1[0], w1[1])
    ra.curves[0] = c2
    ra.set_rows(p2)
    w3 = ra.call(x[2], x[3])
    for t, w, what in zip(o, w1[:2] + w2[:2] + w3[:2], ("a first L", "a first R", "b L", "b R", "a second L", "a second R")):
        same(t.cpu().numpy(), w, what)
    a.close(), b.close()
    a.close()   # a second close is nothing


# ---------------------------------------------------------------- 5. isolation
@pytest.mark.parametrize("R", LAYOUTS)
def test_gpu_comp_a_nan_or_inf_row_moves_no_neighbour(eng, R):
    """a row full of NaN and one full of Inf among the rows of a wave: the others are the bits they
    are without them, the NaN row's gain releases (its level is 0) and the Inf row's gain falls to
    the curve's last point; both stay finite and the rows recover"""
    n, frames = R + 2, 260
    L, Rr = audio(91, frames, n), audio(92, frames, n)
    clean, rc = make(eng, n, 2, R, seed=14)
    wL, wR, _ = check_call(clean, rc, L, Rr, "clean")
    comp, ref = make(eng, n, 2, R, seed=14)
    bL, bR = L.copy(), Rr.copy()
    bL[1], bR[1] = np.nan, np.nan
    bL[2], bR[2] = np.inf, -np.inf
    gL, gR, mt = check_call(comp, ref, bL, bR, "with a NaN row and an Inf row")
    keep = [r for r in range(n) if r not in (1, 2)]
    same(gL[keep], wL[keep], "the neighbours, L"), same(gR[keep], wR[keep], "the neighbours, R")
    assert np.isnan(gL[1]).all()
    # ref.g is the restatement's gain, not the device's.  The device's shows in two ways: the meters of
    # this call, which check_call held to the restatement's in bits, and the call behind it, which
    # starts from the device's g and equals, in bits and meters, the restatement started from ref.g.
    assert np.isfinite(ref.g).all() and (ref.g >= 0).all() and (ref.g <= 1).all()
    assert np.isfinite(mt["min_gain"]).all() and (mt["min_gain"] >= 0).all() and (mt["min_gain"] <= 1).all()
    gL, gR, mt = check_call(comp, ref, L, Rr, "the call behind it")
    assert np.isfinite(gL).all() and np.isfinite(gR).all()
    assert np.isfinite(mt["min_gain"]).all() and (mt["min_gain"] >= 0).all() and (mt["min_gain"] <= 1).all()
    clean.close(), comp.close()


# ---------------------------------------------------------------- 6. meters
def test_gpu_comp_meters_and_a_null_meter_pointer(eng):
    n, frames = 6, 140
    comp, ref = make(eng, n, 1, seed=15)
    L, Rr = audio(95, frames, n), audio(96, frames, n)
    c = np.array([frames, 0, 1, 70, 0, frames], np.uint32)
    _, _, mt = check_call(comp, ref, L, Rr, "meters", counts=c)
    assert (mt["min_gain"][c == 0] == 1.0).all() and (mt["frames"] == c).all() and (mt["min_gain"][c > 1] < 1.0).all()
    check_call(comp, ref, L, Rr, "no meters", meters=False)
    check_call(comp, ref, L, Rr, "no meters, odd", aligned=False, counts=c, meters=False)
    comp.close()


# ---------------------------------------------------------------- 7. refusals
def test_gpu_comp_refusals_write_nothing_and_move_no_state(eng):
    import torch
    import tunebfree_amd as T
    n, frames = 4, 96
    comp, ref = make(eng, n, 2, seed=16)
    L, Rr = audio(81, frames, n), audio(82, frames, n)
    check_call(comp, ref, L, Rr, "before the refusals")
    stride = frames + 4
    x = [torch.from_numpy(np.ascontiguousarray(np.pad(a, ((0, 0), (0, 4))))).cuda() for a in (L, Rr, L, Rr)]
    o = [torch.full((n, stride), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    mt = torch.full((2 * n,), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    xl, xr, kl, kr, ol, orr = [t.data_ptr() for t in x + o]
    good = dict(L_ptr=xl, R_ptr=xr, in_stride=stride, frames=frames, outL_ptr=ol, outR_ptr=orr, out_stride=stride, counts=None,
                key=(kl, kr, stride), meters_ptr=mt.data_ptr())
    over = np.full(n, frames, np.uint32)
    over[2] = frames + 1
    bad = [
        (dict(L_ptr=None), "d_L"), (dict(R_ptr=None), "d_R"), (dict(outL_ptr=None), "d_outL"), (dict(outR_ptr=None), "d_outR"),
        (dict(key=(kl, None, stride)), "d_keyR"), (dict(key=(None, kr, stride)), "d_keyL"),
        (dict(in_stride=frames - 1), "in_stride"), (dict(key=(kl, kr, frames - 1)), "key_stride"),
        (dict(out_stride=frames - 1), "out_stride"),
        (dict(L_ptr=xl + 2), "aligned"), (dict(outR_ptr=orr + 2), "aligned"), (dict(key=(kl + 1, kr, stride)), "aligned"),
        (dict(meters_ptr=mt.data_ptr() + 2), "aligned"),
        (dict(counts=over), r"counts\[2\]"),
        (dict(outL_ptr=xl), "overlap"),                                           # in place
        (dict(outR_ptr=xr + 4 * (stride * (n - 1) + frames - 1)), "overlap"),     # one float of the input's last row
        (dict(outL_ptr=kr + 4 * 8), "overlap"),                                   # the key
        (dict(outR_ptr=ol + 4 * 8), "overlap"),                                   # the two outputs
    ]
    for kw, word in bad:
        with pytest.raises(T.TbfError, match="-22.*" + word):
            comp.process_device(**{**good, **kw})
    with pytest.raises(T.TbfError, match=r"-22.*rows\[1\]"):
        comp.reset([0, n])
    with pytest.raises(T.TbfError, match=r"-22.*rows\[0\]"):
        comp.set_rows(T.params.comp_row(), rows=[n])
    ok = T.params.comp_row(1, 1.0, 50.0, 3.0, RATE)
    for field, v, word in (("curve", 2, "row 3: curve 2"), ("attack", 1.0, "row 3: attack"), ("attack", np.nan, "row 3: attack"),
                           ("release", -0.5, "row 3: release"), ("release", 1.5, "row 3: release"), ("makeup", 300.0, "row 3: makeup"),
                           ("makeup", np.nan, "row 3: makeup"), ("makeup", -1.0, "row 3: makeup")):
        p = np.stack([ok, ok])      # row 1 of the list is fine; nothing of it is kept
        p[field][1] = v
        with pytest.raises(T.TbfError, match="-22.*" + word):
            comp.set_rows(p, rows=[1, 3])
    for i, v in ((0, 1.0001), (768, np.nan), (100, -1e-9), (7, np.inf)):
        c = T.params.comp_curve(-10.0, 2.0)
        c[i] = v
        with pytest.raises(T.TbfError, match=f"-22.*point {i}:"):
            comp.set_curve(1, c)
    with pytest.raises(T.TbfError, match="-22.*curve 2"):
        comp.set_curve(2, T.params.comp_curve(-10.0, 2.0))
    with pytest.raises(T.TbfError, match="-22.*curve 2"):
        comp.curve(2)
    with pytest.raises(T.TbfError, match="-22.*row"):
        comp.row(n)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in o) and (mt.cpu().numpy() == FILL).all()
    same(x[0].cpu().numpy()[:, :frames], L, "the input after the refusals")
    for r in range(n):
        assert comp.row(r).tobytes() == ref.p[r].tobytes(), f"row {r}'s parameters after the refusals"
    for i in range(2):
        assert comp.curve(i).tobytes() == ref.curves[i].tobytes(), f"curve {i} after the refusals"
    check_call(comp, ref, audio(83, frames, n), audio(84, frames, n), "a valid call behind the refusals")
    comp.close()


# ---------------------------------------------------------------- 8. accounting
def test_gpu_comp_accounting():
    """a compressor is no instance or stage memory of the engine, a call that takes frames is one
    launch set and one that takes none is none, the render kernels' launch counts do not move, and
    the engine releases the compressors that are still alive when it closes"""
    import torch
    e = engine(2)
    e.render(2)
    b0, l0 = e.device_bytes(), e.launches()
    comp = e.compressor(64, 8)
    e.compressor(3)   # left to the engine
    comp.set_curve(7, curves(1)[0])
    assert e.device_bytes() == b0
    x = torch.zeros((64, 256), dtype=torch.float32, device="cuda")
    o = [torch.zeros((64, 256), dtype=torch.float32, device="cuda") for _ in range(2)]
    mt = torch.zeros((128,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    call = lambda **kw: comp.process_device(x.data_ptr(), x.data_ptr(), 256, kw.pop("frames", 256), o[0].data_ptr(), o[1].data_ptr(),
                                            256, **kw)
    comp.timing(True)
    for _ in range(3):
        call()
    call(frames=0)
    call(counts=np.zeros(64, np.uint32))
    call(counts=np.zeros(64, np.uint32), meters_ptr=mt.data_ptr())   # writes the meters, takes no frames
    e.synchronize()
    ms, k = comp.timing()
    assert k == 3 and ms > 0.0
    comp.timing(False)
    call()
    assert comp.timing() == (0.0, 0)
    assert e.device_bytes() == b0 and e.launches() == l0
    e.close()
    comp.close()


# ---------------------------------------------------------------- 9. the chain
def test_gpu_comp_between_equaliser_and_limiter_with_ducking():
    """8 tone generators mixed into 2 buses over 8 blocks, then equaliser, compressor, limiter and PCM
    on one stream with nothing waited for: bus 0 is compressed keyed by bus 1 (ducking, its own
    compressor), bus 1 by itself; every stage's planes are the host restatement of the planes before
    it, and the PCM bytes those of pcm_ref"""
    import torch
    import tunebfree_amd as T
    n, nb, buses = 8, 8, 2
    frames = nb * 128
    bus = np.arange(n) % buses
    ceil = float(F32(0.25))
    bands = [T.params.eq_band(T.params.EQ_HPF, 40.0), T.params.eq_band(T.params.EQ_HIGH, 4000.0, gain_db=3.0)]
    curve = T.params.comp_curve(-40.0, 4.0, 6.0)
    duck_row = T.params.comp_row(0, 1.0, 20.0, 0.0, 48000)
    own_row = T.params.comp_row(0, 2.0, 80.0, 12.0, 48000)

    e = engine(n, TONEGEN)
    for i in range(n):
        for (_b, kind, x, v) in S.bench_scenario(i):
            (e.note if kind == "note" else e.set_param)(i, x, v)
    mix, eqo, cpo, lmo = ([torch.full((buses, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)] for _ in range(4))
    pcm = torch.zeros((buses, frames * 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eq = e.equalizer(buses, 2)
    eq.set([bands, bands[:1]])
    duck, own = e.compressor(1), e.compressor(1)
    for c, p in ((duck, duck_row), (own, own_row)):
        c.set_curve(0, curve)
        c.set_rows(p)
    lim = e.limiter(buses, ceil, 64, 32)
    pl = lambda ts, row=0: [t.data_ptr() + 4 * frames * row for t in ts]
    e.render_mix_device(nb, T.params.mix_rows(bus, 0.5), buses, *pl(mix), frames)
    eq.process_device(*pl(mix), frames, frames, *pl(eqo), frames)
    duck.process_device(*pl(eqo), frames, frames, *pl(cpo), frames, key=(*pl(eqo, 1), frames))
    own.process_device(*pl(eqo, 1), frames, frames, *pl(cpo, 1), frames)
    lim.process_device(*pl(cpo), frames, frames, *pl(lmo), frames)
    e.pcm_convert_device(buses, *pl(lmo), frames, frames, pcm.data_ptr(), frames * 4, T.engine.PCM_S16)
    e.synchronize()
    mix, eqo, cpo, lmo = ([t.cpu().numpy() for t in p] for p in (mix, eqo, cpo, lmo))
    pcm = pcm.cpu().numpy()
    e.close()

    assert np.isfinite(mix[0]).all() and float(np.abs(mix[0]).max()) > 1e-2
    want_eq = [T.Engine.eq_ref(mix[0][b], mix[1][b], [T.Engine.eq_coeffs(x, 48000) for x in bl])[:2] for b, bl in enumerate((bands, bands[:1]))]
    for b in range(buses):
        same(eqo[0][b], want_eq[b][0], f"bus {b}: equalised L"), same(eqo[1][b], want_eq[b][1], f"bus {b}: equalised R")
    d = T.Engine.comp_ref(eqo[0][0], eqo[1][0], curve, duck_row["attack"], duck_row["release"], duck_row["makeup"], key=(eqo[0][1], eqo[1][1]))
    o = T.Engine.comp_ref(eqo[0][1], eqo[1][1], curve, own_row["attack"], own_row["release"], own_row["makeup"])
    for b, w in enumerate((d, o)):
        same(cpo[0][b], w[0], f"bus {b}: compressed L"), same(cpo[1][b], w[1], f"bus {b}: compressed R")
        assert w[3].min() < 1.0, f"bus {b}: the compressor did nothing"
    alone = T.Engine.comp_ref(eqo[0][0], eqo[1][0], curve, duck_row["attack"], duck_row["release"], duck_row["makeup"])
    assert not np.array_equal(bits(alone[0]), bits(d[0])), "the key changed nothing"
    for b in range(buses):
        lL, lR, _, _ = T.Engine.limit_ref(cpo[0][b], cpo[1][b], ceil, 64, 32)
        same(lmo[0][b], lL, f"bus {b}: limited L"), same(lmo[1][b], lR, f"bus {b}: limited R")
        fr, _ = T.Engine.pcm_ref(T.engine.PCM_S16, lmo[0][b], lmo[1][b], row=b)
        assert pcm[b].tobytes() == fr.tobytes(), f"bus {b}: the PCM bytes"
    assert pcm.any()
