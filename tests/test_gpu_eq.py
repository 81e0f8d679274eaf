"""The bus equaliser on the GPU (tbf_eq_*, k_eq): identity in bits of every output frame with the host
restatement of the definition (tbf_debug_eq_ref, run per row) at every layout the kernel takes,
rows streaming at their own counts, set and reset mid-stream, isolation, two equalisers on one
engine, set and process back to back, the refusals, the mix -> equalise -> limit -> PCM chain, and the
accounting.

The stage is this project's own definition (include/tbf.h); the restatement
against the plain-Python model, the designer and the order of the operations are checked without a
GPU (tests/test_eq_cpu.py).  The rate is 8000 wherever the stage stands alone."""
import numpy as np
import pytest

import eq_model as M
import scenarios as S

pytestmark = pytest.mark.gpu

TONEGEN = 1
FILL = 777.0
RATE = 8000
bits = M.bits


def same(a, b, what):
    """equal in bits; a NaN equals any NaN: the definition says that a NaN stays one, not which, and
    the host's and the device's invalid operations give NaNs of different signs"""
    both = np.isnan(np.asarray(a, np.float32)) & np.isnan(np.asarray(b, np.float32))
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


def band_list(k, seed, rate=RATE):
    """k stable bands of rotating types inside the accepted ranges"""
    import tunebfree_amd as T
    rng = np.random.default_rng(seed)
    return [T.params.eq_band(int((seed + j) % 9), float(rng.uniform(0.004, 0.45) * rate), float(rng.uniform(0.4, 3.0)),
                             float(rng.uniform(-9.0, 9.0))) for j in range(k)]


def row_lists(n, max_bands, seed):
    """per-row band lists of different lengths, 0 and max_bands among them"""
    lens = [(max_bands, 0, 1, max_bands // 2, max_bands - 1)[r % 5] if n > 1 else max_bands for r in range(n)]
    return [band_list(k, seed + 13 * r) for r, k in enumerate(lens)]


class Ref:
    """the rows of an equaliser on the host: eq_ref per row, the coefficients and states carried"""

    def __init__(self, n, rate=RATE):
        self.n, self.rate = n, rate
        self.c = [np.zeros((0, 5)) for _ in range(n)]
        self.state = [np.zeros((2, 8, 2)) for _ in range(n)]   # every band's, in use or not: a set keeps them

    def set(self, lists, rows=None):
        import tunebfree_amd as T
        for r, bl in zip(range(self.n) if rows is None else rows, lists):
            self.c[r] = np.array([T.Engine.eq_coeffs(b, self.rate) for b in bl], np.float64).reshape(-1, 5)

    def reset(self, rows=None):
        for r in (range(self.n) if rows is None else rows):
            self.state[r][:] = 0.0

    def call(self, L, R, counts=None):
        """the outputs a call must give, FILL where it must write nothing"""
        import tunebfree_amd as T
        oL, oR = np.full(L.shape, FILL, np.float32), np.full(L.shape, FILL, np.float32)
        for r in range(self.n):
            c, nb = L.shape[1] if counts is None else int(counts[r]), len(self.c[r])
            if c == 0:
                continue
            l = L[r, :c]
            oL[r, :c], oR[r, :c], self.state[r][:, :nb] = T.Engine.eq_ref(l, l if R is L else R[r, :c], self.c[r],
                                                                         self.state[r][:, :nb])
        return oL, oR


def run(eq, L, R, aligned=True, counts=None):
    """one tbf_eq_device call in torch memory: aligned -- every row 16-byte aligned, even strides;
    otherwise everything one float into its allocation with odd strides (inputs and outputs with
    different ones).  R is L: one plane passed twice.  Asserts that the call left the inputs, pads
    included, as they were and the outputs' pads at their fill; returns the output rows."""
    import torch
    n, frames = L.shape
    lead = 0 if aligned else 1
    stride = (frames + 3) // 4 * 4 + (0 if aligned else 1)
    ostride = stride if aligned else stride + 2
    host, dev = [], []
    for src in ((L,) if R is L else (L, R)):
        a = np.full(lead + n * stride + 4, FILL, np.float32)
        a[lead:lead + n * stride].reshape(n, stride)[:, :frames] = src
        host.append(a)
        dev.append(torch.from_numpy(a).cuda())
    out = [torch.full((lead + n * ostride + 4,), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 for t in dev + out)
    ptr = [t.data_ptr() + 4 * lead for t in dev]
    eq.process_device(ptr[0], ptr[-1], stride, frames, out[0].data_ptr() + 4 * lead, out[1].data_ptr() + 4 * lead, ostride,
                      counts=counts)
    torch.cuda.synchronize()
    for a, t in zip(host, dev):
        assert a.tobytes() == t.cpu().numpy().tobytes(), "the equaliser wrote into its input"
    res = []
    for t in out:
        o = t.cpu().numpy()
        body = o[lead:lead + n * ostride].reshape(n, ostride)
        assert (o[:lead] == FILL).all() and (o[lead + n * ostride:] == FILL).all() and (body[:, frames:] == FILL).all(), \
            "written outside the output rows"
        res.append(body[:, :frames].copy())
    return res


def check_call(eq, ref, L, R, what, aligned=True, counts=None):
    got = run(eq, L, R, aligned, counts)
    want = ref.call(L, R, counts)
    same(got[0], want[0], what + ": L against eq_ref")
    same(got[1], want[1], what + ": R against eq_ref")
    return got


def counts_for(n, frames, seed):
    """0, 1, partial and full counts"""
    c = np.random.default_rng(seed).integers(0, frames + 1, n).astype(np.uint32)
    c[0::7] = frames
    c[1::7] = 0
    c[2::7] = min(1, frames)
    c[3::7] = frames // 2
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


def grid(max_bands):
    import tunebfree_amd as T
    return T.Engine.eq_grid(max_bands)


# ---------------------------------------------------------------- 1. layouts
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("rows", ["1", "rpw-1", "rpw", "rpw+1", "70"])
@pytest.mark.parametrize("max_bands", [1, 2, 3, 8])
def test_gpu_eq_layouts_against_ref(eng, max_bands, rows, aligned):
    """row counts around a wave's rows, frame counts around P, the wave and the LDS tile, with and
    without counts (0, 1, partial and full, NaN behind each), per-row band lists of every length from
    0 to max_bands, and one call with d_L == d_R; the calls follow each other on one equaliser, so
    every one but the first starts from a state"""
    P, rpw, tile, lds = grid(max_bands)
    assert P in (1, 2, 4, 8) and P >= max_bands and rpw == 32 // P and tile >= 8 and lds <= 160 * 1024
    n = {"1": 1, "rpw-1": rpw - 1, "rpw": rpw, "rpw+1": rpw + 1, "70": 70}[rows]
    eq, ref = eng.equalizer(n, max_bands, RATE), Ref(n)
    lists = row_lists(n, max_bands, 40 + max_bands)
    eq.set(lists)
    ref.set(lists)
    assert {len(b) for b in lists} >= ({0, max_bands} if n >= 2 else {max_bands})
    for r in range(min(n, 5)):
        assert eq.bands(r).tobytes() == ref.c[r].tobytes()
    for k, frames in enumerate(sorted({1, max(P - 1, 1), P, 63, 65, tile - 1, tile, tile + 1, 2 * tile + 5})):
        L, R = M.noise(100 + k, frames, n), M.noise(200 + k, frames, n)
        what = f"max_bands={max_bands} rows={n} aligned={aligned} frames={frames}"
        check_call(eq, ref, L, R, what, aligned)
        c = counts_for(n, frames, 300 + k)
        check_call(eq, ref, with_nan_beyond(L, c), with_nan_beyond(R, c), what + " counts", aligned, c)
        if frames == 65:
            check_call(eq, ref, L, L, what + " mono", aligned)
    assert all(np.isfinite(s).all() for s in ref.state)
    eq.close()


def test_gpu_eq_mono_from_the_first_frame(eng):
    """d_L == d_R on a new equaliser: both output planes are equal and are those of the restatement"""
    n = 5
    eq, ref = eng.equalizer(n, 4, RATE), Ref(n)
    lists = row_lists(n, 4, 7)
    eq.set(lists)
    ref.set(lists)
    L = M.noise(7, 300, n)
    got = check_call(eq, ref, L, L, "mono")
    same(got[0], got[1], "outL against outR")
    eq.close()


# ---------------------------------------------------------------- 2. streaming
def test_gpu_eq_rows_stream_at_their_own_counts(eng):
    """12 rows take random counts over 10 calls: every row's joined output is one eq_ref run over its
    joined frames"""
    import tunebfree_amd as T
    n, calls = 12, 10
    eq, ref = eng.equalizer(n, 8, RATE), Ref(n)
    lists = row_lists(n, 8, 21)
    eq.set(lists)
    ref.set(lists)
    rng = np.random.default_rng(43)
    inL, inR, outL, outR = ([[] for _ in range(n)] for _ in range(4))
    for k in range(calls):
        frames = int(rng.integers(100, 700))
        counts = rng.integers(0, frames + 1, n).astype(np.uint32)
        counts[k % n], counts[(k + 1) % n] = frames, 0
        L, R = with_nan_beyond(M.noise(500 + k, frames, n), counts), with_nan_beyond(M.noise(600 + k, frames, n), counts)
        got = check_call(eq, ref, L, R, f"call {k}", aligned=bool(k % 2), counts=counts)
        for r in range(n):
            c = int(counts[r])
            inL[r].append(L[r, :c]), inR[r].append(R[r, :c]), outL[r].append(got[0][r, :c]), outR[r].append(got[1][r, :c])
    for r in range(n):
        wL, wR, _ = T.Engine.eq_ref(np.concatenate(inL[r]), np.concatenate(inR[r]), ref.c[r])
        same(np.concatenate(outL[r]), wL, f"row {r}: joined L against one eq_ref run")
        same(np.concatenate(outR[r]), wR, f"row {r}: joined R against one eq_ref run")
    assert len({sum(len(x) for x in inL[r]) for r in range(n)}) > 6
    eq.close()


# ---------------------------------------------------------------- 3. set, reset, isolation
def test_gpu_eq_set_reset_nan_and_two_equalizers(eng):
    """set on rows {1, 5} changes those rows alone from the next call on and keeps their state; reset
    restarts rows; a NaN row stays NaN until it is reset and leaves the rows of its wave and its
    P-group clean; a second equaliser with another max_bands goes its own way"""
    n, frames = 8, 333
    a, b = eng.equalizer(n, 3, RATE), eng.equalizer(n, 8, RATE)
    ra, rb = Ref(n), Ref(n)
    la, lb = [band_list(3, 50 + r) for r in range(n)], row_lists(n, 8, 90)
    a.set(la), ra.set(la), b.set(lb), rb.set(lb)
    for k in range(6):
        L, R = M.noise(60 + k, frames, n), M.noise(70 + k, frames, n)
        if k == 1:
            L[3, 17] = np.nan           # row 3, channel L
        if k == 2:
            new = [band_list(2, 777), band_list(3, 778)]
            a.set(new, rows=[1, 5])
            ra.set(new, rows=[1, 5])
            assert a.bands(1).shape == (2, 5) and a.bands(0).tobytes() == ra.c[0].tobytes()
        if k == 3:
            a.reset([3])
            ra.reset([3])
        if k == 4:
            a.reset([1, 5])
            ra.reset([1, 5])
        ga = check_call(a, ra, L, R, f"equaliser a, call {k}", aligned=bool(k % 2))
        check_call(b, rb, L, R, f"equaliser b, call {k}")
        if k in (1, 2):
            assert np.isnan(ga[0][3, 17:]).all() and np.isfinite(ga[1][3]).all(), "the NaN row"
            for r in (0, 1, 2, 4, 5, 6, 7):
                assert np.isfinite(ga[0][r]).all() and np.isfinite(ga[1][r]).all(), f"row {r} beside the NaN row"
        if k >= 3:
            assert np.isfinite(ga[0]).all() and np.isfinite(ga[1]).all()
    with pytest.raises(Exception, match=r"-22.*rows\[1\]"):
        a.reset([0, n])
    a.reset()
    ra.reset()
    L, R = M.noise(91, frames, n), M.noise(92, frames, n)
    check_call(a, ra, L, R, "after a reset of all rows")
    a.close(), b.close()


def test_gpu_eq_set_process_set_process_back_to_back(eng):
    """set, process, set, process on one stream with nothing waited for in between: the bits are the
    sequential ones, the second call's bands acting on the state the first one left"""
    import torch
    import tunebfree_amd as T
    n, frames = 40, 700
    eq, ref = eng.equalizer(n, 8, RATE), Ref(n)
    first, second = row_lists(n, 8, 5), list(reversed(row_lists(n, 8, 6)))
    x = [M.noise(31, frames, n), M.noise(32, frames, n), M.noise(33, frames, n), M.noise(34, frames, n)]
    d = [torch.from_numpy(a).cuda() for a in x]
    o = [torch.full((n, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    eq.set(first)
    eq.process_device(d[0].data_ptr(), d[1].data_ptr(), frames, frames, o[0].data_ptr(), o[1].data_ptr(), frames)
    eq.set(second)
    eq.process_device(d[2].data_ptr(), d[3].data_ptr(), frames, frames, o[2].data_ptr(), o[3].data_ptr(), frames)
    eq.set(first, rows=list(range(n)))   # a third set behind the last call changes nothing already issued
    eng.synchronize()
    ref.set(first)
    w1 = ref.call(x[0], x[1])
    ref.set(second)
    w2 = ref.call(x[2], x[3])
    for t, w, what in zip(o, w1 + w2, ("first L", "first R", "second L", "second R")):
        same(t.cpu().numpy(), w, what)
    eq.close()


def test_gpu_eq_destroyed_and_left_to_the_engine():
    import torch
    e = engine()
    x = torch.from_numpy(M.noise(5, 200, 3)).cuda()
    o = [torch.zeros((3, 200), dtype=torch.float32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    kept, gone = e.equalizer(3, 2, RATE), e.equalizer(3, 2, RATE)
    for k, q in enumerate((kept, gone)):
        q.set(band_list(2, 3))
        q.process_device(x.data_ptr(), x.data_ptr(), 200, 200, o[2 * k].data_ptr(), o[2 * k + 1].data_ptr(), 200)
    e.synchronize()
    same(o[0].cpu().numpy(), o[2].cpu().numpy(), "two equalisers on the same planes")
    gone.close()
    gone.close()                                # a second close is nothing
    kept.process_device(x.data_ptr(), x.data_ptr(), 200, 200, o[0].data_ptr(), o[1].data_ptr(), 200)
    e.synchronize()
    assert np.isfinite(o[0].cpu().numpy()).all()
    e.close()                                   # releases `kept`
    kept.close()


# ---------------------------------------------------------------- 4. refusals
def test_gpu_eq_refusals_write_nothing_and_move_no_state(eng):
    import torch
    import tunebfree_amd as T
    n, frames = 4, 96
    eq, ref = eng.equalizer(n, 4, RATE), Ref(n)
    lists = row_lists(n, 4, 11)
    eq.set(lists)
    ref.set(lists)
    L, R = M.noise(81, frames, n), M.noise(82, frames, n)
    check_call(eq, ref, L, R, "before the refusals")
    stride = frames + 4
    x = [torch.from_numpy(np.ascontiguousarray(np.pad(a, ((0, 0), (0, 4))))).cuda() for a in (L, R)]
    o = [torch.full((n, stride), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    xl, xr, ol, orr = x[0].data_ptr(), x[1].data_ptr(), o[0].data_ptr(), o[1].data_ptr()
    good = dict(L_ptr=xl, R_ptr=xr, in_stride=stride, frames=frames, outL_ptr=ol, outR_ptr=orr, out_stride=stride, counts=None)
    over = np.full(n, frames, np.uint32)
    over[2] = frames + 1
    bad = [
        (dict(L_ptr=None), "d_L"),
        (dict(R_ptr=None), "d_R"),
        (dict(outL_ptr=None), "d_outL"),
        (dict(outR_ptr=None), "d_outR"),
        (dict(in_stride=frames - 1), "in_stride"),
        (dict(out_stride=frames - 1), "out_stride"),
        (dict(L_ptr=xl + 2), "aligned"),
        (dict(outR_ptr=orr + 2), "aligned"),
        (dict(counts=over), r"counts\[2\]"),
        (dict(outL_ptr=xl), "overlap"),                      # in place
        (dict(outR_ptr=xr + 4 * (stride * (n - 1) + frames - 1)), "overlap"),   # one float of the input's last row
        (dict(outR_ptr=ol + 4 * 8), "overlap"),              # the two outputs
    ]
    for kw, word in bad:
        with pytest.raises(T.TbfError, match="-22.*" + word):
            eq.process_device(**{**good, **kw})
    with pytest.raises(T.TbfError, match=r"-22.*rows\[1\]"):
        eq.reset([0, n])
    with pytest.raises(T.TbfError, match=r"-22.*rows\[0\]"):
        eq.set([band_list(1, 1)], rows=[n])
    with pytest.raises(T.TbfError, match=r"-22.*row 2.*5 bands"):
        eq.set([band_list(5, 1)], rows=[2])
    with pytest.raises(T.TbfError, match=r"-22.*row 3 band 1.*q"):   # row 1 of the list is fine; nothing of it is kept
        eq.set([band_list(2, 1), [T.params.eq_band(6, 100.0), T.params.eq_band(6, 100.0, q=6.0)]], rows=[1, 3])
    with pytest.raises(T.TbfError, match=r"-22.*row"):
        eq.bands(n)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in o)
    same(x[0].cpu().numpy()[:, :frames], L, "the input after the refusals")
    for r in range(n):
        assert eq.bands(r).tobytes() == ref.c[r].tobytes(), f"row {r}'s bands after the refusals"
    L2, R2 = M.noise(83, frames, n), M.noise(84, frames, n)
    check_call(eq, ref, L2, R2, "a valid call behind the refusals")
    eq.close()


# ---------------------------------------------------------------- 5. the chain
def test_gpu_eq_between_mix_and_limiter():
    """16 tone generators mixed into 2 buses over 64 blocks; a 40 Hz high-pass and a +3 dB high shelf
    on bus 0, nothing on bus 1, then the limiter and the PCM stage, all on one stream: bus 1's
    equalised planes are the mix planes in bits, bus 0's are eq_ref of them, the limited planes are
    limit_ref of the equalised ones, and the mix planes are those of a twin engine without an
    equaliser"""
    import torch
    import tunebfree_amd as T
    n, nb, buses = 16, 64, 2
    frames = nb * 128
    bus = np.arange(n) % buses
    ceil = float(np.float32(1.0 - 2.0 ** -15))
    bands = [T.params.eq_band(T.params.EQ_HPF, 40.0), T.params.eq_band(T.params.EQ_HIGH, 4000.0, gain_db=3.0)]

    def chain(equalised):
        e = engine(n, TONEGEN)
        for i in range(n):
            for (_b, kind, x, v) in S.bench_scenario(i):
                (e.note if kind == "note" else e.set_param)(i, x, v)
        mix, out, lim_o = ([torch.full((buses, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)] for _ in range(3))
        pcm = torch.zeros((buses, frames * 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eq = lim = None
        if equalised:
            eq = e.equalizer(buses, 2)
            assert eq.rate_hz == 48000
            eq.set([bands, []])
            lim = e.limiter(buses, ceil, 64, 32)
        e.render_mix_device(nb, T.params.mix_rows(bus, 0.5), buses, mix[0].data_ptr(), mix[1].data_ptr(), frames)
        if equalised:   # on the same stream, no synchronize in between
            eq.process_device(mix[0].data_ptr(), mix[1].data_ptr(), frames, frames, out[0].data_ptr(), out[1].data_ptr(), frames)
            lim.process_device(out[0].data_ptr(), out[1].data_ptr(), frames, frames, lim_o[0].data_ptr(), lim_o[1].data_ptr(), frames)
            e.pcm_convert_device(buses, lim_o[0].data_ptr(), lim_o[1].data_ptr(), frames, frames, pcm.data_ptr(), frames * 4,
                                 T.engine.PCM_S16)
        e.synchronize()
        res = [[t.cpu().numpy().copy() for t in p] for p in (mix, out, lim_o)] + [pcm.cpu().numpy().copy()]
        e.close()
        return res

    mix, out, limited, pcm = chain(True)
    assert np.isfinite(mix[0]).all() and float(np.abs(mix[0]).max()) > 1e-3
    coef = [T.Engine.eq_coeffs(b, 48000) for b in bands]
    wL, wR, _ = T.Engine.eq_ref(mix[0][0], mix[1][0], coef)
    same(out[0][0], wL, "bus 0: equalised L against eq_ref of the mix plane")
    same(out[1][0], wR, "bus 0: equalised R against eq_ref of the mix plane")
    assert not np.array_equal(bits(out[0][0]), bits(mix[0][0]))
    same(out[0][1], mix[0][1], "bus 1: no band, L")
    same(out[1][1], mix[1][1], "bus 1: no band, R")
    for b in range(buses):
        lL, lR, _, _ = T.Engine.limit_ref(out[0][b], out[1][b], ceil, 64, 32)
        same(limited[0][b], lL, f"bus {b}: limited L against limit_ref of the equalised plane")
        same(limited[1][b], lR, f"bus {b}: limited R against limit_ref of the equalised plane")
    assert pcm.any()
    twin = chain(False)[0]
    same(mix[0], twin[0], "mix planes with and without an equaliser, L")
    same(mix[1], twin[1], "mix planes with and without an equaliser, R")


# ---------------------------------------------------------------- 6. accounting
def test_gpu_eq_accounting():
    """an equaliser is no instance or stage memory of the engine, a call that takes frames is one
    launch set and one that takes none is none, the render kernels' launch counts do not move, and
    the engine releases the equalisers that are still alive when it closes"""
    import torch
    e = engine(2)
    e.render(2)
    b0, l0 = e.device_bytes(), e.launches()
    eq = e.equalizer(64, 8, RATE)
    e.equalizer(3, 1, RATE)   # left to the engine
    eq.set(band_list(8, 9))
    assert e.device_bytes() == b0
    x = torch.zeros((64, 256), dtype=torch.float32, device="cuda")
    o = [torch.zeros((64, 256), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    call = lambda **kw: eq.process_device(x.data_ptr(), x.data_ptr(), 256, kw.pop("frames", 256), o[0].data_ptr(), o[1].data_ptr(),
                                          256, **kw)
    eq.timing(True)
    for _ in range(3):
        call()
    call(frames=0)
    call(counts=np.zeros(64, np.uint32))
    e.synchronize()
    ms, k = eq.timing()
    assert k == 3 and ms > 0.0
    eq.timing(False)
    call()
    assert eq.timing() == (0.0, 0)
    assert e.device_bytes() == b0 and e.launches() == l0
    e.close()
