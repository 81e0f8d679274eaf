"""The loudness meter on the GPU (tbf_loudness_*, k_loud): identity in bits of every hop energy with
the host restatement of the definition (tbf_debug_loudness_ref) at every layout the kernel takes,
rows streaming at their own positions, reset and isolation, two meters on one engine, the
refusals, the render -> measure -> normalise -> measure chain, and the accounting.

The stage is this project's own definition (include/tbf.h); the restatement
against the plain-Python model, the order of the operations, the compliance figures and the gating
are checked without a GPU (tests/test_loudness_cpu.py).  The rate is 8000 wherever the stage stands
alone, so that hops of 800 frames fall inside small calls."""
import ctypes as C

import numpy as np
import pytest

import loudness_model as M
import scenarios as S

pytestmark = pytest.mark.gpu

TONEGEN = 1
FILL = 777.0
RATE = 8000
HP = RATE // 10
bits = M.bits


def same(a, b, what):
    a, b = bits(a), bits(b)
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


class Ref:
    """the rows of a meter on the host: loudness_ref per row, the states and energies carried"""

    def __init__(self, n, rate=RATE):
        self.n, self.rate = n, rate
        self.state = [None] * n
        self.e = [np.zeros((0, 2)) for _ in range(n)]
        self.pos = np.zeros(n, np.int64)

    def reset(self, rows=None):
        for r in (range(self.n) if rows is None else rows):
            self.state[r], self.e[r], self.pos[r] = None, np.zeros((0, 2)), 0

    def call(self, L, R, counts=None):
        import tunebfree_amd as T
        for r in range(self.n):
            c = L.shape[1] if counts is None else int(counts[r])
            e, self.state[r] = T.Engine.loudness_ref(L[r, :c], L[r, :c] if R is L else R[r, :c], self.rate, state=self.state[r])
            self.e[r] = np.concatenate([self.e[r], e])
            self.pos[r] += c


def measure(lm, L, R, aligned=True, counts=None):
    """one tbf_loudness_device call in torch memory: aligned -- every row 16-byte aligned, even
    strides; otherwise everything one float into its allocation with odd strides.  R is L: one
    plane passed twice.  Asserts that the call left the planes, pads included, as they were."""
    import torch
    n, frames = L.shape
    lead = 0 if aligned else 1
    stride = (frames + 3) // 4 * 4 + (0 if aligned else 1)
    host, dev = [], []
    for src in ((L,) if R is L else (L, R)):
        a = np.full(lead + n * stride + 4, FILL, np.float32)
        a[lead:lead + n * stride].reshape(n, stride)[:, :frames] = src
        host.append(a)
        dev.append(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 for t in dev)
    ptr = [t.data_ptr() + 4 * lead for t in dev]
    lm.measure_device(ptr[0], ptr[-1], stride, frames, counts=counts)
    torch.cuda.synchronize()
    for a, t in zip(host, dev):
        assert a.tobytes() == t.cpu().numpy().tobytes(), "the meter wrote into its input"


def hops_guarded(lm, row, cap):
    """tbf_loudness_hops into a buffer of cap pairs with guard words before and behind"""
    buf = np.full(2 * cap + 8, -5.0)
    n = C.c_uint32()
    rc = lm._lib.tbf_loudness_hops(lm._h, row, buf[4:].ctypes.data, cap, C.byref(n))
    assert rc == 0, rc
    assert (buf[:4] == -5.0).all() and (buf[4 + 2 * n.value:] == -5.0).all(), "hops written outside [0, n_hops)"
    return buf[4:4 + 2 * n.value].reshape(-1, 2).copy()


def read_guarded(lm, rows=None):
    k = lm.n_rows if rows is None else len(rows)
    buf = np.zeros(k + 2, M.RESULT_DTYPE)
    raw = buf.view(np.uint8).reshape(k + 2, 40)
    raw[0], raw[-1] = 0xA5, 0xA5
    r = None if rows is None else np.ascontiguousarray(rows, np.uint32)
    rc = lm._lib.tbf_loudness_read(lm._h, 0 if r is None else len(r), None if r is None else r.ctypes.data, buf[1:].ctypes.data)
    assert rc == 0, rc
    assert (raw[0] == 0xA5).all() and (raw[-1] == 0xA5).all(), "results written outside the rows asked for"
    return buf[1:-1].copy()


def check(lm, ref, what, rows=None):
    """every row's hop energies and position against the reference, in bits"""
    res = read_guarded(lm)
    for r in (range(ref.n) if rows is None else rows):
        same(hops_guarded(lm, r, lm.max_hops), ref.e[r], f"{what}: row {r} hop energies against loudness_ref")
        assert res["hops"][r] == len(ref.e[r]) == ref.pos[r] // (ref.rate // 10), (what, r)


def check_results(lm, ref, what):
    import tunebfree_amd as T
    got = lm.read()
    for r in range(ref.n):
        want = T.Engine.loudness_result(ref.rate, ref.e[r])
        for f in ("integrated", "momentary_max", "short_term_max"):
            assert got[f][r] == want[f] or abs(got[f][r] - want[f]) <= 1e-9, (what, r, f, got[f][r], want[f])
        for f in ("hops", "blocks", "gated"):
            assert got[f][r] == want[f], (what, r, f)


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


def grid():
    import tunebfree_amd as T
    return T.Engine.loudness_grid(1)


# ---------------------------------------------------------------- 1. layouts
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("rows", ["1", "rpg-1", "rpg", "rpg+1", "70"])
def test_gpu_loudness_layouts_against_ref(eng, rows, aligned):
    """row counts around a workgroup's rows, frame counts around the wave, the LDS tile and the hop,
    with and without counts (0, 1, partial and full, NaN behind each), and one call with d_L == d_R;
    the calls follow each other on one meter, so every one but the first starts from a state"""
    rpg, tile, lds = grid()
    assert rpg >= 2 and tile >= 8 and lds <= 160 * 1024
    n = {"1": 1, "rpg-1": rpg - 1, "rpg": rpg, "rpg+1": rpg + 1, "70": 70}[rows]
    lm, ref = eng.loudness(n, RATE, max_hops=16), Ref(n)
    for k, frames in enumerate([1, 63, 65, tile - 1, tile, tile + 1, 2 * tile + 5, 4 * HP + 3]):
        L, R = M.noise(100 + k, frames, n), M.noise(200 + k, frames, n)
        what = f"rows={n} aligned={aligned} frames={frames}"
        measure(lm, L, R, aligned)
        ref.call(L, R)
        c = counts_for(n, frames, 300 + k)
        Ln, Rn = with_nan_beyond(L, c), with_nan_beyond(R, c)
        measure(lm, Ln, Rn, aligned, c)
        ref.call(Ln, Rn, c)
        if frames == 65:
            measure(lm, L, L, aligned)
            ref.call(L, L)
        check(lm, ref, what)
    assert min(len(e) for e in ref.e) >= 4 and all(np.isfinite(e).all() for e in ref.e)
    check_results(lm, ref, f"rows={n}")
    lm.close()


def test_gpu_loudness_equal_channels(eng):
    """d_L == d_R from the first frame: both channels' energies are equal and are those of the
    restatement"""
    n = 5
    lm, ref = eng.loudness(n, RATE, max_hops=8), Ref(n)
    L = M.noise(7, 2 * HP + 9, n)
    measure(lm, L, L)
    ref.call(L, L)
    check(lm, ref, "equal channels")
    e = lm.hops(3)
    assert e.shape == (2, 2)
    same(e[:, 0], e[:, 1], "EL against ER")
    lm.close()


# ---------------------------------------------------------------- 2. streaming
def test_gpu_loudness_rows_stream_at_their_own_positions(eng):
    """12 rows take random counts over 10 calls: the energies, the positions and the read-out are
    those of one loudness_ref run per row over its own frames"""
    import tunebfree_amd as T
    n, calls = 12, 10
    lm, ref = eng.loudness(n, RATE, max_hops=20), Ref(n)
    rng = np.random.default_rng(43)
    rowsL, rowsR = [[] for _ in range(n)], [[] for _ in range(n)]
    for k in range(calls):
        frames = int(rng.integers(300, 1500))
        counts = rng.integers(0, frames + 1, n).astype(np.uint32)
        counts[k % n], counts[(k + 1) % n] = frames, 0
        L, R = with_nan_beyond(M.noise(500 + k, frames, n), counts), with_nan_beyond(M.noise(600 + k, frames, n), counts)
        measure(lm, L, R, aligned=bool(k % 2), counts=counts)
        ref.call(L, R, counts)
        for r in range(n):
            rowsL[r].append(L[r, :counts[r]]), rowsR[r].append(R[r, :counts[r]])
    check(lm, ref, "streaming")
    check_results(lm, ref, "streaming")
    assert len(set(ref.pos.tolist())) > 6 and sum(len(e) >= 4 for e in ref.e) >= 10   # with and without a block
    for r in range(n):   # the reference's own cuts moved nothing either
        one, _ = T.Engine.loudness_ref(np.concatenate(rowsL[r]), np.concatenate(rowsR[r]), RATE)
        same(lm.hops(r), one, f"row {r}: joined against one loudness_ref run")
    lm.close()


# ---------------------------------------------------------------- 3. reset and isolation
def test_gpu_loudness_reset_nan_and_two_meters(eng):
    """rows {1, 5} reset mid-stream start anew and the others go on; a NaN row stays NaN until it is
    reset and leaves its neighbours clean; a second meter at another rate goes its own way"""
    n, frames = 8, HP + 300
    a, b = eng.loudness(n, RATE, max_hops=12), eng.loudness(n, 16000, max_hops=6)
    ra, rb = Ref(n), Ref(n, 16000)
    for k in range(5):
        L, R = M.noise(60 + k, frames, n), M.noise(70 + k, frames, n)
        if k == 1:
            L[3, 17] = np.nan           # row 3, channel L, from its second hop on
        if k == 2:
            a.reset([1, 5])
            ra.reset([1, 5])
        if k == 3:
            a.reset([3])
            ra.reset([3])
        measure(a, L, R, aligned=bool(k % 2))
        ra.call(L, R)
        measure(b, L, R)
        rb.call(L, R)
        check(a, ra, f"meter a, call {k}")
        check(b, rb, f"meter b, call {k}")
        if k == 2:
            e3 = a.hops(3)
            assert np.isfinite(e3[0]).all() and np.isnan(e3[1:, 0]).all() and np.isfinite(e3[:, 1]).all()
            for r in (0, 2, 4, 6, 7):
                assert np.isfinite(a.hops(r)).all(), f"row {r} beside the NaN row"
            assert [len(x) for x in ra.e] == [4, 1, 4, 4, 4, 1, 4, 4]
    assert np.isfinite(a.hops(3)).all() and len(a.hops(3)) == 2     # clean again since its reset
    with pytest.raises(Exception, match=r"-22.*rows\[1\]"):
        a.reset([0, n])
    a.reset()
    ra.reset()
    L, R = M.noise(91, frames, n), M.noise(92, frames, n)
    measure(a, L, R)
    ra.call(L, R)
    check(a, ra, "after a reset of all rows")
    a.close(), b.close()


def test_gpu_loudness_meters_destroyed_and_left_to_the_engine():
    import torch
    e = engine()
    x = torch.from_numpy(M.noise(5, HP + 1, 3)).cuda()
    torch.cuda.synchronize()
    kept, gone = e.loudness(3, RATE, max_hops=4), e.loudness(3, RATE, max_hops=4)
    for lm in (kept, gone):
        lm.measure_device(x.data_ptr(), x.data_ptr(), HP + 1, HP + 1)
    want = kept.hops(1)
    same(gone.hops(1), want, "two meters on the same planes")
    gone.close()
    gone.close()                                # a second close is nothing
    kept.measure_device(x.data_ptr(), x.data_ptr(), HP + 1, HP - 1)
    assert len(kept.hops(1)) == 2
    same(kept.hops(1)[:1], want, "the kept meter after the other's destruction")
    e.close()                                   # releases `kept`
    kept.close()


# ---------------------------------------------------------------- 4. refusals
def test_gpu_loudness_refusals_move_no_state(eng):
    """a call that would exceed max_hops is -28, every bad argument is -22, and a valid call behind
    them gives the bits of a stream that never saw them"""
    import torch
    import tunebfree_amd as T
    n, frames = 4, HP + 100
    lm, ref = eng.loudness(n, RATE, max_hops=3), Ref(n)
    L, R = M.noise(81, frames, n), M.noise(82, frames, n)
    measure(lm, L, R)
    ref.call(L, R)
    stride = frames + 4
    x = [torch.from_numpy(np.ascontiguousarray(np.pad(a, ((0, 0), (0, 4))))).cuda() for a in (L, R)]
    torch.cuda.synchronize()
    xl, xr = x[0].data_ptr(), x[1].data_ptr()
    good = dict(L_ptr=xl, R_ptr=xr, in_stride=stride, frames=frames, counts=None)
    over = np.full(n, frames, np.uint32)
    over[2] = frames + 1
    bad = [
        (dict(L_ptr=None), "d_L"),
        (dict(R_ptr=None), "d_R"),
        (dict(in_stride=frames - 1), "in_stride"),
        (dict(L_ptr=xl + 2), "aligned"),
        (dict(R_ptr=xr + 1), "aligned"),
        (dict(counts=over), r"counts\[2\]"),
    ]
    for kw, word in bad:
        with pytest.raises(T.TbfError, match="-22.*" + word):
            lm.measure_device(**{**good, **kw})
    with pytest.raises(T.TbfError, match=r"-22.*rows\[1\]"):
        lm.reset([0, n])
    with pytest.raises(T.TbfError, match=r"-22.*rows\[0\]"):
        lm.read([n])
    with pytest.raises(T.TbfError, match=r"-22.*row"):
        lm.hops(n)
    # rows stand at 900 of 2400 frames: 1500 more complete the third hop, 2300 a fourth for row 1 alone
    c = np.array([1500, 2300, 0, 100], np.uint32)
    big = torch.zeros((n, 2300), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(T.TbfError, match=r"-28.*row 1.*max_hops"):
        lm.measure_device(big.data_ptr(), big.data_ptr(), 2300, 2300, counts=c)
    with pytest.raises(T.TbfError, match="-28"):
        lm.measure_device(big.data_ptr(), big.data_ptr(), 2300, 2300)
    check(lm, ref, "behind the refusals")
    same(x[0].cpu().numpy()[:, :frames], L, "the input after the refusals")
    L2, R2 = M.noise(83, 1500, n), M.noise(84, 1500, n)
    c2 = np.array([1500, 1400, 0, 100], np.uint32)
    measure(lm, L2, R2, counts=c2)     # row 0 now holds exactly max_hops hops
    ref.call(L2, R2, c2)
    check(lm, ref, "a valid call behind the refusals")
    assert [len(e) for e in ref.e] == [3, 2, 1, 1]
    with pytest.raises(T.TbfError, match=r"-28.*row 0"):
        lm.measure_device(big.data_ptr(), big.data_ptr(), 2300, HP)
    lm.reset([0])
    ref.reset([0])
    c3 = np.array([HP, 0, 0, 0], np.uint32)
    measure(lm, L2[:, :HP], R2[:, :HP], counts=c3)
    ref.call(L2[:, :HP], R2[:, :HP], c3)
    check(lm, ref, "a full row after its reset")
    # tbf_loudness_hops with too small a cap: -28, the count reported, nothing else written
    buf, k = np.full(8, -5.0), C.c_uint32()
    assert lm._lib.tbf_loudness_hops(lm._h, 1, buf.ctypes.data, 1, C.byref(k)) == -28
    assert k.value == 2 and (buf == -5.0).all()
    lm.close()


# ---------------------------------------------------------------- 5. the chain
def test_gpu_loudness_measure_normalise_measure():
    """16 tone generators holding chords at different drawbars, mixed to 2 buses over 1.5 s at
    48 kHz: the meter on the bus planes is loudness_ref of those planes, which are those of a twin
    engine without a meter; the gains of gains(-23) applied through mix_device give planes that are
    gain * x in bits and that a second meter reads at -23 LUFS"""
    import torch
    import tunebfree_amd as T
    n, buses, nb = 16, 2, 563
    frames = nb * 128
    assert frames >= 72000
    bus = np.arange(n) % buses

    def render(metered):
        e = engine(n, TONEGEN)
        for i in range(n):
            for (_b, kind, x, v) in S.bench_scenario(i):
                (e.note if kind == "note" else e.set_param)(i, x, v)
            for j in range(9):   # a registration of its own per instance
                e.set_param(i, S.P_DRAWBAR + j, (3 * i + 5 * j) % 9)
        mix = [torch.full((buses, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        lm = e.loudness(buses, max_hops=32) if metered else None
        e.render_mix_device(nb, T.params.mix_rows(bus, 0.05), buses, mix[0].data_ptr(), mix[1].data_ptr(), frames)
        if metered:
            lm.measure_device(mix[0].data_ptr(), mix[1].data_ptr(), frames, frames)   # on the same stream
        e.synchronize()
        return e, lm, mix

    e, lm, mix = render(True)
    assert lm.rate_hz == 48000
    planes = [t.cpu().numpy().copy() for t in mix]
    assert np.isfinite(planes[0]).all() and float(np.abs(planes[0]).max()) > 1e-3
    res = lm.read()
    for b in range(buses):
        want, _ = T.Engine.loudness_ref(planes[0][b], planes[1][b], 48000)
        got = lm.hops(b)
        assert len(got) == frames // 4800 == 15
        same(got, want, f"bus {b}: the meter against loudness_ref of the mix planes")
        r = T.Engine.loudness_result(48000, want)
        assert abs(res["integrated"][b] - r["integrated"]) <= 1e-9 and res["gated"][b] == r["gated"] > 0
        # no block within 0.01 LU of either gate, so that a gain moves none across
        u = want[:, 0] + want[:, 1]
        z = (((u[:-3] + u[1:-2]) + u[2:-1]) + u[3:]) / (4.0 * 4800)
        l = -0.691 + 10.0 * np.log10(z)
        za = z[l > -70.0]
        gate = -0.691 + 10.0 * np.log10(za.sum() / len(za)) - 10.0
        print(f"bus {b}: integrated {res['integrated'][b]:.4f} LUFS, blocks {np.round(l, 3).tolist()}, relative gate {gate:.4f}")
        assert np.abs(l + 70.0).min() > 0.01 and np.abs(l - gate).min() > 0.01
    gains = lm.gains(-23.0)
    assert gains.dtype == np.float32
    for b in range(buses):
        assert gains[b] == np.float32(10.0 ** ((-23.0 - res["integrated"][b]) / 20.0))
    rows = T.params.gain_rows(gains)
    assert rows["bus"].tolist() == [0, 1] and (rows["ll"] == gains).all() and (rows["rr"] == gains).all()
    assert not rows["lr"].any() and not rows["rl"].any()
    out = [torch.full((buses, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    e.mix_device(buses, mix[0].data_ptr(), mix[1].data_ptr(), frames, frames, rows, buses, out[0].data_ptr(), out[1].data_ptr(), frames)
    lm2 = e.loudness(buses, max_hops=32)
    lm2.measure_device(out[0].data_ptr(), out[1].data_ptr(), frames, frames)
    after = lm2.read()
    norm = [t.cpu().numpy().copy() for t in out]
    for b in range(buses):
        g = np.float32(gains[b])
        same(norm[0][b].astype(np.float64), (g * planes[0][b]).astype(np.float64), f"bus {b}: normalised L against gain * x")
        same(norm[1][b].astype(np.float64), (g * planes[1][b]).astype(np.float64), f"bus {b}: normalised R against gain * x")
        print(f"bus {b}: gain {g}, after {after['integrated'][b]:.7f} LUFS")
        assert abs(after["integrated"][b] + 23.0) <= 1e-4
        assert after["gated"][b] == res["gated"][b] and after["blocks"][b] == res["blocks"][b] == 12
    e.close()
    e2, _, twin = render(False)
    same(twin[0].cpu().numpy(), planes[0], "mix planes with and without a meter, L")
    same(twin[1].cpu().numpy(), planes[1], "mix planes with and without a meter, R")
    e2.close()


# ---------------------------------------------------------------- 6. accounting
def test_gpu_loudness_accounting():
    """a meter is no instance or stage memory of the engine, a call that takes frames is one launch
    set and one that takes none is none, and the render kernels' launch counts do not move"""
    import torch
    e = engine(2)
    e.render(2)
    b0, l0 = e.device_bytes(), e.launches()
    lm = e.loudness(64, RATE, max_hops=4096)
    e.loudness(3, 192000, max_hops=1)   # left to the engine
    assert e.device_bytes() == b0
    x = torch.zeros((64, 256), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lm.timing(True)
    for _ in range(3):
        lm.measure_device(x.data_ptr(), x.data_ptr(), 256, 256)
    lm.measure_device(x.data_ptr(), x.data_ptr(), 256, 256, counts=np.zeros(64, np.uint32))
    lm.measure_device(x.data_ptr(), x.data_ptr(), 256, 0)
    e.synchronize()
    ms, k = lm.timing()
    assert k == 3 and ms > 0.0
    lm.timing(False)
    lm.measure_device(x.data_ptr(), x.data_ptr(), 256, 256)
    assert lm.timing() == (0.0, 0)
    assert lm.read()["hops"].tolist() == [1] * 64          # 1024 frames of 800
    assert e.device_bytes() == b0 and e.launches() == l0
    e.close()
