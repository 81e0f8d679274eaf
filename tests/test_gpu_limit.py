"""The bus limiter on the GPU (tbf_limiter_*, tbf_limit_device, k_limit): identity in bits with the
host restatement of the definition (tbf_debug_limit_ref) at every layout the kernel takes, rows
streaming at different positions, reset, two limiters on one engine, the mix -> limit -> PCM
chain, the refusals and the accounting.

The stage is this project's own definition (include/tbf.h); the restatement
against the numpy model, the order of the sum and the literal cases are checked without a GPU
(tests/test_limit_cpu.py).  Everything here is an identity in bits."""
import numpy as np
import pytest

import limit_model as M
import scenarios as S

pytestmark = pytest.mark.gpu

TONEGEN = 1
FILL = 777.0
CEIL = M.CEILING
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
    """the rows of a limiter on the host: limit_ref per row, the histories carried"""

    def __init__(self, n, A, H, ceiling=CEIL):
        self.n, self.cfg, self.hist = n, (ceiling, A, H), [None] * n

    def reset(self, rows=None):
        for r in (range(self.n) if rows is None else rows):
            self.hist[r] = None

    def call(self, L, R, counts=None):
        """the rows' outputs (lists of [count] arrays) and their meters"""
        import tunebfree_amd as T
        oL, oR, met = [], [], np.zeros(self.n, M.METER_DTYPE)
        for r in range(self.n):
            c = L.shape[1] if counts is None else int(counts[r])
            a, b, met[r], self.hist[r] = T.Engine.limit_ref(L[r, :c], L[r, :c] if R is L else R[r, :c], *self.cfg,
                                                            hist=self.hist[r])
            oL.append(a), oR.append(b)
        return oL, oR, met


def stage_call(lim, L, R, aligned=True, counts=None, meters=True, out_fill=FILL):
    """one tbf_limit_device call in torch memory: aligned -- every row 16-byte aligned, even
    strides; otherwise everything one float into its allocation with odd strides.  Guard floats
    lie before, between and behind the output rows, and two guard records behind the meters.
    R is L: mono, one plane passed twice.  Returns the output bodies [n, frames] and the meters."""
    import torch
    n, frames = L.shape
    mono = R is L
    lead = 0 if aligned else 1
    istride = (frames + 3) // 4 * 4 + (0 if aligned else 1)
    ostride = (frames + 3) // 4 * 4 + (8 if aligned else 5)
    olead = 4 if aligned else 5
    dev = []
    for src in ((L,) if mono else (L, R)):
        a = np.full(lead + n * istride + 4, FILL, np.float32)
        a[lead:lead + n * istride].reshape(n, istride)[:, :frames] = src
        dev.append(torch.from_numpy(a).cuda())
    outs = [torch.full((olead + n * ostride,), out_fill, dtype=torch.float32, device="cuda") for _ in range(2)]
    met = torch.full(((n + 2) * 3,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 for t in dev + outs)
    ptr = [t.data_ptr() + 4 * lead for t in dev]
    lim.process_device(ptr[0], ptr[-1], istride, frames, outs[0].data_ptr() + 4 * olead, outs[1].data_ptr() + 4 * olead,
                       ostride, counts=counts, meters_ptr=met.data_ptr() if meters else None)
    torch.cuda.synchronize()
    got = []
    for o, ch in zip(outs, "LR"):
        a = o.cpu().numpy()
        assert (a[:olead] == out_fill).all(), f"written before {ch}"
        body = a[olead:].reshape(n, ostride)
        for r in range(n):
            c = frames if counts is None else int(counts[r])
            assert (body[r, c:] == out_fill).all(), f"written behind row {r} of {ch}"
        got.append(body[:, :frames].copy())
    m = met.cpu().numpy()
    assert (m[3 * n:] == -1).all(), "meters written beyond n_rows"
    if not meters:
        assert (m == -1).all()
    return got[0], got[1], m[:3 * n].copy().view(M.METER_DTYPE)


def check_call(lim, ref, L, R, what, aligned=True, counts=None):
    gL, gR, gm = stage_call(lim, L, R, aligned, counts)
    wL, wR, wm = ref.call(L, R, counts)
    for r in range(L.shape[0]):
        c = len(wL[r])
        same(gL[r, :c], wL[r], f"{what}: L[{r}] against limit_ref")
        same(gR[r, :c], wR[r], f"{what}: R[{r}] against limit_ref")
    assert gm.tobytes() == wm.tobytes(), f"{what}: meters {gm} against {wm}"
    return gL, gR, gm


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


# ---------------------------------------------------------------- 1. the stage alone
@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("A,H", [(2, 0), (64, 0), (64, 200), (512, 4096)])
def test_gpu_limit_stage_against_ref(eng, A, H, aligned):
    """37 rows at frame counts around the lane group, the wave and the tile, with and without
    counts (0, 1, partial and full, NaN beyond each), and one mono call; the calls follow each
    other on one limiter, so every one but the first starts from a history, and with (512, 4096)
    the halo is longer than most calls and than a tile"""
    import tunebfree_amd as T
    n = 37
    group, tile, hn, lds = T.Engine.limit_grid(CEIL, A, H)
    assert hn == M.history(A, H) and tile % (64 * group) == 0
    if (A, H) == (512, 4096):
        assert hn > tile
    lim, ref = eng.limiter(n, CEIL, A, H), Ref(n, A, H)
    assert lim.latency == A - 1 and lim.history == hn
    reduced = clamped = 0
    for k, frames in enumerate([1, 63, 65, tile - 1, tile, tile + 1, 2 * tile + 5]):
        L, R = M.issue_input(100 + k, frames, n), M.issue_input(200 + k, frames, n)
        what = f"A={A} H={H} aligned={aligned} frames={frames}"
        _, _, gm = check_call(lim, ref, L, R, what, aligned)
        reduced, clamped = reduced + int(gm["reduced"].sum()), clamped + int(gm["clamped"].sum())
        c = counts_for(n, frames, 300 + k)
        check_call(lim, ref, with_nan_beyond(L, c), with_nan_beyond(R, c), what + " counts", aligned, c)
        if frames == 65:
            gL, gR, _ = check_call(lim, ref, L, L, what + " mono", aligned)
            D = A - 1   # the first D frames are the delayed history, which was not mono
            same(gL[:, min(D, frames):], gR[:, min(D, frames):], what + " mono: L against R")
    assert reduced > 0
    print(f"A={A} H={H}: reduced {reduced}, clamped {clamped}")
    lim.close()


def test_gpu_limit_without_meters_and_empty_calls(eng):
    """a call without meters writes none; a call of frames == 0, or with every count 0, moves no
    state and sets the meters to those of empty rows"""
    n, A, H = 5, 16, 5
    lim, ref = eng.limiter(n, CEIL, A, H), Ref(n, A, H)
    L, R = M.issue_input(1, 200, n), M.issue_input(2, 200, n)
    gL, gR, _ = stage_call(lim, L, R, meters=False)
    wL, wR, _ = ref.call(L, R)
    same(gL, np.stack(wL), "no meters: L")
    same(gR, np.stack(wR), "no meters: R")
    zero = np.zeros(n, np.uint32)
    for LL, cc in ((L[:, :0], None), (L, zero)):
        _, _, gm = stage_call(lim, LL, LL.copy(), counts=cc)
        assert (gm["min_gain"] == 1.0).all() and not gm["reduced"].any() and not gm["clamped"].any()
    check_call(lim, ref, L, R, "after the empty calls")
    lim.close()
    mono, mref = eng.limiter(n, CEIL, A, H), Ref(n, A, H)   # mono from its first frame: both outputs are equal
    for k in range(2):
        gL, gR, _ = check_call(mono, mref, L, L, f"mono call {k}", aligned=bool(k))
        same(gL, gR, f"mono call {k}: L against R")
    mono.close()


# ---------------------------------------------------------------- 2. streaming
def test_gpu_limit_rows_stream_at_their_own_positions(eng):
    """12 rows of 2600 frames each, taken in calls of 1, 5, D and Hn + 3 frames and the rest, each
    row with its own count per call: the outputs joined per row are one limit_ref run"""
    import tunebfree_amd as T
    n, total, A, H = 12, 2600, 64, 200
    D, Hn = A - 1, M.history(A, H)
    lim = eng.limiter(n, CEIL, A, H)
    L, R = M.issue_input(41, total, n), M.issue_input(42, total, n)
    one = [T.Engine.limit_ref(L[r], R[r], CEIL, A, H) for r in range(n)]
    rng = np.random.default_rng(43)
    at = np.zeros(n, np.int64)
    gotL, gotR = [[] for _ in range(n)], [[] for _ in range(n)]
    sizes = [1, 5, D, Hn + 3, None, None]
    for k, frames in enumerate(sizes):
        left = total - at
        if frames is None:   # the rest: in two calls, so that the last one starts at different positions too
            frames = int(left.max())
            counts = left // 2 if k == len(sizes) - 2 else left
        else:
            counts = rng.integers(0, frames + 1, n)
            counts[k % n], counts[(k + 1) % n] = frames, 0
        counts = np.minimum(counts, left).astype(np.uint32)
        cl = np.full((n, frames), np.nan, np.float32)
        cr = cl.copy()
        for r in range(n):
            cl[r, :counts[r]], cr[r, :counts[r]] = L[r, at[r]:at[r] + counts[r]], R[r, at[r]:at[r] + counts[r]]
        gL, gR, _ = stage_call(lim, cl, cr, aligned=bool(k % 2), counts=counts)
        for r in range(n):
            gotL[r].append(gL[r, :counts[r]]), gotR[r].append(gR[r, :counts[r]])
        at += counts
    assert (at == total).all() and len(set(int(a) for a in (total - left))) > 1
    for r in range(n):
        same(np.concatenate(gotL[r]), one[r][0], f"row {r}: L joined against one limit_ref run")
        same(np.concatenate(gotR[r]), one[r][1], f"row {r}: R joined against one limit_ref run")
    lim.close()


# ---------------------------------------------------------------- 3. reset, two limiters
def test_gpu_limit_reset_and_two_limiters(eng):
    """rows {1, 5} reset mid-stream behave as new and the others are undisturbed; a second limiter
    of another configuration on the same engine goes its own way"""
    n, frames = 8, 300
    a, b = eng.limiter(n, CEIL, 16, 5), eng.limiter(n, np.float32(0.5), 64, 0)
    ra, rb = Ref(n, 16, 5), Ref(n, 64, 0, np.float32(0.5))
    assert (a.latency, b.latency) == (15, 63)
    for k in range(3):
        L, R = M.issue_input(60 + k, frames, n), M.issue_input(70 + k, frames, n)
        if k == 1:
            a.reset([1, 5])
            ra.reset([1, 5])
        if k == 2:
            a.reset()
            ra.reset()
        ga = check_call(a, ra, L, R, f"limiter a, call {k}")
        check_call(b, rb, L, R, f"limiter b, call {k}")
        if k:   # a reset row equals a new row's output
            fresh = Ref(n, 16, 5).call(L, R)
            for r in ([1, 5] if k == 1 else range(n)):
                same(ga[0][r], fresh[0][r], f"call {k}: reset row {r} against a new row")
            if k == 1:
                assert any(not np.array_equal(bits(ga[0][r]), bits(fresh[0][r])) for r in (0, 2, 3, 4, 6, 7))
    with pytest.raises(Exception, match="rows"):
        a.reset([0, n])
    a.close(), b.close()


# ---------------------------------------------------------------- 4. composition
def test_gpu_limit_between_mix_and_pcm():
    """16 tone generators with a held chord mixed into 2 buses at a bus peak of about 4: the
    unlimited S16 frames clip; limited at 1 - 2^-15 the planes are limit_ref of the mix planes, no
    frame clips and the peak is within the ceiling; and the mix planes are those of a twin engine
    that has no limiter"""
    import torch
    import tunebfree_amd as T
    n, nb, buses = 16, 6, 2
    frames = nb * 128
    bus = np.arange(n) % buses

    def chain(limited):
        e = engine(n, TONEGEN)
        for i in range(n):
            for (_b, kind, x, v) in S.bench_scenario(i):
                (e.note if kind == "note" else e.set_param)(i, x, v)
        mix = [torch.full((buses, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
        pcm = torch.zeros((buses, frames * 4), dtype=torch.uint8, device="cuda")
        met = torch.zeros((buses * 4,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def mix_pcm(gain, src=None):
            if src is None:
                e.render_mix_device(nb, T.params.mix_rows(bus, gain), buses, mix[0].data_ptr(), mix[1].data_ptr(), frames)
                src = mix
            e.pcm_convert_device(buses, src[0].data_ptr(), src[1].data_ptr(), frames, frames, pcm.data_ptr(), frames * 4,
                                 T.engine.PCM_S16, meters_ptr=met.data_ptr())
            e.synchronize()
            return met.cpu().numpy().view(T.engine.METER_DTYPE).copy()

        warm = mix_pcm(1.0)   # the notes' onset, louder than the held chord behind it
        m0 = mix_pcm(1.0)
        p0 = float(max(m0["peakL"].max(), m0["peakR"].max()))
        print(f"unscaled bus peak: onset {float(max(warm['peakL'].max(), warm['peakR'].max()))}, held {p0}")
        assert p0 > 0.0
        m1 = mix_pcm(4.0 / p0)
        planes = [t.cpu().numpy().copy() for t in mix]
        if not limited:
            e.close()
            return planes, m1, None, None
        lim = e.limiter(buses, CEIL, 64, 32)
        out = [torch.full((buses, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        lim.process_device(mix[0].data_ptr(), mix[1].data_ptr(), frames, frames, out[0].data_ptr(), out[1].data_ptr(), frames)
        m2 = mix_pcm(None, out)   # on the same stream, no synchronize in between
        res = [t.cpu().numpy().copy() for t in out]
        e.close()
        return planes, m1, res, m2

    planes, unlimited, got, limited = chain(True)
    peak = max(float(np.abs(planes[0]).max()), float(np.abs(planes[1]).max()))
    print(f"bus peak {peak}, unlimited clips {unlimited['clipL'].tolist()} {unlimited['clipR'].tolist()}")
    assert 1.5 < peak < 10.0
    assert int(unlimited["clipL"].sum() + unlimited["clipR"].sum()) > 0
    for b in range(buses):
        wL, wR, wm, _ = T.Engine.limit_ref(planes[0][b], planes[1][b], CEIL, 64, 32)
        same(got[0][b], wL, f"bus {b}: limited L against limit_ref of the mix plane")
        same(got[1][b], wR, f"bus {b}: limited R against limit_ref of the mix plane")
        assert wm["reduced"] > 0
    assert not limited["clipL"].any() and not limited["clipR"].any()
    assert float(limited["peakL"].max()) <= CEIL and float(limited["peakR"].max()) <= CEIL
    assert float(limited["peakL"].max()) > 0.5
    twin, twin_m, _, _ = chain(False)
    same(planes[0], twin[0], "mix planes with and without a limiter, L")
    same(planes[1], twin[1], "mix planes with and without a limiter, R")
    assert twin_m.tobytes() == unlimited.tobytes()


# ---------------------------------------------------------------- 5. refusals
def test_gpu_limit_refusals_write_nothing_and_move_no_state(eng):
    import torch
    import tunebfree_amd as T
    n, frames, A, H = 4, 96, 16, 5
    lim, ref = eng.limiter(n, CEIL, A, H), Ref(n, A, H)
    L, R = M.issue_input(81, frames, n), M.issue_input(82, frames, n)
    check_call(lim, ref, L, R, "before the refusals")
    stride = frames + 4
    x = [torch.from_numpy(np.ascontiguousarray(np.pad(a, ((0, 0), (0, 4))))).cuda() for a in (L, R)]
    o = [torch.full((n, stride), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    met = torch.full((n * 3,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    xl, xr, ol, orr, mp = x[0].data_ptr(), x[1].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), met.data_ptr()
    good = dict(L_ptr=xl, R_ptr=xr, in_stride=stride, frames=frames, outL_ptr=ol, outR_ptr=orr, out_stride=stride,
                counts=None, meters_ptr=mp)
    over = np.full(n, frames, np.uint32)
    over[2] = frames + 1
    bad = [
        (dict(L_ptr=None), "d_L"),
        (dict(R_ptr=None), "d_R"),
        (dict(outL_ptr=None), "out->L"),
        (dict(outR_ptr=None), "out->R"),
        (dict(in_stride=frames - 1), "in_stride"),
        (dict(out_stride=frames - 1), "out stride"),
        (dict(L_ptr=xl + 2), "aligned"),
        (dict(outR_ptr=orr + 2), "aligned"),
        (dict(meters_ptr=mp + 2), "aligned"),
        (dict(counts=over), r"counts\[2\]"),
        (dict(outL_ptr=xl), "overlap"),                      # in place
        (dict(outR_ptr=xr + 4 * (stride * (n - 1) + frames - 1)), "overlap"),   # one float of the input's last row
        (dict(outR_ptr=ol + 4 * 8), "overlap"),              # the two outputs
        (dict(meters_ptr=ol + 4 * stride), "overlap"),       # the meters inside an output plane
        (dict(meters_ptr=xr), "overlap"),                    # the meters on the input
    ]
    for kw, word in bad:
        with pytest.raises(T.TbfError, match="-22.*" + word):
            lim.process_device(**{**good, **kw})
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in o) and (met.cpu().numpy() == -1).all()
    same(x[0].cpu().numpy()[:, :frames], L, "the input after the refusals")
    with pytest.raises(T.TbfError, match=r"-22.*rows\[1\]"):
        lim.reset([0, n])
    L2, R2 = M.issue_input(83, frames, n), M.issue_input(84, frames, n)
    check_call(lim, ref, L2, R2, "after the refusals")
    lim.close()


# ---------------------------------------------------------------- 6. accounting
def test_gpu_limit_accounting():
    """a limiter is no instance or stage memory of the engine, a call is one launch set, and the
    engine releases the limiters that are still alive when it closes"""
    import torch
    e = engine(2)
    e.render(2)
    b0, l0 = e.device_bytes(), e.launches()
    lim = e.limiter(64, CEIL, 512, 4096)
    e.limiter(3, CEIL, 2, 0)   # left to the engine
    assert e.device_bytes() == b0
    x = torch.zeros((64, 256), dtype=torch.float32, device="cuda")
    o = [torch.zeros((64, 256), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    lim.time(True)
    for _ in range(3):
        lim.process_device(x.data_ptr(), x.data_ptr(), 256, 256, o[0].data_ptr(), o[1].data_ptr(), 256)
    e.synchronize()
    ms, k = lim.time()
    assert k == 3 and ms > 0.0
    lim.time(False)
    lim.process_device(x.data_ptr(), x.data_ptr(), 256, 256, o[0].data_ptr(), o[1].data_ptr(), 256)
    assert lim.time() == (0.0, 0)
    assert e.device_bytes() == b0 and e.launches() == l0
    e.close()
