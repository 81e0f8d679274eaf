"""The bus limiter with a true-peak detector on the GPU (tbf_limiter_create_tp, k_limit_tp):
identity in bits with the host restatement (tbf_debug_limit_tp_ref) at every layout the kernel
takes, rows streaming at their own positions, reset, a plain and a true-peak limiter on one engine,
the limiter in front of the true-peak meter, the refusals and the accounting.

The definition against the numpy model, the literal cases and the derivation of the steady-state
bound are checked without a GPU (tests/test_limit_tp_cpu.py).  The call pattern with its guard
floats is that of tests/test_gpu_limit.py."""
import numpy as np
import pytest

import limit_model as LM
import limit_tp_model as M
import test_gpu_limit as G
import truepeak_model as TP

pytestmark = pytest.mark.gpu

CEIL = M.CEILING
FILL = G.FILL
bits, same = LM.bits, G.same


class Ref(G.Ref):
    """the rows of a true-peak limiter on the host: tbf_debug_limit_tp_ref per row, the histories carried"""

    def __init__(self, n, A, H, F, ceiling=CEIL):
        super().__init__(n, A, H, ceiling)
        self.F = F

    def call(self, L, R, counts=None):
        import tunebfree_amd as T
        oL, oR, met = [], [], np.zeros(self.n, LM.METER_DTYPE)
        for r in range(self.n):
            c = L.shape[1] if counts is None else int(counts[r])
            a, b, met[r], self.hist[r] = T.Engine.limit_ref(L[r, :c], L[r, :c] if R is L else R[r, :c], *self.cfg,
                                                            hist=self.hist[r], oversample=self.F)
            oL.append(a), oR.append(b)
        return oL, oR, met


@pytest.fixture(scope="module")
def eng():
    e = G.engine()
    yield e
    e.close()


# ---------------------------------------------------------------- 1. the stage alone
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("A,H,F", [(2, 0, 4), (64, 1, 4), (64, 1, 2), (64, 200, 4), (512, 4096, 4)])
def test_gpu_limit_tp_stage_against_ref(eng, A, H, F, aligned):
    """37 rows at frame counts around the detector's reach (6, 12), the lane group, the wave and the
    tile, with and without counts (0, 1, partial and full, NaN beyond each), and one mono call; the
    calls follow each other on one limiter, so every one but the first starts from a history, and
    with (512, 4096) the halo is longer than most calls and than a tile and is staged in several
    passes"""
    import tunebfree_amd as T
    n = 37
    group, tile, hn, lds = T.Engine.limit_grid(CEIL, A, H, oversample=F)
    assert hn == M.history(A, H) and tile % (64 * group) == 0 and lds <= 80 * 1024
    if (A, H) == (512, 4096):
        assert hn > tile + 1024
    lim, ref = eng.limiter(n, CEIL, A, H, oversample=F), Ref(n, A, H, F)
    assert lim.latency == A + 5 and lim.history == hn and lim.oversample == F
    reduced = clamped = 0
    for k, frames in enumerate([1, 6, 12, 63, 65, tile - 1, tile, tile + 1, 2 * tile + 5]):
        L, R = LM.issue_input(100 + k, frames, n), LM.issue_input(200 + k, frames, n)
        what = f"A={A} H={H} F={F} aligned={aligned} frames={frames}"
        _, _, gm = G.check_call(lim, ref, L, R, what, aligned)
        reduced, clamped = reduced + int(gm["reduced"].sum()), clamped + int(gm["clamped"].sum())
        c = G.counts_for(n, frames, 300 + k)
        G.check_call(lim, ref, G.with_nan_beyond(L, c), G.with_nan_beyond(R, c), what + " counts", aligned, c)
        if frames == 65:
            gL, gR, _ = G.check_call(lim, ref, L, L, what + " mono", aligned)
            d = A + 5   # the first A + 5 frames are the delayed history, which was not mono
            same(gL[:, min(d, frames):], gR[:, min(d, frames):], what + " mono: L against R")
    assert reduced > 0
    print(f"A={A} H={H} F={F}: reduced {reduced}, clamped {clamped}")
    lim.close()


# ---------------------------------------------------------------- 2. streaming
def test_gpu_limit_tp_rows_stream_at_their_own_positions(eng):
    """12 rows of 2600 frames each, taken in calls of 1, 5, 6, 11, D + 6 and Hn_tp + 3 frames and the
    rest in two, each row with its own count per call: the outputs joined per row are one ref run"""
    import tunebfree_amd as T
    n, total, A, H, F = 12, 2600, 64, 200, 4
    D, Hn = A - 1, M.history(A, H)
    lim = eng.limiter(n, CEIL, A, H, oversample=F)
    L, R = LM.issue_input(41, total, n), LM.issue_input(42, total, n)
    one = [T.Engine.limit_ref(L[r], R[r], CEIL, A, H, oversample=F) for r in range(n)]
    rng = np.random.default_rng(43)
    at = np.zeros(n, np.int64)
    gotL, gotR = [[] for _ in range(n)], [[] for _ in range(n)]
    sizes = [1, 5, 6, 11, D + 6, Hn + 3, None, None]
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
        gL, gR, _ = G.stage_call(lim, cl, cr, aligned=bool(k % 2), counts=counts)
        for r in range(n):
            gotL[r].append(gL[r, :counts[r]]), gotR[r].append(gR[r, :counts[r]])
        at += counts
    assert (at == total).all() and len(set(int(a) for a in (total - left))) > 1
    for r in range(n):
        same(np.concatenate(gotL[r]), one[r][0], f"row {r}: L joined against one ref run")
        same(np.concatenate(gotR[r]), one[r][1], f"row {r}: R joined against one ref run")
    lim.close()


# ---------------------------------------------------------------- 3. reset, both kinds
def test_gpu_limit_tp_reset(eng):
    """rows {1, 5} reset mid-stream behave as new and the others are undisturbed"""
    n, frames, A, H, F = 8, 300, 16, 5, 4
    a, ra = eng.limiter(n, CEIL, A, H, oversample=F), Ref(n, A, H, F)
    for k in range(3):
        L, R = LM.issue_input(60 + k, frames, n), LM.issue_input(70 + k, frames, n)
        if k == 1:
            a.reset([1, 5])
            ra.reset([1, 5])
        if k == 2:
            a.reset()
            ra.reset()
        ga = G.check_call(a, ra, L, R, f"call {k}")
        if k:   # a reset row equals a new row's output
            fresh = Ref(n, A, H, F).call(L, R)
            for r in ([1, 5] if k == 1 else range(n)):
                same(ga[0][r], fresh[0][r], f"call {k}: reset row {r} against a new row")
            if k == 1:
                assert any(not np.array_equal(bits(ga[0][r]), bits(fresh[0][r])) for r in (0, 2, 3, 4, 6, 7))
    with pytest.raises(Exception, match="rows"):
        a.reset([0, n])
    a.close()


def test_gpu_limit_tp_and_plain_on_one_engine(eng):
    """a plain and a true-peak limiter of one configuration take the same planes in turn: the plain
    one's output is the plain restatement's in bits, the other's its own, and they differ"""
    n, frames, A, H = 8, 1500, 64, 32
    plain, tp = eng.limiter(n, CEIL, A, H), eng.limiter(n, CEIL, A, H, oversample=4)
    rp, rt = G.Ref(n, A, H), Ref(n, A, H, 4)
    assert (plain.oversample, plain.latency, plain.history) == (None, A - 1, LM.history(A, H))
    assert (tp.oversample, tp.latency, tp.history) == (4, A + 5, M.history(A, H))
    for k in range(2):
        L, R = LM.issue_input(90 + k, frames, n), LM.issue_input(95 + k, frames, n)
        gt = G.check_call(tp, rt, L, R, f"true-peak limiter, call {k}", aligned=bool(k))
        gp = G.check_call(plain, rp, L, R, f"plain limiter, call {k}", aligned=bool(k))
        assert not np.array_equal(bits(gt[0][:, M.E:]), bits(gp[0][:, :frames - M.E]))
    plain.close(), tp.close()


# ---------------------------------------------------------------- 4. with the meter
def test_gpu_limit_tp_in_front_of_the_true_peak_meter(eng):
    """the quarter-rate sine at 45 degrees (samples under the ceiling, crests over it) through the
    limiter and, on the same stream with no synchronize in between, through the true-peak meter:
    the meter's words are those of true_peak_ref on the ref output, and over the frames of constant
    gain the output's true peak is within c (1 + 2^-18) (derived in tests/test_limit_tp_cpu.py)
    where the plain limiter's reads over the ceiling"""
    import torch
    import tunebfree_amd as T
    A, H, F, amp = 64, 1, 4, 1.2
    Hn = M.history(A, H)
    start = Hn + 12 + 11
    n, frames = 4, start + 1000
    x = np.stack([TP.sine(frames, 0.25, 45.0, amp * (1.0 + 0.1 * r)) for r in range(n)])
    assert float(np.abs(x[0]).max()) < float(CEIL) < amp
    bound = float(CEIL) * (1.0 + 2.0 ** -18)

    def steady(out):
        h = np.concatenate([out[start - 11:start], out[start - 11:start]])
        return float(np.uint32(T.Engine.true_peak_ref(out[start:], out[start:], oversample=F, hist=h)[0].max()).view(np.float32))

    for kind in (F, None):
        lim, meter = eng.limiter(n, CEIL, A, H, oversample=kind), eng.true_peak(n, oversample=F)
        src = torch.from_numpy(x).cuda()
        out = [torch.full((n, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        lim.process_device(src.data_ptr(), src.data_ptr(), frames, frames, out[0].data_ptr(), out[1].data_ptr(), frames)
        meter.measure_device(out[0].data_ptr(), out[1].data_ptr(), frames, frames)
        res = meter.read()
        got = [t.cpu().numpy() for t in out]
        for r in range(n):
            wL, wR, wm, _ = T.Engine.limit_ref(x[r], x[r], CEIL, A, H, oversample=kind)
            same(got[0][r], wL, f"kind {kind}, row {r}: L against the ref")
            same(got[1][r], wR, f"kind {kind}, row {r}: R against the ref")
            words, _ = T.Engine.true_peak_ref(wL, wR, oversample=F)
            mine = np.concatenate([bits(res[r]["sample_peak"]), bits(res[r]["inter_peak"])])
            assert np.array_equal(mine, words), (kind, r, mine, words)
            top = steady(got[0][r])
            print(f"kind {kind}, row {r}: reduced {int(wm['reduced'])}, steady true peak {top!r}, ceiling {float(CEIL)!r}")
            if kind:
                assert wm["reduced"] > 0 and 0.99 * float(CEIL) < top <= bound
            else:
                assert (wm["reduced"] == 0) == (r < 2) and top > bound   # rows 2, 3: the samples themselves are over
        lim.close(), meter.close()


# ---------------------------------------------------------------- 5. refusals
def test_gpu_limit_tp_refusals_write_nothing_and_move_no_state(eng):
    import torch
    import tunebfree_amd as T
    n, frames, A, H, F = 4, 96, 16, 5, 4
    with pytest.raises(T.TbfError, match="-22.*oversample"):
        eng.limiter(n, CEIL, A, H, oversample=3)
    lim, ref = eng.limiter(n, CEIL, A, H, oversample=F), Ref(n, A, H, F)
    L, R = LM.issue_input(81, frames, n), LM.issue_input(82, frames, n)
    G.check_call(lim, ref, L, R, "before the refusals")
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
        (dict(in_stride=frames - 1), "in_stride"),
        (dict(out_stride=frames - 1), "out stride"),
        (dict(counts=over), r"counts\[2\]"),
        (dict(outL_ptr=xl), "overlap"),                      # in place
        (dict(outR_ptr=xr + 4 * (stride * (n - 1) + frames - 1)), "overlap"),   # one float of the input's last row
        (dict(outR_ptr=ol + 4 * 8), "overlap"),              # the two outputs
        (dict(meters_ptr=xr), "overlap"),                    # the meters on the input
    ]
    for kw, word in bad:
        with pytest.raises(T.TbfError, match="-22.*" + word):
            lim.process_device(**{**good, **kw})
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in o) and (met.cpu().numpy() == -1).all()
    same(x[0].cpu().numpy()[:, :frames], L, "the input after the refusals")
    L2, R2 = LM.issue_input(83, frames, n), LM.issue_input(84, frames, n)
    G.check_call(lim, ref, L2, R2, "after the refusals")
    lim.close()


# ---------------------------------------------------------------- 6. accounting
def test_gpu_limit_tp_accounting():
    """a true-peak limiter is no instance or stage memory of the engine, a call is one launch set,
    and the engine releases the limiters that are still alive when it closes"""
    import torch
    e = G.engine(2)
    e.render(2)
    b0, l0 = e.device_bytes(), e.launches()
    lim = e.limiter(64, CEIL, 512, 4096, oversample=4)
    e.limiter(3, CEIL, 2, 0, oversample=2)   # left to the engine
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
