"""The mixdown stage on the GPU (tbf_mix_device, tbf_render_mix* / tbf_process_mix*, k_mix):
identity in bits with the host restatement of the definition (tbf_debug_mix_ref) on synthetic
planes at every layout the kernel takes, on the planes a twin engine's plain render delivers, cut
invariance with events, the scratch pieces of a long call, composition with the rate converter
and the PCM stage, the memory contract, the refusals and the accounting.

The stage is this project's own definition (include/tbf.h); its arithmetic
against float64 and the proof that the order of the sum is observable are checked without a GPU
(tests/test_mix_cpu.py).  Everything here is an identity in bits."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import mix_model as M
import scenarios as S

# the scenarios and call helpers of test_gpu_resample.py, loaded under a name of their own so
# that pytest's own import of that file is not pre-empted
_spec = importlib.util.spec_from_file_location("_gpu_resample_helpers_mix", Path(__file__).with_name("test_gpu_resample.py"))
RS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(RS)

pytestmark = pytest.mark.gpu

FULL, TONEGEN, FX = 0, 1, 4
NONE = M.NONE
FILL = 777.0
SIZES = [0, 1, 2, 9, 17, 33]  # members per bus: 62 rows, and 8 in no bus
same = RS.same


def grid(frames, n_buses):
    import tunebfree_amd as T
    return T.Engine.mix_grid(frames, n_buses)


# ---------------------------------------------------------------- 1. the stage alone
def layout(copies, seed=17):
    """70 x copies rows over 6 x copies buses: each group of 70 rows holds buses of 0, 1, 2, 9, 17
    and 33 members, interleaved, and 8 rows in no bus; random coefficients, all four in use"""
    rng = np.random.default_rng(seed)
    base = np.concatenate([[b] * k for b, k in enumerate(SIZES)] + [[-1] * 8])
    bus = []
    for c in range(copies):
        g = base.copy()
        rng.shuffle(g)
        bus.append(np.where(g < 0, -1, g + len(SIZES) * c))
    bus = np.concatenate(bus)
    rows = M.rows_of(bus, *rng.uniform(-1.5, 1.5, (4, len(bus))).astype(np.float32))
    assert np.diff(np.flatnonzero(rows["bus"] == 5)).max() > 1  # a bus's rows are not contiguous
    return rows, len(SIZES) * copies


def planes(rows, frames, seed=23):
    """the issue's inputs, randn * 10^uniform (-3, 0), with which the order of a sum shows; NaN in
    the rows that are in no bus"""
    rng = np.random.default_rng(seed)
    n = len(rows)
    L = (rng.standard_normal((n, frames)) * 10.0 ** rng.uniform(-3, 0, (n, frames))).astype(np.float32)
    R = (rng.standard_normal((n, frames)) * 10.0 ** rng.uniform(-3, 0, (n, frames))).astype(np.float32)
    L[rows["bus"] == NONE] = np.nan
    R[rows["bus"] == NONE] = np.nan
    return L, R


def counts_for(rows, frames, seed=29):
    """0, 1, partial and full counts, the first four among each group's members; beyond its count a
    row holds NaN"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, frames + 1, len(rows)).astype(np.uint32)
    members = np.flatnonzero(rows["bus"] != NONE)
    c[members[0::7]] = frames
    c[members[1::7]] = 0
    c[members[2::7]] = min(1, frames)
    c[members[3::7]] = frames // 2
    return c


def stage_case(eng, rows, n_buses, frames, aligned, counts=None, mono=False, seed=23):
    """one tbf_mix_device call in torch memory: aligned -- every row 16-byte aligned, even
    strides; otherwise everything one float into its allocation with odd strides.  Four guard
    floats or more lie around every output row.  Returns the two bus planes."""
    import torch
    import tunebfree_amd as T
    n = len(rows)
    L, R = planes(rows, frames, seed)
    if counts is not None:
        for r in range(n):
            L[r, counts[r]:] = np.nan
            R[r, counts[r]:] = np.nan
    if mono:
        R = L
    lead = 0 if aligned else 1
    istride = (frames + 3) // 4 * 4 + (0 if aligned else 1)
    ostride = (frames + 3) // 4 * 4 + (8 if aligned else 5)
    olead = 4 if aligned else 5
    assert (istride % 2 == 0) == aligned and (ostride % 2 == 0) == aligned
    dev = []
    for src in ((L,) if mono else (L, R)):
        a = np.full(lead + n * istride + 4, FILL, np.float32)
        a[lead:lead + n * istride].reshape(n, istride)[:, :frames] = src
        dev.append(torch.from_numpy(a).cuda())
    outs = [torch.full((olead + n_buses * ostride,), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 for t in dev + outs)
    ptr = [t.data_ptr() + 4 * lead for t in dev]
    eng.mix_device(n, ptr[0], ptr[-1], istride, frames, rows, n_buses, outs[0].data_ptr() + 4 * olead,
                   outs[1].data_ptr() + 4 * olead, ostride, counts=counts)
    eng.synchronize()
    wantL, wantR = T.Engine.mix_ref(L, R, rows, n_buses, counts=counts)
    what = f"{n} rows, {n_buses} buses, {frames} frames, aligned {aligned}, counts {counts is not None}, mono {mono}"
    got = []
    for o, want, ch in zip(outs, (wantL, wantR), "LR"):
        a = o.cpu().numpy()
        assert (a[:olead] == FILL).all(), f"{what}: written before {ch}"
        body = a[olead:].reshape(n_buses, ostride)
        assert (body[:, frames:] == FILL).all(), f"{what}: written behind a row of {ch}"
        same(body[:, :frames], want, f"{what}: {ch} against mix_ref")
        got.append(body[:, :frames].copy())
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any() and got[0].any()
    return got


@pytest.fixture(scope="module")
def stage_engine():
    eng = RS.engine(n=1)
    yield eng
    eng.close()


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
def test_gpu_mix_stage_against_ref(stage_engine, aligned):
    """70 rows into 6 buses of 0, 1, 2, 9, 17 and 33 members (below, at and across the members a
    lane keeps in flight, with a remainder), at frame counts around the lane group, the wave and
    the tile, with and without counts"""
    rows, nb = layout(1)
    assert len(rows) == 70 and nb == 6 and int((rows["bus"] == NONE).sum()) == 8
    tile = grid(128, nb)[1]
    for frames in (1, 3, 5, 127, 128, 129, tile + 1):
        assert grid(frames, nb)[1] == tile
        stage_case(stage_engine, rows, nb, frames, aligned)
        stage_case(stage_engine, rows, nb, frames, aligned, counts=counts_for(rows, frames))
    stage_case(stage_engine, rows, nb, 130, aligned, mono=True)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("copies,per_lane,lengths", [(250, 2, (129, 131, 256)), (350, 4, (3, 255, 257, 259))],
                         ids=["two-per-lane", "four-per-lane"])
def test_gpu_mix_stage_wider_lanes(stage_engine, copies, per_lane, lengths, aligned):
    """the same groups of rows repeated until the call has the waves for two and for four frames
    per lane: the wide loads and stores, their tails, and one tile + 1"""
    rows, nb = layout(copies)
    assert 64 * per_lane + 1 in lengths
    for frames in lengths:
        g, tile, _s = grid(frames, nb)
        assert (g, tile) == (per_lane, 64 * per_lane), (frames, nb, g)
        stage_case(stage_engine, rows, nb, frames, aligned, counts=counts_for(rows, frames))
    stage_case(stage_engine, rows, nb, lengths[1], aligned)


def test_gpu_mix_no_layout_changes_a_bit(stage_engine):
    """the same 70 rows into the same 6 buses, with empty buses behind them that change nothing
    but the grid: one, two and four frames per lane give the same bits"""
    rows, nb = layout(1)
    frames, ref = 300, None
    for buses, per_lane in ((nb, 1), (700, 2), (1100, 4)):
        assert grid(frames, buses)[0] == per_lane
        gL, gR = stage_case(stage_engine, rows, buses, frames, True)
        assert not gL[nb:].any() and not gR[nb:].any()
        if ref is None:
            ref = (gL[:nb], gR[:nb])
        same(gL[:nb], ref[0], f"{per_lane} frames per lane against one, L")
        same(gR[:nb], ref[1], f"{per_lane} frames per lane against one, R")


def test_gpu_mix_repeat(stage_engine):
    """the same call twice: identical bits"""
    rows, nb = layout(1)
    a = stage_case(stage_engine, rows, nb, 129, False, counts=counts_for(rows, 129))
    b = stage_case(stage_engine, rows, nb, 129, False, counts=counts_for(rows, 129))
    same(a[0], b[0], "repeat, L")
    same(a[1], b[1], "repeat, R")


def test_gpu_mix_slices(stage_engine):
    """more buses than one launch takes, with tiny rows: the slice loop.  Bus b holds row b, the
    first three buses a second row, the last bus none"""
    slice_buses = grid(3, 1)[2]
    nb = slice_buses + 6
    bus = np.concatenate([np.arange(nb - 1), [0, 1, 2], [-1, -1]])
    rng = np.random.default_rng(31)
    rows = M.rows_of(bus, *rng.uniform(-1.5, 1.5, (4, len(bus))).astype(np.float32))
    assert nb > slice_buses
    got = stage_case(stage_engine, rows, nb, 3, False)
    assert not got[0][-1].any() and got[0][slice_buses + 2].any()


# ---------------------------------------------------------------- 2. the render families
N5 = 5
SEEDS5 = [5100 + 41 * i for i in range(N5)]


def rows5():
    """two buses and one unmixed instance, pans and gains through the helper, then cross terms"""
    import tunebfree_amd as T
    rows = T.params.mix_rows([0, 1, 0, -1, 1], [1.0, 0.7, 0.5, 1.0, 1.2], [-0.5, 0.25, 1.0, 0.0, -1.0])
    rows["lr"] = np.float32([0.1, 0.0, -0.2, 0.0, 0.3])
    rows["rl"] = np.float32([0.0, 0.25, 0.0, 0.0, -0.1])
    return rows


def engine5(chain, whirl_out=0, n=N5):
    return RS.engine(48000, None, chain, n, whirl_out, seeds=SEEDS5)


def twin_planes(chain, whirl_out, sc, nb, x, n=N5):
    """a twin engine's plain render, controls by direct call"""
    twin = engine5(chain, whirl_out, n)
    tl, tr = [], []
    for s, e in RS.stretches(sc, 0, nb):
        RS.apply(twin, sc, s)
        l, r = twin.render(e - s) if x is None else twin.process(x[:, s * 128:e * 128])
        tl.append(l)
        tr.append(r)
    twin.close()
    L, R = np.concatenate(tl, axis=1), np.concatenate(tr, axis=1)
    assert float(np.abs(L).max()) > 1e-4
    return L, R


def device_mix(eng, sc, nb, rows, n_buses, b0=0, x=None, guard=3):
    """one device call with the scripts' events of [b0, b0 + nb) into torch memory"""
    import torch
    frames = nb * 128
    outs = [torch.full((n_buses, frames + guard), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    ev = RS.event_rows(eng, sc, b0, b0 + nb)
    if x is None:
        torch.cuda.synchronize()
        eng.render_mix_device(nb, rows, n_buses, outs[0].data_ptr(), outs[1].data_ptr(), frames + guard, events=ev)
    else:
        xt = torch.from_numpy(np.ascontiguousarray(x[:, b0 * 128:(b0 + nb) * 128])).cuda()
        torch.cuda.synchronize()
        eng.process_mix_device(nb, xt.data_ptr(), xt.shape[1], rows, n_buses, outs[0].data_ptr(), outs[1].data_ptr(),
                               frames + guard, events=ev)
    eng.synchronize()
    res = []
    for o in outs:
        a = o.cpu().numpy()
        assert (a[:, frames:] == FILL).all(), "written behind a bus row"
        res.append(a[:, :frames].copy())
    return res


@pytest.mark.parametrize("chain,whirl_out", [(FULL, 0), (FULL, 1), (TONEGEN, 0), (FX, 0)],
                         ids=["full-mic", "full-direct", "tonegen", "fx"])
def test_gpu_mix_render_families(chain, whirl_out):
    """render_mix / process_mix and their device forms equal mix_ref of the planes a twin engine
    in the same state renders: 5 instances with keys down, 2 buses and one unmixed instance"""
    import tunebfree_amd as T
    nb, rows = 4, rows5()
    sc = [S.bench_scenario(i) for i in range(N5)]
    x = RS.noise(nb, N5) if chain == FX else None
    L, R = twin_planes(chain, whirl_out, sc, nb, x)
    wantL, wantR = T.Engine.mix_ref(L, R, rows, 2)
    assert float(np.abs(wantL).max()) > 1e-4 and float(np.abs(wantR).max()) > 1e-4
    eng = engine5(chain, whirl_out)
    RS.apply(eng, sc, 0)
    gotL, gotR = eng.render_mix(nb, rows, 2) if x is None else eng.process_mix(x, rows, 2)
    eng.close()
    same(gotL, wantL, f"chain {chain} whirl_out {whirl_out}: host call, L")
    same(gotR, wantR, f"chain {chain} whirl_out {whirl_out}: host call, R")
    eng = engine5(chain, whirl_out)
    dL, dR = device_mix(eng, sc, nb, rows, 2, x=x)
    eng.close()
    same(dL, wantL, f"chain {chain} whirl_out {whirl_out}: device call with events, L")
    same(dR, wantR, f"chain {chain} whirl_out {whirl_out}: device call with events, R")


@pytest.mark.parametrize("chain", [FULL, FX])
def test_gpu_mix_cuts_and_events(chain):
    """12 blocks as one call, as 5 + 7 and as 12 calls of one block, with a note and a drawbar
    event in the middle: identical in bits, and equal to mix_ref of a twin's render"""
    import tunebfree_amd as T
    nb, rows = 12, rows5()
    sc = [S.bench_scenario(i) + [(6, "note", 40 + 3 * i, 1), (6, "param", S.P_DRAWBAR + 2, 3 + i)] for i in range(N5)]
    x = RS.noise(nb, N5) if chain == FX else None
    eng = engine5(chain)
    one = device_mix(eng, sc, nb, rows, 2, x=x)
    eng.close()
    for cuts in ([5, 7], [1] * 12):
        eng = engine5(chain)
        parts, at = [], 0
        for c in cuts:
            parts.append(device_mix(eng, sc, c, rows, 2, b0=at, x=x))
            at += c
        eng.close()
        for k, ch in enumerate("LR"):
            same(np.concatenate([p[k] for p in parts], axis=1), one[k], f"chain {chain}: cuts {cuts} against one call, {ch}")
    L, R = twin_planes(chain, 0, sc, nb, x)
    wantL, wantR = T.Engine.mix_ref(L, R, rows, 2)
    same(one[0], wantL, f"chain {chain}: one call against mix_ref of a twin's render, L")
    same(one[1], wantR, f"chain {chain}: one call against mix_ref of a twin's render, R")
    assert not np.array_equal(L[:, 5 * 128:6 * 128], L[:, 7 * 128:8 * 128])


def test_gpu_mix_pieces_of_a_long_call():
    """one call of 260 blocks crosses a scratch piece (256 blocks), with a note and a drawbar
    event at the second piece's first block: it equals the same render mixed in one mix_ref.  The
    host form, which takes no events, likewise without those events."""
    import tunebfree_amd as T
    nb, n = 260, 2
    sc0 = [S.bench_scenario(i) for i in range(n)]
    sc = [s + [(256, "note", 77 + i, 1), (256, "param", S.P_DRAWBAR + 3, 8)] for i, s in enumerate(sc0)]
    rows = T.params.mix_rows([0, 0], [1.0, 0.5], [-0.3, 0.6])
    eng = engine5(FULL, n=n)
    gL, gR = device_mix(eng, sc, nb, rows, 1)
    eng.close()
    L, R = twin_planes(FULL, 0, sc, nb, None, n=n)
    wantL, wantR = T.Engine.mix_ref(L, R, rows, 1)
    same(gL, wantL, "260 blocks against one mix_ref, L")
    same(gR, wantR, "260 blocks against one mix_ref, R")
    L0, R0 = twin_planes(FULL, 0, sc0, nb, None, n=n)
    assert not np.array_equal(L0[:, 256 * 128:], L[:, 256 * 128:])  # the events are heard
    eng = engine5(FULL, n=n)
    RS.apply(eng, sc0, 0)
    hL, hR = eng.render_mix(nb, rows, 1)
    eng.close()
    wantL, wantR = T.Engine.mix_ref(L0, R0, rows, 1)
    same(hL, wantL, "the host form over 260 blocks, L")
    same(hR, wantR, "the host form over 260 blocks, R")


# ---------------------------------------------------------------- 3. composition
def test_gpu_mix_behind_the_rate_converter():
    """render_resampled_device at 48000 -> 22050, then mix_device over the converted rows with
    their counts: mix_ref of those rows"""
    import torch
    import tunebfree_amd as T
    n, nb = RS.N, RS.NB
    sc = RS.scens()
    eng = RS.engine(fo=22050)
    cap = eng.resampled_frames(nb)
    res, rows_, _alloc = RS.one_call(eng, sc, nb, raw=False, stride=cap + 5, lead=1)
    counts = res["counts"][0]
    assert 0 < counts.min() and counts.max() <= cap
    counts = counts.copy()
    counts[1] = counts[1] // 2  # a caller may mix less than a row holds
    frames, stride = cap, cap + 5
    host = [np.ascontiguousarray(rows_[k]) for k in ("L", "R")]
    dev = [torch.from_numpy(a).cuda() for a in host]
    mrows = T.params.mix_rows([0, 0, 0], [1.0, 0.8, 0.6], [-1.0, 0.0, 1.0])
    outs = [torch.full((1, frames + 3), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    eng.mix_device(n, dev[0].data_ptr(), dev[1].data_ptr(), stride, frames, mrows, 1, outs[0].data_ptr(), outs[1].data_ptr(),
                   frames + 3, counts=counts)
    eng.synchronize()
    eng.close()
    wantL, wantR = T.Engine.mix_ref(host[0][:, :frames], host[1][:, :frames], mrows, 1, counts=counts)
    for o, want, ch in zip(outs, (wantL, wantR), "LR"):
        a = o.cpu().numpy()
        assert (a[:, frames:] == FILL).all()
        same(a[:, :frames], want, f"resampled rows mixed, {ch}")
    assert float(np.abs(wantL).max()) > 1e-4 and not wantL[0, counts.max():].any()


def test_gpu_mix_into_pcm_on_one_stream(stage_engine):
    """mix_device, then pcm_convert_device over the bus planes on the same stream with no
    synchronize between: the bytes and meters of pcm_ref of mix_ref"""
    import torch
    import tunebfree_amd as T
    rows, nb = layout(1)
    frames = 1000
    L, R = planes(rows, frames)
    dev = [torch.from_numpy(a).cuda() for a in (L, R)]
    bus = [torch.full((nb, frames), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    pcm = torch.full((nb, frames * 4), 0xA5, dtype=torch.uint8, device="cuda")
    met = torch.full((nb * 4,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stage_engine.mix_device(len(rows), dev[0].data_ptr(), dev[1].data_ptr(), frames, frames, rows, nb, bus[0].data_ptr(),
                            bus[1].data_ptr(), frames)
    stage_engine.pcm_convert_device(nb, bus[0].data_ptr(), bus[1].data_ptr(), frames, frames, pcm.data_ptr(), frames * 4,
                                    T.engine.PCM_S16, meters_ptr=met.data_ptr())
    stage_engine.synchronize()
    wantL, wantR = T.Engine.mix_ref(L, R, rows, nb)
    got, gm = pcm.cpu().numpy(), met.cpu().numpy().view(T.engine.METER_DTYPE)
    for b in range(nb):
        wb, wm = T.Engine.pcm_ref(T.engine.PCM_S16, wantL[b], wantR[b], row=b)
        assert got[b].tobytes() == wb.tobytes(), f"bus {b}: frames"
        assert gm[b].tobytes() == wm.tobytes(), f"bus {b}: meters"
    assert int(gm["clipL"].sum()) > 0 and float(gm["peakL"][0]) == 0.0  # loud buses clip; bus 0 is empty


# ---------------------------------------------------------------- 4. refusals
def test_gpu_mix_refusals_render_nothing():
    """refused calls render nothing, step no control and write nothing: the buffers keep their
    fill and the next plain render is that of an engine that never saw them"""
    import torch
    import tunebfree_amd as T
    lib = T.load_library()
    n, nb = N5, 2
    frames = nb * 128
    sc = [S.bench_scenario(i) for i in range(n)]
    L, R = twin_planes(FULL, 0, sc, nb, None)
    eng = engine5(FULL)
    good = rows5()
    outs = [torch.full((2, frames + 4), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
    x = torch.full((n, frames), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ev = RS.event_rows(eng, sc, 0, 1)
    assert len(ev) > 0

    def call(rows=good, buses=2, l=outs[0].data_ptr(), r=outs[1].data_ptr(), stride=frames + 4, e=ev):
        mo = T.engine.MixOut(l, r, stride)
        return lib.tbf_render_mix_device(eng._h, nb, e.ctypes.data, len(e), rows.ctypes.data, buses, C.byref(mo), None)
    bad = good.copy()
    bad["bus"][4] = 2
    assert call(rows=bad) == -22 and call(buses=0) == -22
    bad = good.copy()
    bad["rr"][0] = np.nan
    assert call(rows=bad) == -22
    assert call(l=None) == -22 and call(stride=frames - 1) == -22 and call(r=outs[1].data_ptr() + 2) == -22
    assert call(r=outs[0].data_ptr() + 4 * 8) == -22  # the two bus planes in each other
    assert call(e=eng.events([(0, 0, 0, 60, 1.0), (1, 0, 0, 62, 1.0)])[::-1].copy()) == -22  # events out of order
    mo = T.engine.MixOut(outs[0].data_ptr(), outs[1].data_ptr(), frames + 4)
    assert lib.tbf_process_mix_device(eng._h, nb, None, 0, x.data_ptr(), frames, good.ctypes.data, 2, C.byref(mo), None) == -22
    cnt = np.array([frames + 1, 0, 0, 0, 0], np.uint32)
    assert lib.tbf_mix_device(eng._h, n, x.data_ptr(), x.data_ptr(), frames, frames, cnt.ctypes.data, good.ctypes.data, 2,
                              C.byref(mo), None) == -22
    mo2 = T.engine.MixOut(x.data_ptr() + 4 * frames, outs[1].data_ptr(), frames + 4)  # a bus plane inside the input rows
    assert lib.tbf_mix_device(eng._h, n, x.data_ptr(), x.data_ptr(), frames, frames, None, good.ctypes.data, 2, C.byref(mo2),
                              None) == -22
    eng.synchronize()
    assert all((o.cpu().numpy() == FILL).all() for o in outs) and (x.cpu().numpy() == FILL).all()
    RS.apply(eng, sc, 0)
    gl, gr = eng.render(nb)
    eng.close()
    same(gl, L, "after the refusals, L")
    same(gr, R, "after the refusals, R")


# ---------------------------------------------------------------- 5. accounting
def test_gpu_mix_accounting():
    """the stage holds no instance or stage memory and launches no render kernel of its own:
    device_bytes () is what it was, a mix call leaves launches () alone, a mixed render counts the
    launches of a plain render, and mix_time counts k_mix's launches"""
    import torch
    eng = engine5(FULL)
    rows = rows5()
    eng.render(2)
    b0, l0 = eng.device_bytes(), eng.launches()
    eng.render(2)
    l1 = eng.launches()
    plain = {k: l1[k] - l0[k] for k in l0}
    assert sum(plain.values()) > 0
    x = torch.zeros((N5, 256), dtype=torch.float32, device="cuda")
    outs = [torch.zeros((2, 256), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    eng.mix_time(True)
    for _ in range(3):
        eng.mix_device(N5, x.data_ptr(), x.data_ptr(), 256, 256, rows, 2, outs[0].data_ptr(), outs[1].data_ptr(), 256)
    eng.synchronize()
    ms, n = eng.mix_time()
    assert n == 3 and ms > 0.0
    assert eng.launches() == l1 and eng.device_bytes() == b0
    eng.render_mix(2, rows, 2)
    l2 = eng.launches()
    assert {k: l2[k] - l1[k] for k in l2} == plain and eng.device_bytes() == b0
    ms, n = eng.mix_time()
    assert n == 1 and ms > 0.0
    eng.mix_time(False)
    eng.render_mix(2, rows, 2)
    assert eng.mix_time() == (0.0, 0)
    eng.close()
