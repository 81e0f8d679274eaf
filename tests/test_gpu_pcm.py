"""The PCM output stage on the GPU (tbf_pcm_convert_device, tbf_render_pcm* / tbf_process_pcm*,
k_pcm): identity in bytes with the numpy model of the definition (tests/pcm_model.py) on the
planes a twin engine's plain render delivers, meters equal exactly, cut invariance with running
dither frames, the scratch pieces of a long call, composition with the rate converter, the
memory contract and the accounting.

The stage is this project's own definition (include/tbf.h); everything here
is an identity in bytes."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import pcm_model as M
import scenarios as S

# the scenarios and call helpers of test_gpu_resample.py, loaded under a name of their own so
# that pytest's own import of that file is not pre-empted
_spec = importlib.util.spec_from_file_location("_gpu_resample_helpers", Path(__file__).with_name("test_gpu_resample.py"))
RS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(RS)

pytestmark = pytest.mark.gpu

FULL, FX = 0, 4
N, NB = RS.N, RS.NB
FB = M.FRAME_BYTES
SEED = 0x5EED1234
FIDS = [f"fmt{f}-flags{g}" for f, g in M.FORMATS]


def engine(chain=FULL, n=N, whirl_out=0, fo=None):
    return RS.engine(48000, fo, chain, n, whirl_out)


def meters_of(fmt, Lr, Rr, flags=0, seed=0, frame0=None, rows=None):
    """the model over rows: (list of byte rows, METER_DTYPE array)"""
    import tunebfree_amd as T
    out, met = [], np.zeros(len(Lr), T.engine.METER_DTYPE)
    for i, (l, r) in enumerate(zip(Lr, Rr)):
        b, m = M.convert(fmt, l, r, flags, seed, i if rows is None else rows[i], 0 if frame0 is None else int(frame0[i]))
        out.append(b)
        met[i] = m
    return out, met


def same_meters(got, want, what):
    assert got.tobytes() == want.tobytes(), (what, got, want)


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} bytes differ, first at {bad[0]}")


# ---------------------------------------------------------------- 1. the converter alone
@pytest.fixture(scope="module")
def conv_engine():
    eng = engine(n=1)
    yield eng
    eng.close()


def crafted_rows(rows, frames):
    """rows of the crafted values, repeated to `frames` and rotated per row (edge cases first)"""
    L, R = M.crafted()
    reps = frames // len(L) + 2
    Lr = np.stack([np.roll(np.tile(L, reps), -5 * r)[:frames] for r in range(rows)]) if frames else np.zeros((rows, 0), np.float32)
    Rr = np.stack([np.roll(np.tile(R, reps), -9 * r)[:frames] for r in range(rows)]) if frames else np.zeros((rows, 0), np.float32)
    return Lr, Rr


def convert_case(eng, fmt, flags, frames, counts, aligned, row_frame0=None, frame0=0):
    """one tbf_pcm_convert_device call over 3 rows in torch memory: the input rows at an odd
    stride one float into their allocation (aligned: a stride of whole 16 bytes, no offset), the
    output rows with 12 bytes of slack behind them, everything not to be written holding 0xA5"""
    import torch
    import tunebfree_amd as T
    rows = 3
    Lr, Rr = crafted_rows(rows, frames)
    istride = (frames + 3) // 4 * 4 + (0 if aligned else 3)
    lead = 0 if aligned else 1
    planes = []
    for src in (Lr, Rr):
        a = np.full(lead + rows * istride + 8, 777.0, np.float32)
        for r in range(rows):
            a[lead + r * istride: lead + r * istride + frames] = src[r]
        planes.append(torch.from_numpy(a).cuda())
    rowb = (frames * FB[fmt] + 3) // 4 * 4
    ostride = rowb + (16 if aligned else 12)
    out = torch.full((rows * ostride + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    met = torch.full((rows * 4,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert out.data_ptr() % 16 == 0 and planes[0].data_ptr() % 16 == 0
    eng.pcm_convert_device(rows, planes[0].data_ptr() + 4 * lead, planes[1].data_ptr() + 4 * lead, istride, frames,
                           out.data_ptr(), ostride, fmt, counts=counts, flags=flags, seed=SEED, frame0=frame0,
                           row_frame0=row_frame0, meters_ptr=met.data_ptr())
    eng.synchronize()
    got = out.cpu().numpy()
    gm = met.cpu().numpy().view(T.engine.METER_DTYPE)
    cnt = [frames] * rows if counts is None else list(counts)
    f0 = [frame0] * rows if row_frame0 is None else list(row_frame0)
    want, wm = meters_of(fmt, [Lr[r, :cnt[r]] for r in range(rows)], [Rr[r, :cnt[r]] for r in range(rows)], flags, SEED, f0)
    what = f"format {fmt} flags {flags} frames {frames} counts {counts} aligned {aligned}"
    for r in range(rows):
        row = got[r * ostride:(r + 1) * ostride]
        nbytes = cnt[r] * FB[fmt]
        same_bytes(row[:nbytes], want[r], f"{what}: row {r}")
        assert (row[nbytes:] == 0xA5).all(), f"{what}: row {r} written behind its {nbytes} bytes"
    assert (got[rows * ostride:] == 0xA5).all()
    same_meters(gm, wm, what)


@pytest.mark.parametrize("aligned", [False, True], ids=["odd", "aligned"])
@pytest.mark.parametrize("fmt,flags", M.FORMATS, ids=FIDS)
def test_gpu_pcm_convert_against_model(conv_engine, fmt, flags, aligned):
    """frame counts around the lane group (4), the wave (256 frames) and the tile (1024), rows
    with their own counts, and a row of several tiles"""
    for frames in (0, 1, 2, 3, 63, 64, 65, 127, 129, 257, 1000, 1023, 1025, 2051):
        convert_case(conv_engine, fmt, flags, frames, None, aligned, frame0=(1 << 32) - 600)
    convert_case(conv_engine, fmt, flags, 130, [0, 1, 130], aligned, row_frame0=[7, (1 << 32) - 1, (1 << 40) + 3])
    convert_case(conv_engine, fmt, flags, 1500, [1029, 3, 1500], aligned)


def test_gpu_pcm_convert_mono_and_no_meters(conv_engine):
    """the same plane as L and R; without meters nothing but the frames is written"""
    import torch
    x = torch.from_numpy(M.crafted()[0][:600].copy()).cuda()
    out = torch.full((600 * 4 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    conv_engine.pcm_convert_device(1, x.data_ptr(), x.data_ptr(), 600, 600, out.data_ptr(), 2400, M.S16)
    conv_engine.synchronize()
    l = x.cpu().numpy()
    want, _ = M.convert(M.S16, l, l)
    got = out.cpu().numpy()
    same_bytes(got[:2400], want, "mono")
    assert (got[2400:] == 0xA5).all()


# ---------------------------------------------------------------- 2. the full chain
_planes = {}


def twin_planes(chain, whirl_out, nb=NB, n=N):
    """a twin engine's plain render of the scenarios, controls by direct call: (L, R) [n, nb*128],
    computed once per chain and output mode"""
    key = (chain, whirl_out, nb, n)
    if key not in _planes:
        sc = RS.scens(n)
        x = RS.noise(nb, n) if chain == FX else None
        twin = engine(chain, n, whirl_out)
        tl, tr = [], []
        for s, e in RS.stretches(sc, 0, nb):
            RS.apply(twin, sc, s)
            l, r = twin.render(e - s) if x is None else twin.process(x[:, s * 128:e * 128])
            tl.append(l)
            tr.append(r)
        twin.close()
        L, R = np.concatenate(tl, axis=1), np.concatenate(tr, axis=1)
        assert float(np.abs(L).max()) > 1e-4
        L.setflags(write=False)
        R.setflags(write=False)
        _planes[key] = (L, R, x)
    return _planes[key]


def host_calls(eng, sc, nb, fmt, flags, x=None, cuts=None):
    """blocks [0, nb) as host calls, one per stretch between the events and the cut points, the
    dither's frame0 running; returns the rows' bytes joined and the meters per call"""
    parts, mets, spans = [], [], RS.stretches(sc, 0, nb, cuts)
    for s, e in spans:
        RS.apply(eng, sc, s)
        kw = dict(fmt=fmt, flags=flags, seed=SEED, frame0=s * 128, meters=True)
        out, m = eng.render_pcm(e - s, **kw) if x is None else eng.process_pcm(x[:, s * 128:e * 128], **kw)
        parts.append(out.reshape(out.shape[0], -1).view(np.uint8))
        mets.append(m)
    return np.concatenate(parts, axis=1), mets, spans


@pytest.mark.parametrize("chain,whirl_out", [(FULL, 0), (FULL, 1), (FX, 0)], ids=["full-mic", "full-direct", "fx"])
@pytest.mark.parametrize("fmt,flags", M.FORMATS, ids=FIDS)
def test_gpu_pcm_full_chain(fmt, flags, chain, whirl_out):
    """render_pcm / process_pcm bytes are the model's of a twin's render planes; the meters of
    each call are the model's of that call's stretch"""
    L, R, x = twin_planes(chain, whirl_out)
    sc = RS.scens()
    eng = engine(chain, N, whirl_out)
    got, mets, spans = host_calls(eng, sc, NB, fmt, flags, x)
    eng.close()
    want, _ = meters_of(fmt, L, R, flags, SEED)
    for i in range(N):
        same_bytes(got[i], want[i], f"chain {chain} whirl_out {whirl_out} format {fmt} flags {flags}: instance {i}")
    for (s, e), m in zip(spans, mets):
        _b, wm = meters_of(fmt, L[:, s * 128:e * 128], R[:, s * 128:e * 128], flags, SEED, [s * 128] * N)
        same_meters(m, wm, f"meters of blocks {s}..{e}")
    if fmt == M.S16:
        assert max(float(m["peakL"].max()) for m in mets) > 1e-4


# ---------------------------------------------------------------- 3. cuts
def device_call(eng, sc, nb, fmt, flags, b0=0, x=None, n=N, slack=0):
    """one device call with the scripts' events of [b0, b0 + nb) into torch memory; returns (the
    rows' bytes [n, nb * 128 * frame bytes], meters)"""
    import torch
    import tunebfree_amd as T
    rowb = nb * 128 * FB[fmt]
    out = torch.full((n * (rowb + slack),), 0xA5, dtype=torch.uint8, device="cuda")
    met = torch.full((n * 4,), -1, dtype=torch.int32, device="cuda")
    ev = RS.event_rows(eng, sc, b0, b0 + nb)
    kw = dict(fmt=fmt, flags=flags, seed=SEED, frame0=b0 * 128, meters_ptr=met.data_ptr(), events=ev)
    if x is None:
        torch.cuda.synchronize()
        eng.render_pcm_device(nb, out.data_ptr(), rowb + slack, **kw)
    else:
        xt = torch.from_numpy(np.ascontiguousarray(x[:, b0 * 128:(b0 + nb) * 128])).cuda()
        torch.cuda.synchronize()
        eng.process_pcm_device(nb, xt.data_ptr(), xt.shape[1], out.data_ptr(), rowb + slack, **kw)
    eng.synchronize()
    rows = out.cpu().numpy().reshape(n, rowb + slack)
    assert (rows[:, rowb:] == 0xA5).all(), "written behind a row"
    return rows[:, :rowb], met.cpu().numpy().view(T.engine.METER_DTYPE)


@pytest.mark.parametrize("chain", [FULL, FX])
def test_gpu_pcm_cuts_and_events(chain):
    """with dither on: one device call with events, device calls cut 1 + 5 + 6 with frame0
    running, and host calls with controls by direct call, all deliver the model's bytes"""
    L, R, x = twin_planes(chain, 0)
    sc = RS.scens()
    want, wm = meters_of(M.S16, L, R, M.DITHER, SEED)
    eng = engine(chain)
    one, m = device_call(eng, sc, NB, M.S16, M.DITHER, x=x, slack=20)
    eng.close()
    for i in range(N):
        same_bytes(one[i], want[i], f"chain {chain}: one call with events, instance {i}")
    same_meters(m, wm, "one call with events")
    eng = engine(chain)
    parts, at = [], 0
    for c in (1, 5, 6):
        parts.append(device_call(eng, sc, c, M.S16, M.DITHER, b0=at, x=x)[0])
        at += c
    eng.close()
    same_bytes(np.concatenate(parts, axis=1), one, f"chain {chain}: 1 + 5 + 6 against one call")
    eng = engine(chain)
    host, _m, _s = host_calls(eng, sc, NB, M.S16, M.DITHER, x, cuts=[1, 5, 6])
    eng.close()
    same_bytes(host, one, f"chain {chain}: host calls cut 1 + 5 + 6 against one call")


@pytest.mark.parametrize("fmt,flags", [(M.S16, M.DITHER), (M.S24, 0)], ids=["s16-dither", "s24"])
def test_gpu_pcm_pieces_of_a_long_call(fmt, flags):
    """one call of 257 blocks crosses a scratch piece (256 blocks), with a rotor event at the
    second piece's first block: its bytes are those of two calls of 256 + 1, and of the model on a
    twin's planes, and its meters are numpy's over the whole call"""
    nb, n = 257, 1
    sc = [RS.scen(0) + [(256, "param", S.P_HORN, 1)]]
    eng = engine(n=n)
    one, m = device_call(eng, sc, nb, fmt, flags, n=n)
    eng.close()
    eng = engine(n=n)
    a, _ma = device_call(eng, sc, 256, fmt, flags, n=n)
    b, _mb = device_call(eng, sc, 1, fmt, flags, b0=256, n=n)
    eng.close()
    same_bytes(np.concatenate([a, b], axis=1), one, "257 blocks against 256 + 1")
    twin = engine(n=n)
    tl, tr = [], []
    for s, e in RS.stretches(sc, 0, nb):
        RS.apply(twin, sc, s)
        l, r = twin.render(e - s)
        tl.append(l)
        tr.append(r)
    twin.close()
    L, R = np.concatenate(tl, axis=1), np.concatenate(tr, axis=1)
    want, wm = meters_of(fmt, L, R, flags, SEED)
    same_bytes(one[0], want[0], "257 blocks against the model")
    same_meters(m, wm, "meters over 257 blocks")
    assert float(m["peakL"][0]) == float(np.abs(L).max()) > 1e-4


# ---------------------------------------------------------------- 4. composition with the rate converter
def test_gpu_pcm_behind_the_rate_converter():
    """render_resampled_device at 48000 -> 16000, then pcm_convert_device with its counts: the
    model on those rows"""
    import torch
    import tunebfree_amd as T
    sc = RS.scens()
    eng = engine(fo=16000)
    res, rows, _alloc = RS.one_call(eng, sc, NB, raw=False, stride=eng.resampled_frames(NB) + 5, lead=1)
    counts = res["counts"][0]
    assert counts.tolist() == [eng.resampled_frames(NB)] * N == [512] * N
    frames = int(counts.max())
    stride = frames + 5
    planes = [torch.from_numpy(np.ascontiguousarray(rows[k])).cuda() for k in ("L", "R")]
    for fmt, flags in M.FORMATS:
        rowb = frames * FB[fmt] + 12
        out = torch.full((N * rowb,), 0xA5, dtype=torch.uint8, device="cuda")
        met = torch.full((N * 4,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.pcm_convert_device(N, planes[0].data_ptr(), planes[1].data_ptr(), stride, frames, out.data_ptr(), rowb, fmt,
                               counts=counts, flags=flags, seed=SEED, frame0=1000, meters_ptr=met.data_ptr())
        eng.synchronize()
        got = out.cpu().numpy().reshape(N, rowb)
        want, wm = meters_of(fmt, res["L"], res["R"], flags, SEED, [1000] * N)
        for i in range(N):
            same_bytes(got[i, :counts[i] * FB[fmt]], want[i], f"format {fmt}: resampled row {i}")
            assert (got[i, counts[i] * FB[fmt]:] == 0xA5).all()
        same_meters(met.cpu().numpy().view(T.engine.METER_DTYPE), wm, f"format {fmt}: meters of the resampled rows")
    eng.close()


# ---------------------------------------------------------------- 5. refusals
def test_gpu_pcm_refusals_render_nothing():
    """refused calls render nothing and step no control: the buffers keep their fill and the next
    render delivers what a twin's first render delivers"""
    import torch
    import tunebfree_amd as T
    lib = T.load_library()
    L, R, _x = twin_planes(FULL, 0)
    sc = RS.scens()
    eng = engine()
    nb = 1
    rowb = nb * 128 * 8
    buf = torch.full((N * rowb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    met = torch.full((N * 4,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ev = RS.event_rows(eng, sc, 0, 1)
    assert len(ev) > 0

    def call(out=buf.data_ptr(), stride=rowb, meters=met.data_ptr(), fmt=M.S16, flags=0, e=ev):
        po = T.engine.PcmOut(out, stride, meters, fmt, flags, 0, 0, None)
        return lib.tbf_render_pcm_device(eng._h, nb, e.ctypes.data, len(e), C.byref(po), None)
    assert call(fmt=3) == -22 and call(flags=2) == -22
    assert call(fmt=M.S24, flags=M.DITHER) == -22 and call(fmt=M.F32, flags=M.DITHER) == -22
    assert call(out=None) == -22
    assert call(stride=nb * 128 * 4 - 4) == -22 and call(stride=nb * 128 * 4 + 2) == -22
    assert call(fmt=M.F32, stride=rowb - 4) == -22
    assert call(out=buf.data_ptr() + 2) == -22 and call(meters=met.data_ptr() + 2) == -22
    assert call(meters=buf.data_ptr() + 32) == -22  # the meters inside the frames
    assert call(e=eng.events([(0, 0, 0, 60, 1.0), (1, 0, 0, 62, 1.0)])[::-1].copy()) == -22  # events out of order
    x = torch.zeros((N, 128), dtype=torch.float32, device="cuda")
    po = T.engine.PcmOut(buf.data_ptr(), rowb, None, M.S16, 0, 0, 0, None)
    assert lib.tbf_process_pcm_device(eng._h, nb, None, 0, x.data_ptr(), 128, C.byref(po), None) == -22  # the wrong family
    cnt = np.array([129, 0, 0], np.uint32)
    assert lib.tbf_pcm_convert_device(eng._h, N, x.data_ptr(), x.data_ptr(), 128, 128, cnt.ctypes.data, C.byref(po), None) == -22
    assert lib.tbf_pcm_convert_device(eng._h, N, x.data_ptr(), buf.data_ptr() + 64, 128, 128, None, C.byref(po), None) == -22
    eng.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all() and (met.cpu().numpy() == -1).all()
    got, _m, _s = host_calls(eng, sc, NB, M.F32, 0)
    eng.close()
    got = got.view(np.float32).reshape(N, NB * 128, 2)
    RS.same(got[:, :, 0], L, "after the refusals, L")
    RS.same(got[:, :, 1], R, "after the refusals, R")


# ---------------------------------------------------------------- 6. accounting
def test_gpu_pcm_accounting():
    """the stage holds no instance or stage memory and launches no render kernel of its own:
    device_bytes () is what it was, a converter call leaves launches () alone, and a PCM render
    counts the launches of a plain render"""
    import torch
    eng = engine()
    eng.render(2)
    b0, l0 = eng.device_bytes(), eng.launches()
    eng.render(2)
    l1 = eng.launches()
    plain = {k: l1[k] - l0[k] for k in l0}
    assert sum(plain.values()) > 0
    x = torch.zeros((N, 256), dtype=torch.float32, device="cuda")
    out = torch.zeros((N * 256 * 8,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for fmt, flags in M.FORMATS:
        eng.pcm_convert_device(N, x.data_ptr(), x.data_ptr(), 256, 256, out.data_ptr(), 256 * FB[fmt], fmt, flags=flags)
    eng.synchronize()
    assert eng.launches() == l1 and eng.device_bytes() == b0
    for fmt, flags in M.FORMATS:
        before = eng.launches()
        eng.render_pcm(2, fmt, flags, meters=True)
        after = eng.launches()
        assert {k: after[k] - before[k] for k in after} == plain
        assert eng.device_bytes() == b0
    eng.pcm_time(True)
    eng.render_pcm(2)
    ms, n = eng.pcm_time()
    assert n == 1 and ms > 0.0
    eng.pcm_time(False)
    eng.close()
