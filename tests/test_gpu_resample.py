"""The output rate converter on the GPU (tbf_render_resampled* / tbf_process_resampled*,
k_resample): identity in bits with the host restatement of the definition
(tbf_debug_resample_ref) on the call's own engine-rate rows, those rows against a twin engine's
plain render, cut invariance bit for bit, the state through clone / save / load / remove / add,
positions across 2^32, the device-memory contract and the memory accounting.

The converter is this project's own definition (include/tbf.h); its
arithmetic against float64 is checked without a GPU (tests/test_resample_cpu.py).  Everything
here is an identity in bits."""
import ctypes as C

import numpy as np
import pytest

import resample_model as M
import scenarios as S

pytestmark = pytest.mark.gpu

FULL, FX = 0, 4
N = 3
NB = 12
SEEDS = [4100 + 37 * i for i in range(N)]
PAIRS = [(fi, fo) for (fi, fo, *_r) in M.PAIRS]
CUT_PAIRS = [(48000, 8000), (48000, 22050)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} of {a.size} differ, first at {tuple(bad[0])}")


def same_rows(a, b, what):
    """two lists of per-instance rows (the rows differ in length between instances)"""
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        same(x, y, f"{what}, instance {i}")


def scen(i):
    """a held chord plus rotor speed changes at block 3"""
    return S.bench_scenario(i) + [(3, "param", S.P_DRUM, 2), (3, "param", S.P_HORN, 2)]


def scens(n=N):
    return [scen(i) for i in range(n)]


def noise(nb, n=N, seed=11):
    return (np.random.default_rng(seed).standard_normal((n, nb * 128)) * 0.1).astype(np.float32)


def engine(fi=48000, fo=None, chain=FULL, n=N, whirl_out=0, seeds=None):
    import tunebfree_amd as T
    eng = T.Engine(sample_rate=float(fi), device=0, chain=chain, whirl_out=whirl_out)
    if fo is not None:
        eng.set_output_rate(fo)
    tid = eng.template(seed=7)
    if n:
        eng.add_instances([tid] * n, (seeds or SEEDS)[:n])
    return eng


def apply(eng, sc, s, insts=None):
    for i, script in enumerate(sc):
        for (b, kind, a, v) in script:
            if b != s:
                continue
            k = i if insts is None else insts[i]
            if kind == "note":
                eng.note(k, a, v)
            else:
                eng.set_param(k, a, v)


def stretches(sc, b0, b1, cuts=None):
    bounds = {b0, b1}
    for script in sc:
        bounds.update(b for (b, *_r) in script if b0 < b < b1)
    at = b0
    for c in cuts or []:
        at += c
        if at < b1:
            bounds.add(at)
    bounds = sorted(bounds)
    return list(zip(bounds[:-1], bounds[1:]))


def run_calls(eng, sc, b0, b1, cuts=None, x=None, raw=True, insts=None):
    """blocks [b0, b1) as host calls: one per stretch between the scripts' events and the cut
    points, controls by direct call in between.  Returns L, R as lists of per-instance rows (each
    call's [0, counts[i]) joined), rawL / rawR as arrays (with raw) and the counts per call."""
    n = eng.n_instances
    L, R = [[] for _ in range(n)], [[] for _ in range(n)]
    rawL, rawR, counts = [], [], []
    for s, e in stretches(sc, b0, b1, cuts):
        apply(eng, sc, s, insts)
        out = eng.render_resampled(e - s, raw=raw) if x is None else eng.process_resampled(x[:, s * 128:e * 128], raw=raw)
        c = out[-1]
        assert c.dtype == np.uint32 and len(c) == n
        for i in range(n):
            assert c[i] <= out[0].shape[1]
            L[i].append(out[0][i, :c[i]])
            R[i].append(out[1][i, :c[i]])
            assert not out[0][i, c[i]:].any() and not out[1][i, c[i]:].any()  # nothing written behind the count
        if raw:
            rawL.append(out[2])
            rawR.append(out[3])
        counts.append(c.copy())
    res = {"L": [np.concatenate(r) for r in L], "R": [np.concatenate(r) for r in R], "counts": counts}
    if raw:
        res["rawL"], res["rawR"] = np.concatenate(rawL, axis=1), np.concatenate(rawR, axis=1)
    return res


def event_rows(eng, sc, b0, b1):
    rows = []
    for i, script in enumerate(sc):
        for (b, kind, a, v) in script:
            if b0 <= b < b1:
                rows.append((b - b0, i, 0, a, float(v)) if kind == "note" else (b - b0, i, 1, a, float(v)))
    rows.sort(key=lambda r: r[0])
    return eng.events(rows)


def one_call(eng, sc, nb, b0=0, raw=True, stride=None, raw_stride=None, lead=0, fill=0.0, x=None):
    """One device call with the scripts' events of [b0, b0 + nb), into torch buffers of the given
    row strides that start `lead` floats into their allocation and are filled with `fill`.
    Returns the result as run_calls does, plus the whole rows and raw allocations by name."""
    import torch
    n = eng.n_instances
    stride = stride or eng.resampled_frames(nb)
    raw_stride = raw_stride or nb * 128
    names = ("L", "R") + (("rawL", "rawR") if raw else ())
    size = {k: (stride if k in ("L", "R") else raw_stride) for k in names}
    flat = {k: torch.full((lead + n * size[k],), fill, dtype=torch.float32, device="cuda") for k in names}
    ptr = {k: t.data_ptr() + 4 * lead for k, t in flat.items()}
    rp = (ptr["rawL"], ptr["rawR"]) if raw else None
    ev = event_rows(eng, sc, b0, b0 + nb)
    if x is None:
        counts = eng.render_resampled_device(nb, (ptr["L"], ptr["R"]), stride, rp, raw_stride, events=ev)
    else:
        xt = torch.from_numpy(np.ascontiguousarray(x[:, b0 * 128:(b0 + nb) * 128])).cuda()
        torch.cuda.synchronize()
        counts = eng.process_resampled_device(nb, xt.data_ptr(), xt.shape[1], (ptr["L"], ptr["R"]), stride, rp, raw_stride,
                                              events=ev)
    counts = counts.copy()  # filled before the call returned: no synchronisation needed for them
    eng.synchronize()
    alloc = {k: t.cpu().numpy() for k, t in flat.items()}
    rows = {k: a[lead:].reshape(n, size[k]) for k, a in alloc.items()}
    res = {"L": [rows["L"][i, :counts[i]] for i in range(n)], "R": [rows["R"][i, :counts[i]] for i in range(n)],
           "counts": [counts]}
    if raw:
        res["rawL"], res["rawR"] = rows["rawL"][:, :nb * 128], rows["rawR"][:, :nb * 128]
    return res, rows, alloc


def check_ref(eng, res, what, pos0=0, hist=None):
    """L / R over [0, counts[i]) against the host restatement on the raw rows, in bits"""
    assert float(np.abs(res["rawL"]).max()) > 1e-4, f"{what}: silent"
    for ch in "LR":
        for i, row in enumerate(res["raw" + ch]):
            want = eng.resample_ref(row, None if hist is None else hist[ch][i], pos0)
            assert len(want) == len(res[ch][i]) > 0, (what, ch, i, len(want), len(res[ch][i]))
            same(res[ch][i], want, f"{what}: {ch}[{i}] against resample_ref")


# ---------------------------------------------------------------- 1. identity with the host restatement
@pytest.mark.parametrize("chain", [FULL, FX])
@pytest.mark.parametrize("fi,fo", PAIRS)
def test_gpu_resample_identity(fi, fo, chain):
    x = noise(NB) if chain == FX else None
    sc = scens()
    eng = engine(fi, fo, chain)
    info = eng.resampler_info(table=False)
    L, Mm = info["L"], info["M"]
    res, _rows, _alloc = one_call(eng, sc, NB, x=x)
    assert res["counts"][0].tolist() == [M.count(NB * 128, L, Mm)] * N
    twin = engine(fi, None, chain)
    tl, tr = [], []
    for s, e in stretches(sc, 0, NB):
        apply(twin, sc, s)
        l, r = twin.render(e - s) if x is None else twin.process(x[:, s * 128:e * 128])
        tl.append(l)
        tr.append(r)
    twin.close()
    same(res["rawL"], np.concatenate(tl, axis=1), f"{fi} -> {fo} chain {chain}: rawL against a twin's render")
    same(res["rawR"], np.concatenate(tr, axis=1), f"{fi} -> {fo} chain {chain}: rawR against a twin's render")
    check_ref(eng, res, f"{fi} -> {fo} chain {chain}")
    eng.close()


@pytest.mark.parametrize("fi,fo,what", [
    (48000, 47900, "L = 479: the phase table is too large for LDS and is read from memory"),
    (48000, 500, "L = 1, M = 96, T = 6144: a tile's window has no room for all taps, so they are staged in two "
                 "segments; and the history is longer than the call"),
    (48000, 32000, "L = 2: two phases in LDS")])
def test_gpu_resample_identity_other_kernel_paths(fi, fo, what):
    """the pairs above each take another path through k_resample than the four of the issue"""
    sc = scens()
    eng = engine(fi, fo)
    res, _rows, _alloc = one_call(eng, sc, NB)
    check_ref(eng, res, f"{fi} -> {fo} ({what})")
    more = run_calls(eng, sc, NB, NB + 2, cuts=[1])  # two more one-block calls: the long history shifts
    for ch in "LR":
        for i in range(N):
            whole = eng.resample_ref(np.concatenate([res["raw" + ch][i], more["raw" + ch][i]]))
            same(np.concatenate([res[ch][i], more[ch][i]]), whole, f"{fi} -> {fo}: {ch}[{i}] over both stretches")
    eng.close()


def test_gpu_resample_identity_direct_sum():
    """a post-stage on whatever L / R whirl_out delivers: whirlProc's direct sum"""
    sc = scens()
    eng = engine(48000, 22050, whirl_out=1)
    res, _rows, _alloc = one_call(eng, sc, NB)
    twin = engine(48000, None, whirl_out=1)
    tw = [(apply(twin, sc, s), twin.render(e - s))[1] for s, e in stretches(sc, 0, NB)]
    twin.close()
    same(res["rawL"], np.concatenate([t[0] for t in tw], axis=1), "direct sum: rawL against a twin's render")
    same(res["rawR"], np.concatenate([t[1] for t in tw], axis=1), "direct sum: rawR against a twin's render")
    check_ref(eng, res, "direct sum")
    eng.close()


# ---------------------------------------------------------------- 2. cut invariance
@pytest.mark.parametrize("chain", [FULL, FX])
@pytest.mark.parametrize("fi,fo", CUT_PAIRS)
def test_gpu_resample_cut_invariance(fi, fo, chain):
    x = noise(NB) if chain == FX else None
    sc = scens()

    def variant(how):
        eng = engine(fi, fo, chain)
        if how == "one call":
            p = one_call(eng, sc, NB, x=x)[0]
        elif how == "one call, steady chunk 64":
            assert eng.set_steady_chunk(64) == 64
            p = one_call(eng, sc, NB, x=x)[0]
        elif how == "one call, engine scratch":
            p = one_call(eng, sc, NB, x=x, raw=False)[0]
        elif how == "12 calls":
            p = run_calls(eng, sc, 0, NB, cuts=[1] * NB, x=x)
        elif how == "12 calls, engine scratch":
            p = run_calls(eng, sc, 0, NB, cuts=[1] * NB, x=x, raw=False)
        else:
            p = run_calls(eng, sc, 0, NB, cuts=[1, 5, 6], x=x)
        eng.close()
        return p
    ref = variant("one call")
    assert float(np.abs(ref["L"][0]).max()) > 1e-4
    for how in ("12 calls", "1 + 5 + 6", "one call, steady chunk 64", "one call, engine scratch", "12 calls, engine scratch"):
        got = variant(how)
        for k in ("L", "R"):
            same_rows(got[k], ref[k], f"{fi} -> {fo} chain {chain}: {how} against one call, {k}")
        assert sum(int(c[0]) for c in got["counts"]) == len(ref["L"][0])
        if "rawL" in got:
            same(got["rawL"], ref["rawL"], f"{how}: rawL")


def test_gpu_resample_pieces_of_a_long_call():
    """a call without raw planes longer than a scratch piece (256 blocks), one instance, with a
    rotor event inside the second piece, against the same call with the caller's raw planes"""
    nb = 260
    sc = [scen(0) + [(257, "param", S.P_HORN, 1)]]
    out = []
    for raw in (True, False):
        eng = engine(48000, 22050, n=1)
        p = one_call(eng, sc, nb, raw=raw)[0]
        eng.close()
        out.append(p)
    assert out[0]["counts"][0].tolist() == out[1]["counts"][0].tolist() == [M.count(nb * 128, 147, 320)]
    for k in ("L", "R"):
        same_rows(out[1][k], out[0][k], f"pieces against one piece, {k}")


# ---------------------------------------------------------------- 3. state
def test_gpu_resample_state_clone_and_rewind():
    sc = scens()
    eng = engine(48000, 22050)
    run_calls(eng, sc, 0, 5)
    blob = eng.save(list(range(N)))
    assert eng.clone(1) == N
    a = run_calls(eng, sc + [sc[1]], 5, NB)
    for k in ("L", "R"):
        same(a[k][N], a[k][1], f"the clone's next blocks, {k}")
        assert not np.array_equal(bits(a[k][0]), bits(a[k][1]))
    eng.remove([N])
    eng.load(list(range(N)), blob)
    b = run_calls(eng, sc, 5, NB)
    eng.close()
    for k in ("L", "R"):
        same_rows(b[k], a[k][:N], f"rewind: blocks 5..12 again, {k}")
    assert [c.tolist() for c in b["counts"]] == [c[:N].tolist() for c in a["counts"]]


def test_gpu_resample_state_remove_and_late_instance():
    """removing the middle instance leaves the survivors' later samples unchanged; an instance
    added after 5 blocks has P = 0 beside the others' 640, so counts differ within one launch,
    and it renders a fresh engine's first samples"""
    sc = scens()
    eng, twin = engine(48000, 22050), engine(48000, 22050)
    run_calls(eng, sc, 0, 5)
    run_calls(twin, sc, 0, 5)
    assert eng.remove([1]).tolist() == [0, -1, 1]
    assert eng.add_instances([0], [SEEDS[1] + 5]) == 2
    late = [(5 + b, kind, a_, v) for (b, kind, a_, v) in scen(1)]
    a = run_calls(eng, [sc[0], sc[2], late], 5, NB)
    b = run_calls(twin, sc, 5, NB)
    twin.close()
    eng.close()
    for k in ("L", "R"):
        same_rows(a[k][:2], [b[k][0], b[k][2]], f"the survivors' next blocks, {k}")
    # (640 * 147 / 320 is an integer, so the late instance's counts equal the others' although its
    # output indices do not; tests 4 and 5 have counts that differ within a launch)
    at = 5 * 128
    for c, (s, e) in zip(a["counts"], stretches([late], 5, NB)):
        n_in = (e - s) * 128
        assert c.tolist() == [M.count(p + n_in, 147, 320) - M.count(p, 147, 320) for p in (at, at, at - 640)]
        at += n_in
    fresh = engine(48000, 22050, n=1, seeds=[SEEDS[1] + 5])
    f = run_calls(fresh, [scen(1)], 0, NB - 5)
    fresh.close()
    for k in ("L", "R"):
        same(a[k][2], f[k][0], f"a late instance against a fresh engine, {k}")
    assert [int(c[2]) for c in a["counts"]] == [int(c[0]) for c in f["counts"]]


# ---------------------------------------------------------------- 4. positions across 2^32
def test_gpu_resample_position_across_2_32():
    L, Mm = 147, 320
    pos = ((1 << 32) // L) // 128 * 128 - 128  # n M passes 2^32 inside the next two blocks
    n0, n1 = M.count(pos, L, Mm), M.count(pos + 256, L, Mm)
    assert n0 * Mm < (1 << 32) <= (n1 - 1) * Mm
    sc = scens()
    eng = engine(48000, 22050)
    for i in range(N):
        eng.resampler_pos(i, pos + 128 * i)  # the instances at different positions, one past the crossing sooner
    apply(eng, sc, 0)
    res = run_calls(eng, [[]] * N, 0, 2)
    for i in range(N):
        p = pos + 128 * i
        assert int(res["counts"][0][i]) == M.count(p + 256, L, Mm) - M.count(p, L, Mm)
        for ch in "LR":
            want = eng.resample_ref(res["raw" + ch][i], None, p)  # set before the first block: the history is zeros
            same(res[ch][i], want, f"{ch}[{i}] from position {p}")
    assert float(np.abs(res["L"][0]).max()) > 1e-6
    eng.close()


# ---------------------------------------------------------------- 5. the memory contract
@pytest.mark.parametrize("chain", [FULL, FX])
def test_gpu_resample_memory_contract(chain):
    fi, fo = 48000, 22050
    per = NB * 128
    x = noise(NB) if chain == FX else None
    sc = scens()
    eng = engine(fi, fo, chain)
    frames = eng.resampled_frames(NB)
    ref = one_call(eng, sc, NB, x=x)[0]
    eng.close()
    fill = 12345.5
    for raw in (True, False):
        eng = engine(fi, fo, chain)
        eng.resampler_pos(1, 1)  # instance 1 one sample on: its count differs
        got, rows, alloc = one_call(eng, sc, NB, x=x, raw=raw, stride=frames + 131, raw_stride=per + 77, lead=1, fill=fill)
        eng.close()
        counts = got["counts"][0]
        assert counts.tolist() == [M.count(p + per, 147, 320) - M.count(p, 147, 320) for p in (0, 1, 0)]
        for k in ("L", "R"):
            for i in (0, 2):
                same(got[k][i], ref[k][i], f"chain {chain} raw {raw}: odd stride rows, {k}[{i}]")
            for i in range(N):
                assert (rows[k][i, counts[i]:] == fill).all(), f"{k}[{i}]: written behind its count"
            assert alloc[k][0] == fill
        if raw:
            for k in ("rawL", "rawR"):
                same(got[k], ref[k], f"chain {chain}: odd stride raw rows, {k}")
                assert (rows[k][:, per:] == fill).all() and alloc[k][0] == fill, f"{k}: sentinel overwritten"


def test_gpu_resample_refusals_render_nothing():
    """the short-stride, overlap and missing-pointer -22s render nothing, step no control and
    leave P alone: the next call delivers what a fresh engine's first call delivers"""
    import torch
    import tunebfree_amd as T
    lib = T.load_library()
    sc = scens()
    eng = engine(48000, 22050)
    nb = 1
    frames = eng.resampled_frames(nb)
    buf = torch.full((4 * N * 256,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    base = buf.data_ptr()
    counts = np.full(N, 77, np.uint32)
    ev = event_rows(eng, sc, 0, 1)
    assert len(ev) > 0

    def call(L, R, rawL, rawR, stride, raw_stride, cnt=counts.ctypes.data):
        ro = T.engine.ResampledOut(L, R, rawL, rawR, stride, raw_stride, cnt)
        return lib.tbf_render_resampled_device(eng._h, nb, ev.ctypes.data, len(ev), C.byref(ro), None)
    plane = 4 * N * 256
    l, r, rl, rr = base, base + plane, base + 2 * plane, base + 3 * plane
    assert call(l, r, rl, rr, frames - 1, 128) == -22        # short stride
    assert call(l, r, rl, rr, frames, 127) == -22            # short raw stride
    assert call(l, l + 4 * (frames - 1), rl, rr, frames, 128) == -22  # R inside L's range
    assert call(l, r, rl, rl + 4 * 127, frames, 128) == -22  # the raw rows overlap
    assert call(l, r, r, rr, 256, 256) == -22                # rawL on R
    assert call(None, r, rl, rr, frames, 128) == -22
    assert call(l, r, None, rr, frames, 128) == -22          # half a pair
    assert call(l, r, rl, rr, frames, 128, None) == -22      # no counts
    eng.synchronize()
    assert (buf.cpu().numpy() == 7.0).all() and (counts == 77).all()
    got = one_call(eng, sc, NB)[0]
    eng.close()
    fresh = engine(48000, 22050)
    ref = one_call(fresh, sc, NB)[0]
    fresh.close()
    assert got["counts"][0].tolist() == ref["counts"][0].tolist()
    for k in ("L", "R"):
        same_rows(got[k], ref[k], f"after the refusals, {k}")


# ---------------------------------------------------------------- 6. accounting
@pytest.mark.parametrize("fi,fo", PAIRS)
def test_gpu_resample_device_bytes(fi, fo):
    """the history is 2 * pad4 (T - 1) * 4 B per instance, counted when a converter is set"""
    Tt = M.ratio(fi, fo)[2]
    share = 2 * ((Tt - 1 + 3) // 4 * 4) * 4
    eng, plain = engine(fi, fo), engine(fi, None)
    eng.render_resampled(1)
    plain.render(1)
    assert eng.device_bytes()[0] - plain.device_bytes()[0] == N * share
    eng.remove([1])
    plain.remove([1])
    assert eng.device_bytes()[0] - plain.device_bytes()[0] == (N - 1) * share
    eng.close()
    plain.close()


# ---------------------------------------------------------------- 7. timing
def test_gpu_resample_time():
    """resample_time counts k_resample's launches while it is on, hands them out once, and counts
    nothing while it is off: one instance, one block, the pair with the shortest filter (T 64)"""
    eng = engine(44100, 48000, n=1)
    eng.resample_time(True)
    for _ in range(2):
        eng.render_resampled(1)
    ms, n = eng.resample_time()
    assert n == 2 and ms > 0.0
    assert eng.resample_time() == (0.0, 0)
    eng.resample_time(False)
    eng.render_resampled(1)
    assert eng.resample_time() == (0.0, 0)
    eng.close()
