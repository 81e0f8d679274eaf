"""The seam between the output families (rotor planes, cabinet convolver, rate converter, PCM
frames, mixdown) on engines that have the cabinet and the converter set together: the other
feature's presence changes nothing, the families alternate on one engine as include/tbf.h states
(the chain underneath advances whichever family renders a block; the cabinet history advances in
cabinet calls alone, the converter's history, P and counts in resampled calls alone; a
convolution.mix taken in another family's call is what the next cabinet call mixes with), the
same plan as device calls queued on one stream without a synchronize (every family works in the
engine's one scratch, which regrows on the way), the state record with both histories through
clone, save, load, rewind, remove and a late add, the accounting, and the cabinet at other rates
and whirl outputs and in front of the mixdown and PCM stages.

The references are the per-family suites' own: a twin engine's plain render_rotors (bit-exact
against the oracle elsewhere), Engine.resample_ref, pcm_ref and mix_ref, and cab_model.  The one
inequality is the cabinet's accuracy bound of test_gpu_cabinet.py (err_gpu <= 4 err_model); the two
"not vacuous" floors are its 1e-3; everything else is an identity in bits."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import cab_model as CM
import resample_model as RM
import scenarios as S


def _helpers(name):
    """the scenarios and call helpers of another test file, loaded under a name of their own so
    that pytest's own import of that file is not pre-empted"""
    spec = importlib.util.spec_from_file_location(f"_{name}_helpers_families", Path(__file__).with_name(f"test_{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CB = _helpers("gpu_cabinet")
RS = _helpers("gpu_resample")

pytestmark = pytest.mark.gpu

FULL, FX = 0, 4
N = 3
SEEDS = [6100 + 43 * i for i in range(5)]
PLANES = CB.PLANES
ROTORS = PLANES[4:]
same = CB.same
f32 = np.float32


def engine(fi=48000, fo=None, ir=None, chain=FULL, n=N, whirl_out=0, seeds=None):
    """an engine at fi Hz with a converter to fo (or none), a cabinet of the responses ir (or
    none) and n instances; with a converter, k_resample's launches are counted (resample_time)"""
    import tunebfree_amd as T
    eng = T.Engine(sample_rate=float(fi), device=0, chain=chain, whirl_out=whirl_out)
    if ir is not None:
        eng.set_cabinet(*ir)
    if fo is not None:
        eng.set_output_rate(fo)
        eng.resample_time(True)
    tid = eng.template(seed=7)
    if n:
        eng.add_instances([tid] * n, (seeds or SEEDS)[:n])
    return eng


def ran_both(eng, what):
    """the engine launched k_cabinet and k_resample"""
    assert eng.cabinet_info()["launches"] > 0, f"{what}: no k_cabinet launch"
    assert eng.resample_time()[1] > 0, f"{what}: no k_resample launch"


def loud(a, what):
    assert float(np.abs(a).max()) > 1e-4, f"{what}: silent"


# ---------------------------------------------------------------- 1. the other feature's presence changes nothing
@pytest.mark.parametrize("chain", [FULL, FX], ids=["full", "fx"])
@pytest.mark.parametrize("taps,fo", [(300, 22050), (129, 16000)])
def test_gpu_families_other_feature_changes_nothing(taps, fo, chain):
    nb, cuts = 18, [5, 7, 6]
    ir = CB.responses(taps)
    sc = CB.scens(nb)
    x = CB.noise(nb) if chain == FX else None
    what = f"taps {taps} -> {fo} chain {chain}"
    both, cab = engine(fo=fo, ir=ir, chain=chain), engine(ir=ir, chain=chain)
    assert both.cabinet_info()["partitions"] == (taps + 127) // 128
    p = CB.run_calls(both, sc, 0, nb, cuts=cuts, x=x)
    q = CB.run_calls(cab, sc, 0, nb, cuts=cuts, x=x)
    assert both.cabinet_info()["launches"] > 0 and both.resample_time()[1] == 0
    both.close()
    cab.close()
    for k in PLANES:
        same(p[k], q[k], f"{what}: cabinet calls with a converter set, {k}")
        loud(p[k], f"{what} {k}")
    both, conv = engine(fo=fo, ir=ir, chain=chain), engine(fo=fo, chain=chain)
    a = RS.run_calls(both, sc, 0, nb, cuts=cuts, x=x)
    b = RS.run_calls(conv, sc, 0, nb, cuts=cuts, x=x)
    assert both.resample_time()[1] > 0 and both.cabinet_info()["launches"] == 0
    both.close()
    conv.close()
    for k in ("L", "R"):
        RS.same_rows(a[k], b[k], f"{what}: resampled calls with a cabinet set, {k}")
        same(a["raw" + k], b["raw" + k], f"{what}: raw rows with a cabinet set, {k}")
        loud(a[k][0], f"{what} {k}")
    assert [c.tolist() for c in a["counts"]] == [c.tolist() for c in b["counts"]]
    assert sum(int(c[0]) for c in a["counts"]) == RM.count(nb * 128, *RM.ratio(48000, fo)[:2])


# ---------------------------------------------------------------- 2. alternating families on one engine
PLAN = [(0, "cab", 3), (3, "plain", 2), (5, "rs", 4), (9, "f32", 1), (10, "cab", 5), (15, "mix", 3), (18, "rot", 2),
        (20, "rs", 1), (21, "cab", 1), (22, "rs", 6), (28, "s16", 2)]
NB = 30
TAIL = [(30, "cab", 2), (32, "rs", 2)]  # behind the plan: the clone's and the rewind's four blocks
MIXV = [40, 100, 0]  # the convolution.mix control of block 5, per instance
CASES = {"48000-22050-mic": (48000, 22050, 0), "44100-48000-direct": (44100, 48000, 1)}
IR300 = CB.responses(300)


def plan_scripts(n=N):
    """every control on a call's first block: rotor speeds at 3 and 10, a note at 15, the mix at 5
    (inside a resampled call's stretch), a drawbar at 22"""
    return [S.bench_scenario(i) + [(3, "param", S.P_DRUM, 2), (3, "param", S.P_HORN, 2), (5, "control", "convolution.mix", MIXV[i]),
                                   (10, "param", S.P_HORN, 0), (10, "param", S.P_DRUM, 1), (15, "note", 40 + 3 * i, 1),
                                   (22, "param", S.P_DRAWBAR + 2, 3 + i)] for i in range(n)]


def mix_rows3():
    """two buses, pans and gains through the helper, then cross terms (test_gpu_mix's rows5, for three)"""
    import tunebfree_amd as T
    rows = T.params.mix_rows([0, 1, 0], [1.0, 0.7, 0.5], [-0.5, 0.25, 1.0])
    rows["lr"] = f32([0.1, 0.0, -0.2])
    rows["rl"] = f32([0.0, 0.25, 0.0])
    return rows


def host_call(eng, kind, nb):
    """one host call of a family; its outputs by name"""
    import tunebfree_amd as T
    if kind == "cab":
        return dict(zip(PLANES, eng.render_cabinet(nb, wet=True, rotors=True)))
    if kind == "plain":
        return dict(zip("LR", eng.render(nb)))
    if kind == "rot":
        return dict(zip(("L", "R") + ROTORS, eng.render_rotors(nb)))
    if kind == "mix":
        return dict(zip("LR", eng.render_mix(nb, mix_rows3(), 2)))
    if kind == "f32":
        return {"frames": eng.render_pcm(nb, fmt=T.engine.PCM_F32)}
    if kind == "s16":
        return dict(zip(("frames", "meters"), eng.render_pcm(nb, fmt=T.engine.PCM_S16, meters=True)))
    assert kind == "rs"
    L, R, rawL, rawR, c = eng.render_resampled(nb, raw=True)
    for i in range(len(c)):
        assert not L[i, c[i]:].any() and not R[i, c[i]:].any()  # nothing behind the count
    return {"L": [L[i, :c[i]].copy() for i in range(len(c))], "R": [R[i, :c[i]].copy() for i in range(len(c))],
            "rawL": rawL, "rawR": rawR, "counts": c.copy()}


def run_host(eng, sc, plan):
    """the plan as host calls, controls by direct call before the call whose first block they sit on"""
    out = []
    for b0, kind, nb in plan:
        CB.apply(eng, sc, b0)
        out.append(host_call(eng, kind, nb))
    return out


_cache = {}


def twin_run(case):
    """a twin with neither feature: the plan's 30 blocks through render_rotors, cut at the same
    boundaries, with the same controls; L, R and the rotor planes [N, 30 * 128], computed once"""
    if ("twin", case) not in _cache:
        fi, _fo, wo = CASES[case]
        twin, sc = engine(fi, whirl_out=wo), plan_scripts()
        parts = []
        for b0, _kind, nb in PLAN:
            CB.apply(twin, sc, b0)
            parts.append(twin.render_rotors(nb))
        twin.close()
        tw = dict(zip(("L", "R") + ROTORS, (np.concatenate(p, axis=1) for p in zip(*parts))))
        for k, v in tw.items():
            loud(v, f"twin {k}")
            v.setflags(write=False)
        _cache["twin", case] = tw
    return _cache["twin", case]


def host_run(case):
    """engine B with both features through the plan as host calls, then the state steps behind it
    (save, clone, four blocks, remove, load, the four blocks again); computed once per case"""
    if ("host", case) not in _cache:
        fi, fo, wo = CASES[case]
        eng, sc = engine(fi, fo, IR300, whirl_out=wo), plan_scripts()
        res = {"seg": [], "wet": []}
        for b0, kind, nb in PLAN:
            CB.apply(eng, sc, b0)
            if kind == "cab":
                res["wet"].append([eng.cabinet_info(i)["wet"] for i in range(N)])
            res["seg"].append(host_call(eng, kind, nb))
        res["info"] = eng.resampler_info(table=False)
        blob = eng.save(list(range(N)))
        res["clone"] = eng.clone(1)
        res["tail_a"] = run_host(eng, [[]] * (N + 1), TAIL)
        res["map"] = eng.remove([N]).tolist()
        eng.load(list(range(N)), blob)
        res["tail_b"] = run_host(eng, [[]] * N, TAIL)
        ran_both(eng, case)
        # the host restatement needs the engine's table: the references of the resampled calls now
        res["rs_ref"], res["rs_ref_twin"] = resample_refs(eng, res, twin_run(case))
        eng.close()
        _cache["host", case] = res
    return _cache["host", case]


def resample_refs(eng, res, tw):
    """per resampled call of the plan and channel, resample_ref's rows with (a) the header's
    history: the last T - 1 samples of the raw rows of the earlier resampled calls joined, zeros in
    front, and (b) the history a converter that had heard every block would hold: the twin's
    contiguous audio before the call"""
    Tt = res["info"]["T"]
    own, contiguous = [], []
    heard = {ch: np.zeros((N, Tt - 1), f32) for ch in "LR"}
    pos0 = 0
    for (b0, kind, nb), seg in zip(PLAN, res["seg"]):
        if kind != "rs":
            continue
        a, b = {}, {}
        for ch in "LR":
            before = np.concatenate([np.zeros((N, Tt - 1), f32), tw[ch][:, :b0 * 128]], axis=1)[:, -(Tt - 1):]
            a[ch] = [eng.resample_ref(seg["raw" + ch][i], heard[ch][i, -(Tt - 1):], pos0) for i in range(N)]
            b[ch] = [eng.resample_ref(seg["raw" + ch][i], before[i], pos0) for i in range(N)]
            heard[ch] = np.concatenate([heard[ch], seg["raw" + ch]], axis=1)
        own.append((pos0, a))
        contiguous.append(b)
        pos0 += nb * 128
    return own, contiguous


def span(b0, nb):
    return slice(b0 * 128, (b0 + nb) * 128)


def pcm_rows_equal(seg, L, R, fmt, what):
    """a PCM call's frames and meters against pcm_ref of the planes L, R, row = instance"""
    import tunebfree_amd as T
    for i in range(len(L)):
        wb, wm = T.Engine.pcm_ref(fmt, L[i], R[i], row=i)
        assert np.ascontiguousarray(seg["frames"][i]).tobytes() == wb.tobytes(), f"{what}: instance {i} frames"
        if "meters" in seg:
            assert seg["meters"][i].tobytes() == wm.tobytes(), f"{what}: instance {i} meters"
            assert float(wm["peakL"]) > 1e-4


@pytest.mark.parametrize("case", CASES)
def test_gpu_families_plan_chain_continuity(case):
    """whichever family renders a block, the chain underneath advances as a twin's render_rotors"""
    import tunebfree_amd as T
    tw, res = twin_run(case), host_run(case)
    for (b0, kind, nb), seg in zip(PLAN, res["seg"]):
        s, what = span(b0, nb), f"{case}: {kind} at block {b0}"
        L, R = tw["L"][:, s], tw["R"][:, s]
        if kind in ("cab", "rot"):
            for k in ROTORS:
                same(seg[k], tw[k][:, s], f"{what}, {k} against the twin")
        if kind in ("plain", "rot"):
            same(seg["L"], L, f"{what}, L against the twin")
            same(seg["R"], R, f"{what}, R against the twin")
        elif kind == "rs":
            same(seg["rawL"], L, f"{what}, rawL against the twin")
            same(seg["rawR"], R, f"{what}, rawR against the twin")
        elif kind == "f32":
            same(seg["frames"][:, :, 0], L, f"{what}, frames' L against the twin")
            same(seg["frames"][:, :, 1], R, f"{what}, frames' R against the twin")
            pcm_rows_equal(seg, L, R, T.engine.PCM_F32, what)
        elif kind == "s16":
            pcm_rows_equal(seg, L, R, T.engine.PCM_S16, what)
        elif kind == "mix":
            wL, wR = T.Engine.mix_ref(L, R, mix_rows3(), 2)
            same(seg["L"], wL, f"{what}, bus L against mix_ref of the twin")
            same(seg["R"], wR, f"{what}, bus R against mix_ref of the twin")
            loud(wL, what)
    if CASES[case][2]:  # the direct sum is another signal than the microphone mix of the same planes
        mic = engine(CASES[case][0], n=1)
        CB.apply(mic, plan_scripts(1), 0)
        assert not np.array_equal(CB.bits(mic.render(3)[0][0]), CB.bits(tw["L"][0, :3 * 128]))
        mic.close()


@pytest.mark.parametrize("case", CASES)
def test_gpu_families_plan_cabinet(case):
    """the cabinet hears its own calls' blocks alone: accuracy on the joined horn planes of the
    cabinet calls, the law per call with the mix in effect (the control of block 5 arrived in a
    resampled call), and not the convolution of the unspliced stream"""
    tw, res = twin_run(case), host_run(case)
    cabs = [(b0, nb, seg) for (b0, kind, nb), seg in zip(PLAN, res["seg"]) if kind == "cab"]
    assert [nb for _b0, nb, _s in cabs] == [3, 5, 1]
    joined = {k: np.concatenate([seg[k] for _b0, _nb, seg in cabs], axis=1) for k in PLANES}
    CB.check_accuracy(joined, IR300, f"{case}: the cabinet calls' 9 blocks joined")
    for (b0, _nb, seg), wet in zip(cabs, res["wet"]):
        want = [1.0] * N if b0 < 5 else [f32(v / 127.0) for v in MIXV]
        assert wet == [f32(w) for w in want], (b0, wet)
        CB.check_law(seg, f32(wet)[:, None], f"{case}: cabinet call at block {b0}")
        loud(seg["wetL"], f"{case}: wet at block {b0}")
    for ch, h in zip("LR", IR300):
        for i in range(N):
            whole = CM.direct64(tw["horn" + ch][i], h)
            there = np.concatenate([whole[span(b0, nb)] for b0, nb, _s in cabs])
            scale = np.abs(joined["horn" + ch][i]).max() * np.abs(h.astype(np.float64)).sum()
            assert np.abs(joined["wet" + ch][i] - there).max() / scale > 1e-3, f"{case}: {ch}[{i}] is the unspliced stream's"


@pytest.mark.parametrize("case", CASES)
def test_gpu_families_plan_converter(case):
    """the converter hears its own calls' blocks alone: each resampled call's rows are resample_ref
    of its raw rows behind the raw rows of the earlier resampled calls, P counts those alone"""
    fi, fo, _wo = CASES[case]
    res = host_run(case)
    info = res["info"]
    L, Mm, Tt = info["L"], info["M"], info["T"]
    assert (L, Mm, Tt) == RM.ratio(fi, fo)
    segs = [(b0, nb, seg) for (b0, kind, nb), seg in zip(PLAN, res["seg"]) if kind == "rs"]
    assert [nb for _b0, nb, _s in segs] == [4, 1, 6]
    if fo == 22050:  # the one-block call feeds fewer samples than the history holds: it shifts the old history up
        assert 128 < Tt - 1 == 139
    differ = 0
    for (b0, nb, seg), (pos0, want), other in zip(segs, res["rs_ref"], res["rs_ref_twin"]):
        assert seg["counts"].tolist() == [RM.count(pos0 + nb * 128, L, Mm) - RM.count(pos0, L, Mm)] * N
        for ch in "LR":
            for i in range(N):
                assert len(want[ch][i]) == seg["counts"][i] > 0
                same(seg[ch][i], want[ch][i], f"{case}: resampled call at block {b0}, {ch}[{i}] against resample_ref")
                differ += not np.array_equal(CB.bits(seg[ch][i]), CB.bits(other[ch][i]))
        loud(seg["L"][0], f"{case}: resampled call at block {b0}")
    assert differ > 0, "a converter that heard every block would deliver the same rows"


def tails_equal(a, b, ia, ib, what):
    """instances ia of the tail a against instances ib of the tail b: cabinet planes, rows, counts"""
    for k in PLANES:
        same(a[0][k][ia], b[0][k][ib], f"{what}, {k}")
    for k in ("L", "R"):
        RS.same_rows([a[1][k][i] for i in ia], [b[1][k][i] for i in ib], f"{what}, resampled {k}")
        same(a[1]["raw" + k][ia], b[1]["raw" + k][ib], f"{what}, raw{k}")
    assert a[1]["counts"][ia].tolist() == b[1]["counts"][ib].tolist()


@pytest.mark.parametrize("case", CASES)
def test_gpu_families_plan_state_travels(case):
    """the record with both histories: a clone made at block 30 renders its source's next
    [cabinet 2][resampled 2]; with the clone removed and the blob of block 30 loaded, the same
    four blocks come again"""
    res = host_run(case)
    a, b = res["tail_a"], res["tail_b"]
    assert res["clone"] == N and res["map"] == [0, 1, 2, -1]
    tails_equal(a, a, [N], [1], f"{case}: the clone against instance 1")
    tails_equal(b, a, [0, 1, 2], [0, 1, 2], f"{case}: rewind")
    loud(a[0]["wetL"], case)
    loud(a[1]["L"][1], case)
    assert not np.array_equal(CB.bits(a[0]["wetL"][0]), CB.bits(a[0]["wetL"][1]))
    L, Mm = res["info"]["L"], res["info"]["M"]
    p = 11 * 128  # P after the plan's resampled calls, the clone's too
    assert a[1]["counts"].tolist() == [RM.count(p + 256, L, Mm) - RM.count(p, L, Mm)] * (N + 1)


# ---------------------------------------------------------------- 3. the same plan as device calls on one stream
def device_plan(eng, sc, stream):
    """every call of the plan in its *_device form into torch buffers filled with NaN, a guard
    behind every row; controls as the call's events; no rotor planes to the cabinet calls and no
    raw rows to the resampled calls, so every family works in the engine's scratch; nothing waits
    until the last call is queued.  Returns per call the rows read back, by name."""
    import torch
    import tunebfree_amd as T
    E = T.engine
    G = 5  # guard floats behind a row
    bufs, counts = [], []

    def nan(rows, cols):
        return torch.full((rows, cols), float("nan"), dtype=torch.float32, device="cuda")
    for _b0, kind, nb in PLAN:
        per = nb * 128
        if kind == "cab":
            bufs.append({k: nan(N, per + G) for k in PLANES[:4]})
        elif kind == "plain":
            bufs.append({k: nan(N, per + G) for k in "LR"})
        elif kind == "rot":
            bufs.append({k: nan(N, per + G) for k in ("L", "R") + ROTORS})
        elif kind == "mix":
            bufs.append({k: nan(2, per + G) for k in "LR"})
        elif kind == "rs":
            bufs.append({k: nan(N, eng.resampled_frames(nb) + G) for k in "LR"})
        elif kind == "f32":
            bufs.append({"frames": nan(N, 2 * per + G)})
        else:
            bufs.append({"frames": torch.full((N, per * 4 + 4 * G), 0xA5, dtype=torch.uint8, device="cuda"),
                         "meters": torch.full((N * 4,), -1, dtype=torch.int32, device="cuda")})
    torch.cuda.synchronize()
    st = None if stream is None else stream.cuda_stream
    for (b0, kind, nb), t in zip(PLAN, bufs):
        per = nb * 128
        ev = CB.event_rows(eng, sc, b0, b0 + nb)
        assert len(ev) == 0 or int(ev["block"].max()) == 0  # every control sits on the call's first block
        p = {k: v.data_ptr() for k, v in t.items()}
        if kind == "cab":
            eng.render_cabinet_device(nb, [p[k] for k in PLANES[:4]], per + G, None, 0, events=ev, stream=st)
        elif kind == "plain":
            eng.render_events_device(nb, ev, p["L"], p["R"], per + G, stream=st)
        elif kind == "rot":
            eng.render_rotors_device(nb, p["L"], p["R"], per + G, [p[k] for k in ROTORS], per + G, events=ev, stream=st)
        elif kind == "mix":
            eng.render_mix_device(nb, mix_rows3(), 2, p["L"], p["R"], per + G, events=ev, stream=st)
        elif kind == "rs":
            counts.append(eng.render_resampled_device(nb, (p["L"], p["R"]), t["L"].shape[1], None, 0, events=ev, stream=st).copy())
        elif kind == "f32":
            eng.render_pcm_device(nb, p["frames"], 4 * (2 * per + G), E.PCM_F32, events=ev, stream=st)
        else:
            eng.render_pcm_device(nb, p["frames"], per * 4 + 4 * G, E.PCM_S16, meters_ptr=p["meters"], events=ev, stream=st)
    if stream is not None:
        stream.synchronize()
    eng.synchronize()
    return [{k: v.cpu().numpy() for k, v in t.items()} for t in bufs], counts


@pytest.mark.parametrize("where", ["engine-stream", "caller-stream"])
def test_gpu_families_plan_as_queued_device_calls(where):
    """the scratch all families share regrows between queued calls; every buffer holds what the
    host-call run of the plan delivered, and nothing is written behind a row"""
    import torch
    import tunebfree_amd as T
    case = "48000-22050-mic"
    fi, fo, wo = CASES[case]
    res = host_run(case)
    eng = engine(fi, fo, IR300, whirl_out=wo)
    got, counts = device_plan(eng, plan_scripts(), torch.cuda.Stream() if where == "caller-stream" else None)
    ran_both(eng, where)
    assert [eng.cabinet_info(i)["wet"] for i in range(N)] == [f32(v / 127.0) for v in MIXV]
    eng.close()
    counts = iter(counts)
    for (b0, kind, nb), g, want in zip(PLAN, got, res["seg"]):
        per, what = nb * 128, f"{where}: {kind} at block {b0}"
        if kind == "rs":
            c = next(counts)
            assert c.tolist() == want["counts"].tolist(), what
            for k in "LR":
                for i in range(N):
                    same(g[k][i, :c[i]], want[k][i], f"{what}, {k}[{i}]")
                    assert np.isnan(g[k][i, c[i]:]).all(), f"{what}: written behind {k}[{i}]'s count"
        elif kind == "s16":
            for i in range(N):
                assert g["frames"][i, :per * 4].tobytes() == want["frames"][i].tobytes(), f"{what}: instance {i} frames"
                assert (g["frames"][i, per * 4:] == 0xA5).all(), f"{what}: written behind row {i}"
            assert g["meters"].view(T.engine.METER_DTYPE).tobytes() == want["meters"].tobytes(), what
        elif kind == "f32":
            same(g["frames"][:, :2 * per], want["frames"].reshape(N, 2 * per), f"{what}, frames")
            assert np.isnan(g["frames"][:, 2 * per:]).all(), f"{what}: written behind a row"
        else:
            for k, rows in g.items():
                same(rows[:, :per], want[k], f"{what}, {k}")
                assert np.isnan(rows[:, per:]).all(), f"{what}: written behind a row of {k}"
                loud(want[k], what)


# ---------------------------------------------------------------- 4. remove, late add and accounting with both histories
def test_gpu_families_remove_late_add_and_accounting():
    n, fo = 5, 22050
    L, Mm, Tt = RM.ratio(48000, fo)
    sc = CB.scens(8, n)
    eng, twin, plain = engine(fo=fo, ir=IR300, n=n), engine(fo=fo, ir=IR300, n=n), engine(n=n)
    for e in (eng, twin):
        CB.run_calls(e, sc, 0, 4)
        RS.run_calls(e, sc, 4, 8)
    plain.render(1)
    share = eng.cabinet_info()["instance_bytes"] + 2 * ((Tt - 1 + 3) // 4 * 4) * 4
    assert eng.resampler_info(table=False)["T"] == Tt and eng.cabinet_info()["instance_bytes"] >= 2 * 2 * 128 * 4
    assert eng.device_bytes()[0] - plain.device_bytes()[0] == n * share
    assert eng.remove([1, 3]).tolist() == [0, -1, 1, -1, 2]
    plain.remove([1, 3])
    assert eng.device_bytes()[0] - plain.device_bytes()[0] == (n - 2) * share
    plain.close()
    keep = [0, 2, 4]
    quiet = [[]] * n
    a = (CB.run_calls(eng, quiet[:3], 8, 12), RS.run_calls(eng, quiet[:3], 12, 16))
    b = (CB.run_calls(twin, quiet, 8, 12), RS.run_calls(twin, quiet, 12, 16))
    twin.close()
    for k in PLANES:
        same(a[0][k], b[0][k][keep], f"the survivors' next cabinet blocks, {k}")
        loud(a[0][k], k)
    for k in ("L", "R"):
        RS.same_rows(a[1][k], [b[1][k][i] for i in keep], f"the survivors' next resampled blocks, {k}")
        loud(a[1][k][0], k)
    assert [c.tolist() for c in a[1]["counts"]] == [c[keep].tolist() for c in b[1]["counts"]]
    # a late instance: P = 0 beside the others' 1024, zero histories beside theirs
    assert eng.add_instances([0], [SEEDS[1] + 5]) == 3
    late = [[], [], [], [(16 + blk, kind, a_, v) for (blk, kind, a_, v) in CB.scen(1, 6)]]
    r = RS.run_calls(eng, late, 16, 19)
    p = CB.run_calls(eng, late, 19, 22)
    ran_both(eng, "remove and late add")
    CB.check_law(p, f32(1.0), "the cabinet call beside the late instance")
    assert len(r["counts"]) == 1
    old, new = RM.count(1024 + 384, L, Mm) - RM.count(1024, L, Mm), RM.count(384, L, Mm)
    assert old != new and r["counts"][0].tolist() == [old] * 3 + [new]
    for ch in "LR":
        same(r[ch][3], eng.resample_ref(r["raw" + ch][3], None, 0), f"the late instance's rows, {ch}")
        for i in range(3):  # the survivors: the history of their last resampled call, P = 1024
            hist = a[1]["raw" + ch][i, -(Tt - 1):]
            same(r[ch][i], eng.resample_ref(r["raw" + ch][i], hist, 1024), f"survivor {i} beside the late instance, {ch}")
        loud(r[ch][3], f"the late instance's {ch}")
    eng.close()
    fresh = {k: v[3:4] for k, v in p.items()}
    CB.check_accuracy(fresh, IR300, "the late instance's first cabinet blocks")
    CB.check_accuracy(fresh, IR300, "the late instance's first cabinet block", nb=1)
    for ch in "LR":
        nz = np.flatnonzero(fresh["horn" + ch][0])
        assert len(nz) > 0
        assert not fresh["wet" + ch][0, :nz[0] // 128 * 128].any(), "wet before the first horn sample"


# ---------------------------------------------------------------- 5. cabinet edges the cabinet suite leaves out
@pytest.mark.parametrize("fi,whirl_out", [(44100, 0), (96000, 0), (48000, 1)], ids=["44100", "96000", "48000-direct"])
def test_gpu_families_cabinet_at_other_rates_and_outputs(fi, whirl_out):
    nb = 12
    sc = CB.scens(nb)
    eng = engine(fi, ir=IR300, whirl_out=whirl_out)
    if fi == 96000:
        assert eng.layout()["wring_len"] == 1024
    p = CB.run_calls(eng, sc, 0, nb)
    assert eng.cabinet_info()["launches"] > 0
    eng.close()
    what = f"{fi} Hz whirl_out {whirl_out}"
    CB.check_accuracy(p, IR300, what)
    CB.check_law(p, f32(1.0), what)
    twin = engine(fi, whirl_out=whirl_out)
    q = CB.run_calls(twin, sc, 0, nb, call=lambda s, e: (lambda six: (six[0], six[1]) * 2 + tuple(six[2:]))(twin.render_rotors(e - s)))
    twin.close()
    for k in ROTORS:
        same(p[k], q[k], f"{what}: {k} against an engine without a cabinet")
        loud(p[k], k)
    loud(p["wetL"], what)
    for ch, other in zip("LR", IR300[::-1]):
        assert CM.err(p["wet" + ch][0], p["horn" + ch][0], other) > 1e-3


def test_gpu_families_cabinet_into_mix_into_pcm_on_one_stream():
    """render_cabinet_device, mix_device over the cabinet L / R and pcm_convert_device over the
    buses, queued on one stream with no synchronize in between: the bytes and meters of pcm_ref of
    mix_ref of the cabinet planes read back afterwards"""
    import torch
    import tunebfree_amd as T
    nb = 6
    per = nb * 128
    sc = CB.scens(nb)
    rows = mix_rows3()
    eng = engine(fo=22050, ir=IR300)
    cab = {k: torch.full((N, per), float("nan"), dtype=torch.float32, device="cuda") for k in "LR"}
    bus = {k: torch.full((2, per), float("nan"), dtype=torch.float32, device="cuda") for k in "LR"}
    pcm = torch.full((2, per * 6), 0xA5, dtype=torch.uint8, device="cuda")
    met = torch.full((2 * 4,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.render_cabinet_device(nb, [cab["L"].data_ptr(), cab["R"].data_ptr()], per, None, 0, events=CB.event_rows(eng, sc, 0, nb))
    eng.mix_device(N, cab["L"].data_ptr(), cab["R"].data_ptr(), per, per, rows, 2, bus["L"].data_ptr(), bus["R"].data_ptr(), per)
    eng.pcm_convert_device(2, bus["L"].data_ptr(), bus["R"].data_ptr(), per, per, pcm.data_ptr(), per * 6, T.engine.PCM_S24_3LE,
                           meters_ptr=met.data_ptr())
    eng.synchronize()
    assert eng.cabinet_info()["launches"] > 0
    eng.close()
    L, R = cab["L"].cpu().numpy(), cab["R"].cpu().numpy()
    loud(L, "cabinet L")
    wL, wR = T.Engine.mix_ref(L, R, rows, 2)
    same(bus["L"].cpu().numpy(), wL, "bus L against mix_ref of the cabinet planes")
    same(bus["R"].cpu().numpy(), wR, "bus R against mix_ref of the cabinet planes")
    got, gm = pcm.cpu().numpy(), met.cpu().numpy().view(T.engine.METER_DTYPE)
    for b in range(2):
        wb, wm = T.Engine.pcm_ref(T.engine.PCM_S24_3LE, wL[b], wR[b], row=b)
        assert got[b].tobytes() == wb.tobytes(), f"bus {b}: frames"
        assert gm[b].tobytes() == wm.tobytes(), f"bus {b}: meters"
        assert float(wm["peakL"]) > 1e-4
