"""Generate tests/golden/rotor_vectors.npz: the six outputs of the reference's whirlProc2
(outL, outR = whirlProc's direct sum; outHL, outHR, outDL, outDR = the horn and drum pairs) for
chosen cases of the committed ref_vectors_<i>.npz.  Run where the reference tree exists; the
archive is data only.

oracle/_ref/libtbfref.so exports whirlProc3 alone, so this script compiles rotor_shim.cpp (a few
extern "C" wrappers, next to this file) with the reference's src/whirl.cpp and src/eqcomp.cpp,
flags as oracle/Makefile's strict build, into a temporary directory.  Per case it feeds the
committed <case>/C stream (the reference's reverb output, the whirl's input) block by block
through whirlProc2 and replays the scenario's whirl-facing events (P_DRUM / P_HORN ->
useRevOption, P_WHIRL_BYPASS) the way oracle/ref_harness.cpp's ref_set_param maps them.  Before
anything is written it asserts that whirlProc3's mix of the four rotor streams, ((HL*hll +
HR*hlr) + DL*dll) + DR*dlr in float32, equals the committed <case>/L and /R bit for bit: that
ties the new vectors to the old ones and proves the replay.

The `levels` case has no committed L / R: whirl.horn.level and whirl.horn.leak are not the
defaults.  They reach nothing before the whirl, so its input is the C stream of its base case;
the script renders the full reference chain with that cfg (oracle/_ref/libtbfref.so), asserts
that its C is the committed one, and ties the rotor streams to that render's L / R instead.

Per case the npz holds <case>/L, /R, /HL, /HR, /DL, /DR and `cases`, the JSON case table
(name, base = the ref_vectors case, cfg = the cfg keys the engine needs, window = the compact
ring window the case is meant to cover).
"""
import ctypes as C
import json
import math
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import scenarios as S  # noqa: E402
from make_ref_vectors import load_vectors, scenario  # noqa: E402
from orc_bind import Cfg, Chain, Template, load_oracle, load_ref  # noqa: E402

REF_SRC = Path("/root/reference/src")
STRICT = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC"]  # oracle/Makefile STRICT

# name, base case of ref_vectors, cfg keys, ring window (tbf_debug_layout) the case covers:
# one per window; sweep48_3 goes fast -> stop -> fast -> stop, events192_p4 and events48 fast ->
# slow at block 32; the 72-block cases cross the engine's 64-block event chunk
CASES = [
    ("sweep48_3", "sweep48_3", {}, 512),
    ("bench96_p4", "bench96_p4", {}, 1024),
    ("events192_p4", "events192_p4", {}, 2048),
    ("levels48", "events48", {"whirl.horn.level": 0.55, "whirl.horn.leak": 0.3}, 512),
]

_fp = C.POINTER(C.c_float)


def _f(a):
    return a.ctypes.data_as(_fp)


def build_shim(tmp):
    so = Path(tmp) / "librotorshim.so"
    subprocess.run(["g++", "-std=c++17", *STRICT, "-DCLAP", f"-I{REF_SRC}", "-shared", "-o", str(so),
                    str(HERE / "rotor_shim.cpp"), str(REF_SRC / "whirl.cpp"), str(REF_SRC / "eqcomp.cpp"), "-lm"],
                   check=True)
    lib = C.CDLL(str(so))
    lib.rs_new.restype, lib.rs_new.argtypes = C.c_void_p, [C.c_double, C.c_int, C.c_double, C.c_double]
    lib.rs_free.argtypes = [C.c_void_p]
    lib.rs_rev_option.argtypes = [C.c_void_p, C.c_int]
    lib.rs_bypass.argtypes = [C.c_void_p, C.c_int]
    lib.rs_mic.argtypes = [C.c_void_p, _fp]
    lib.rs_proc2.argtypes = [C.c_void_p] + [_fp] * 7 + [C.c_int]
    return lib


def mic_mix(m, HL, HR, DL, DR):
    """whirlProc3's mix (src/whirl.cpp:1676-1680) in float32, left to right"""
    m = m.astype(np.float32)
    L = ((HL * m[0] + HR * m[1]) + DL * m[2]) + DR * m[3]
    R = ((HL * m[4] + HR * m[5]) + DL * m[6]) + DR * m[7]
    return L.astype(np.float32), R.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def whirl_events(scen):
    """the scenario's events that reach the whirl, by block, in order"""
    by_block = {}
    for (blk, kind, a, b) in scen:
        assert kind != "control", "whirl control functions are not replayed here"
        if kind == "param" and a in (S.P_DRUM, S.P_HORN, S.P_WHIRL_BYPASS):
            by_block.setdefault(blk, []).append((a, float(b)))
    return by_block


def proc2(shim, sr, cfg, scen, Cin):
    """the six whirlProc2 streams and the mic mix for input Cin under the scenario's events"""
    nb = len(Cin) // 128
    w = shim.rs_new(float(sr), 1 if cfg else 0, float(cfg.get("whirl.horn.level", 0)),
                    float(cfg.get("whirl.horn.leak", 0)))
    ev = whirl_events(scen)
    par = {S.P_DRUM: 1.0, S.P_HORN: 1.0}  # the CLAP defaults (oracle/orc_chain.c orc_param_defaults)
    out = [np.zeros(nb * 128, np.float32) for _ in range(6)]
    Cin = np.ascontiguousarray(Cin, np.float32)
    for b in range(nb):
        for (a, v) in ev.get(b, []):
            if a == S.P_WHIRL_BYPASS:
                shim.rs_bypass(w, int(round(v)))
            else:
                par[a] = float(np.float32(v))
                shim.rs_rev_option(w, int(math.floor(par[S.P_DRUM]) + 3 * math.floor(par[S.P_HORN])))
        o = b * 128
        shim.rs_proc2(w, _f(Cin[o:]), *[_f(x[o:]) for x in out], 128)
    m = np.zeros(8, np.float32)
    shim.rs_mic(w, _f(m))
    shim.rs_free(w)
    return out, m


def main():
    if not REF_SRC.is_dir():
        raise SystemExit(f"{REF_SRC} not found: the vectors are generated where the reference tree exists")
    vec = load_vectors()
    table = {t["name"]: t for t in json.loads(str(vec["cases"]))}
    orc, ref = load_oracle(), load_ref()
    if ref is None:
        raise SystemExit("oracle/_ref/libtbfref.so not built (make -C oracle ref)")
    tunings = json.loads((HERE / "tunings.json").read_text())
    out, cases = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        shim = build_shim(tmp)
        for (name, base, cfg, window) in CASES:
            t = table[base]
            scen = scenario(*t["scenario"])
            Cin, wantL, wantR = vec[f"{base}/C"], vec[f"{base}/L"], vec[f"{base}/R"]
            if cfg:
                # the reference's full chain with the cfg: the same C, its own L / R
                m128 = None if t["tuning"] is None else np.array(tunings[t["tuning"]], np.float64)
                c = Cfg(orc, cfg)
                ch = Chain(ref, Template(orc, sr=t["sr"], mts128=m128, seed=t["tpl_seed"]), t["inst_seed"], ref=True,
                           cfg=c)
                wantL, wantR, _, _, C2 = S.run(ch, scen, t["nblocks"], stages=True)
                assert np.array_equal(bits(C2), bits(Cin)), f"{name}: the cfg changed the whirl's input"
                assert not np.array_equal(bits(wantL), bits(vec[f"{base}/L"])), f"{name}: the cfg changed nothing"
            (L, R, HL, HR, DL, DR), m = proc2(shim, t["sr"], cfg, scen, Cin)
            mL, mR = mic_mix(m, HL, HR, DL, DR)
            assert np.array_equal(bits(mL), bits(wantL)), f"{name}: L of the replay is not the reference's"
            assert np.array_equal(bits(mR), bits(wantR)), f"{name}: R of the replay is not the reference's"
            for k, v in zip(("L", "R", "HL", "HR", "DL", "DR"), (L, R, HL, HR, DL, DR)):
                assert np.isfinite(v).all() and float(np.abs(v).max()) > 1e-3, (name, k)
                out[f"{name}/{k}"] = v
            differs = int((bits(L) != bits((HL + DL).astype(np.float32))).sum())
            print(f"{name}: {t['nblocks']} blocks at {t['sr']:.0f} Hz, mic {m.tolist()}, "
                  f"L != float32(HL + DL) on {differs} of {len(L)} samples")
            cases.append({"name": name, "base": base, "cfg": cfg, "window": window, "mic": [float(x) for x in m]})
    out["cases"] = np.array(json.dumps(cases))
    np.savez_compressed(HERE / "rotor_vectors.npz", **out)
    print(f"wrote rotor_vectors.npz: {len(cases)} cases, {(HERE / 'rotor_vectors.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main()
