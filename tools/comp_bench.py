#!/usr/bin/env python3
"""tools/comp_bench.py -- what the bus compressor costs.

k_comp alone: tbf_comp_device at 48 kHz over 4096 rows x 8192 frames and 2 rows x 480000 frames of
noise whose level wanders around the curve's threshold, at the rows-per-wave the library takes, with
and without a key pair, timed by the HIP events around its
launch (tbf_debug_comp_time), one query per call: the median of --reps calls behind --warmup, with
the least, the largest and the 10th and 90th percentiles.  Beside each shape stands the yardstick
from existing code in the same process: k_eq with one band at the same shape (tbf_debug_eq_time), a
9-operation double chain a frame in one lane.
  One wave: a compressor of R rows at layout R over --wave-frames frames is one wave on one SIMD;
its time per frame is the serial walk plus R times the parallel phases' share.  When two layouts are
given (two builds existed: 4 and 16), they give both: walk = (R2 t1 - R1 t2) / (R2 - R1) per frame.
Reported in cycles at 2.4 GHz.
  TBF_LIB names another build of the library (a kernel variant); --tag names it in the result and
--out says where the result goes, so that runs of two builds can alternate.  A variant that lays its
waves out by a switch of its own, not by the library's hook, says so with --variant-rows N: the record
then carries N as rows_per_wave (and "layout_from": "variant") and no layout is forced; --wave-rows
names the row counts of the one-wave cases when they are not the layouts.  Writes
profiles/comp/comp_bench.json by default and prints the result as one JSON line.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CLOCK_HZ = 2.4e9
SIMDS = 256 * 4
RATE = 48000


def spread(ms):
    import numpy as np
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]),
            "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)), "calls": len(a)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="*", default=[4096, 8192, 2, 480000], help="rows frames [rows frames ...]")
    ap.add_argument("--layouts", type=int, nargs="*", default=[0], help="rows per wave: 0 or what the library takes (a variant build: what its own switch takes)")
    ap.add_argument("--wave-frames", type=int, default=65536)
    ap.add_argument("--wave-rows", type=int, nargs="*", default=None, help="rows of the one-wave cases (default: the layouts)")
    ap.add_argument("--variant-rows", type=int, default=0, help="rows per wave of a variant build that ignores the library's layout")
    ap.add_argument("--reps", type=int, default=21, help="timed calls per case (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="k_comp")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "comp" / "comp_bench.json"))
    a = ap.parse_args()
    assert a.reps >= 20
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    import tunebfree_amd as T

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    eng = T.Engine(sample_rate=float(RATE), device=torch.cuda.current_device())
    P = T.params
    curve = P.comp_curve(-24.0, 4.0, 6.0)
    row = P.comp_row(0, 5.0, 120.0, 3.0, RATE)

    def timed(obj, call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        obj.timing(True)
        ms = []
        for _ in range(a.reps):
            call()
            torch.cuda.synchronize()
            t, n = obj.timing()
            assert n == 1
            ms.append(t)
        obj.timing(False)
        return spread(ms)

    def noise(B, F):
        # a level that wanders over six octaves around -24 dB, so that the gain moves all the time
        return torch.randn((B, F), dtype=torch.float32, device="cuda") * torch.exp2(torch.rand((B, F), device="cuda") * 6.0 - 7.0)

    def compressor(B, layout):
        comp = eng.compressor(B, 1)
        comp.set_curve(0, curve, stream=sp)
        comp.set_rows(row, stream=sp)
        assert a.variant_rows or layout in (0, T.Engine.comp_grid(B, 1)[0]), "the library has one layout for these rows"
        return comp

    cases = []
    for B, F in zip(a.shapes[0::2], a.shapes[1::2]):
        planes = [noise(B, F) for _ in range(2)]
        keys = [noise(B, F) for _ in range(2)]
        outs = [torch.empty((B, F), dtype=torch.float32, device="cuda") for _ in range(2)]
        eq = eng.equalizer(B, 1, RATE)
        eq.set([P.eq_band(P.EQ_HPF, 40.0)], stream=sp)
        yard = timed(eq, lambda: eq.process_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, outs[0].data_ptr(),
                                                   outs[1].data_ptr(), F, stream=sp))
        eq.close()
        rows = []
        for layout in a.layouts:
            for keyed in (False, True):
                rpw, tile, lds = T.Engine.comp_grid(B, 1)
                rpw = a.variant_rows or layout or rpw
                comp = compressor(B, layout)
                key = (keys[0].data_ptr(), keys[1].data_ptr(), F) if keyed else None
                r = timed(comp, lambda: comp.process_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, outs[0].data_ptr(),
                                                            outs[1].data_ptr(), F, key=key, stream=sp))
                waves = (B + rpw - 1) // rpw
                r.update(layout=layout, rows_per_wave=rpw, layout_from="variant" if a.variant_rows else "library", keyed=keyed, tile_frames=tile, waves=waves,
                         GB_per_s=B * F * (24 if keyed else 16) / r["median_ms"] * 1e-6, against_k_eq_1_band=r["median_ms"] / yard["median_ms"],
                         out_finite=bool(torch.isfinite(outs[0]).all().item()), moved=bool((outs[0] != planes[0]).any().item()))
                rows.append(r)
                comp.close()
        cases.append({"rows": B, "frames": F, "rate_hz": RATE, "k_eq_1_band": yard, "k_comp": rows})
        del planes, keys, outs
        torch.cuda.empty_cache()

    # one wave: R rows at layout R
    F = a.wave_frames
    wave = []
    for R in (a.wave_rows if a.wave_rows is not None else [x for x in a.layouts if x] or [T.Engine.comp_grid(1, 1)[0]]):
        planes = [noise(R, F) for _ in range(2)]
        outs = [torch.empty((R, F), dtype=torch.float32, device="cuda") for _ in range(2)]
        comp = compressor(R, R)
        r = timed(comp, lambda: comp.process_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, outs[0].data_ptr(),
                                                    outs[1].data_ptr(), F, stream=sp))
        r.update(rows_per_wave=a.variant_rows or R, rows=R, frames=F, cycles_per_frame=r["median_ms"] * 1e-3 / F * CLOCK_HZ)
        wave.append(r)
        comp.close()
    split = None
    if len(wave) >= 2:
        (r1, t1), (r2, t2) = [(w["rows_per_wave"], w["cycles_per_frame"]) for w in wave[:2]]
        split = {"walk_cycles_per_frame": (r2 * t1 - r1 * t2) / (r2 - r1), "parallel_cycles_per_frame_and_row": (t2 - t1) / (r2 - r1)}
    eng.close()
    line = {"tool": "comp_bench", "tag": a.tag,
            "config": f"k_comp alone at {RATE} Hz on noise around the threshold (-24 dB, 4:1, knee 6 dB, attack 5 ms, release 120 ms, make-up "
                      f"3 dB), one tbf_debug_comp_time query per call, median of {a.reps} calls behind {a.warmup}; the yardstick k_eq with "
                      f"one band at the same shape likewise; cycles at {CLOCK_HZ / 1e9} GHz; {SIMDS} SIMDs",
            "cases": cases, "one_wave": wave, "one_wave_split": split}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
