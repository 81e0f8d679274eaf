#!/usr/bin/env python3
"""tools/eq_bench.py -- what the bus equaliser costs.

k_eq alone: tbf_eq_device at 48 kHz over 4096 rows x 8192 frames, 4 rows x 8192 frames and 2 rows x
480000 frames of noise, each with 1, 4 and 8 bands a row (max_bands = the bands, so P = 1, 4, 8
lanes a row and channel), timed by the HIP events around its launch (tbf_debug_eq_time), one query
per call: the median of --reps calls behind --warmup, with the least, the largest and the 10th and
90th percentiles.  Beside each shape stands the yardstick from existing code in the same process:
k_loud at the same shape (tbf_debug_loudness_time), 17 dependent-chain double operations a frame in
one lane against 9 per band here.  A lane owns one band of one row's channel, so while the waves
are fewer than the SIMDs the time is one wave's: the tool reports it in cycles per frame at 2.4 GHz.
Writes profiles/eq/eq_bench.json and prints it as one JSON line.
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
    ap.add_argument("--shapes", type=int, nargs="*", default=[4096, 8192, 4, 8192, 2, 480000], help="rows frames [rows frames ...]")
    ap.add_argument("--bands", type=int, nargs="*", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=21, help="timed calls per case (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eq" / "eq_bench.json"))
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
    # eight bands of a plausible bus chain; a row with k bands takes the first k
    P = T.params
    chain = [P.eq_band(P.EQ_HPF, 40.0), P.eq_band(P.EQ_LOW, 120.0, 0.7071, 2.0), P.eq_band(P.EQ_PEQ, 250.0, 1.4, -3.0),
             P.eq_band(P.EQ_PEQ, 800.0, 2.0, 1.5), P.eq_band(P.EQ_NOTCH, 1000.0, 5.0), P.eq_band(P.EQ_PEQ, 3000.0, 1.0, 2.5),
             P.eq_band(P.EQ_HIGH, 8000.0, 0.7071, 3.0), P.eq_band(P.EQ_LPF, 18000.0)]

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

    cases = []
    for B, F in zip(a.shapes[0::2], a.shapes[1::2]):
        planes = [torch.randn((B, F), dtype=torch.float32, device="cuda") * 0.1 for _ in range(2)]
        outs = [torch.empty((B, F), dtype=torch.float32, device="cuda") for _ in range(2)]
        lm = eng.loudness(B, RATE, max_hops=F // (RATE // 10) + 1)

        def loud():
            lm.reset(stream=sp)
            lm.measure_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, stream=sp)
        rpg = T.Engine.loudness_grid(1)[0]
        lw = (B + rpg - 1) // rpg
        yard = timed(lm, loud)
        yard.update(waves=lw, cycles_per_frame_per_wave=yard["median_ms"] * 1e-3 / F * CLOCK_HZ / ((lw + SIMDS - 1) // SIMDS))
        lm.close()
        rows = []
        for k in a.bands:
            lanes, rpw, tile, lds = T.Engine.eq_grid(k)
            eq = eng.equalizer(B, k, RATE)
            eq.set(chain[:k], stream=sp)
            r = timed(eq, lambda: eq.process_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, outs[0].data_ptr(),
                                                    outs[1].data_ptr(), F, stream=sp))
            waves = (B + rpw - 1) // rpw
            rounds = (waves + SIMDS - 1) // SIMDS
            r.update(bands=k, lanes=lanes, rows_per_wave=rpw, tile_frames=tile, lds_bytes=lds, waves=waves,
                     cycles_per_frame_per_wave=r["median_ms"] * 1e-3 / F * CLOCK_HZ / rounds,
                     GB_per_s=B * F * 16 / r["median_ms"] * 1e-6, against_k_loud=r["median_ms"] / yard["median_ms"],
                     out_finite=bool(torch.isfinite(outs[0]).all().item()))
            rows.append(r)
            eq.close()
        for r in rows:
            r["against_own_1_band"] = r["median_ms"] / rows[0]["median_ms"] if rows[0]["bands"] == 1 else None
        cases.append({"rows": B, "frames": F, "rate_hz": RATE, "k_loud": yard, "k_eq": rows})
        del planes, outs
        torch.cuda.empty_cache()
    eng.close()
    line = {"tool": "eq_bench",
            "config": f"k_eq alone at {RATE} Hz on noise (sigma 0.1), one tbf_debug_eq_time query per call, median of {a.reps} "
                      f"calls behind {a.warmup}; max_bands = the bands; the yardstick k_loud at the same shape likewise; cycles at "
                      f"{CLOCK_HZ / 1e9} GHz, one wave a SIMD up to {SIMDS}",
            "cases": cases}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
