#!/usr/bin/env python3
"""tools/truepeak_bench.py -- what the true-peak meter costs.

k_tpeak alone: tbf_true_peak_device at F = 4 over 4096 rows x 8192 frames and over 2 rows x 480000
frames of noise (the two shapes of DESIGN.md section 4.14), timed by the HIP events around its
launch (tbf_debug_true_peak_time): --warmup untimed calls, then --reps timed ones, reported as
median, minimum and maximum.  Beside it its two bounds, both derived and neither a budget:
  bytes: 8 B per frame pair (two float32 planes read once) at the measured copy rate of an MI355X;
  issue: 96 v_fma_f32 per frame pair (2 channels x 4 phases x 12 taps), each a wave-wide
         instruction at the cycles profiles/valu_calib.json measured for v_fma_f32, a wave's 64
         frame pairs at a time, the waves spread over 1024 SIMDs, at 2.4 GHz.
And k_loud at the same shapes in the same run (tbf_debug_loudness_time), whose serial chain along a
row's time is what the 2-row shape costs there.
Writes profiles/truepeak/truepeak_bench.json and prints it as one JSON line.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_COPY_TB_PER_S = 6.29  # a float4 copy's rate on an MI355X, as DESIGN.md sections 4.13 and 4.14 use
CLOCK_HZ = 2.4e9
SIMDS = 256 * 4
FMA_PER_PAIR = 96
RATE = 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="*", default=[4096, 8192, 2, 480000], help="rows frames [rows frames ...]")
    ap.add_argument("--reps", type=int, default=20, help="timed calls per case")
    ap.add_argument("--warmup", type=int, default=5, help="untimed calls per case")
    ap.add_argument("--loud-reps", type=int, default=3, help="timed k_loud calls per case")
    ap.add_argument("--oversample", type=int, default=4)
    ap.add_argument("--calib", default=str(ROOT / "profiles" / "valu_calib.json"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "truepeak" / "truepeak_bench.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    import tunebfree_amd as T

    cyc_fma = json.loads(Path(a.calib).read_text())["ops"]["fma32"]["cycles_per_wave64_inst"]
    tile, per_lane, _g, lds = T.Engine.true_peak_grid(1, 1)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    eng = T.Engine(sample_rate=float(RATE), device=torch.cuda.current_device())

    def timed(meter, call, warmup, reps):
        """every timed call's own milliseconds: one query per call"""
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        meter.timing(True)
        ms = []
        for _ in range(reps):
            call()
            torch.cuda.synchronize()
            t, k = meter.timing()
            assert k == 1
            ms.append(t)
        meter.timing(False)
        return ms

    def case(B, F):
        planes = [torch.rand((B, F), dtype=torch.float32, device="cuda") * 2.0 - 1.0 for _ in range(2)]
        tp = eng.true_peak(B, oversample=a.oversample)

        def call():
            tp.reset(stream=sp)
            tp.measure_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, stream=sp)
        ms = timed(tp, call, a.warmup, a.reps)
        res = tp.read([0])
        groups = T.Engine.true_peak_grid(B, F)[2]
        tp.close()
        lm = eng.loudness(B, RATE, max_hops=F // (RATE // 10) + 1)

        def lcall():
            lm.reset(stream=sp)
            lm.measure_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, stream=sp)
        lms = timed(lm, lcall, 1, a.loud_reps)
        lm.close()
        med = statistics.median(ms)
        byte_ms = B * F * 8 / (HBM_COPY_TB_PER_S * 1e12) * 1e3
        phases = {4: 4, 2: 2, 1: 0}[a.oversample]
        fma = 2 * phases * 12
        issue_ms = (B * F / 64.0) * fma * cyc_fma / SIMDS / CLOCK_HZ * 1e3
        gov = max(byte_ms, issue_ms)
        return {"rows": B, "frames": F, "oversample": a.oversample, "workgroups": groups,
                "k_tpeak_ms_median": med, "k_tpeak_ms_min": min(ms), "k_tpeak_ms_max": max(ms), "reps": len(ms),
                "bytes_read": B * F * 8, "GB_per_s": B * F * 8 / med * 1e-6, "fma_per_s": B * F * fma / med * 1e3,
                "byte_bound_ms": byte_ms, "issue_bound_ms": issue_ms,
                "governing_bound": "bytes" if byte_ms >= issue_ms else "issue", "share_of_governing_bound": gov / med,
                "k_loud_ms_median": statistics.median(lms), "k_loud_ms_min": min(lms), "k_loud_reps": len(lms),
                "k_loud_over_k_tpeak": statistics.median(lms) / med,
                "row0_dbtp": float(res["dbtp"][0])}

    shapes = list(zip(a.shapes[0::2], a.shapes[1::2]))
    cases = [case(B, F) for B, F in shapes]
    eng.close()
    line = {"tool": "truepeak_bench",
            "config": f"k_tpeak alone at F = {a.oversample} on uniform noise in [-1, 1], by HIP events around each launch, "
                      f"{a.warmup} warm-up calls then {a.reps} timed ones (median, min, max); workgroups of 256 lanes on "
                      f"{tile}-frame tiles, {per_lane} frames a lane, {lds} B of LDS; bounds: 8 B per frame pair at "
                      f"{HBM_COPY_TB_PER_S} TB/s; {FMA_PER_PAIR} v_fma_f32 per frame pair at {cyc_fma:.3f} cycles per wave-wide "
                      f"instruction over {SIMDS} SIMDs at {CLOCK_HZ / 1e9} GHz; k_loud on the same planes in the same run, "
                      f"{a.loud_reps} timed calls",
            "cases": cases}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
