#!/usr/bin/env python3
"""tools/limit_tp_bench.py -- what the true-peak detector costs inside the bus limiter.

1. k_limit_tp alone: tbf_limit_device of a limiter with a true-peak detector over rows x frames of
   noise that exceeds the ceiling now and then, for each shape, (ahead, hold) and oversampling F,
   timed by the HIP events around its launches (tbf_debug_limit_time).  Beside it, in the same
   process and alternating with it round by round, the plain k_limit of the same configuration and
   k_tpeak of the same F on the same planes: the two stages a host would otherwise run.
   Every case: --warm untimed calls of each kernel, then --rounds rounds of --reps calls of each in
   turn; the figure is the median of the rounds' means, the spread their (max - min) / median.
   The model, per output frame:
     bytes:  16 B (8 B read, 8 B written), at the measured copy rate of an MI355X;
     chains: 24 F v_fma_f32 per staged frame (2 channels x F phases x 12 taps), and a tile stages
             tile + Hn frames for tile outputs: 24 F (1 + Hn / tile);
     adds:   A float32 adds, two a lane and clock where the compiler pairs them (v_pk_add_f32).
   The bound is the larger of bytes / rate and (chains + adds / 2) / the VALU's lanes per second.
2. Overshoot on transient material: rows of limit_model.issue_input scaled to a peak of 4 through
   the plain and the true-peak limiter (64, 32, F = 4, ceiling 1 - 2^-15), each output through the
   project's true-peak meter on the same stream: the dBTP of the worst row and the mean.
Writes profiles/limit_tp/limit_tp_bench.json and profiles/limit_tp/overshoot.json and prints the
first as one JSON line.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_COPY_TB_PER_S = 6.29  # a float4 copy's rate on an MI355X (8.0 TB/s is the interface's own)
VALU_LANES_PER_S = 256 * 4 * 16 * 2.4e9  # float32 lanes a second: one v_fma_f32 or v_add_f32 result each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x8192,2x480000", help="rows x frames, comma separated")
    ap.add_argument("--configs", default="64:0,64:32,512:4096", help="ahead:hold, comma separated")
    ap.add_argument("--oversample", type=int, nargs="*", default=[4, 2])
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="timed calls per kernel and round")
    ap.add_argument("--overshoot-rows", type=int, default=64)
    ap.add_argument("--overshoot-frames", type=int, default=48000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "limit_tp" / "limit_tp_bench.json"))
    ap.add_argument("--overshoot-out", default=str(ROOT / "profiles" / "limit_tp" / "overshoot.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    import limit_model as LM
    import tunebfree_amd as T

    ceiling = 1.0 - 2.0 ** -15
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    eng = T.Engine(sample_rate=48000.0, device=torch.cuda.current_device())
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    configs = [tuple(int(v) for v in s.split(":")) for s in a.configs.split(",")]

    def figure(per_round):
        med = statistics.median(per_round)
        return {"ms": med, "spread": (max(per_round) - min(per_round)) / med, "rounds_ms": per_round}

    cases = []
    for B, N in shapes:
        planes = [torch.randn((B, N), dtype=torch.float32, device="cuda") * 0.5 for _ in range(2)]
        outs = [torch.empty((B, N), dtype=torch.float32, device="cuda") for _ in range(2)]
        met = torch.zeros((B * 3,), dtype=torch.int32, device="cuda")
        for A, H in configs:
            for F in a.oversample:
                _g, tile, hn_tp, lds = T.Engine.limit_grid(ceiling, A, H, oversample=F)
                _g, _t, hn, lds_plain = T.Engine.limit_grid(ceiling, A, H)
                tp, plain, meter = eng.limiter(B, ceiling, A, H, oversample=F), eng.limiter(B, ceiling, A, H), eng.true_peak(B, oversample=F)

                def limit(lim):
                    lim.process_device(planes[0].data_ptr(), planes[1].data_ptr(), N, N, outs[0].data_ptr(), outs[1].data_ptr(), N,
                                       meters_ptr=met.data_ptr(), stream=sp)

                # kernel: (its event timer's accessor, one call): Limiter.time, TruePeak.timing
                calls = {"k_limit_tp": (tp.time, lambda: limit(tp)), "k_limit": (plain.time, lambda: limit(plain)),
                         "k_tpeak": (meter.timing,
                                     lambda: meter.measure_device(planes[0].data_ptr(), planes[1].data_ptr(), N, N, stream=sp))}
                for _timer, call in calls.values():
                    for _ in range(a.warm):
                        call()
                torch.cuda.synchronize()
                per = {k: [] for k in calls}
                for _ in range(a.rounds):
                    for k, (timer, call) in calls.items():
                        timer(True)
                        for _ in range(a.reps):
                            call()
                        torch.cuda.synchronize()
                        ms, n = timer()
                        assert n == a.reps
                        timer(False)
                        per[k].append(ms / n)
                limit(tp)
                torch.cuda.synchronize()
                m = met.cpu().numpy().view(T.params.LIMIT_METER_DTYPE)
                tp.close(), plain.close(), meter.close()
                fig = {k: figure(v) for k, v in per.items()}
                frames = B * N
                halo = 1.0 + hn / tile
                fma = 24.0 * F * halo
                byte_ms = frames * 16 / (HBM_COPY_TB_PER_S * 1e12) * 1e3
                valu_ms = frames * (fma + A / 2.0) / VALU_LANES_PER_S * 1e3
                bound = max(byte_ms, valu_ms)
                both = fig["k_limit"]["ms"] + fig["k_tpeak"]["ms"]
                cases.append({
                    "rows": B, "frames": N, "ahead": A, "hold": H, "oversample": F, "history": hn_tp, "tile_frames": tile,
                    "lds_bytes": lds, "lds_bytes_plain": lds_plain, **{k: v for k, v in fig.items()},
                    "ratio_to_plain_plus_meter": fig["k_limit_tp"]["ms"] / both,
                    "ratio_to_plain": fig["k_limit_tp"]["ms"] / fig["k_limit"]["ms"],
                    "halo_factor": halo, "fma_per_output_frame": fma, "adds_per_output_frame": A,
                    "fma_per_output_frame_without_halo": 24.0 * F,
                    "byte_bound_ms": byte_ms, "valu_bound_ms": valu_ms,
                    "governing_bound": "bytes" if byte_ms >= valu_ms else "VALU (fma + packed adds)",
                    "share_of_governing_bound": bound / fig["k_limit_tp"]["ms"],
                    "frames_reduced_share": float(m["reduced"].sum()) / frames, "min_gain": float(m["min_gain"].min())})
                print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
        del planes, outs, met
        torch.cuda.empty_cache()

    line = {"tool": "limit_tp_bench",
            "config": f"noise of sigma 0.5 against a ceiling of 1 - 2^-15; per case {a.warm} warm calls of each kernel, then {a.rounds} "
                      f"rounds of {a.reps} calls of k_limit_tp, k_limit and k_tpeak in turn, by HIP events; ms = median of the rounds' "
                      f"means, spread = (max - min) / median; bounds: 16 B per frame at {HBM_COPY_TB_PER_S} TB/s, "
                      f"24 F (1 + Hn / tile) fma + A / 2 packed adds per frame at {VALU_LANES_PER_S:.4g} float32 lanes per second",
            "cases": cases}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(line, indent=1) + "\n")

    # overshoot on transient material
    B, N, A, H, F = a.overshoot_rows, a.overshoot_frames, 64, 32, 4
    x = [LM.issue_input(7000 + k, N, B) for k in range(2)]
    top = np.maximum(np.abs(x[0]).max(axis=1), np.abs(x[1]).max(axis=1))[:, None]
    x = [(v * (4.0 / top)).astype(np.float32) for v in x]
    src = [torch.from_numpy(v).cuda() for v in x]
    out = [torch.empty((B, N), dtype=torch.float32, device="cuda") for _ in range(2)]
    over = {"tool": "limit_tp_bench (overshoot)",
            "config": f"{B} rows x {N} frames of limit_model.issue_input (seeds 7000, 7001), each row scaled to a peak of 4; "
                      f"ahead {A}, hold {H}, ceiling 1 - 2^-15 = {20.0 * np.log10(ceiling):.6f} dBFS; the output measured by "
                      f"tbf_true_peak_device (F = {F}) on the same stream",
            "input_dbtp_max": None}
    meter = eng.true_peak(B, oversample=F)
    meter.measure_device(src[0].data_ptr(), src[1].data_ptr(), N, N, stream=sp)
    over["input_dbtp_max"] = float(meter.read()["dbtp"].max())
    meter.close()
    for name, kind in (("plain", None), ("true_peak", F)):
        lim, meter = eng.limiter(B, ceiling, A, H, oversample=kind), eng.true_peak(B, oversample=F)
        lim.process_device(src[0].data_ptr(), src[1].data_ptr(), N, N, out[0].data_ptr(), out[1].data_ptr(), N, stream=sp)
        meter.measure_device(out[0].data_ptr(), out[1].data_ptr(), N, N, stream=sp)
        res = meter.read()
        over[name] = {"output_dbtp_max": float(res["dbtp"].max()), "output_dbtp_mean": float(res["dbtp"].mean()),
                      "output_sample_peak_max": float(res["sample_peak"].max()),
                      "rows_over_the_ceiling": int((res["dbtp"] > 20.0 * np.log10(ceiling) + 1e-9).sum())}
        lim.close(), meter.close()
    eng.close()
    op = Path(a.overshoot_out)
    op.parent.mkdir(parents=True, exist_ok=True)
    op.write_text(json.dumps(over, indent=1) + "\n")
    print(json.dumps(over), file=sys.stderr, flush=True)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
