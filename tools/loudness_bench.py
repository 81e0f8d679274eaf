#!/usr/bin/env python3
"""tools/loudness_bench.py -- what the loudness meter costs.

1. k_loud alone: tbf_loudness_device at 48 kHz over 4096 rows x 8192 frames and over 2 rows x
   480000 frames of noise, timed by the HIP events around its launches (tbf_debug_loudness_time),
   --reps calls, beside its two bounds, both derived and neither a budget:
     bytes: 8 B per frame (two float32 planes read) at the measured copy rate of an MI355X;
     issue: the 17 double operations of the recurrence per channel and frame (9 multiplies,
            8 adds), each a wave-wide instruction at the cycles profiles/valu_calib.json measured
            for v_mul_f64 / v_add_f64, on one wave per 32 rows, every wave on a SIMD of its own
            (1024 SIMDs), at 2.4 GHz.
   A lane owns a row's channel, so while the waves are fewer than the SIMDs the time is one wave's:
   the frames times what a lone wave needs per frame.  The tool reports that in cycles per frame,
   per operation of the 17, and per operation of the 3 on the recurrence's cycle (y = .. + s1,
   a1 * y, s1 = .. - ..): what a double add or multiply costs as this kernel sees it, an upper
   estimate of its dependent latency (DESIGN.md section 4.14 on why it is the former).
2. The chain render_mix_device -> mix_device (per-bus gains) -> limit_device -> pcm_convert_device:
   --chain-batch instances into --buses buses, --chain-blocks blocks a call, on one stream; wall
   time per call with and without the meter on the gained planes, and the meter's own time.
Writes profiles/loudness/loudness_bench.json and prints it as one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_COPY_TB_PER_S = 6.29  # a float4 copy's rate on an MI355X, as DESIGN.md section 4.13 uses
CLOCK_HZ = 2.4e9
SIMDS = 256 * 4
MULS, ADDS, CHAIN_OPS = 9, 8, 3
RATE = 48000


def finite(v):
    """a float for JSON: None where there is no figure (-inf)"""
    v = float(v)
    return v if v == v and abs(v) != float("inf") else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="*", default=[4096, 8192, 2, 480000], help="rows frames [rows frames ...]")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per case")
    ap.add_argument("--chain-batch", type=int, default=256)
    ap.add_argument("--chain-blocks", type=int, default=64)
    ap.add_argument("--buses", type=int, default=4)
    ap.add_argument("--calib", default=str(ROOT / "profiles" / "valu_calib.json"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "loudness" / "loudness_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    import scenarios as S
    import tunebfree_amd as T

    ops = json.loads(Path(a.calib).read_text())["ops"]
    cyc_mul, cyc_add = ops["mul64"]["cycles_per_wave64_inst"], ops["f64"]["cycles_per_wave64_inst"]
    issue_cycles = MULS * cyc_mul + ADDS * cyc_add   # per frame, per wave
    rpg, tile, lds = T.Engine.loudness_grid(1)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    eng = T.Engine(sample_rate=float(RATE), device=torch.cuda.current_device())

    def alone(B, F):
        planes = [torch.randn((B, F), dtype=torch.float32, device="cuda") * 0.1 for _ in range(2)]
        lm = eng.loudness(B, RATE, max_hops=F // (RATE // 10) + 1)

        def call():
            lm.reset(stream=sp)
            lm.measure_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, stream=sp)
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        lm.timing(True)
        for _ in range(a.reps):
            call()
        torch.cuda.synchronize()
        ms, n = lm.timing()
        assert n == a.reps
        ms /= n
        res = lm.read([0])
        lm.close()
        waves = (B + rpg - 1) // rpg
        byte_ms = B * F * 8 / (HBM_COPY_TB_PER_S * 1e12) * 1e3
        issue_ms = F * issue_cycles * ((waves + SIMDS - 1) // SIMDS) / CLOCK_HZ * 1e3
        cyc_frame = ms * 1e-3 / F * CLOCK_HZ / ((waves + SIMDS - 1) // SIMDS)
        return {"rows": B, "frames": F, "rate_hz": RATE, "waves": waves, "k_loud_ms": ms, "bytes_read": B * F * 8,
                "GB_per_s": B * F * 8 / ms * 1e-6, "byte_bound_ms": byte_ms, "issue_bound_ms": issue_ms,
                "governing_bound": "bytes" if byte_ms >= issue_ms else "issue",
                "share_of_governing_bound": max(byte_ms, issue_ms) / ms,
                "cycles_per_frame_per_wave_at_2.4GHz": cyc_frame,
                "cycles_per_op_of_the_3_on_the_recurrence_cycle": cyc_frame / CHAIN_OPS,
                "cycles_per_op_of_the_17": cyc_frame / (MULS + ADDS),
                "row0_hops": int(res["hops"][0]), "row0_integrated_lufs": finite(res["integrated"][0])}

    shapes = list(zip(a.shapes[0::2], a.shapes[1::2]))
    cases = [alone(B, F) for B, F in shapes]
    eng.close()
    torch.cuda.empty_cache()

    # the chain
    n, nb, buses = a.chain_batch, a.chain_blocks, a.buses
    frames = nb * 128
    eng = T.Engine(sample_rate=float(RATE), device=torch.cuda.current_device())
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, [1000 + i for i in range(n)])
    for i in range(n):
        for (_b, kind, x, v) in S.bench_scenario(i):
            (eng.note if kind == "note" else eng.set_param)(i, x, v)
    rows = T.params.mix_rows(np.arange(n) % buses, 1.0)
    grows = T.params.gain_rows(np.full(buses, 0.25, np.float32))
    mix, gained, ltd = ([torch.empty((buses, frames), dtype=torch.float32, device="cuda") for _ in range(2)] for _ in range(3))
    pcm = torch.empty((buses, frames * 4), dtype=torch.uint8, device="cuda")
    pmet = torch.zeros((buses * 4,), dtype=torch.int32, device="cuda")
    lim = eng.limiter(buses, 1.0 - 2.0 ** -15, 64, 0)
    lm = eng.loudness(buses, max_hops=frames // (RATE // 10) + 1)

    def chain(metered):
        eng.render_mix_device(nb, rows, buses, mix[0].data_ptr(), mix[1].data_ptr(), frames, stream=sp)
        eng.mix_device(buses, mix[0].data_ptr(), mix[1].data_ptr(), frames, frames, grows, buses, gained[0].data_ptr(),
                       gained[1].data_ptr(), frames, stream=sp)
        if metered:
            lm.reset(stream=sp)
            lm.measure_device(gained[0].data_ptr(), gained[1].data_ptr(), frames, frames, stream=sp)
        lim.process_device(gained[0].data_ptr(), gained[1].data_ptr(), frames, frames, ltd[0].data_ptr(), ltd[1].data_ptr(),
                           frames, stream=sp)
        eng.pcm_convert_device(buses, ltd[0].data_ptr(), ltd[1].data_ptr(), frames, frames, pcm.data_ptr(), frames * 4,
                               T.engine.PCM_S16, meters_ptr=pmet.data_ptr(), stream=sp)

    def wall(metered):
        for _ in range(2):
            chain(metered)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            chain(metered)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    plain_ms = wall(False)
    lm.timing(True)
    met_ms = wall(True)
    kms, kn = lm.timing()
    plain2_ms = wall(False)
    lufs = [finite(v) for v in lm.read()["integrated"]]   # one hop a call: no block, no figure
    eng.close()
    line = {"tool": "loudness_bench",
            "config": f"k_loud alone at {RATE} Hz on noise (sigma 0.1), mean of {a.reps} calls by HIP events, {rpg} rows a "
                      f"workgroup of one wave, {tile}-frame LDS tiles, {lds} B of LDS; bounds: 8 B per frame at "
                      f"{HBM_COPY_TB_PER_S} TB/s; {MULS} v_mul_f64 at {cyc_mul:.3f} and {ADDS} v_add_f64 at {cyc_add:.3f} cycles "
                      f"per frame and wave = {issue_cycles:.1f} cycles at {CLOCK_HZ / 1e9} GHz, one wave a SIMD up to {SIMDS}; "
                      f"chain: {n} instances, {buses} buses, {nb} blocks a call, wall time over {a.reps} calls",
            "k_loud": cases,
            "chain": {"instances": n, "buses": buses, "blocks": nb, "mix_gain_limit_pcm_ms": [plain_ms, plain2_ms],
                      "with_meter_ms": met_ms, "k_loud_ms_per_call": kms / max(kn, 1), "bus_integrated_lufs": lufs}}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
