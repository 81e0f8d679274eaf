#!/usr/bin/env python3
"""tools/limit_bench.py -- what the bus limiter costs.

1. k_limit alone: tbf_limit_device over --batch rows of --frames frames of noise that exceeds the
   ceiling now and then, at each --ahead (hold --hold), timed by the HIP events around its launches
   (tbf_debug_limit_time), beside its two bounds:
     bytes: 16 B per frame (8 B read, 8 B written) at the measured copy rate of an MI355X;
     adds:  A float32 adds per frame at the VALU's rate, 256 CUs x 4 SIMDs x 16 lanes a clock at
            2.4 GHz: one add a lane with v_add_f32, two with v_pk_add_f32 (both figures are given;
            the packed one is the bound, since the compiler pairs the accumulators).
2. The chain render_mix_device -> limiter -> pcm_convert_device: --chain-batch instances into
   --buses buses, --chain-blocks blocks a call, on one stream; wall time per call with and without
   the limiter between the two, and the limiter's own time.
Writes profiles/limit/limit_bench.json and prints it as one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_COPY_TB_PER_S = 6.29  # a float4 copy's rate on an MI355X (8.0 TB/s is the interface's own)
VALU_LANES_PER_S = 256 * 4 * 16 * 2.4e9  # float32 lanes a second: one v_add_f32 result each, two with v_pk_add_f32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--ahead", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--hold", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per case")
    ap.add_argument("--chain-batch", type=int, default=256)
    ap.add_argument("--chain-blocks", type=int, default=64)
    ap.add_argument("--buses", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "limit" / "limit_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    import scenarios as S
    import tunebfree_amd as T

    B, F = a.batch, a.frames
    ceiling = 1.0 - 2.0 ** -15
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    eng = T.Engine(sample_rate=48000.0, device=torch.cuda.current_device())
    planes = [torch.randn((B, F), dtype=torch.float32, device="cuda") * 0.5 for _ in range(2)]
    outs = [torch.empty((B, F), dtype=torch.float32, device="cuda") for _ in range(2)]
    met = torch.zeros((B * 3,), dtype=torch.int32, device="cuda")

    def alone(A):
        lim = eng.limiter(B, ceiling, A, a.hold)
        _g, tile, hn, lds = T.Engine.limit_grid(ceiling, A, a.hold)

        def call():
            lim.process_device(planes[0].data_ptr(), planes[1].data_ptr(), F, F, outs[0].data_ptr(), outs[1].data_ptr(), F,
                               meters_ptr=met.data_ptr(), stream=sp)
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        lim.time(True)
        for _ in range(a.reps):
            call()
        torch.cuda.synchronize()
        ms, n = lim.time()
        assert n == a.reps
        ms /= n
        m = met.cpu().numpy().view(T.params.LIMIT_METER_DTYPE)
        lim.close()
        total = B * F * 16
        byte_ms = total / (HBM_COPY_TB_PER_S * 1e12) * 1e3
        add_ms = B * F * A / VALU_LANES_PER_S * 1e3
        pk_ms = add_ms / 2
        return {"rows": B, "frames": F, "ahead": A, "hold": a.hold, "history": hn, "tile_frames": tile, "lds_bytes": lds,
                "k_limit_ms": ms, "bytes_moved": total, "GB_per_s": total / ms * 1e-6, "byte_bound_ms": byte_ms,
                "add_bound_ms_v_add_f32": add_ms, "add_bound_ms_v_pk_add_f32": pk_ms,
                "governing_bound": "bytes" if byte_ms >= pk_ms else "adds (v_pk_add_f32)",
                "share_of_governing_bound": max(byte_ms, pk_ms) / ms,
                "frames_reduced_share": float(m["reduced"].sum()) / (B * F), "min_gain": float(m["min_gain"].min())}

    cases = [alone(A) for A in a.ahead]
    eng.close()
    del planes, outs
    torch.cuda.empty_cache()

    # the chain
    n, nb, buses = a.chain_batch, a.chain_blocks, a.buses
    frames = nb * 128
    eng = T.Engine(sample_rate=48000.0, device=torch.cuda.current_device())
    tid = eng.template(seed=7)
    eng.add_instances([tid] * n, [1000 + i for i in range(n)])
    for i in range(n):
        for (_b, kind, x, v) in S.bench_scenario(i):
            (eng.note if kind == "note" else eng.set_param)(i, x, v)
    rows = T.params.mix_rows(np.arange(n) % buses, 1.0)
    mix = [torch.empty((buses, frames), dtype=torch.float32, device="cuda") for _ in range(2)]
    ltd = [torch.empty((buses, frames), dtype=torch.float32, device="cuda") for _ in range(2)]
    pcm = torch.empty((buses, frames * 4), dtype=torch.uint8, device="cuda")
    pmet = torch.zeros((buses * 4,), dtype=torch.int32, device="cuda")
    lim = eng.limiter(buses, ceiling, 64, a.hold)

    def chain(limited):
        eng.render_mix_device(nb, rows, buses, mix[0].data_ptr(), mix[1].data_ptr(), frames, stream=sp)
        src = mix
        if limited:
            lim.process_device(mix[0].data_ptr(), mix[1].data_ptr(), frames, frames, ltd[0].data_ptr(), ltd[1].data_ptr(),
                               frames, stream=sp)
            src = ltd
        eng.pcm_convert_device(buses, src[0].data_ptr(), src[1].data_ptr(), frames, frames, pcm.data_ptr(), frames * 4,
                               T.engine.PCM_S16, meters_ptr=pmet.data_ptr(), stream=sp)

    def wall(limited):
        for _ in range(2):
            chain(limited)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            chain(limited)
        torch.cuda.synchronize()
        clips = pmet.cpu().numpy().view(T.engine.METER_DTYPE)
        return (time.perf_counter() - t0) / a.reps * 1e3, int(clips["clipL"].sum() + clips["clipR"].sum())

    plain_ms, plain_clips = wall(False)
    lim.time(True)
    ltd_ms, ltd_clips = wall(True)
    kms, kn = lim.time()
    plain2_ms, _ = wall(False)
    eng.close()
    line = {"tool": "limit_bench",
            "config": f"k_limit alone on {B} rows x {F} frames of noise (sigma 0.5, ceiling 1 - 2^-15), hold {a.hold}, mean of "
                      f"{a.reps} calls by HIP events; bounds: 16 B per frame at {HBM_COPY_TB_PER_S} TB/s, A adds per frame at "
                      f"{VALU_LANES_PER_S:.4g} float32 lanes per second (x 2 packed); chain: {n} instances, {buses} buses, "
                      f"{nb} blocks a call, wall time over {a.reps} calls",
            "k_limit": cases,
            "chain": {"instances": n, "buses": buses, "blocks": nb, "mix_pcm_ms": [plain_ms, plain2_ms],
                      "mix_limit_pcm_ms": ltd_ms, "k_limit_ms_per_call": kms / max(kn, 1),
                      "s16_clips_unlimited": plain_clips, "s16_clips_limited": ltd_clips}}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
