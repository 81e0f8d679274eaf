#!/usr/bin/env python3
"""tools/fx_bench.py -- the effects-only chain (TBF_CHAIN_FX) at the bench batch.

4096 instances at 48 kHz push a device-resident input tensor (seeded Gaussian noise at 0.1
RMS, one row per instance) through overdrive -> reverb -> whirl in steps of 2048 blocks, with
the effect part of the Jazz-1 registration (overdrive on, character 0.5, reverb mix 0.1,
chorale).  Warm-up steps, then the timed steps between two device synchronisations; then, in
passes of their own, the per-stage kernel times (as rendered, and mode 2: each kernel alone)
and the parity of the last timed step's first --check instances against the effects oracle
(tests/fx_oracle.py), bit for bit.  Prints one JSON line.

Run it beside `python bench.py` on the same build, alternating the two: the yardstick is
that build's full-chain step.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-steps", type=int, default=2, help="steps of each kernel-time pass (0: none)")
    ap.add_argument("--check", type=int, default=1, help="instances checked against the effects oracle")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    import scenarios as S
    import tunebfree_amd as T
    from tunebfree_amd import params as P

    B, nsamp = a.batch, a.blocks * 128
    eng = T.Engine(sample_rate=a.sr, device=torch.cuda.current_device(), chain=P.CHAIN_FX)
    tid = eng.template(seed=7)
    seeds = [1000 + i for i in range(B)]
    eng.add_instances([tid] * B, seeds)
    fx = [(k, p, v) for (k, p, v) in S.jazz1_params() if p in (S.P_OVERDRIVE, S.P_CHARACTER, S.P_REVERB, S.P_DRUM, S.P_HORN)]
    for i in range(B):
        for (_, p, v) in fx:
            eng.set_param(i, p, v)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.randn((B, nsamp), generator=g, dtype=torch.float32, device="cuda") * 0.1
    outL = torch.empty((B, nsamp), dtype=torch.float32, device="cuda")
    outR = torch.empty_like(outL)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    torch.cuda.synchronize()

    def step():
        eng.process_device(a.blocks, x.data_ptr(), nsamp, outL.data_ptr(), outR.data_ptr(), nsamp, stream.cuda_stream)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    times = []
    t0 = time.perf_counter()
    for _ in range(a.steps):
        t1 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t1)  # enqueue time only: the steps are not synchronised apart
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    gL = outL[: a.check].cpu().numpy()
    gR = outR[: a.check].cpu().numpy()
    hx = x[: a.check].cpu().numpy()
    line = {
        "metric": "fx_stereo_samples_per_sec", "value": B * nsamp * a.steps / elapsed,
        "ms_per_step": elapsed / a.steps * 1e3, "steps": a.steps, "warmup": a.warmup,
        "config": f"TBF_CHAIN_FX: caller audio -> overdrive -> reverb -> whirl, {B} instances, {a.sr:.0f} Hz, "
                  f"{a.blocks} blocks/step, Gaussian input at 0.1 RMS, overdrive on, character 0.5, mix 0.1, chorale",
        "steady_chunk": eng.chunks()[1], "host_enqueue_ms_max": max(times) * 1e3,
    }
    for mode, key in ((True, "kernel_ms_as_rendered"), ("serial", "kernel_ms_alone")):
        if not a.kernel_steps:
            break
        eng.kernel_times(mode)
        for _ in range(a.kernel_steps):
            step()
        torch.cuda.synchronize()
        kt = eng.kernel_times()
        eng.kernel_times(False)
        # per step: a stage's launches of one step summed (k_tonegen never runs)
        line[key] = {k: v[0] / a.kernel_steps for k, v in kt.items()}
        line[key + "_launches_per_step"] = {k: v[1] // a.kernel_steps for k, v in kt.items()}
    line["launches"] = eng.launches()
    if a.check:
        from fx_oracle import FxOracle
        from orc_bind import load_oracle
        lib = load_oracle()
        total = (a.warmup + a.steps) * a.blocks
        bad, err = 0, 0.0
        for i in range(a.check):
            o = FxOracle(lib, seeds[i], a.sr)
            for (_, p, v) in fx:
                o.param(p, v)
            for b in range(total):
                k = b % a.blocks
                blk = o.block(hx[i, k * 128:(k + 1) * 128])
                if b >= total - a.blocks:
                    for got, ref in ((gL, blk[2]), (gR, blk[3])):
                        seg = got[i, k * 128:(k + 1) * 128]
                        bad += int((seg.view(np.uint32) != ref.view(np.uint32)).sum())
                        err = max(err, float(np.abs(seg.astype(np.float64) - ref).max()))
            o.close()
        line["parity"] = {"instances": a.check, "blocks_replayed": total, "samples_differing": bad, "max_err": err,
                          "bit_exact": bad == 0}
    print(json.dumps(line), flush=True)
    eng.close()
    if a.check and line["parity"]["samples_differing"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
