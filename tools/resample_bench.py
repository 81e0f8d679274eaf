#!/usr/bin/env python3
"""tools/resample_bench.py -- what the output rate converter costs at the bench batch.

4096 instances at 48 kHz play bench.py's workload (the Jazz-1 registration, a held chord per
instance).  For each output rate (16000 and 22050 Hz) one engine alternates two kinds of step
of --blocks blocks into device memory: the plain step (tbf_render_device into L / R) and the
resampled step (tbf_render_resampled_device with the caller's raw planes, and once more with
engine scratch, where a step is cut into pieces of 256 blocks).  All are timed between device
synchronisations over --steps steps after --warmup; the difference is the converter's cost as
rendered, reported as a share of the plain step of the same session.  k_resample's own time
comes from HIP events around its launches (tbf_debug_resample_time) in a pass of its own.
Writes profiles/resample/resample_bench.json and prints it as one JSON line.
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
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rates", type=int, nargs="*", default=[16000, 22050])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resample" / "resample_bench.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    import scenarios as S
    import tunebfree_amd as T

    B, nsamp = a.batch, a.blocks * 128
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    raw = [torch.empty((B, nsamp), dtype=torch.float32, device="cuda") for _ in range(2)]
    rawp = [p.data_ptr() for p in raw]
    runs = []
    for fo in a.rates:
        eng = T.Engine(sample_rate=float(a.sr), device=torch.cuda.current_device())
        eng.set_output_rate(fo)
        tid = eng.template(seed=7)
        eng.add_instances([tid] * B, [1000 + i for i in range(B)])
        for i in range(B):
            for (_b, kind, p, v) in S.bench_scenario(i):
                eng.note(i, p, v) if kind == "note" else eng.set_param(i, p, v)
        frames = eng.resampled_frames(a.blocks)
        out = [torch.empty((B, frames), dtype=torch.float32, device="cuda") for _ in range(2)]
        outp = [p.data_ptr() for p in out]

        def plain_step():
            eng.render_device(a.blocks, rawp[0], rawp[1], nsamp, stream=stream.cuda_stream)

        def resampled_step():
            eng.render_resampled_device(a.blocks, outp, frames, rawp, nsamp, stream=stream.cuda_stream)

        def scratch_step():
            eng.render_resampled_device(a.blocks, outp, frames, stream=stream.cuda_stream)

        def timed(step):
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e3
        # plain, resampled, plain, resampled: the pairs show the session's spread
        ms = [timed(plain_step), timed(resampled_step), timed(plain_step), timed(resampled_step)]
        sms = timed(scratch_step)
        eng.resample_time(True)
        for _ in range(2):
            resampled_step()
        torch.cuda.synchronize()
        kms, kn = eng.resample_time()
        eng.resample_time(False)
        plain, res = min(ms[0], ms[2]), min(ms[1], ms[3])
        info = eng.resampler_info(table=False)
        runs.append({
            "out_rate_hz": fo, "L": info["L"], "M": info["M"], "T": info["T"], "latency_samples": info["latency"],
            "history_bytes_per_instance": 2 * ((info["T"] - 1 + 3) // 4 * 4) * 4,
            "render_device_step_ms": [ms[0], ms[2]], "resampled_step_ms": [ms[1], ms[3]],
            "resampled_step_engine_scratch_ms": sms,
            "resample_cost_ms": res - plain, "resample_cost_share_of_render_device_step": (res - plain) / plain,
            "k_resample_ms_per_step": kms / 2, "k_resample_launches_per_step": kn // 2,
            "k_resample_share_of_render_device_step": kms / 2 / plain,
            "k_resample_ns_per_stereo_input_sample": kms / 2 * 1e6 / (B * nsamp),
            "stereo_input_samples_per_sec_plain": B * nsamp / plain * 1e3,
            "stereo_input_samples_per_sec_resampled": B * nsamp / res * 1e3,
        })
        eng.close()
        del out
    line = {"tool": "resample_bench", "config": f"{B} instances, {a.sr} Hz, {a.blocks} blocks/step, {a.steps} steps after "
                                                f"{a.warmup} warm-up, bench workload (Jazz 1, held chords)", "runs": runs}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
