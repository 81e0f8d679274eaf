#!/usr/bin/env python3
"""tools/cab_bench.py -- what the cabinet convolver costs at the bench batch.

4096 instances at 48 kHz play bench.py's workload (the Jazz-1 registration, a held chord per
instance).  For each response length (1024 and 8192 taps of seeded decaying noise) one engine
alternates two kinds of step of --blocks blocks into device memory: the rotor step
(tbf_render_rotors_device into four planes, what a host that convolves elsewhere calls) and the
cabinet step (tbf_render_cabinet_device with the same four planes plus L / R).  Both are timed
between device synchronisations over --steps steps after --warmup; the difference is the
convolver's cost as rendered, reported as a share of the rotor step of the same session.
k_cabinet's own time comes from HIP events around its launches (tbf_debug_cabinet_time) in a
pass of its own.  Writes profiles/cabinet/cab_bench.json and prints it as one JSON line.
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
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--taps", type=int, nargs="*", default=[1024, 8192])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cabinet" / "cab_bench.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    import cab_model as M
    import scenarios as S
    import tunebfree_amd as T

    B, nsamp = a.batch, a.blocks * 128
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    planes = [torch.empty((B, nsamp), dtype=torch.float32, device="cuda") for _ in range(6)]
    cab, rot = [p.data_ptr() for p in planes[:2]], [p.data_ptr() for p in planes[2:]]
    runs = []
    for taps in a.taps:
        eng = T.Engine(sample_rate=a.sr, device=torch.cuda.current_device())
        eng.set_cabinet(M.decaying_noise(taps, 1), M.decaying_noise(taps, 2))
        tid = eng.template(seed=7)
        eng.add_instances([tid] * B, [1000 + i for i in range(B)])
        for i in range(B):
            for (_b, kind, p, v) in S.bench_scenario(i):
                eng.note(i, p, v) if kind == "note" else eng.set_param(i, p, v)

        def rotor_step():
            eng.render_rotors_device(a.blocks, None, None, 0, rot, nsamp, stream=stream.cuda_stream)

        def cabinet_step():
            eng.render_cabinet_device(a.blocks, cab, nsamp, rot, nsamp, stream=stream.cuda_stream)

        def timed(step):
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e3
        # rotor, cabinet, rotor, cabinet: the pairs show the session's spread
        ms = [timed(rotor_step), timed(cabinet_step), timed(rotor_step), timed(cabinet_step)]
        eng.cabinet_time(True)
        for _ in range(2):
            cabinet_step()
        torch.cuda.synchronize()
        kms, kn = eng.cabinet_time()
        eng.cabinet_time(False)
        rotor, cabinet = min(ms[0], ms[2]), min(ms[1], ms[3])
        info = eng.cabinet_info()
        runs.append({
            "taps": taps, "partitions": info["partitions"], "history_bytes_per_instance": info["instance_bytes"],
            "rotor_step_ms": [ms[0], ms[2]], "cabinet_step_ms": [ms[1], ms[3]],
            "cabinet_cost_ms": cabinet - rotor, "cabinet_cost_share_of_rotor_step": (cabinet - rotor) / rotor,
            "k_cabinet_ms_per_step": kms / 2, "k_cabinet_launches_per_step": kn // 2,
            "k_cabinet_share_of_rotor_step": kms / 2 / rotor,
            "k_cabinet_ns_per_stereo_sample": kms / 2 * 1e6 / (B * nsamp),
            "stereo_samples_per_sec_rotor": B * nsamp / rotor * 1e3,
            "stereo_samples_per_sec_cabinet": B * nsamp / cabinet * 1e3,
        })
        eng.close()
    line = {"tool": "cab_bench", "config": f"{B} instances, {a.sr:.0f} Hz, {a.blocks} blocks/step, {a.steps} steps after "
                                          f"{a.warmup} warm-up, bench workload (Jazz 1, held chords)", "runs": runs}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
