#!/usr/bin/env python3
"""tools/pcm_bench.py -- what the PCM output stage costs.

1. k_pcm alone: tbf_pcm_convert_device over --batch x --blocks x 128 frames of noise per format
   (with meters), timed by the HIP events around its launches (tbf_debug_pcm_time), as GB/s over
   the bytes it moves (8 B in and 4 / 6 / 8 B out per frame), beside a device-to-device copy that
   moves the same byte total (half of it read, half written), timed by events in the same process.
2. The PCM device step (tbf_render_pcm_device: render into engine scratch in pieces of 256 blocks,
   k_pcm behind each) against the plain step (tbf_render_device) of the same engine, alternating,
   on bench.py's workload; the difference as a share of the plain step.  Reported, not gated.
3. The host path: tbf_render (two float planes to the host) against tbf_render_pcm (S16 frames to
   the host) at --host-batch x --host-blocks, wall time in alternation, into buffers allocated
   once.
Writes profiles/pcm/pcm_bench.json and prints it as one JSON line.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

NAMES = ("s16", "s16_dither", "s24_3le", "f32")


def organ(T, S, torch, batch, sr):
    eng = T.Engine(sample_rate=float(sr), device=torch.cuda.current_device())
    tid = eng.template(seed=7)
    eng.add_instances([tid] * batch, [1000 + i for i in range(batch)])
    for i in range(batch):
        for (_b, kind, p, v) in S.bench_scenario(i):
            eng.note(i, p, v) if kind == "note" else eng.set_param(i, p, v)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10, help="k_pcm and copy launches timed per format")
    ap.add_argument("--host-batch", type=int, default=1024)
    ap.add_argument("--host-blocks", type=int, default=64)
    ap.add_argument("--host-steps", type=int, default=6)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pcm" / "pcm_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    import scenarios as S
    import tunebfree_amd as T
    E = T.engine
    formats = [(E.PCM_S16, 0), (E.PCM_S16, E.PCM_DITHER), (E.PCM_S24_3LE, 0), (E.PCM_F32, 0)]

    B, frames = a.batch, a.blocks * 128
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream

    # ---- 1. k_pcm alone against a copy of the same bytes
    eng = organ(T, S, torch, 1, a.sr)
    planes = [torch.randn((B, frames), dtype=torch.float32, device="cuda") * 0.3 for _ in range(2)]
    out = torch.empty((B * frames * 8,), dtype=torch.uint8, device="cuda")
    met = torch.zeros((B * 4,), dtype=torch.int32, device="cuda")
    kernel = []
    for name, (fmt, flags) in zip(NAMES, formats):
        fb = E.PCM_FRAME_BYTES[fmt]
        total = B * frames * (8 + fb)
        src = torch.empty((total // 2,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def convert():
            eng.pcm_convert_device(B, planes[0].data_ptr(), planes[1].data_ptr(), frames, frames, out.data_ptr(), frames * fb,
                                   fmt, flags=flags, seed=1, meters_ptr=met.data_ptr(), stream=sp)
        for _ in range(2):
            convert()
            dst.copy_(src)
        torch.cuda.synchronize()
        eng.pcm_time(True)
        copies = []
        for _ in range(a.reps):  # alternating, each between its own events
            convert()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            dst.copy_(src)
            e1.record(stream)
            copies.append((e0, e1))
        torch.cuda.synchronize()
        kms, kn = eng.pcm_time()
        eng.pcm_time(False)
        assert kn == a.reps
        cms = sum(e0.elapsed_time(e1) for e0, e1 in copies)
        m = met.cpu().numpy().view(E.METER_DTYPE)
        kernel.append({
            "format": name, "frames": B * frames, "bytes_moved": total,
            "k_pcm_ms": kms / kn, "k_pcm_GB_per_s": total / (kms / kn) * 1e-6,
            "copy_ms": cms / a.reps, "copy_GB_per_s": total / (cms / a.reps) * 1e-6,
            "k_pcm_over_copy": (kms / kn) / (cms / a.reps), "yardstick_at_most": 2.0,
            "clipped_samples": int(m["clipL"].astype(np.int64).sum() + m["clipR"].astype(np.int64).sum()),
        })
        del src, dst
    eng.close()
    del planes, out

    # ---- 2. the PCM device step against the plain step
    eng = organ(T, S, torch, B, a.sr)
    raw = [torch.empty((B, frames), dtype=torch.float32, device="cuda") for _ in range(2)]
    pcm = torch.empty((B * frames * 8,), dtype=torch.uint8, device="cuda")

    def timed(step):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3

    def plain_step():
        eng.render_device(a.blocks, raw[0].data_ptr(), raw[1].data_ptr(), frames, stream=sp)
    steps = []
    for name, (fmt, flags) in zip(NAMES, formats):
        fb = E.PCM_FRAME_BYTES[fmt]

        def pcm_step():
            eng.render_pcm_device(a.blocks, pcm.data_ptr(), frames * fb, fmt, flags=flags, seed=1, meters_ptr=met.data_ptr(),
                                  stream=sp)
        ms = [timed(plain_step), timed(pcm_step), timed(plain_step), timed(pcm_step)]
        eng.pcm_time(True)
        for _ in range(2):
            pcm_step()
        torch.cuda.synchronize()
        kms, kn = eng.pcm_time()
        eng.pcm_time(False)
        plain, p = min(ms[0], ms[2]), min(ms[1], ms[3])
        steps.append({
            "format": name, "render_device_step_ms": [ms[0], ms[2]], "render_pcm_device_step_ms": [ms[1], ms[3]],
            "pcm_cost_ms": p - plain, "pcm_cost_share_of_render_device_step": (p - plain) / plain,
            "k_pcm_ms_per_step": kms / 2, "k_pcm_launches_per_step": kn // 2, "k_pcm_share_of_render_device_step": kms / 2 / plain,
            "stereo_samples_per_sec_plain": B * frames / plain * 1e3, "stereo_samples_per_sec_pcm": B * frames / p * 1e3,
        })
    eng.close()
    del raw, pcm

    # ---- 3. the host path
    hb, hframes = a.host_batch, a.host_blocks * 128
    eng = organ(T, S, torch, hb, a.sr)
    lib = T.load_library()
    fl = [np.zeros((hb, hframes), np.float32) for _ in range(2)]
    fr = np.zeros((hb, hframes, 2), np.int16)
    po = E.PcmOut(fr.ctypes.data, hframes * 4, None, E.PCM_S16, 0, 0, 0, None)
    fp = C.POINTER(C.c_float)

    def host_plain():
        assert lib.tbf_render(eng._h, a.host_blocks, fl[0].ctypes.data_as(fp), fl[1].ctypes.data_as(fp), hframes) == 0

    def host_pcm():
        assert lib.tbf_render_pcm(eng._h, a.host_blocks, C.byref(po)) == 0

    def wall(step):
        t0 = time.perf_counter()
        for _ in range(a.host_steps):
            step()
        return (time.perf_counter() - t0) / a.host_steps * 1e3
    host_plain()
    host_pcm()
    hms = [wall(host_plain), wall(host_pcm), wall(host_plain), wall(host_pcm)]
    eng.close()
    host = {"instances": hb, "blocks": a.host_blocks, "tbf_render_ms": [hms[0], hms[2]], "tbf_render_pcm_s16_ms": [hms[1], hms[3]],
            "bytes_to_host_render": hb * hframes * 8, "bytes_to_host_pcm": hb * hframes * 4,
            "pcm_over_render": min(hms[1], hms[3]) / min(hms[0], hms[2])}

    line = {"tool": "pcm_bench",
            "config": f"{B} instances, {a.sr} Hz, {a.blocks} blocks/step, {a.steps} steps after {a.warmup} warm-up, bench "
                      f"workload (Jazz 1, held chords); k_pcm and the copy over {a.reps} launches each; host path "
                      f"{hb} instances x {a.host_blocks} blocks over {a.host_steps} calls",
            "k_pcm": kernel, "device_step": steps, "host_path": host}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
