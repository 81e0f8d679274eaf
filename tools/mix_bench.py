#!/usr/bin/env python3
"""tools/mix_bench.py -- what the mixdown stage costs.

k_mix alone: tbf_mix_device over --batch rows of noise, timed by the HIP events around its launches
(tbf_debug_mix_time), as GB/s over the bytes of its byte model (8 B read per member row and frame,
8 B written per bus and frame, 24 B of member list per member and tile of frames), beside the HBM
bound (the measured copy rate of an MI355X) and beside a device-to-device copy that moves the same
byte total (half of it read, half written), timed by events in the same process:
  1. calls of --frames frames with buses of 1, 8, 64 and --batch rows (contiguous groups of rows);
  2. one call of --short-frames frames on a single bus of --batch rows, the low-latency corner,
     where the definition leaves one serial chain per frame and nothing else to spread.
Writes profiles/mix/mix_bench.json and prints it as one JSON line.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_COPY_TB_PER_S = 6.29  # a float4 copy's rate on an MI355X (8.0 TB/s is the interface's own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--short-frames", type=int, default=128)
    ap.add_argument("--bus-sizes", type=int, nargs="*", default=None)
    ap.add_argument("--reps", type=int, default=10, help="k_mix and copy launches timed per case")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mix" / "mix_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    import tunebfree_amd as T

    B = a.batch
    sizes = a.bus_sizes or [1, 8, 64, B]
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    eng = T.Engine(sample_rate=48000.0, device=torch.cuda.current_device())
    planes = [torch.randn((B, a.frames), dtype=torch.float32, device="cuda") * 0.1 for _ in range(2)]
    rng = np.random.default_rng(1)
    gain, pan = rng.uniform(0.2, 1.0, B), rng.uniform(-1.0, 1.0, B)

    def case(size, frames):
        nb = (B + size - 1) // size
        rows = T.params.mix_rows(np.arange(B) // size, gain, pan)
        outs = [torch.empty((nb, frames), dtype=torch.float32, device="cuda") for _ in range(2)]
        per_lane, tile, _slice = T.Engine.mix_grid(frames, nb)
        tiles = (frames + tile - 1) // tile
        total = B * frames * 8 + nb * frames * 8 + B * tiles * 24
        src = torch.empty((total // 2,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def mix():
            eng.mix_device(B, planes[0].data_ptr(), planes[1].data_ptr(), a.frames, frames, rows, nb, outs[0].data_ptr(),
                           outs[1].data_ptr(), frames, stream=sp)
        for _ in range(2):
            mix()
            dst.copy_(src)
        torch.cuda.synchronize()
        eng.mix_time(True)
        copies = []
        for _ in range(a.reps):  # alternating, each between its own events
            mix()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            dst.copy_(src)
            e1.record(stream)
            copies.append((e0, e1))
        torch.cuda.synchronize()
        kms, kn = eng.mix_time()
        eng.mix_time(False)
        assert kn == a.reps
        cms = sum(e0.elapsed_time(e1) for e0, e1 in copies) / a.reps
        ms = kms / kn
        bound_ms = total / (HBM_COPY_TB_PER_S * 1e12) * 1e3
        return {"rows": B, "bus_size": size, "buses": nb, "frames": frames, "frames_per_lane": per_lane,
                "waves": tiles * nb, "bytes_moved": total, "k_mix_ms": ms, "k_mix_GB_per_s": total / ms * 1e-6,
                "hbm_bound_ms": bound_ms, "share_of_hbm_bound": bound_ms / ms,
                "copy_ms": cms, "copy_GB_per_s": total / cms * 1e-6, "k_mix_over_copy": ms / cms,
                "peak": float(max(o.abs().max().item() for o in outs))}

    long_calls = [case(s, a.frames) for s in sizes]
    short_call = case(B, a.short_frames)
    eng.close()
    line = {"tool": "mix_bench",
            "config": f"{B} rows of noise, calls of {a.frames} frames with buses of {sizes} rows and one call of "
                      f"{a.short_frames} frames on one bus of {B}; k_mix and the copy over {a.reps} launches each; HBM bound "
                      f"at {HBM_COPY_TB_PER_S} TB/s",
            "long_calls": long_calls, "short_call": short_call}
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
