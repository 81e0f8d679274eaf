#!/usr/bin/env python3
"""tools/fork_bench.py -- tbf_instances_clone / _save / _load / _remove at the bench batch.

Times, each as one synchronous call on an engine whose instances have rendered --blocks
blocks of the bench registration:
  clone 4095 from 1       one source read by every pair (fan-out), 1 -> 4096 instances
  clone 2048 from 2048    every instance forked once, 2048 -> 4096 instances
  save 4096 / load 4096   k_state_move into / out of the packed staging plus the one
                          device <-> host copy of the blob
  remove 1 of 4096        tbf_instances_remove: the survivors compacted into fresh arrays
  remove every other        (the bytes of a case are its survivors' records), the old arrays
  remove 4095 of 4096       and the stage buffers released, the host arrays compacted
in milliseconds and in GB/s of device state moved (the device record of DESIGN.md's "Forking
and checkpointing": st + wring + rslab + tgc + the persistent program slots), beside a plain
hipMemcpy device-to-device of the same byte count in the same process.  A clone call
includes what growing an engine costs anyway (new arrays, the existing instances' state
moved along, the tables uploaded again), so the hipMemcpy figure is a floor, not a target.
No thresholds: nothing here had been measured before.  Writes profiles/fork/fork_bench.json
and prints it as one JSON line.
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

DEV_STRIDE_AT = 104  # the blob header's device record size (uint64), csrc/tbf_fork.cpp BlobHdr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=8, help="blocks rendered before the calls")
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fork" / "fork_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    import scenarios as S
    import tunebfree_amd as T
    lib = T.load_library()
    u32p = C.POINTER(C.c_uint32)
    B = a.batch

    def organ(n):
        eng = T.Engine(sample_rate=a.sr, device=torch.cuda.current_device())
        tid = eng.template(seed=7)
        eng.add_instances([tid] * n, [1000 + i for i in range(n)])
        for i in range(n):
            for (_, kind, p, v) in S.bench_scenario(i):
                eng.note(i, p, v) if kind == "note" else eng.set_param(i, p, v)
        L = torch.empty((n, a.blocks * 128), dtype=torch.float32, device="cuda")
        R = torch.empty_like(L)
        eng.render_device(a.blocks, L.data_ptr(), R.data_ptr(), a.blocks * 128)
        eng.synchronize()
        return eng

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    try:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.restype, hip.hipMemcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    except OSError:
        hip = None

    def memcpy_ms(nbytes):
        """hipMemcpy device-to-device of nbytes: the best of three after a warm-up"""
        src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            if hip is not None:
                assert hip.hipMemcpy(dst.data_ptr(), src.data_ptr(), nbytes, 3) == 0  # hipMemcpyDeviceToDevice
            else:
                dst.copy_(src)
        copy()
        return min(timed(copy) for _ in range(3))

    warm = organ(2)              # loads k_state_move's code object outside the timed calls
    warm.clone([0, 1])
    head = warm.save([0]).tobytes()[:DEV_STRIDE_AT + 8]
    assert head[:8] == b"TFSTATE1", "not the blob layout this tool knows"
    rec = int(np.frombuffer(head[DEV_STRIDE_AT:], np.uint64)[0])
    assert rec > 0 and rec % 16 == 0, rec
    warm.close()

    res = {"batch": B, "sample_rate": a.sr, "device_record_bytes": rec, "cases": {}}

    def case(name, ms, n):
        nbytes = n * rec
        ref = memcpy_ms(nbytes)
        res["cases"][name] = {"instances": n, "bytes": nbytes, "ms": ms, "GBps": nbytes / ms / 1e6,
                              "hipMemcpy_d2d_ms": ref, "hipMemcpy_d2d_GBps": nbytes / ref / 1e6}

    eng = organ(1)
    src = np.zeros(B - 1, np.uint32)
    case(f"clone {B - 1} from 1", timed(lambda: eng.clone(src)), B - 1)
    assert eng.n_instances == B
    eng.close()

    half = B // 2
    eng = organ(half)
    case(f"clone {half} from {half}", timed(lambda: eng.clone(np.arange(half, dtype=np.uint32))), half)
    assert eng.n_instances == 2 * half
    n = eng.n_instances
    inst = np.arange(n, dtype=np.uint32)
    size = C.c_uint64()
    assert lib.tbf_instances_save(eng._h, n, inst.ctypes.data_as(u32p), None, 0, C.byref(size)) == 0
    blob = np.zeros(size.value, np.uint8)

    def save():
        assert lib.tbf_instances_save(eng._h, n, inst.ctypes.data_as(u32p), blob.ctypes.data, blob.nbytes, C.byref(size)) == 0

    def load():
        assert lib.tbf_instances_load(eng._h, n, inst.ctypes.data_as(u32p), blob.ctypes.data, blob.nbytes) == 0
    case(f"save {n}", timed(save), n)
    case(f"load {n}", timed(load), n)
    res["blob_bytes"] = int(blob.nbytes)

    # tbf_instances_remove: the bytes a case moves are its survivors' records (compacted into
    # fresh arrays); the batch is cloned back up to n between the cases
    def remove(name, gone):
        gone = np.ascontiguousarray(gone, dtype=np.uint32)
        assert eng.n_instances == n
        case(name, timed(lambda: eng.remove(gone)), n - len(gone))
        assert eng.n_instances == n - len(gone)
        eng.clone(np.arange(len(gone), dtype=np.uint32) % max(eng.n_instances, 1))
    remove(f"remove 1 of {n}", [n // 2])
    remove(f"remove every other of {n}", np.arange(0, n, 2))
    remove(f"remove {n - 1} of {n}", np.arange(1, n))
    eng.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
