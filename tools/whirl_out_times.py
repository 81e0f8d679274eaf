"""k_whirl's time per 512-block launch at the bench batch, per output mode.
usage: python tools/whirl_out_times.py <repository root to import from> <out.json> mode [mode ...]
modes: mic direct rotors_mic rotors_direct (a tree without whirl_out takes mic only).  Another
build of the library is measured through TBF_LIB (make -C tunebfree_amd variant NAME=out4
VFLAGS=-DWH_WAVES_OUT=4: the new modes of k_whirl<512> at 4 waves per SIMD).  Records:
profiles/rotors/."""
import json
import sys
import time

root, out, modes = sys.argv[1], sys.argv[2], sys.argv[3:]
sys.path.insert(0, root)
sys.path.insert(0, root + "/tests")
import torch  # noqa: E402

torch.cuda.set_device(0)
import bench  # noqa: E402
import tunebfree_amd as T  # noqa: E402

B, BLOCKS, REPS = 4096, 1024, 3
res = {}
for mode in modes:
    kw = {} if mode == "mic" else {"whirl_out": 1 if mode.endswith("direct") else 0}
    eng = T.Engine(sample_rate=48000.0, device=0, **kw)
    bench.setup_instances(eng, bench.Workload("cfg3", 48000.0), 0, B)
    nplanes = 6 if mode.startswith("rotors") else 2
    buf = [torch.empty((B, BLOCKS * 128), dtype=torch.float32, device="cuda") for _ in range(nplanes)]
    p = [b.data_ptr() for b in buf]
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream

    def step():
        if nplanes == 6:
            eng.render_rotors_device(BLOCKS, p[0], p[1], BLOCKS * 128, p[2:], BLOCKS * 128, stream=sptr)
        else:
            eng.render_device(BLOCKS, p[0], p[1], BLOCKS * 128, sptr)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    r = {"chunk": eng.chunks()[1], "launches": eng.launches(),
         "ms_per_2048_blocks_as_rendered": (time.perf_counter() - t0) / 6 * 1e3 * (2048 / BLOCKS)}
    print(mode, "ms per 2048 blocks:", r["ms_per_2048_blocks_as_rendered"], flush=True)
    for key, how in (("alone", "serial"), ("as_rendered", True)):
        eng.kernel_times(how)
        for _ in range(REPS):
            step()
        torch.cuda.synchronize()
        kt = eng.kernel_times()
        eng.kernel_times(False)
        r[key] = {k: [v[0] / v[1], v[1]] for k, v in kt.items() if v[1]}
    res[mode] = r
    print(mode, "k_whirl ms per launch alone / as rendered:", r["alone"]["k_whirl"][0], r["as_rendered"]["k_whirl"][0],
          flush=True)
    eng.close()
    del buf
    torch.cuda.empty_cache()
json.dump(res, open(out, "w"), indent=1)
