"""k_rv_post role clocks (profiling variant RVP_PROF=1, never the product): the bench's batch
and registration in the reverb-tap chain mode, one 512-block launch after warm-up launches;
workgroup 0's waves write their s_memtime sums (k cycles) of work and barrier wait, the SIMD
they ran on and their role over instance 0's first output samples.

    TBF_LIB=tunebfree_amd/_variants/libtbf_rvpprof.so python tools/rvp_prof.py"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    import torch
    import tunebfree_amd as T
    import scenarios as S
    B, nb = 4096, 512
    eng = T.Engine(sample_rate=48000.0, device=0, chain=3)
    tid = eng.template(seed=7)
    eng.add_instances([tid] * B, [1000 + i for i in range(B)])
    for i in range(B):
        for (_, kind, a, v) in S.bench_scenario(i):
            (eng.note if kind == "note" else eng.set_param)(i, a, v)
    L = torch.empty((B, nb * 128), dtype=torch.float32, device="cuda")
    R = torch.empty_like(L)
    for _ in range(3):
        eng.render_device(nb, L.data_ptr(), R.data_ptr(), nb * 128)
        eng.synchronize()
    v = L[0, :64].cpu().numpy()
    it = nb * 4 + 4
    print(f"k_rv_post per iteration (cycles), {it} iterations:")
    for name, o in (("serial", 0), ("dither", 4), ("helper0", 8)):
        print(f"  {name:8s} work {v[o] * 1e3 / it:8.0f}  barrier {v[o + 1] * 1e3 / it:8.0f}")
    waves = int(v[12])
    print(f"the {waves} waves of workgroup 0 (wave: role, work / barrier cycles per iteration, SIMD):")
    by_simd = {}
    for w in range(waves):
        work, barrier, simd, role = (float(x) for x in v[16 + 4 * w:20 + 4 * w])
        name = {-2: "serial", -1: "dither"}.get(int(role), f"helper, {int(role)} task{'s' if role > 1 else ''}")
        print(f"  wave {w:2d}: {name:15s} {work * 1e3 / it:8.0f} / {barrier * 1e3 / it:8.0f}  SIMD {simd:.0f}")
        by_simd.setdefault(int(simd), []).append((w, work * 1e3 / it))
    print("by SIMD (waves, the last one's work cycles):")
    for simd, ws in sorted(by_simd.items()):
        print(f"  SIMD {simd}: waves {[w for w, _ in ws]}  {max(c for _, c in ws):8.0f}")


if __name__ == "__main__":
    main()
