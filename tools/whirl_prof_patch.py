"""Build-variant generator (profiling only, never the product): a copy of
csrc/tbf_render.hip whose k_whirl accumulates s_memtime cycles per phase of stage_whirl on
lane 0 and writes them, as floats, over the first 16 output samples of instances 0..7
(tools/whirl_prof.py reads them back and names the phases).
usage: python tools/whirl_prof_patch.py OUT.hip"""
import sys
from pathlib import Path

SRC = Path(__file__).resolve().parents[1] / "tunebfree_amd" / "csrc" / "tbf_render.hip"


def sub(s, old, new):
    assert s.count(old) == 1, (old, s.count(old))
    return s.replace(old, new)


def mark(k, tabs):
    t = "\t" * tabs
    return (f"{t}if (threadIdx.x == 0) {{ const unsigned long long _t = __builtin_amdgcn_s_memtime (); "
            f"sm.wp[{k}] += _t - sm.wplast; sm.wplast = _t; }}\n")


def after(s, anchor, k, tabs=2):
    return sub(s, anchor, anchor + mark(k, tabs))


def before(s, anchor, k, tabs=2):
    return sub(s, anchor, mark(k, tabs) + anchor)


def function(s, head):
    a = s.index(head)
    return a, s.index("\n}\n", a)


def main():
    s = SRC.read_text()
    s = sub(s, "\tint          ap;\n};", "\tint          ap;\n\tunsigned long long wp[16], wplast;\n};")
    a, b = function(s, "__device__ void stage_whirl (")
    body = s[a:b]
    # block start, then whirl_speed (lane 0; the rare path: a steady block adds next to nothing)
    body = after(body, "\tR.ran             = 1;\n", 10, 1)
    body = after(body, "\t\tR.brake = uni (sm.brake);\n\t\twave_sync ();\n\t}\n", 9, 1)
    # the sub-block's phases
    body = after(body, "\t\t\tsm.ab[ap][n] = (float)((double)(sb + 1 < TBF_BLK / TBF_SUB ? in1 : nx0) + 1e-14);\n\t\twave_sync ();\n", 1)
    body = before(body, "\t\t/* the filter outputs: horn B -> xf", 3)
    body = after(body, "\t\t\tR.drumAngle = uni (de);\n\t\t}\n\t\twave_sync ();\n", 4)
    body = after(body, "\t\tconst float xd2v = (float)((0.4 * xd1v) + (0.4 * xd1p));\n\t\twave_sync ();\n", 5)
    body = before(body, "\t\t\tbool okr[WH_RG];\n", 6, 3)
    body = before(body, "\t\t/* ---- outputs (whirlProc2 outHL/outHR/outDL/outDR + whirlProc3 mix) ---- */\n", 7)
    body = after(body, "\t\tR.outpos = (R.outpos + TBF_SUB) & 2047u;\n\t\twave_sync ();\n", 8)
    s = s[:a] + body + s[b:]
    # init and write-out in k_whirl
    a, b = function(s, "k_whirl (const tbf_launch P")
    body = s[a:b]
    body = sub(body, "\twh_reg_load (sm, R);\n",
               "\twh_reg_load (sm, R);\n\tif (threadIdx.x < 16) sm.wp[threadIdx.x] = 0;\n"
               "\tif (threadIdx.x == 0) sm.wplast = __builtin_amdgcn_s_memtime ();\n")
    assert body.endswith("\t\twr[i] = sm.wring[i / W][i % W];")
    body += ("\n\tif (inst < 8 && threadIdx.x < 16) P.outL[(size_t)inst * P.outStride + P.outOffset + threadIdx.x] = "
             "(float)sm.wp[threadIdx.x];")
    s = s[:a] + body + s[b:]
    Path(sys.argv[1]).write_text(s)


if __name__ == "__main__":
    main()
