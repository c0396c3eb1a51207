"""Timing of the scene encoder's pillar-stage FORWARD at the reference size (64^3 cells x 3 source views, latent
(3, 512, 240, 320)) in both arithmetics, and of the baseline an exact forward would cost without csrc/pillar_f32.hip.

  python tools/bench_pillar_f32.py [--runs K] [--warmup W] [--only split|f32] [--composed PATH] [--out FILE]

  (a) split    GridEncoder.floorplans, precision "f16x3": csrc/pillar.hip (k_pillar_dense x 6 + k_pillar_aggregate x 3)
  (b) f32      the same call, precision "f32": csrc/pillar_f32.hip (k_pillar_dense_f32 x 6 + the same aggregation)
  (c) composed tools/pillar_composed_bench (a stand-alone program built from tools/pillar_composed_bench.hip): k_gather_x +
               one k_pt_gemm per layer, the kernels of csrc/pillar_train.hip - run when --composed names the built program

Device events around the whole call after warm-up, median of --runs (>= 5).  (b) is also reported in algorithmic TFLOP/s
(786,432 rows x 2 x 1,579,008 MAC = 2.48 TFLOP) and as a fraction of the 157.3 TFLOP/s fp32 matrix peak (floor: 15.8 ms).
`--only split` works on a tree that has no "f32" pillar stage.  One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import cases  # noqa: E402
from neo360_amd import encoder, synth  # noqa: E402

DEV = "cuda"
PEAK_F32 = 157.3              # TFLOP/s, fp32 MFMA (v_mfma_f32_32x32x2_f32) at the rated clock
FWD_MACS = 518 * 512 + 2 * 512 * 512 + 3 * (513 * 512 + 512)


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("split", "f32"), default=None)
    ap.add_argument("--composed", default=None, help="path of the built tools/pillar_composed_bench program")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.runs = max(5, a.runs)
    grid = (64, 64, 64)
    nv = cases.NV
    M = nv * grid[0] * grid[1] * grid[2]
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    latent = torch.randn(nv, 512, *cases.FULL_LATENT_HW, device=DEV, generator=g) * 0.1
    poses, focal, centre = (t.to(DEV) for t in synth.source_views(nv, *cases.FULL_WH))
    wh = (float(cases.FULL_WH[0]), float(cases.FULL_WH[1]))
    params = synth.pillar_state(1)
    res = {"grid": list(grid), "views": nv, "cell_views": M, "latent_hw": list(cases.FULL_LATENT_HW), "runs": a.runs,
           "algorithmic_tflop": 2.0 * FWD_MACS * M / 1e12, "f32_floor_ms": 2.0 * FWD_MACS * M / PEAK_F32 / 1e9}
    with torch.no_grad():
        for name, prec in (("split", "f16x3"), ("f32", "f32")):
            if a.only and a.only != name:
                continue
            enc = encoder.GridEncoder(grid_size=grid).to(DEV)
            enc.load_state_dict(params, strict=False)
            enc.precision = prec
            med, lo, hi = timed(lambda: enc.floorplans(latent, poses, focal, centre, wh), a.runs, a.warmup)
            res[name + "_ms"], res[name + "_min_ms"], res[name + "_max_ms"] = med, lo, hi
            res[name + "_tflops_algorithmic"] = 2.0 * FWD_MACS * M / med / 1e9
            enc.close()
            del enc
    if "f32_ms" in res:
        res["f32_frac_of_f32_peak"] = res["f32_tflops_algorithmic"] / PEAK_F32
    if a.composed:
        out = subprocess.run([a.composed, str(a.runs), str(a.warmup)], stdout=subprocess.PIPE, text=True, check=True, timeout=300).stdout
        res.update(json.loads(out.strip().splitlines()[-1]))
        if "f32_ms" in res:
            res["f32_over_composed"] = res["f32_ms"] / res["composed_ms"]
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
