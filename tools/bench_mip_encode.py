"""Cost of neo_mip_encode (mip_train.hip:k_mip_encode) on its own: --rays x --intervals rows of 504 features between two device
events, --reps times after a warm-up; median and spread, and the rate at which the rows are written (the kernel is store-bound:
2016 B per row).  $NEO360_HIP_LIB selects another build of the library for an A/B (two processes, alternated).

  python tools/bench_mip_encode.py --out profiles/mip_encode_f64_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--intervals", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import cases
    from neo360_amd import training
    from oracle import mip360
    torch.set_grad_enabled(False)
    R, n = args.rays, args.intervals
    rays = cases.mip_rays(R)
    t = torch.sort(torch.rand(R, n + 1, generator=torch.Generator().manual_seed(1)) * 5 + 0.2, dim=-1).values.cuda()
    o, d, rad, basis = rays["rays_o"].cuda(), rays["rays_d"].cuda(), rays["radii"].cuda(), mip360.icosahedron_basis().cuda()
    for _ in range(3):
        training.mip_encode(o, d, rad, t, basis)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        training.mip_encode(o, d, rad, t, basis)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    rec = dict(kernel="k_mip_encode", library=os.environ.get("NEO360_HIP_LIB") and "NEO360_HIP_LIB" or "in-tree", rays=R, intervals=n,
               rows=R * n, reps=args.reps, median_ms=med, min_ms=min(ms), max_ms=max(ms), bytes_written=R * n * 504 * 4,
               store_tb_per_s=R * n * 504 * 4 / (med * 1e-3) / 1e12)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
