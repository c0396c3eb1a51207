"""Cost of MipNeRF360.compute_extras on the 640 x 480 Mip-NeRF 360 evaluation frame (bench.py's mip360 workload: 64 / 64 / 32
samples, synthetic weights, ONE forward call per frame through render.render_frame_sharded).

Frames with the attribute off and on ALTERNATE in one process, every frame between two device events; medians and spread (min,
quartiles, max) over --frames frames per side after --warmup.  Next to the frame time, the three extra launches on their own:
ops.mip_extras on each level's histogram of the last frame, between two device events, --reps times per level, against the traffic
the launch needs (R x (2 n + 1) floats read, 5 floats per ray written: acc, mean and three percentiles).

  python tools/bench_mip_extras.py --out profiles/mip_extras_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

H, W, CHUNK, NEAR, FAR = 480, 640, 1024, 0.2, 3.0
COUNTS = (64, 64, 32)


def spread(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), q1_ms=q[0], q3_ms=q[2], max_ms=max(ms))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mip_extras.py measures on a ROCm device: there is no CPU figure for a frame time"
    torch.set_grad_enabled(False)
    from neo360_amd import models, ops, render, synth
    dev = torch.device("cuda:0")
    net = models.MipNeRF360(num_prop_samples=COUNTS[0], num_nerf_samples=COUNTS[2]).to(dev)
    net.load_state_dict(synth.mip360_state(0, weight_gain=0.5))
    ro, vd, rd, radii = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
    batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd, radii=radii[:, None])
    R = H * W

    def frame(on):
        net.compute_extras = on
        try:
            return render.render_frame_sharded(net, batch, 1, 0, chunk=CHUNK, n_rays=R, near=NEAR, far=FAR, check=False)
        finally:
            net.compute_extras = False

    for _ in range(args.warmup):
        frame(False)
        frame(True)
    torch.cuda.synchronize()
    off, on = [], []
    for _ in range(args.frames):                      # alternating: both sides see the same clocks and neighbours
        off.append(timed(lambda: frame(False))[0])
        tile = timed(lambda: frame(True))
        on.append(tile[0])
    net.check_flags()
    depth = tile[1][:, 3]
    result = dict(frame="mipnerf360 640x480, %d / %d / %d samples, one forward call per frame" % COUNTS, rays=R,
                  extras_off=spread(off), extras_on=spread(on),
                  difference_of_medians_ms=statistics.median(on) - statistics.median(off),
                  depth_min_max=[float(depth.min()), float(depth.max())])
    # the three launches on their own, on the histograms of a frame
    _, hist = net(batch, 1.0, False, False, NEAR, FAR)
    net.check_flags()
    launches = []
    for lv, h in enumerate(hist):
        n = h["weights"].shape[-1]
        call = lambda: ops.mip_extras(h["sdist"], h["weights"], net.EXTRA_QUANTILES, NEAR, FAR)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = [timed(call)[0] for _ in range(args.reps)]
        moved = R * (2 * n + 1) * 4 + R * 5 * 4
        launches.append(dict(level=lv, intervals=n, bytes_read=R * (2 * n + 1) * 4, bytes_written=R * 5 * 4, **spread(ms),
                             gb_per_s_at_median=moved / statistics.median(ms) / 1e6))
        print("level %d (n = %d): %.4f ms median [%.4f .. %.4f], %.1f MB moved, %.0f GB/s"
              % (lv, n, statistics.median(ms), min(ms), max(ms), moved / 1e6, launches[-1]["gb_per_s_at_median"]), flush=True)
    result["launches"] = launches
    result["sum_of_launch_medians_ms"] = sum(x["median_ms"] for x in launches)
    print("frame: extras off %.2f ms [%.2f .. %.2f], on %.2f ms [%.2f .. %.2f], difference of medians %+.3f ms; launches alone %.3f ms"
          % (result["extras_off"]["median_ms"], min(off), max(off), result["extras_on"]["median_ms"], min(on), max(on),
             result["difference_of_medians_ms"], result["sum_of_launch_medians_ms"]))
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
