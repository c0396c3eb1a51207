"""Early ray termination carried through the outside-sphere march, on the 640 x 480 NeO-360 frame of bench.py's default line
(129 + 385 samples, chunk 1024, the synthetic scene and weights of tools/bench_terminate.py): `render.render_marching_rays` with
outside=True against its comparison arm in one process, alternating, segment 64, no occupancy grid:

    eps = 0             synthetic weights; outside=True against `render_terminating_rays(eps=0)` and against the plain frame: the
                        price of the outside point lists and segment launches with nothing saved (all three bitwise equal);
    eps = 1e-2, 1e-3    foreground bias 0 and both BACKGROUND density biases raised by each value of --bias (a homogeneous fog
                        outside the sphere, which real scenes are not - the kept fractions say what the arm saved, not what a trained
                        scene would); outside=True against outside=False at the same eps.

Per arm: the call's own kept fractions outside the sphere per level and culled fraction (its device counters), the two frame times
and the largest |rgb change| against the outside=False frame next to the a-priori bound 1.003 eps.
GPU only; reads nothing outside the repository.

    python tools/bench_march_outside.py --frames 5 --warmup 2 --out profiles/march_outside_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 480, 640
CHUNK = 1024
BIASED = ("bg_coarse_mlp.density_layer.bias", "bg_fine_mlp.density_layer.bias")
EPS = (1e-2, 1e-3)


def spread(ms):
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bias", type=float, nargs="+", default=[6.0, 12.0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from neo360_amd import models, ops, render, synth
    dev = torch.device("cuda:0")
    nv = 3
    net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(dev)
    sc = {k: v.to(dev) for k, v in synth.scene_features(0, nv, 128, (120, 160), 512, (240, 320), std=0.1).items()}
    net.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], (float(W), float(H)))
    poses, focal, centre = synth.source_views(nv, W, H)
    ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
    batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd, src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                 src_imgs=torch.zeros(nv, 3, H, W, device=dev))

    def load(bias):
        state = synth.nerf_tp_state(0)
        for k in BIASED:
            state[k] = state[k] + bias
        net.load_state_dict(state)

    def hinted(fn):
        prev = getattr(net, "ray_grid", None)
        net.ray_grid = (W, 0)
        try:
            return fn()
        finally:
            net.ray_grid = prev

    def plain():
        return render.render_rays_test(net, batch, chunk=CHUNK, near=0.0, far=0.0, check=False, image_width=W)

    def terminating(eps):
        return hinted(lambda: render.render_terminating_rays(net, batch, eps, chunk=CHUNK, check=False))

    def marching(eps, outside):
        return hinted(lambda: render.render_marching_rays(net, batch, eps, chunk=CHUNK, outside=outside, grid=False, check=False))

    result = dict(workload="neo360 640x480, 129 + 385 samples, chunk 1024, f16x3 (bench.py's default line), segment 64, no grid",
                  rays=H * W, frames=args.frames, warmup=args.warmup, raised_background_bias=list(args.bias), arms=[])

    def run(weights, eps, name, other, this):
        for _ in range(args.warmup):
            other()
            this()
        torch.cuda.synchronize()
        o_ms, t_ms = [], []
        ref = out = None
        for _ in range(args.frames):          # alternating: both sides see the same clocks and neighbours
            ms, ref = timed(other)
            o_ms.append(ms)
            ms, out = timed(this)
            t_ms.append(ms)
        net.check_flags()
        o, t = statistics.median(o_ms), statistics.median(t_ms)
        lo = max(min(o_ms), min(t_ms)) - min(max(o_ms), max(t_ms))          # > 0: the two min..max ranges do not overlap
        arm = dict(weights=weights, eps=eps, against=name, kept_fraction_outside_level0=float(out["kept_fraction_outside"][0]),
                   kept_fraction_outside_level1=float(out["kept_fraction_outside"][1]),
                   kept_fraction_inside_level1=float(out["kept_fraction"][1]), culled_fraction=float(out["culled_fraction"]),
                   comparison_frame=spread(o_ms), outside_frame=spread(t_ms), outside_over_comparison=t / o, ranges_apart_ms=lo,
                   max_abs_rgb_change=float((out["rgb"] - ref["rgb"]).abs().max()), bound_1_003_eps=1.003 * eps,
                   max_abs_depth_change=float((out["depth"] - ref["depth"]).abs().max()),
                   bitwise_comparison=bool(torch.equal(out["rgb"], ref["rgb"]) and torch.equal(out["depth"], ref["depth"])))
        result["arms"].append(arm)
        print("%s eps %g against %s: outside kept %.3f / %.3f, culled %.3f, %.1f ms [%.1f .. %.1f] against %.1f ms [%.1f .. %.1f] (x %.3f), "
              "max |d rgb| %.3e" % (weights, eps, name, arm["kept_fraction_outside_level0"], arm["kept_fraction_outside_level1"],
                                    arm["culled_fraction"], t, min(t_ms), max(t_ms), o, min(o_ms), max(o_ms), t / o, arm["max_abs_rgb_change"]),
              flush=True)
        if args.out:          # after every arm: a run that is cut short keeps what it measured
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)

    load(0.0)
    run("synthetic", 0.0, "render_terminating(eps=0)", lambda: terminating(0.0), lambda: marching(0.0, True))
    run("synthetic", 0.0, "the plain frame", plain, lambda: marching(0.0, True))
    for b in args.bias:
        load(b)
        for eps in EPS:
            run("synthetic, background density bias +%g" % b, eps, "outside=False", lambda: marching(eps, False), lambda: marching(eps, True))
    print(json.dumps(dict(arms=[(a["weights"], a["eps"], a["against"], a["outside_over_comparison"]) for a in result["arms"]])))


if __name__ == "__main__":
    main()
