"""Occupancy skipping and early ray termination together on the 640 x 480 NeO-360 frame of bench.py's default line (129 + 385
samples, chunk 1024, the synthetic scene of tools/bench_objects.py with both FOREGROUND density biases raised by --bias, the +12
weights of tools/bench_terminate.py's table), four arms in one process, alternating frame by frame:

    (a) forward              `render.render_rays_test`
    (b) render_skipping      a centred-ball grid at G = 128 whose radius is bisected until about --kept (0.25) of the level-0 samples
                             are kept (tools/bench_occupancy.py's grid)
    (c) render_terminating   eps = --eps (1e-2), segment 64
    (d) render_accelerated   the grid of (b) and the eps of (c)

and the two NEUTRAL pairs of `render_accelerated`, which price its extra classify launches with nothing saved by them:

    no grid, eps = 0         against (c) at eps = 0 (the same launches: without a grid the call takes the terminating path)
    the (b) grid, eps = 0    against (b) (segment launches with a classify + compact each, against whole-row windows)

Per arm: median [min .. max] of the frame time, the call's own kept fractions per level and culled fraction (its device counters)
and the time inside the evaluator launches of one extra frame (the context's spans).  The synthetic scene is a homogeneous fog
seen through a ball-shaped grid: the kept fractions say what an arm saved HERE, not what a trained scene would save.  GPU only;
reads nothing outside the repository.

    python tools/bench_accelerate.py --frames 5 --warmup 2 --out profiles/accelerate_bench.json
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
G = 128
BIASED = ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias")


def spread(ms):
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def ball(radius):
    """bool (G,G,G): cells whose centre lies within `radius` of the origin."""
    c = -1.0 + (torch.arange(G, dtype=torch.float64) + 0.5) * (2.0 / G)
    return (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= radius * radius


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bias", type=float, default=12.0)
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--kept", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from neo360_amd import models, ops, render, synth
    dev = torch.device("cuda:0")
    nv = 3
    state = synth.nerf_tp_state(0)
    for k in BIASED:
        state[k] = state[k] + args.bias
    net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(dev)
    net.load_state_dict(state)
    sc = {k: v.to(dev) for k, v in synth.scene_features(0, nv, 128, (120, 160), 512, (240, 320), std=0.1).items()}
    net.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], (float(W), float(H)))
    poses, focal, centre = synth.source_views(nv, W, H)
    ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
    batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd, src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                 src_imgs=torch.zeros(nv, 3, H, W, device=dev))

    def with_ray_grid(fn):
        def run():
            prev = getattr(net, "ray_grid", None)
            net.ray_grid = (W, 0)
            try:
                return fn()
            finally:
                net.ray_grid = prev
        return run

    def spans(fn):
        ctx = net._context(dev)
        ctx.set_timing(True)
        try:
            ms, _ = timed(fn)
            torch.cuda.synchronize()
            got = [(name, t) for t, name, _, _ in ctx.read_spans()]
        finally:
            ctx.set_timing(False)
        return dict(frame_ms=ms, evaluator_launches=len(got), evaluator_ms=sum(t for _, t in got),
                    everything_else_ms=ms - sum(t for _, t in got))

    # the grid of (b): the ball whose radius keeps about args.kept of the frame's own level-0 samples
    t0 = net.sample_positions(batch, CHUNK)[0][0]
    lo, hi = 0.0, 1.8
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        frac = float(ops.occupancy_keep(ball(mid), ro, rd, t0).float().mean())
        lo, hi = (mid, hi) if frac < args.kept else (lo, mid)
    grid = ball(hi)
    del t0

    forward = lambda: render.render_rays_test(net, batch, chunk=CHUNK, near=0.0, far=0.0, check=False, image_width=W)
    skipping = with_ray_grid(lambda: render.render_skipping_rays(net, batch, chunk=CHUNK, check=False))
    terminating = lambda eps: with_ray_grid(lambda: render.render_terminating_rays(net, batch, eps, chunk=CHUNK, segment=64, check=False))
    accelerated = lambda eps: with_ray_grid(lambda: render.render_accelerated_rays(net, batch, eps, chunk=CHUNK, segment=64, check=False))

    def compare(arms):
        """arms: [(name, grid or None, fn)]; frames alternate over the arms.  Returns {name: dict}."""
        for name, g, fn in arms:
            net.set_occupancy(g)
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in arms}
        last = {}
        for _ in range(args.frames):              # alternating: every arm sees the same clocks and neighbours
            for name, g, fn in arms:
                net.set_occupancy(g)
                torch.cuda.synchronize()
                t, last[name] = timed(fn)
                ms[name].append(t)
        net.check_flags()
        out = {}
        for name, g, fn in arms:
            net.set_occupancy(g)
            res = last[name]
            arm = dict(frame=spread(ms[name]), breakdown_of_one_more_frame=spans(fn))
            if "kept_fraction" in res:
                arm["kept_fraction_level0"], arm["kept_fraction_level1"] = (float(x) for x in res["kept_fraction"])
            if "culled_fraction" in res:
                arm["culled_fraction"] = float(res["culled_fraction"])
            out[name] = arm
            print("%s: %.1f ms [%.1f .. %.1f]%s" % (name, arm["frame"]["median_ms"], arm["frame"]["min_ms"], arm["frame"]["max_ms"],
                                                   "".join(", %s %.3f" % (k, v) for k, v in arm.items() if isinstance(v, float))), flush=True)
        net.set_occupancy(None)
        return out, last

    result = dict(workload="neo360 640x480, 129 + 385 samples, chunk 1024, f16x3 (bench.py's default line)", rays=H * W,
                  frames=args.frames, warmup=args.warmup, raised_foreground_bias=args.bias, eps=args.eps, segment=64,
                  grid=dict(resolution=G, shape="centred ball", radius=hi, target_kept_fraction_level0=args.kept,
                            occupied_cells_fraction=float(grid.float().mean())))

    def save():
        if args.out:          # after every comparison: a run that is cut short keeps what it measured
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)

    arms, last = compare([("a_forward", None, forward), ("b_skipping", grid, skipping), ("c_terminating", None, terminating(args.eps)),
                          ("d_accelerated", grid, accelerated(args.eps))])
    result["arms"] = arms
    med = {k: v["frame"]["median_ms"] for k, v in arms.items()}
    d = arms["d_accelerated"]["frame"]
    result["d_over_a"], result["d_over_b"], result["d_over_c"] = (med["d_accelerated"] / med[k] for k in ("a_forward", "b_skipping", "c_terminating"))
    result["d_faster_than_b_and_c_beyond_their_spreads"] = bool(d["max_ms"] < arms["b_skipping"]["frame"]["min_ms"] and
                                                                d["max_ms"] < arms["c_terminating"]["frame"]["min_ms"])
    result["d_max_abs_rgb_change_against_b"] = float((last["d_accelerated"]["rgb"] - last["b_skipping"]["rgb"]).abs().max())
    result["bound_1_003_eps"] = 1.003 * args.eps
    save()

    pair, last = compare([("terminating_eps0", None, terminating(0.0)), ("accelerated_no_grid_eps0", None, accelerated(0.0))])
    pair["bitwise"] = bool(torch.equal(last["terminating_eps0"]["rgb"], last["accelerated_no_grid_eps0"]["rgb"]))
    pair["accelerated_over_parent"] = pair["accelerated_no_grid_eps0"]["frame"]["median_ms"] / pair["terminating_eps0"]["frame"]["median_ms"]
    result["neutral_no_grid_eps0"] = pair
    save()
    pair, last = compare([("skipping", grid, skipping), ("accelerated_grid_eps0", grid, accelerated(0.0))])
    pair["bitwise"] = bool(torch.equal(last["skipping"]["rgb"], last["accelerated_grid_eps0"]["rgb"]))
    pair["accelerated_over_parent"] = pair["accelerated_grid_eps0"]["frame"]["median_ms"] / pair["skipping"]["frame"]["median_ms"]
    result["neutral_grid_eps0"] = pair
    save()
    print(json.dumps({k: result[k] for k in ("d_over_a", "d_over_b", "d_over_c", "d_faster_than_b_and_c_beyond_their_spreads")}))


if __name__ == "__main__":
    main()
