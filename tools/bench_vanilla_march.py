"""Occupancy skipping and early ray termination on the 640 x 480 vanilla frame of `bench.py --workload vanilla` (64 + 128 samples,
synth.vanilla_state(0)), every arm alternating frame by frame with the plain frame (`render.render_rays_test`) in one process:

    ones_eps0            an all-ones grid at eps = 0: the machinery's price with nothing saved
    ball_0.5 / 0.25 / 0.1    centred-ball grids at G = 128 over [-1, 1]^3 with clip=True, the radius bisected until about that share of
                         the level-0 samples is kept, at eps = 0
    fog_eps / fog_eps_ball_0.25   eps = --eps (1e-3) on a dense synthetic fog (both density biases raised by --fog-bias), without a
                         grid and with the 0.25 grid, against the plain frame of the same fog

Per arm: median [min .. max] of the frame time and the kept fractions per level from the call's own device counters.  The synthetic
scene is a homogeneous fog seen through a ball-shaped grid: the kept fractions say what an arm saved HERE, not what a trained scene
would save.  GPU only; reads nothing outside the repository.

    python tools/bench_vanilla_march.py --frames 5 --warmup 2 --out profiles/vanilla_march_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 480, 640
CHUNK = 4096
G = 128
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
NEAR, FAR = 0.2, 3.0


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
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--fog-bias", type=float, default=6.0)
    ap.add_argument("--march-chunk", type=int, default=32768)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from neo360_amd import marching, ops, render, synth
    dev = torch.device("cuda:0")

    def module(bias):
        state = synth.vanilla_state(0)
        for k in ("coarse_mlp.density_layer.bias", "fine_mlp.density_layer.bias"):
            state[k] = state[k] + bias
        net = marching.MarchingNeRF(num_coarse_samples=64, num_fine_samples=128).to(dev)
        net.load_state_dict(state)
        return net
    ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
    batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd)

    # the ball whose radius keeps about `kept` of the frame's own level-0 samples (clip=True: outside the box nothing is kept)
    t0 = torch.linspace(0.0, 1.0, 65, device=dev)
    t0 = (NEAR * (1.0 - t0) + FAR * t0)[None, :].expand(H * W, 65)
    grids = {}
    for kept in (0.5, 0.25, 0.1):
        lo, hi = 0.0, 1.8
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            frac = float(marching.occupancy_keep_box(ball(mid), BOX, ro, vd, t0, clip=True).float().mean())
            lo, hi = (mid, hi) if frac < kept else (lo, mid)
        grids[kept] = (ball(hi), hi)
    del t0

    def plain(net):
        return lambda: render.render_rays_test(net, batch, chunk=CHUNK, near=NEAR, far=FAR, check=False)

    def march(net, eps):
        return lambda: marching.render_marching_rays(net, batch, eps, chunk=args.march_chunk, near=NEAR, far=FAR, check=False)

    def compare(net, arms):
        """arms: [(name, (grid, clip) or None, fn)]; frames alternate over the arms.  Returns {name: dict} and the last results."""
        def install(g):
            if g is None:
                net.set_occupancy(None)
            else:
                net.set_occupancy(g[0], BOX, g[1])
        for name, g, fn in arms:
            install(g)
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in arms}
        last = {}
        for _ in range(args.frames):              # alternating: every arm sees the same clocks and neighbours
            for name, g, fn in arms:
                install(g)
                torch.cuda.synchronize()
                t, last[name] = timed(fn)
                ms[name].append(t)
        net.check_flags()
        net.set_occupancy(None)
        out = {}
        for name, g, fn in arms:
            arm = dict(frame=spread(ms[name]))
            if "kept_fraction" in last[name]:
                arm["kept_fraction_level0"], arm["kept_fraction_level1"] = (float(x) for x in last[name]["kept_fraction"])
            out[name] = arm
            print("%s: %.1f ms [%.1f .. %.1f]%s" % (name, arm["frame"]["median_ms"], arm["frame"]["min_ms"], arm["frame"]["max_ms"],
                                                   "".join(", %s %.3f" % (k, v) for k, v in arm.items() if isinstance(v, float))), flush=True)
        return out, last

    result = dict(workload="vanilla 640x480, 65 + 193 samples, f16x3 (bench.py --workload vanilla)", rays=H * W, frames=args.frames,
                  warmup=args.warmup, segment=64, march_chunk=args.march_chunk,
                  grids={str(k): dict(resolution=G, box=BOX, clip=True, shape="centred ball", radius=r,
                                      occupied_cells_fraction=float(g.float().mean())) for k, (g, r) in grids.items()})

    def save():
        if args.out:          # after every comparison: a run that is cut short keeps what it measured
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)

    net = module(0.0)
    ones = torch.ones(G, G, G, dtype=torch.bool)
    arms, last = compare(net, [("plain", None, plain(net)), ("ones_eps0", (ones, False), march(net, 0.0))] +
                         [("ball_%g" % k, (grids[k][0], True), march(net, 0.0)) for k in (0.5, 0.25, 0.1)])
    arms["ones_eps0"]["bitwise_plain"] = bool(torch.equal(last["ones_eps0"]["rgb"], last["plain"]["rgb"]))
    for k, v in arms.items():
        v["over_plain"] = v["frame"]["median_ms"] / arms["plain"]["frame"]["median_ms"]
    result["synthetic_weights"] = arms
    save()
    net.close()

    fog = module(args.fog_bias)
    arms, last = compare(fog, [("plain", None, plain(fog)), ("fog_eps", None, march(fog, args.eps)),
                               ("fog_eps_ball_0.25", (grids[0.25][0], True), march(fog, args.eps))])
    for k, v in arms.items():
        v["over_plain"] = v["frame"]["median_ms"] / arms["plain"]["frame"]["median_ms"]
    arms["fog_eps"]["max_abs_rgb_change_against_plain"] = float((last["fog_eps"]["rgb"] - last["plain"]["rgb"]).abs().max())
    result["fog"] = dict(density_bias=args.fog_bias, eps=args.eps, bound_1_003_eps=1.003 * args.eps, arms=arms)
    save()
    print(json.dumps({k: v["over_plain"] for part in (result["synthetic_weights"], result["fog"]["arms"]) for k, v in part.items()}))


if __name__ == "__main__":
    main()
