"""Training the vanilla NeRF through its occupancy grid (`marching.MarchingNeRF.render_train_marching`): one step = forward + backward
of the reference's two-level MSE loss (vanilla_nerf/model.py:281-283) on 4096 rays at 64 + 128 samples - a size chosen here, not the
reference's - with synth.vanilla_state(0), randomized=True.  Arms, each ALTERNATING step by step with the plain one in one process:

    plain                 training.nerf_render_train: every sample through the MLP
    no_grid               render_train_marching without a grid: the row builder, two count reads and the scatter, nothing saved
    ones                  an all-ones grid at G = 128 over [-1, 1]^3, clip=False: the same, with the grid read as well
    ball_0.5 / 0.25 / 0.1   centred-ball grids (tests/vanilla_march_cases.ball) at G = 128 over [-1, 1]^3 with clip=True, the radius
                          bisected until about that share of the level-0 samples is kept

Per arm: median [min .. max] of --steps (5) step times, the plain arm's times taken in the same alternation, and the kept
fractions per level from `last_train_kept`.  Also the time of one `update_occupancy` at G = 128.  The synthetic scene is a near
uniform fog seen through a ball-shaped grid: the kept fractions say what an arm saved HERE, not what a trained scene would save.
GPU only; reads nothing outside the repository.

    python tools/bench_vanilla_train_march.py --steps 5 --warmup 2 --out profiles/vanilla_train_march_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

RAYS = 4096
COUNTS = (64, 128)
G = 128
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
NEAR, FAR = 0.2, 3.0


def spread(ms):
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import vanilla_march_cases as vc
    from neo360_amd import marching, synth, training
    dev = torch.device("cuda:0")
    net = marching.MarchingNeRF(num_coarse_samples=COUNTS[0], num_fine_samples=COUNTS[1]).to(dev)
    net.load_state_dict(synth.vanilla_state(0))
    b = {k: v.to(dev) for k, v in vc.rays(RAYS).items()}
    target = synth.uniform(91, "vanilla_target", (RAYS, 3), 0.0, 1.0).to(dev)
    total = (RAYS * (COUNTS[0] + 1), RAYS * (COUNTS[0] + 1 + COUNTS[1]))

    # the ball whose radius keeps about `kept` of the deterministic level-0 samples (clip=True: outside the box nothing is kept)
    lin = torch.linspace(0.0, 1.0, COUNTS[0] + 1, device=dev)
    t0 = (NEAR * (1.0 - lin) + FAR * lin)[None, :].expand(RAYS, COUNTS[0] + 1).contiguous()
    grids = {}
    for kept in (0.5, 0.25, 0.1):
        lo, hi = 0.0, 1.8
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            frac = float(marching.occupancy_keep_box(vc.ball(G, mid), BOX, b["rays_o"], b["viewdirs"], t0, clip=True).float().mean())
            lo, hi = (mid, hi) if frac < kept else (lo, mid)
        grids[kept] = (vc.ball(G, hi), hi)

    def step(call, seed):
        """One forward + backward; returns (device ms between events, host ms until the gradients are complete)."""
        for p in net.parameters():
            p.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        e0.record()
        with torch.enable_grad():
            out = call(seed)
            loss = ((out[0][0] - target) ** 2).mean() + ((out[1][0] - target) ** 2).mean()
            loss.backward()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - h0) * 1e3

    plain = lambda seed: training.nerf_render_train(net, b, True, False, NEAR, FAR, seed=seed)
    through = lambda seed: net.render_train_marching(b, True, False, NEAR, FAR, seed=seed)
    arms = [("no_grid", None), ("ones", (torch.ones(G, G, G, dtype=torch.bool), False))] + \
           [("ball_%g" % k, (grids[k][0], True)) for k in (0.5, 0.25, 0.1)]
    for p in net.parameters():
        p.requires_grad_(True)

    def install(g):
        if g is None:
            net.set_occupancy(None)
        else:
            net.set_occupancy(g[0], BOX, g[1])

    result = dict(workload="vanilla training step, %d rays, %d + %d samples, forward + backward of the two-level MSE" % (RAYS, *COUNTS),
                  steps=args.steps, warmup=args.warmup,
                  grids={str(k): dict(resolution=G, box=BOX, clip=True, shape="centred ball", radius_half_widths=r,
                                      occupied_cells_fraction=float(g.float().mean())) for k, (g, r) in grids.items()}, arms={})

    def save():
        if args.out:          # after every arm: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)

    all_plain = []
    for name, g in arms:
        install(g)
        for i in range(args.warmup):
            step(plain, 1 + i)
            step(through, 1 + i)
        ms = {"plain": [], name: []}
        host = {"plain": [], name: []}
        for i in range(args.steps):              # alternating: both arms see the same clocks and neighbours
            for key, call in (("plain", plain), (name, through)):
                d, h = step(call, 10 + i)
                ms[key].append(d)
                host[key].append(h)
        all_plain += ms["plain"]
        kept = net.last_train_kept
        arm = dict(step=spread(ms[name]), step_host=spread(host[name]), plain_alongside=spread(ms["plain"]),
                   plain_alongside_host=spread(host["plain"]), kept_fraction_level0=kept[0] / total[0], kept_fraction_level1=kept[1] / total[1])
        arm["over_plain"] = arm["step"]["median_ms"] / arm["plain_alongside"]["median_ms"]
        result["arms"][name] = arm
        print("%s: %.2f ms [%.2f .. %.2f], plain alongside %.2f ms [%.2f .. %.2f], x%.3f, kept %.3f / %.3f"
              % (name, arm["step"]["median_ms"], arm["step"]["min_ms"], arm["step"]["max_ms"], arm["plain_alongside"]["median_ms"],
                 arm["plain_alongside"]["min_ms"], arm["plain_alongside"]["max_ms"], arm["over_plain"], arm["kept_fraction_level0"],
                 arm["kept_fraction_level1"]), flush=True)
        save()
    result["plain"] = spread(all_plain)
    net.set_occupancy(None)

    # one update of the running grid at G = 128: 2 M probe points through both MLPs, the density update, threshold + dilation, install
    for p in net.parameters():
        p.requires_grad_(False)
    net.init_occupancy(BOX, G, clip=True)
    ms = []
    for i in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        grid = net.update_occupancy(1.0)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    result["update_occupancy"] = dict(resolution=G, sigma_threshold=1.0, occupied_cells_fraction=float(grid.float().mean()), call=spread(ms))
    print("update_occupancy at G = %d: %.2f ms [%.2f .. %.2f]" % (G, result["update_occupancy"]["call"]["median_ms"], min(ms), max(ms)), flush=True)
    save()
    net.check_flags()
    print(json.dumps({k: v["over_plain"] for k, v in result["arms"].items()}))


if __name__ == "__main__":
    main()
