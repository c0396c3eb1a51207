"""Empty-space skipping on the 640 x 480 NeO-360 frame of bench.py's default line (129 + 385 samples, chunk 1024, the synthetic
scene and weights of tools/bench_objects.py): `render.render_rays_test` against `render.render_skipping_rays` in one process,
alternating, at synthetic occupancy grids - a centred ball whose radius is bisected until about 100, 50, 25 and 10 % of the level-0
inside-sphere samples are kept (the kept fractions of BOTH levels are then read from the call's own counters and reported).

Also recorded: the classifier alone per level (`ops.occupancy_keep` on the level's dense rows); what the skipping machinery costs per
frame beyond the evaluators (the all-zeros grid's frame, which evaluates no inside-sphere point, minus the outside-sphere evaluator
launches and the small kernels of the plain frame: classify + compact + scatter + the empty compact launches of both levels); the
extra device memory the first skipping frame allocates; and - a diagnostic, not a bound - the largest density `eval_mlp` finds among
the samples a grid from `build_occupancy` skips on this synthetic scene.  GPU only; reads nothing outside the repository.

    python tools/bench_occupancy.py --frames 5 --warmup 2 --out profiles/occupancy_bench.json
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
BIASED = ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias", "bg_coarse_mlp.density_layer.bias", "bg_fine_mlp.density_layer.bias")
TARGETS = (1.0, 0.5, 0.25, 0.10)
G = 128


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from neo360_amd import models, ops, render, synth
    dev = torch.device("cuda:0")
    nv = 3
    state = synth.nerf_tp_state(0)
    for k in BIASED:
        state[k] = state[k] + 6.0
    net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(dev)
    net.load_state_dict(state)
    sc = {k: v.to(dev) for k, v in synth.scene_features(0, nv, 128, (120, 160), 512, (240, 320), std=0.1).items()}
    net.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], (float(W), float(H)))
    poses, focal, centre = synth.source_views(nv, W, H)
    ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
    batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd, src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                 src_imgs=torch.zeros(nv, 3, H, W, device=dev))
    R = H * W
    n_level = (129, 385)

    def plain():
        return render.render_rays_test(net, batch, chunk=CHUNK, near=0.0, far=0.0, check=False, image_width=W)

    def skipping():
        prev = getattr(net, "ray_grid", None)
        net.ray_grid = (W, 0)
        try:
            return render.render_skipping_rays(net, batch, chunk=CHUNK, check=False)
        finally:
            net.ray_grid = prev

    def spans(fn):
        ctx = net._context(dev)
        ctx.set_timing(True)
        try:
            ms, _ = timed(fn)
            torch.cuda.synchronize()
            got = [(name, t) for t, name, _, _ in ctx.read_spans()]
        finally:
            ctx.set_timing(False)
        return got, ms

    result = dict(workload="neo360 640x480, 129 + 385 samples, chunk 1024, f16x3 (bench.py's default line)", rays=R, grid_resolution=G,
                  frames=args.frames, warmup=args.warmup)
    for _ in range(args.warmup):
        plain()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(dev)[0]
    net.set_occupancy(torch.ones(G, G, G, dtype=torch.bool))
    frame = skipping()
    torch.cuda.synchronize()
    free_after = torch.cuda.mem_get_info(dev)[0]
    same = plain()
    net.check_flags()
    result["all_ones_bitwise_plain"] = bool(torch.equal(frame["rgb"], same["rgb"]) and torch.equal(frame["depth"], same["depth"]))
    window = 4096
    cap = window * n_level[1]
    result["extra_memory"] = dict(
        window_rays=window,
        compact_rows_bytes=cap * 64, direction_sum_rows_bytes=cap * 128, keep_mask_bytes=cap,
        device_free_memory_drop_of_first_skipping_frame_bytes=int(free_before - free_after))

    # the frame's own sample rows, for the bisection of the ball radius (level 0) and the classifier timing (both levels)
    rows = net.render_skipping(batch, chunk=CHUNK, return_samples=True)[2]
    net.check_flags()
    t_level = [rows[0][0].clone(), rows[1][0].clone()]
    del rows
    t0 = t_level[0]
    grids = {}
    for target in TARGETS:
        if target >= 1.0:
            grids[target] = torch.ones(G, G, G, dtype=torch.bool)
            continue
        lo, hi = 0.0, 1.8
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            frac = float(ops.occupancy_keep(ball(mid), ro, rd, t0).float().mean())
            lo, hi = (mid, hi) if frac < target else (lo, mid)
        grids[target] = ball(hi)
    arms = []
    for target in TARGETS:
        net.set_occupancy(grids[target])
        for _ in range(args.warmup):
            skipping()
        torch.cuda.synchronize()
        p_ms, s_ms = [], []
        kept = None
        for _ in range(args.frames):          # alternating: both sides see the same clocks and neighbours
            p_ms.append(timed(plain)[0])
            ms, out = timed(skipping)
            s_ms.append(ms)
            kept = out["kept_fraction"]
        net.check_flags()
        p, s = statistics.median(p_ms), statistics.median(s_ms)
        arms.append(dict(target_kept_fraction=target, kept_fraction_level0=float(kept[0]), kept_fraction_level1=float(kept[1]),
                         occupied_cells_fraction=float(grids[target].float().mean()), plain_frame=spread(p_ms), skipping_frame=spread(s_ms),
                         skipping_over_plain=s / p))
        print("kept %.3f / %.3f: plain %.1f ms, skipping %.1f ms (x %.3f)" % (float(kept[0]), float(kept[1]), p, s, s / p), flush=True)
    result["arms"] = arms

    # the machinery alone: the all-zeros grid evaluates no inside-sphere point
    net.set_occupancy(torch.zeros(G, G, G, dtype=torch.bool))
    for _ in range(args.warmup):
        skipping()
    zero_ms = [timed(skipping)[0] for _ in range(args.frames)]
    zero_spans, zero_with_spans = spans(skipping)
    plain_spans, plain_with_spans = spans(plain)
    net.check_flags()
    plain_small = plain_with_spans - sum(t for _, t in plain_spans)
    zero_eval = sum(t for _, t in zero_spans)
    result["all_zeros_grid"] = dict(
        frame=spread(zero_ms), evaluator_launches_ms=[[n, t] for n, t in zero_spans],
        plain_frame_evaluator_launches_ms=[[n, t] for n, t in plain_spans], plain_frame_small_kernels_and_host_ms=plain_small,
        classify_compact_scatter_and_host_ms_both_levels=zero_with_spans - zero_eval - plain_small)
    cls = {}
    for lv, n in enumerate(n_level):
        t = t_level[lv]
        assert t.shape[1] == n
        grid = grids[0.5]
        ops.occupancy_keep(grid, ro, rd, t)
        torch.cuda.synchronize()
        cls["level%d" % lv] = spread([timed(lambda: ops.occupancy_keep(grid, ro, rd, t))[0] for _ in range(args.frames)])
    result["classifier_stage_op_ms_including_grid_packing"] = cls

    # diagnostic: the largest density among the samples a built grid skips, on 4096 strided rays
    idx = torch.arange(0, R, R // 4096, device=dev)[:4096]
    sub = {k: (v[idx].contiguous() if k in ("rays_o", "rays_d", "viewdirs") else v) for k, v in batch.items()}
    lattice = net._occupancy_sigma(sub, 64, 1)
    thr = float(lattice.median())
    built = net.build_occupancy(sub, 64, thr, probes=1, dilate=1)
    res = net.render_skipping(sub, chunk=CHUNK, return_samples=True)
    net.check_flags()
    worst = []
    for lv in range(2):
        fg_t, _, _, fg_keep = res[2][lv]
        sigma = net.eval_mlp(lv, sub, fg_t, chunk=CHUNK)[..., 3]
        skipped = sigma[~fg_keep]
        worst.append(float(skipped.max()) if skipped.numel() else 0.0)
    result["built_grid_diagnostic"] = dict(resolution=64, probes=1, dilate=1, sigma_threshold_median_of_lattice=thr,
                                           occupied_cells_fraction=float(built.float().mean()), rays=4096,
                                           kept_fraction=[float(x) / (4096 * n) for x, n in zip(net.last_skip_kept.tolist(), n_level)],
                                           largest_skipped_sigma_per_level=worst)
    print(json.dumps(result["built_grid_diagnostic"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(arms=[(a["kept_fraction_level1"], a["skipping_over_plain"]) for a in arms])))


if __name__ == "__main__":
    main()
