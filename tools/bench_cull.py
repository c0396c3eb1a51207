"""Frame time of the NeO-360 evaluation frame with and without background culling (NeRF_TP.cull_background).

The frame is bench.py's: 640 x 480 rays from look_at_origin(40), 3 source views, 128 + 256 samples, reference chunk 1024, the
synthetic N(0, 0.1) scene, ONE library call per frame through render.render_frame_sharded with the pixel-grid hint.  The
foreground density biases are raised until the UN-culled render itself puts about 0 %, 50 % and 100 % of its rays in the culled
set at eps = 1e-2 (bisection on the bias for the middle arm: the fraction is monotone in it).

Per arm: culled and un-culled frames ALTERNATE in one process, every frame between two device events, medians and spread
(min, quartiles, max) over --frames frames per side after --warmup.

  python tools/bench_cull.py --out profiles/cull_bench.json [--parent-lib PATH]     the arms (a) + the library A/B (c)
  python tools/bench_cull.py --trace-bias 8.0 --frames 3                            a few culled frames for a kernel trace of its own

(c) --parent-lib: the un-culled frame of this tree's library against another build of the library (the parent commit's), in
fresh processes that alternate on the same box (one library per process: $NEO360_HIP_LIB), the parent also against itself.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

H, W, CHUNK, EPS = 480, 640, 1024, 1e-2
BIASED = ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias")


def spread(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), q1_ms=q[0], q3_ms=q[2], max_ms=max(ms))


class Frame:
    def __init__(self, dev):
        from neo360_amd import _lib, models, ops, render, synth
        if os.environ.get("NEO360_HIP_LIB"):
            # another build of the library may predate the culled entry point: the un-culled A/B does not call it
            import ctypes
            other = ctypes.CDLL(_lib.LIB_PATH)
            for name in [n for n in _lib.SIGNATURES if not hasattr(other, n)]:
                del _lib.SIGNATURES[name]
        self.dev, self.render, self.synth = dev, render, synth
        nv = 3
        self.state = synth.nerf_tp_state(0)
        self.net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(dev)
        self.net.load_state_dict(self.state)
        sc = {k: v.to(dev) for k, v in synth.scene_features(0, nv, 128, (120, 160), 512, (240, 320), std=0.1).items()}
        self.net.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], (float(W), float(H)))
        poses, focal, centre = synth.source_views(nv, W, H)
        ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
        self.batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd, src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                          src_imgs=torch.zeros(nv, 3, H, W, device=dev))

    def set_bias(self, bias):
        st = dict(self.state)
        for k in BIASED:
            st[k] = st[k] + bias
        self.net.load_state_dict(st)

    def frame(self, eps):
        self.net.cull_background = eps
        try:
            return self.render.render_frame_sharded(self.net, self.batch, 1, 0, chunk=CHUNK, n_rays=H * W, image_width=W,
                                                    near=0.0, far=0.0, check=False)
        finally:
            self.net.cull_background = None

    def timed(self, eps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.frame(eps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def culled_fraction(self):
        """What the UN-culled render itself reports: rays with both lambdas below eps."""
        self.net.cull_background = None
        out = self.net(self.batch, False, False, 0.0, 0.0, out_depth=True, chunk=CHUNK)
        self.net.check_flags()
        l0, l1 = out[0][4].reshape(-1), out[1][4].reshape(-1)
        return float(((l0 < EPS) & (l1 < EPS)).float().mean())

    def bias_for(self, target, lo=0.0, hi=8.0, steps=12):
        for _ in range(steps):
            mid = 0.5 * (lo + hi)
            self.set_bias(mid)
            if self.culled_fraction() < target:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)

    def arm(self, bias, frames, warmup):
        self.set_bias(bias)
        frac = self.culled_fraction()
        for _ in range(warmup):
            self.frame(None)
            self.frame(EPS)
        torch.cuda.synchronize()
        plain, culled = [], []
        for _ in range(frames):                   # alternating: both sides see the same clocks and neighbours
            plain.append(self.timed(None))
            culled.append(self.timed(EPS))
        self.net.check_flags()
        survivors = int(self.net.last_cull_survivors)
        return dict(bias=bias, eps=EPS, culled_fraction_from_unculled_render=frac, survivors=survivors, rays=H * W,
                    unculled=spread(plain), culled=spread(culled),
                    speedup_of_medians=statistics.median(plain) / statistics.median(culled))


def child_unculled(frames, warmup):
    fr = Frame(torch.device("cuda:0"))
    for _ in range(warmup):
        fr.frame(None)
    torch.cuda.synchronize()
    print("CHILD " + json.dumps([fr.timed(None) for _ in range(frames)]))


def library_ab(parent_lib, rounds, frames, warmup):
    """(c): fresh processes, this tree's library and the other build alternating; the other build twice per round so that its
    spread against ITSELF comes from the same run."""
    runs = {"this": [], "parent": []}
    for r in range(rounds):
        for which in ("parent", "this", "parent"):
            env = dict(os.environ)
            env.pop("NEO360_HIP_LIB", None)
            if which == "parent":
                env["NEO360_HIP_LIB"] = parent_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-unculled", "--frames", str(frames), "--warmup",
                                str(warmup)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
            if p.returncode != 0:
                raise RuntimeError("child (%s library) exited %d: the A/B stops here\n%s" % (which, p.returncode, p.stderr[-2000:]))
            ms = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
            runs[which].append(statistics.median(ms))
            print("library A/B round %d %-6s median %.2f ms" % (r, which, runs[which][-1]), flush=True)
    pm, tm = runs["parent"], runs["this"]
    return dict(frames_per_process=frames, parent_process_medians_ms=pm, this_process_medians_ms=tm,
                parent_median_ms=statistics.median(pm), parent_spread_ms=max(pm) - min(pm),
                this_median_ms=statistics.median(tm), difference_ms=statistics.median(tm) - statistics.median(pm),
                # the criterion: this tree's median lies between the parent's own fastest and slowest process of the same run
                inside_parent_spread=min(pm) <= statistics.median(tm) <= max(pm))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, dest="parent_lib")
    ap.add_argument("--ab-rounds", type=int, default=3, dest="ab_rounds")
    ap.add_argument("--ab-frames", type=int, default=8, dest="ab_frames")
    ap.add_argument("--trace-bias", type=float, default=None, dest="trace_bias")
    ap.add_argument("--child-unculled", action="store_true", dest="child")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cull.py measures on a ROCm device: there is no CPU figure for a frame time"
    torch.set_grad_enabled(False)
    if args.child:
        return child_unculled(args.frames, args.warmup)
    fr = Frame(torch.device("cuda:0"))
    if args.trace_bias is not None:
        fr.set_bias(args.trace_bias)
        print("culled fraction", fr.culled_fraction())
        for _ in range(args.warmup + args.frames):
            fr.frame(EPS)
        torch.cuda.synchronize()
        fr.net.check_flags()
        return
    if args.frames < 20:
        print("note: fewer than 20 frames per side", file=sys.stderr)
    half = fr.bias_for(0.5)
    result = dict(frame="640x480, 3 views, 128+256 samples, chunk 1024, one library call per frame", eps=EPS, arms=[])
    for bias in (0.0, half, 8.0):
        a = fr.arm(bias, args.frames, args.warmup)
        result["arms"].append(a)
        print("bias %+.3f: culled %.3f  un-culled %.2f ms [%.2f .. %.2f]  culled %.2f ms [%.2f .. %.2f]  x%.3f"
              % (bias, a["culled_fraction_from_unculled_render"], a["unculled"]["median_ms"], a["unculled"]["min_ms"],
                 a["unculled"]["max_ms"], a["culled"]["median_ms"], a["culled"]["min_ms"], a["culled"]["max_ms"],
                 a["speedup_of_medians"]), flush=True)
    del fr
    torch.cuda.empty_cache()
    if args.parent_lib:
        result["library_ab_unculled"] = library_ab(os.path.abspath(args.parent_lib), args.ab_rounds, args.ab_frames, args.warmup)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
