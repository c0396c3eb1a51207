"""Frame time of the object-level render (NeRF_TP.render_objects through render.render_object_rays) against the full NeO-360
evaluation frame.

The frame is bench.py's: 640 x 480 rays from look_at_origin(40), 3 source views, 128 + 256 samples, reference chunk 1024, the
synthetic N(0, 0.1) scene, ONE library call per frame.  The per-ray intervals come from ops.sample_rays_in_bbox for the two
oriented boxes of the object tests (tests/object_cases.py): both boxes, box A alone, box B alone (a one-element RTs).

Per arm and precision: object frames and full render_rays_test frames ALTERNATE in one process, every frame between two device
events, median [min .. max] over --frames frames per side after --warmup.  The hit fraction is read back after the timing.  One
more frame of each kind is then run with the library's launch spans on, for the durations of the evaluator launches alone: the
expectation an object frame is compared with is  hit fraction x (the full frame's two foreground launches) + the small kernels.

  python tools/bench_objects.py --out profiles/objects_bench.json [--parent-lib PATH]

--parent-lib: the default (un-culled) full frame of this tree's library against another build of the library (the parent
commit's), in fresh processes that alternate on the same device (one library per process: $NEO360_HIP_LIB), the parent also
against itself.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, CHUNK = 480, 640, 1024
BIASED = ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias")


def _rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _bounds(h):
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
    return np.stack([-h, h])


# the boxes of tests/object_cases.py (the reference's RTs entries: box-to-world R, T and the corner bounds in the box frame)
BOX_A = dict(R=_rot_z(0.4) @ _rot_x(-0.3), T=np.array([0.05, -0.05, 0.0]), s=_bounds((0.18, 0.12, 0.15)))
BOX_B = dict(R=np.eye(3), T=np.array([-0.25, 0.2, 0.05]), s=_bounds(0.1))
ARMS = (("A+B", (BOX_A, BOX_B)), ("A", (BOX_A,)), ("B", (BOX_B,)))


def spread(ms):
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


class Frame:
    def __init__(self, dev, precision=None):
        from neo360_amd import _lib, models, ops, render, synth
        if os.environ.get("NEO360_HIP_LIB"):
            # another build of the library may predate the object entry point: the full-frame A/B does not call it
            import ctypes
            other = ctypes.CDLL(_lib.LIB_PATH)
            for name in [n for n in _lib.SIGNATURES if not hasattr(other, n)]:
                del _lib.SIGNATURES[name]
        self.dev, self.render, self.ops = dev, render, ops
        nv = 3
        state = synth.nerf_tp_state(0)
        for k in BIASED:
            state[k] = state[k] + 6.0
        self.net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(dev)
        self.net.load_state_dict(state)
        if precision is not None:
            self.net.precision = precision
        sc = {k: v.to(dev) for k, v in synth.scene_features(0, nv, 128, (120, 160), 512, (240, 320), std=0.1).items()}
        self.net.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], (float(W), float(H)))
        poses, focal, centre = synth.source_views(nv, W, H)
        ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
        self.batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd, src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                          src_imgs=torch.zeros(nv, 3, H, W, device=dev))

    def set_boxes(self, boxes):
        rts = dict(R=[b["R"] for b in boxes], T=[b["T"] for b in boxes], s=[b["s"] for b in boxes])
        near, far, mask = self.ops.sample_rays_in_bbox(rts, self.batch["rays_o"], self.batch["viewdirs"])
        self.batch["near_obj"], self.batch["far_obj"] = near, far
        return float(mask.float().mean())

    def full(self):
        return self.render.render_rays_test(self.net, self.batch, chunk=CHUNK, near=0.0, far=0.0, check=False, image_width=W)

    def objects(self):
        return self.render.render_object_rays(self.net, self.batch, chunk=CHUNK, check=False)

    @staticmethod
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def spans(self, fn):
        """[(kernel, ms)] of the evaluator launches of one frame, and that frame's duration with the spans on."""
        ctx = self.net._context(self.dev)
        ctx.set_timing(True)
        try:
            ms = self.timed(fn)
            torch.cuda.synchronize()
            got = [(name, t) for t, name, _, _ in ctx.read_spans()]
        finally:
            ctx.set_timing(False)
        return got, ms

    def arm(self, name, boxes, frames, warmup):
        mask_fraction = self.set_boxes(boxes)
        for _ in range(warmup):
            self.full()
            self.objects()
        torch.cuda.synchronize()
        full, obj = [], []
        for _ in range(frames):                   # alternating: both sides see the same clocks and neighbours
            full.append(self.timed(self.full))
            obj.append(self.timed(self.objects))
        self.net.check_flags()
        hits = int(self.net.last_object_hits)
        full_spans, _ = self.spans(self.full)
        obj_spans, obj_ms_with_spans = self.spans(self.objects)
        self.net.check_flags()
        fg_full = full_spans[0][1] + full_spans[2][1]          # launch order: fg coarse, bg coarse, fg fine, bg fine
        obj_eval = sum(t for _, t in obj_spans)
        frac = hits / float(H * W)
        f, o = statistics.median(full), statistics.median(obj)
        return dict(boxes=name, rays=H * W, hits=hits, hit_fraction=frac, mask_fraction_of_sample_rays_in_bbox=mask_fraction,
                    full_frame=spread(full), object_frame=spread(obj), object_over_full=o / f,
                    full_frame_evaluator_launches_ms=[[n, t] for n, t in full_spans],
                    object_frame_evaluator_launches_ms=[[n, t] for n, t in obj_spans],
                    full_frame_foreground_launches_ms=fg_full,
                    expected_evaluator_ms_hit_fraction_times_foreground=frac * fg_full,
                    object_frame_evaluator_ms=obj_eval,
                    object_frame_small_kernels_and_host_ms=obj_ms_with_spans - obj_eval)


def child_full(frames, warmup):
    fr = Frame(torch.device("cuda:0"))
    for _ in range(warmup):
        fr.full()
    torch.cuda.synchronize()
    print("CHILD " + json.dumps([fr.timed(fr.full) for _ in range(frames)]))


def library_ab(parent_lib, rounds, frames, warmup):
    """Fresh processes, this tree's library and the other build alternating; the other build twice per round so that its spread
    against ITSELF comes from the same run."""
    runs = {"this": [], "parent": []}
    for r in range(rounds):
        for which in ("parent", "this", "parent"):
            env = dict(os.environ)
            env.pop("NEO360_HIP_LIB", None)
            if which == "parent":
                env["NEO360_HIP_LIB"] = parent_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-full", "--frames", str(frames), "--warmup",
                                str(warmup)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
            if p.returncode != 0:
                raise RuntimeError("child (%s library) exited %d: the A/B stops here\n%s" % (which, p.returncode, p.stderr[-2000:]))
            ms = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
            runs[which].append(statistics.median(ms))
            print("library A/B round %d %-6s median %.2f ms" % (r, which, runs[which][-1]), flush=True)
    pm, tm = runs["parent"], runs["this"]
    return dict(frames_per_process=frames, parent_process_medians_ms=pm, this_process_medians_ms=tm,
                parent_median_ms=statistics.median(pm), parent_spread_ms=max(pm) - min(pm),
                this_median_ms=statistics.median(tm), this_spread_ms=max(tm) - min(tm),
                difference_ms=statistics.median(tm) - statistics.median(pm),
                criterion="this tree's median of process medians lies between the parent library's fastest and slowest process of the same run",
                inside_parent_spread=min(pm) <= statistics.median(tm) <= max(pm))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--precisions", default="f16x3,f32")
    ap.add_argument("--parent-lib", default=None, dest="parent_lib")
    ap.add_argument("--ab-rounds", type=int, default=3, dest="ab_rounds")
    ap.add_argument("--ab-frames", type=int, default=8, dest="ab_frames")
    ap.add_argument("--child-full", action="store_true", dest="child")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_objects.py measures on a ROCm device: there is no CPU figure for a frame time"
    torch.set_grad_enabled(False)
    if args.child:
        return child_full(args.frames, args.warmup)
    if args.frames < 20:
        print("note: fewer than 20 frames per side", file=sys.stderr)
    result = dict(frame="640x480, 3 views, 128+256 samples, chunk 1024, one library call per frame", precisions={})

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")
    for precision in [p for p in args.precisions.split(",") if p]:
        fr = Frame(torch.device("cuda:0"), precision)
        arms = result["precisions"][precision] = []
        for name, boxes in ARMS:
            a = fr.arm(name, boxes, args.frames, args.warmup)
            arms.append(a)
            print("%-5s boxes %-3s: hits %.3f  full %.2f ms [%.2f .. %.2f]  objects %.2f ms [%.2f .. %.2f]  = %.3f of the full frame; "
                  "evaluators %.2f ms against %.2f ms expected"
                  % (precision, name, a["hit_fraction"], a["full_frame"]["median_ms"], a["full_frame"]["min_ms"], a["full_frame"]["max_ms"],
                     a["object_frame"]["median_ms"], a["object_frame"]["min_ms"], a["object_frame"]["max_ms"], a["object_over_full"],
                     a["object_frame_evaluator_ms"], a["expected_evaluator_ms_hit_fraction_times_foreground"]), flush=True)
            save()
        fr.net.close()
        del fr
        torch.cuda.empty_cache()
    if args.parent_lib:
        result["library_ab_default_frame"] = library_ab(os.path.abspath(args.parent_lib), args.ab_rounds, args.ab_frames, args.warmup)
    save()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
