"""Frame time of rendering every instance of a scene: the loop of one `render_objects` call per instance against the one
`render_instances` call.

The frame is bench.py's: 640 x 480 rays from look_at_origin(40), 3 source views, 128 + 256 samples, reference chunk 1024, the
synthetic N(0, 0.1) scene with both foreground density biases raised by +6.  The instances are the five boxes of the instance
tests (tests/instance_cases.py: A, B, F, G, D).

  loop      per box: ops.sample_rays_in_bbox on a one-element RTs + model.render_objects           (K interval + K render calls)
  one call  ops.sample_rays_in_bbox_list on all boxes + model.render_instances                      (1 interval + 1 render call)

Both sides ALTERNATE in one process, every frame between two device events, medians and spread (min, quartiles, max) over
--frames frames per side after --warmup.  Two arms: `boxes` (the five boxes) and `all_miss` (five instances whose intervals are
all zero: the fixed cost of the K empty windows of the one call, against K render_objects calls without a hit).  The pair count
and the per-box hit counts are read back after the timing.

  python tools/bench_instances.py --out profiles/instances_bench.json
"""
import argparse
import json
import math
import os
import statistics
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


# the boxes of tests/object_cases.py and tests/instance_cases.py (the reference's RTs entries)
BOXES = (
    ("A", dict(R=_rot_z(0.4) @ _rot_x(-0.3), T=np.array([0.05, -0.05, 0.0]), s=_bounds((0.18, 0.12, 0.15)))),
    ("B", dict(R=np.eye(3), T=np.array([-0.25, 0.2, 0.05]), s=_bounds(0.1))),
    ("F", dict(R=_rot_z(0.4) @ _rot_x(-0.3), T=np.array([0.29, 0.18, 0.18]), s=_bounds((0.06, 0.06, 0.02)))),
    ("G", dict(R=_rot_z(0.8), T=np.array([0.10, 0.02, 0.02]), s=_bounds((0.10, 0.16, 0.10)))),
    ("D", dict(R=np.eye(3), T=np.array([0.0, 0.0, 0.9]), s=_bounds(0.03))),
)


def spread(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), q1_ms=q[0], q3_ms=q[2], max_ms=max(ms))


def rts(boxes):
    return dict(R=[b["R"] for b in boxes], T=[b["T"] for b in boxes], s=[b["s"] for b in boxes])


class Frame:
    def __init__(self, dev):
        from neo360_amd import models, ops, synth
        self.dev, self.ops = dev, ops
        nv = 3
        state = synth.nerf_tp_state(0)
        for k in BIASED:
            state[k] = state[k] + 6.0
        self.net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(dev)
        self.net.load_state_dict(state)
        sc = {k: v.to(dev) for k, v in synth.scene_features(0, nv, 128, (120, 160), 512, (240, 320), std=0.1).items()}
        self.net.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], (float(W), float(H)))
        poses, focal, centre = synth.source_views(nv, W, H)
        ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
        self.batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd, src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                          src_imgs=torch.zeros(nv, 3, H, W, device=dev))
        self.boxes = [b for _, b in BOXES]
        self.zero = torch.zeros(len(self.boxes), H * W, device=dev)

    # the five boxes
    def loop(self):
        out = []
        for box in self.boxes:
            near, far, _ = self.ops.sample_rays_in_bbox(rts([box]), self.batch["rays_o"], self.batch["viewdirs"])
            out.append(self.net.render_objects(self.batch, near, far, chunk=CHUNK))
        return out

    def one_call(self):
        near, far, _ = self.ops.sample_rays_in_bbox_list(rts(self.boxes), self.batch["rays_o"], self.batch["viewdirs"])
        return self.net.render_instances(self.batch, near, far, chunk=CHUNK)

    # five instances without a hit: given intervals, no box test on either side
    def loop_miss(self):
        return [self.net.render_objects(self.batch, self.zero[i], self.zero[i], chunk=CHUNK) for i in range(len(self.boxes))]

    def one_call_miss(self):
        return self.net.render_instances(self.batch, self.zero, self.zero, chunk=CHUNK)

    @staticmethod
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def arm(self, name, loop, one, frames, warmup):
        for _ in range(warmup):
            loop()
            one()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(frames):                   # alternating: both sides see the same clocks and neighbours
            a.append(self.timed(loop))
            b.append(self.timed(one))
        self.net.check_flags()
        pairs = int(self.net.last_instance_pairs)
        la, lb = spread(a), spread(b)
        diff = lb["median_ms"] - la["median_ms"]
        return dict(arm=name, rays=H * W, instances=len(self.boxes), hit_pairs=pairs, loop=la, one_call=lb,
                    one_call_minus_loop_ms=diff, loop_spread_ms=la["max_ms"] - la["min_ms"],
                    one_call_over_loop=lb["median_ms"] / la["median_ms"],
                    one_call_slower_than_the_loops_spread_allows=bool(diff > la["max_ms"] - la["min_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_instances.py measures on a ROCm device: there is no CPU figure for a frame time"
    torch.set_grad_enabled(False)
    if args.frames < 20:
        print("note: fewer than 20 frames per side", file=sys.stderr)
    fr = Frame(torch.device("cuda:0"))
    _, _, hit = fr.ops.sample_rays_in_bbox_list(rts(fr.boxes), fr.batch["rays_o"], fr.batch["viewdirs"])
    result = dict(frame="640x480, 3 views, 128+256 samples, chunk 1024, density bias +6, five boxes A B F G D",
                  device=torch.cuda.get_device_name(0),
                  hits_per_box={n: int(h) for (n, _), h in zip(BOXES, hit.sum(dim=1).tolist())}, arms=[])
    for name, loop, one in (("boxes", fr.loop, fr.one_call), ("all_miss", fr.loop_miss, fr.one_call_miss)):
        a = fr.arm(name, loop, one, args.frames, args.warmup)
        result["arms"].append(a)
        print("%-8s pairs %d: loop %.2f ms [%.2f .. %.2f]  one call %.2f ms [%.2f .. %.2f]  x%.3f"
              % (name, a["hit_pairs"], a["loop"]["median_ms"], a["loop"]["min_ms"], a["loop"]["max_ms"], a["one_call"]["median_ms"],
                 a["one_call"]["min_ms"], a["one_call"]["max_ms"], a["one_call_over_loop"]), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
