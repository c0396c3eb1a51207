"""Frame time of the edited render against the plain frame render.

The frame is bench.py's: 640 x 480 rays from look_at_origin(40), 3 source views, 128 + 256 samples, reference chunk 1024, the
synthetic N(0, 0.1) scene with both foreground density biases raised by +6.  The instances are the five boxes of the instance
tests (tests/instance_cases.py: A, B, F, G, D); their intervals are computed once, outside the timing.

  forward   model(batch, False, False, near, far, out_depth=True, chunk=1024)                  (both levels returned)
  removed   model.render_edited with all five instances at density scale 0                     (one k_tp_edit launch per level)
  moved     render.render_edited_rays with instance A moved by a rigid transform               (instance_layers: one interval call
            and one render_objects call on the transformed rays; then render_edited with one layer; includes its check_flags wait)

All three ALTERNATE in one process, every frame between two device events, medians and spread (min, quartiles, max) over
--frames frames per side after --warmup.  No target: nobody has measured these paths before.

  python tools/bench_edit.py --out profiles/edit_bench.json
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_instances import BOXES, CHUNK, H, W, Frame, rts, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edit.py measures on a ROCm device: there is no CPU figure for a frame time"
    torch.set_grad_enabled(False)
    if args.frames < 20:
        print("note: fewer than 20 frames per side", file=sys.stderr)
    from neo360_amd import render
    fr = Frame(torch.device("cuda:0"))
    net, batch, K = fr.net, fr.batch, len(fr.boxes)
    RTs = rts(fr.boxes)
    near, far, hit = fr.ops.sample_rays_in_bbox_list(RTs, batch["rays_o"], batch["viewdirs"])
    with_bounds = dict(batch, near_inst=near, far_inst=far)
    move = np.eye(4)
    c, s = math.cos(0.5), math.sin(0.5)
    move[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    move[:3, 3] = [-0.2, 0.15, 0.05]

    sides = (("forward", lambda: net(batch, False, False, 0.0, 0.0, out_depth=True, chunk=CHUNK)),
             ("removed", lambda: net.render_edited(batch, near, far, density_scale=[0.0] * K, chunk=CHUNK)),
             ("moved", lambda: render.render_edited_rays(net, with_bounds, RTs=RTs, moves={0: move}, chunk=CHUNK)))
    for _ in range(args.warmup):
        for _, fn in sides:
            fn()
    torch.cuda.synchronize()
    net.check_flags()
    ms = {name: [] for name, _ in sides}
    for _ in range(args.frames):                  # alternating: every side sees the same clocks and neighbours
        for name, fn in sides:
            ms[name].append(Frame.timed(fn))
    net.check_flags()
    res = {name: spread(v) for name, v in ms.items()}
    base = res["forward"]["median_ms"]
    result = dict(frame="640x480, 3 views, 128+256 samples, chunk 1024, density bias +6, five boxes A B F G D",
                  device=torch.cuda.get_device_name(0), rays=H * W,
                  hits_per_box={n: int(h) for (n, _), h in zip(BOXES, hit.sum(dim=1).tolist())},
                  moved_instance="A, rot_z(0.5) and (-0.2, 0.15, 0.05)", sides=res,
                  removed_minus_forward_ms=res["removed"]["median_ms"] - base, moved_minus_forward_ms=res["moved"]["median_ms"] - base,
                  forward_spread_ms=res["forward"]["max_ms"] - res["forward"]["min_ms"])
    for name, _ in sides:
        r = res[name]
        print("%-8s %.2f ms [%.2f .. %.2f]  x%.3f" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["median_ms"] / base), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
