"""Frame time of the decomposed render against the plain frame render.

The frame is bench.py's: 640 x 480 rays from look_at_origin(40), 3 source views, 128 + 256 samples, reference chunk 1024, the
synthetic N(0, 0.1) scene with both foreground density biases raised by +6.  The instances are the five boxes of the instance
tests (tests/instance_cases.py: A, B, F, G, D); their intervals are computed once, outside the timing.

  forward      model(batch, False, False, near, far, out_depth=True, chunk=1024)               (both levels returned)
  decomposed   model.render_decomposed(batch, near_inst, far_inst, chunk=1024, levels=(1,))    (one k_tp_decompose launch, on the
               fine level's 385-sample rows: about 118 M float4 rows plus their weights and positions, 2.8 GB)

Both ALTERNATE in one process, every frame between two device events, medians and spread (min, quartiles, max) over --frames
frames per side after --warmup.  No target: nobody has measured this launch before.  The one-call `render_instances` time of
profiles/instances_bench.json (the same frame and boxes) is copied into the result for context when that file is there.

  python tools/bench_decompose.py --out profiles/decompose_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench_instances import BOXES, CHUNK, H, W, Frame, rts, spread  # noqa: E402


def _instances_context():
    path = os.path.join(ROOT, "profiles", "instances_bench.json")
    try:
        with open(path) as f:
            arms = json.load(f)["arms"]
        return next(a["one_call"]["median_ms"] for a in arms if a.get("arm") == "boxes")
    except (OSError, KeyError, StopIteration, ValueError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decompose.py measures on a ROCm device: there is no CPU figure for a frame time"
    torch.set_grad_enabled(False)
    if args.frames < 20:
        print("note: fewer than 20 frames per side", file=sys.stderr)
    fr = Frame(torch.device("cuda:0"))
    net, batch = fr.net, fr.batch
    near, far, hit = fr.ops.sample_rays_in_bbox_list(rts(fr.boxes), batch["rays_o"], batch["viewdirs"])

    sides = (("forward", lambda: net(batch, False, False, 0.0, 0.0, out_depth=True, chunk=CHUNK)),
             ("decomposed", lambda: net.render_decomposed(batch, near, far, chunk=CHUNK, levels=(1,))))
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
    # what the frame holds: the last decomposed frame against the last plain one
    plain = net(batch, False, False, 0.0, 0.0, out_depth=True, chunk=CHUNK)
    dec = net.render_decomposed(batch, near, far, chunk=CHUNK, levels=(1,))
    net.check_flags()
    same = all(torch.equal(x, y) for lv in range(2) for x, y in zip(plain[lv], dec[lv][:6]))
    ids = dec[1][6]["id"]
    res = {name: spread(v) for name, v in ms.items()}
    base = res["forward"]["median_ms"]
    added = res["decomposed"]["median_ms"] - base
    width = res["forward"]["max_ms"] - res["forward"]["min_ms"]
    result = dict(frame="640x480, 3 views, 128+256 samples, chunk 1024, density bias +6, five boxes A B F G D",
                  device=torch.cuda.get_device_name(0), rays=H * W,
                  hits_per_box={n: int(h) for (n, _), h in zip(BOXES, hit.sum(dim=1).tolist())}, sides=res,
                  decomposed_minus_forward_ms=added, forward_spread_ms=width, added_time_inside_forward_spread=bool(abs(added) <= width),
                  six_tuples_bitwise_forward=bool(same),
                  id_histogram={str(int(v)): int((ids == v).sum()) for v in ids.unique()},
                  render_instances_one_call_median_ms_for_context=_instances_context())
    for name, _ in sides:
        r = res[name]
        print("%-10s %.2f ms [%.2f .. %.2f]  x%.3f" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["median_ms"] / base), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
