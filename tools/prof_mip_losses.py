"""Times Mip-NeRF 360's interlevel + distortion losses, forward and backward, (a) on the native kernels (training.lossfun_outer /
lossfun_distortion) and (b) as eager torch (the restatement of the reference's formulas in tests/mip_loss_cases.py, on the same
GPU), and the whole training step (mip_render_train + training_step's loss + backward) with either.  Device events around each
repeat, warm-up first, the two variants alternating in one process; per variant the median and the spread (min, max, quartiles) of
the repeats.  Writes profiles/mip_losses_timing.json (--out).

Histograms of one training step: two proposal levels of 64 intervals and a final level of 32 (the reference's defaults) or 128
(mip360_128), at 1024 rays (its default batch) and 4096.

    python tools/prof_mip_losses.py [--repeats 30] [--step-repeats 8] [--out profiles/mip_losses_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import cases  # noqa: E402
import mip_loss_cases as M  # noqa: E402
from neo360_amd import models, synth, training  # noqa: E402

DEV = "cuda"
N_PROP = 64
CONFIGS = [(1024, 32), (4096, 32), (1024, 128), (4096, 128)]      # (rays, final-level intervals)


def histogram(R, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.sort(torch.rand(R, n + 1, generator=g), -1).values
    t[:, 0], t[:, -1] = 0, 1
    w = torch.rand(R, n, generator=g) ** 3
    return t.to(DEV), (w / w.sum(-1, keepdim=True)).to(DEV)


def losses_native(history):
    return training.mip_interlevel_loss(history) + 0.01 * training.mip_distortion_loss(history)


def losses_eager(history):
    return M.interlevel_loss(history) + 0.01 * M.distortion_loss(history)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, repeats, warmup=3):
    """variants: name -> callable.  Returns name -> dict(median_ms, min_ms, max_ms, q1_ms, q3_ms, repeats)."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    out = {}
    for k, v in ms.items():
        q = statistics.quantiles(v, n=4)
        out[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), q1_ms=q[0], q3_ms=q[2], repeats=len(v))
    return out


def verdict(res):
    """(a) is not slower than (b) beyond the run-to-run spread: the medians compared, the larger interquartile range allowed."""
    a, b = res["native"], res["eager"]
    spread = max(a["q3_ms"] - a["q1_ms"], b["q3_ms"] - b["q1_ms"])
    return dict(speedup=b["median_ms"] / a["median_ms"], spread_ms=spread, native_not_slower=a["median_ms"] <= b["median_ms"] + spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--step-repeats", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mip_losses_timing.json"))
    args = ap.parse_args()
    torch.set_grad_enabled(True)
    report = dict(device=torch.cuda.get_device_name(0), n_prop=N_PROP, losses=[], step=[])
    for R, n in CONFIGS:
        hist = [dict(zip(("sdist", "weights"), histogram(R, m, 17 + l))) for l, m in enumerate((N_PROP, N_PROP, n))]
        ws = [h["weights"].requires_grad_(True) for h in hist]

        def run(fn):
            return lambda: torch.autograd.grad(fn(hist), ws)

        got_a, got_b = run(losses_native)(), run(losses_eager)()
        agree = max(float((x - y).abs().max()) for x, y in zip(got_a, got_b))
        res = alternate(dict(native=run(losses_native), eager=run(losses_eager)), args.repeats)
        row = dict(rays=R, n_final=n, max_abs_gradient_difference=agree, **res, **verdict(res))
        report["losses"].append(row)
        print("losses  R=%d n=%d  native %.3f ms  eager %.3f ms  x%.1f" % (R, n, res["native"]["median_ms"], res["eager"]["median_ms"], row["speedup"]))
    for R, n in CONFIGS:
        net = models.MipNeRF360(num_prop_samples=N_PROP, num_nerf_samples=n).to(DEV)
        net.load_state_dict(synth.mip360_state(0, weight_gain=0.25))
        params = [p for p in net.parameters()]
        rays = {k: v.to(DEV) for k, v in cases.mip_rays(R).items()}
        target = synth.uniform(93, "mip_target", (R, 3), 0.0, 1.0).to(DEV)

        def step(native):
            def go():
                for p in params:
                    p.grad = None
                rend, hist = training.mip_render_train(net, rays, 0.5, True, 0.2, 3.0, seed=13)
                if native:
                    loss, _ = training.mip_training_loss(rend, hist, target)
                else:
                    loss = M.training_loss(rend[-1]["rgb"], hist, target)
                loss.backward()
            return go

        res = alternate(dict(native=step(True), eager=step(False)), args.step_repeats, warmup=2)
        row = dict(rays=R, n_final=n, **res, **verdict(res))
        report["step"].append(row)
        print("step    R=%d n=%d  native %.2f ms  eager %.2f ms  x%.2f" % (R, n, res["native"]["median_ms"], res["eager"]["median_ms"], row["speedup"]))
        del net
    report["condition_met"] = all(r["native_not_slower"] for r in report["losses"] + report["step"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print("condition met:", report["condition_met"], "->", args.out)


if __name__ == "__main__":
    main()
