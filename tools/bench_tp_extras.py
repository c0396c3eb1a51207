"""Cost of NeRF_TP.compute_extras on the 640 x 480 NeO-360 evaluation frame (bench.py's frame: rays from look_at_origin(40),
3 source views, 128 + 256 samples, reference chunk 1024, the synthetic N(0, 0.1) scene, ONE library call per frame through
render.render_frame_sharded with the pixel-grid hint; the frame API asks for the fine level only, so one level carries extras).

Frames with the attribute off and on ALTERNATE in one process, every frame between two device events; medians and spread (min,
quartiles, max) over --frames frames per side after --warmup.  With the attribute on, the two level-1 composites also write their
weights (2 x R x 385 floats) and one k_tp_extras launch follows the merge.  Next to the frame time, that launch on its own:
ops.tp_extras on the level-1 rows of the frame, between two device events, --reps times, against the traffic it needs (4 rows of
385 floats and 8 floats of ray and scalars read per ray, 5 floats written).

  python tools/bench_tp_extras.py --out profiles/tp_extras_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

H, W, CHUNK, NV = 480, 640, 1024, 3
N_COARSE, N_FINE = 128, 256


def spread(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), q1_ms=q[0], q3_ms=q[2], max_ms=max(ms))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tp_extras.py measures on a ROCm device: there is no CPU figure for a frame time"
    torch.set_grad_enabled(False)
    from neo360_amd import models, ops, render, synth
    dev = torch.device("cuda:0")
    net = models.NeRF_TP(num_coarse_samples=N_COARSE, num_fine_samples=N_FINE, num_src_views=NV).to(dev)
    net.load_state_dict(synth.nerf_tp_state(0))
    sc = {k: v.to(dev) for k, v in synth.scene_features(0, NV, 128, (120, 160), 512, (240, 320), std=0.1).items()}
    net.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], (float(W), float(H)))
    poses, focal, centre = synth.source_views(NV, W, H)
    ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
    batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd, src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                 src_imgs=torch.zeros(NV, 3, H, W, device=dev))
    R = H * W

    def frame(on):
        net.compute_extras = on
        try:
            return render.render_rays_test(net, batch, CHUNK, near=0.0, far=0.0, check=False, image_width=W)
        finally:
            net.compute_extras = False

    for _ in range(args.warmup):
        frame(False)
        frame(True)
    torch.cuda.synchronize()
    off, on = [], []
    for _ in range(args.frames):                      # alternating: both sides see the same clocks and neighbours
        off.append(timed(lambda: frame(False))[0])
        last = timed(lambda: frame(True))
        on.append(last[0])
    net.check_flags()
    out = last[1]
    med = out["distance_median"]
    result = dict(frame="neo360 640x480, %d views, %d + %d samples, chunk %d, one library call per frame" % (NV, N_COARSE, N_FINE, CHUNK),
                  rays=R, extras_off=spread(off), extras_on=spread(on),
                  difference_of_medians_ms=statistics.median(on) - statistics.median(off),
                  relative_difference=statistics.median(on) / statistics.median(off) - 1.0,
                  rays_whose_median_leaves=int(torch.isinf(med).sum()),
                  finite_median_min_max=[float(med[torch.isfinite(med)].min()), float(med[torch.isfinite(med)].max())],
                  opacity_min_max=[float(out["opacity"].min()), float(out["opacity"].max())])
    # the launch on its own, on the level-1 rows of the frame
    n = N_COARSE + 1 + N_FINE
    full = net(batch, False, False, 0.0, 0.0, out_depth=True, chunk=CHUNK)
    rows = net._forward_train(batch, False, False, CHUNK, None, _raw=True)[1]
    far, _ = ops.intersect_sphere(ro, rd)
    net.check_flags()
    call = lambda: ops.tp_extras(rows["fg_t"], rows["fg_w"], far, ro, rd, rows["bg_t"], rows["bg_w"], full[1][4])
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = [timed(call)[0] for _ in range(args.reps)]
    read, written = R * (4 * n + 8) * 4, R * 5 * 4
    result["launch"] = dict(samples_per_region=n, bytes_read=read, bytes_written=written, **spread(ms),
                            gb_per_s_at_median=(read + written) / statistics.median(ms) / 1e6)
    result["extra_weight_bytes_written_per_frame"] = 2 * R * n * 4
    print("frame: extras off %.2f ms [%.2f .. %.2f], on %.2f ms [%.2f .. %.2f], difference of medians %+.3f ms (%+.3f %%); "
          "launch alone %.4f ms median [%.4f .. %.4f], %.0f GB/s"
          % (result["extras_off"]["median_ms"], min(off), max(off), result["extras_on"]["median_ms"], min(on), max(on),
             result["difference_of_medians_ms"], 100 * result["relative_difference"], statistics.median(ms), min(ms), max(ms),
             result["launch"]["gb_per_s_at_median"]), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
