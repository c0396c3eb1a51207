"""Headline benchmark: rays/s of the full-frame render path on synthetic 640x480
frames (BASELINE.json metric), one process per GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload neo360|vanilla|mip360|mip360_128|pixelnerf]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
(the first form with N > 1 starts its N ranks itself, one process per GPU; both forms run the same code)

Default workload = the north-star path, BASELINE.json configs[2] (and [3] when N > 1): the NeO-360
tri-planar decoder, 3 source views, 640x480, 128 coarse + 256 fine samples per ray, inside + outside
sphere, reference chunk 1024.  `--workload vanilla` = configs[1], `mip360` / `mip360_128` = configs[4]
(reference default 64/64/32 and BASELINE's wording 64 + 128).

A plain run sets up, warms up, times the K steps and prints the line (headline + the roofline of the timed
steps).  `--full` adds everything that needs runs of its own: the CPU baseline and parity against it, the
once-per-scene set-up time, the reference-style chunk loop, and at N = 1 the exact fp32 kernels, one-step
numbers of the vanilla and mip360 configurations (`other_workloads`) and the training step.  The single
--cpu-rays / --others / --exact-f32 / --setup-timing / --chunk-loop / --train-step switches override either.
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (see dump_outputs).

A step = ray generation for this rank's range of the frame + coarse and fine render of its
contiguous range of whole 1024-ray chunks (+ ONE RCCL all-gather of the packed (rgb,depth,acc)
tiles when N > 1).  The frame is fixed, so scaling is "strong".  Rank 0 prints ONE JSON line.
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H, W = 480, 640
CHUNK = 1024
PEAK_F32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: dense fp32 MFMA (= fp32 vector peak)
PEAK_F16_MFMA_TFLOPS = 2500.0         # MI355X_MICROARCH.md: dense fp16/bf16 MFMA
PEAK_HBM_BYTES = 8.0e12               # MI355X_MICROARCH.md: HBM3E spec peak
PEAK_CLOCK_MHZ = 2400.0               # the clock the MFMA peaks above are quoted at (256 CUs x 2.4 GHz)
# torch threads of the CPU leg = the fastest setting of a sweep on the GPU box's host (2 x EPYC 9575F, 128 physical cores):
# NeO-360 is fastest on 8 threads (26.5 rays/s; 16: 21.5, 32: 8.4, 64: 6.3, 128: 2.5 - profiles/r03_cpu_threads_neo360.log:
# the gathers are memory-bound and the container's threads migrate), the dense vanilla / mip360 MLPs on 32
# (profiles/cpu_threads_r01.log)
CPU_THREADS = {"neo360": 8, "pixelnerf": 8}
CPU_THREADS_DEFAULT = 32
CPU_REPS = 3                          # >= 3 repetitions of the CPU sample
CPU_BUDGET_S = 150.0                  # no further repetition once the CPU leg has used this much (the default run finishes in minutes)


def physical_cores():
    """Physical cores of the host (unique (package, core) pairs of /proc/cpuinfo); os.cpu_count() counts SMT threads."""
    try:
        seen, pkg, core = set(), None, None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("physical id"):
                    pkg = line.split(":")[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":")[1].strip()
                elif not line.strip():
                    if pkg is not None and core is not None:
                        seen.add((pkg, core))
                    pkg = core = None
        if pkg is not None and core is not None:
            seen.add((pkg, core))
        if seen:
            return len(seen)
    except OSError:
        pass
    return os.cpu_count() or 1


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: the arrays a caller of the timed path received from its last step, one DIR/<name>.npy each, float32
    (float64 stays float64).  Above DUMP_LIMIT_BYTES in all, every array keeps the same fixed, seeded sample of its rows."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    out = {}
    for name, v in arrays.items():
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        out[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        for name, a in out.items():
            if a.ndim and a.shape[0] > 1:
                keep = max(1, int(a.shape[0] * DUMP_LIMIT_BYTES / total))
                rows = np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))
                out[name] = a[rows]
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)


def frame_outputs(frame):
    """The (R, 5) frame of render_frame_sharded as its caller reads it: rgb, depth, acc."""
    return {"rgb": frame[:, :3], "depth": frame[:, 3], "acc": frame[:, 4]}


# the translation unit of each workload's dominant kernel (split arithmetic) + the headers it is built from
KERNEL_SOURCES = {
    "neo360": ("mlp_tp_hp.hip", "mlp_tp_hpp.hip", "tp_hp_layout.h", "tp_common.h", "split_tile.h", "mfma_tile.h", "common.h", "kernels.h"),
    "vanilla": ("mlp_vanilla_h.hip", "mfma_tile.h", "common.h", "kernels.h"),
    "mip360": ("mlp_mip_h.hip", "mip_gemm_h.h", "mip_layered.h", "split_tile.h", "mfma_tile.h", "common.h", "kernels.h"),
    "mip360_128": ("mlp_mip_h.hip", "mip_gemm_h.h", "mip_layered.h", "split_tile.h", "mfma_tile.h", "common.h", "kernels.h"),
    "pixelnerf": ("mlp_pix_h.hip", "tp_common.h", "split_tile.h", "mfma_tile.h", "common.h", "kernels.h"),
    "neo360_train": ("train_mlp.hip", "train_chain.h", "training.hip", "train_kernels.h", "mfma_tile.h", "common.h", "kernels.h"),
}


def kernel_source_hash(workload="neo360"):
    """sha256 (first 16 hex digits) over the HIP source of the workload's dominant kernel and the headers it includes:
    stamps PMC summaries (tools/pmc_summarize.py) so a profile of an OLDER kernel is never attached to this build's numbers."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "neo-360_amd", "csrc")
    for name in KERNEL_SOURCES[workload]:
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


# MFMA products k_tp_mlp_hp really issues per point (NV source views; each algorithmic multiply = 3 fp16 products
# a_hi b_hi + a_hi b_lo + a_lo b_hi; padded k-steps counted): per view the streamed [world | pos_enc] stage
# (12 k-steps of 16 inside the sphere, 14 outside, x 256 outputs) + L1, L2, L3 (3 x 128 x 128); once per point the
# view-mean tail (view layer 0 with the bottleneck folded in, 160 x 64, and view layer 1, 64 x 64).  The 512-channel latent does
# not appear: it is pre-projected once per scene (scene_setup_ms).
def executed_flop_per_point_tp_hp(nv, outside, planes_projected=False):
    # planes_projected (mlp_tp_hpp.hip): the 8 world k-steps are gone as well (tri-planes pre-projected once per scene)
    per_view = ((14 if outside else 12) - (8 if planes_projected else 0)) * 16 * 256 + 3 * 128 * 128
    macs = nv * per_view + 160 * 64 + 64 * 64          # the bottleneck (128 x 128) is folded into view layer 0 at pack time (round 4)
    return macs * 3 * 2.0


def build_vanilla(dev):
    from neo360_amd import models, synth
    state = synth.vanilla_state(0)
    net = models.NeRF(num_coarse_samples=64, num_fine_samples=128).to(dev)
    net.load_state_dict(state)
    desc = ("vanilla_nerf 640x480 full frame, 64 coarse + 128 fine samples/ray (65+193 = 258 MLP points/ray), "
            "random-init 8x256 MLP, raygen + both levels")
    return net, state, {}, None, desc, dict(near=0.2, far=3.0), "k_vanilla_mlp", 4096


_SCENE_CACHE = {}

# what limits each split evaluator (PMC summaries + power envelope; `bound` stays the priced roofline)
LIMITER = {
    "neo360": "socket power limit (1.33-1.35 kW of 1.4 kW, clock 2.0-2.2 GHz): time = joules / power, and the ~222 J of an inside-sphere "
              "launch are set by its matrix instructions (3 fp16 products per multiply), their operand delivery and the gathers - removing "
              "6 % of the VALU instructions moved neither time nor joules (profiles/r05_tp_hp_experiments.log); matrix pipe ~40 % busy, "
              "VALU ~41 % of SIMD issue cycles (7.9 per MFMA), HBM < 5 %",
    "pixelnerf": "vector-ALU issue (9 VALU per MFMA) + socket power limit; matrix pipe ~40 % busy",
    "vanilla": "socket power limit (1.9 GHz at ~1.3 kW; the same instruction stream on zero operands runs at 2.4 GHz) on top of "
               "operand delivery (matrix pipe ~62 % busy)",
    "mip360": "socket power limit on top of operand delivery of the 256 x 256-tile GEMM chain (matrix pipe ~55 % busy)",
    "mip360_128": "socket power limit on top of operand delivery of the 256 x 256-tile GEMM chain (matrix pipe ~55 % busy)",
    "f32": "the fp32 matrix pipe itself (v_mfma_f32_32x32x2_f32 at 1/16 of the fp16 rate) + operand delivery; not power-limited",
}


def build_neo360(dev):
    from neo360_amd import models, synth
    nv = 3
    state = synth.nerf_tp_state(0)
    net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(dev)
    net.load_state_dict(state)
    # stand-ins for the scene encoder's outputs, reference shapes: N(0, 0.1^2) from the hash generator -
    # the very scene the reference was run on for the fixture tests/golden/g4_neo_full.npz (tests/golden/cases.py:full_scene)
    if "neo360" not in _SCENE_CACHE:
        _SCENE_CACHE["neo360"] = synth.scene_features(0, nv, 128, (120, 160), 512, (240, 320), std=0.1)
    scene = {k: v.to(dev) for k, v in _SCENE_CACHE["neo360"].items()}
    scene["image_wh"] = (float(W), float(H))
    net.set_scene(scene["plane_xz"], scene["plane_xy"], scene["plane_yz"], scene["latent"], scene["image_wh"])
    poses, focal, centre = synth.source_views(nv, W, H)
    extra = dict(src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                 src_imgs=torch.zeros(nv, 3, H, W, device=dev))
    desc = ("neo360 tri-planar decoder 640x480 full frame, 3 source views, 128 coarse + 256 fine samples/ray, "
            "inside + outside sphere ((129+385)x2 = 1028 MLP points/ray x 3 views), reference chunk 1024, "
            "random-init MLPs, synthetic N(0,0.1) tri-planes (3x128x120x160) + latents (3x512x240x320) from the hash generator "
            "(= the scene of the reference-generated fixture g4_neo_full)")
    return net, state, extra, scene, desc, dict(near=0.0, far=0.0), "k_tp_mlp", CHUNK


def build_pixelnerf(dev):
    from neo360_amd import models, synth
    nv = 3
    state = synth.pixelnerf_state(0)
    net = models.PixelNeRF(num_coarse_samples=64, num_fine_samples=64, num_src_views=nv).to(dev)
    net.load_state_dict(state)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    scene = {"latent": torch.randn(nv, 512, 240, 320, device=dev, generator=g) * 0.1, "image_wh": (float(W), float(H))}
    net.set_scene(scene["latent"], scene["image_wh"])
    poses, focal, centre = synth.source_views(nv, W, H)
    extra = dict(src_poses=poses.to(dev), src_focal=focal.to(dev), src_c=centre.to(dev),
                 src_imgs=torch.zeros(nv, 3, H, W, device=dev))
    desc = ("PixelNeRF baseline decoder 640x480 full frame, 3 source views, 64 coarse + 64 fine samples/ray "
            "((65+129) MLP points/ray x 3 views), reference chunk 1024, random-init MLPs, synthetic N(0,0.1) "
            "latents (3x512x240x320)")
    return net, state, extra, scene, desc, dict(near=0.2, far=3.0), "k_pix_mlp", 512


def build_mip360(dev, n_nerf=32):
    from neo360_amd import models, synth
    state = synth.mip360_state(0, weight_gain=0.5)
    net = models.MipNeRF360(num_prop_samples=64, num_nerf_samples=n_nerf).to(dev)
    net.load_state_dict(state)
    desc = ("mipnerf360 640x480 full frame, 2 proposal levels x 64 samples (PropMLP 4x256) + %d NeRF samples "
            "(NeRFMLP 8x1024), cone casting + contraction + 504-d IPE, random-init MLPs (kaiming x0.5)" % n_nerf)
    return net, state, {}, None, desc, dict(near=0.2, far=3.0, train_frac=1.0), "k_mip_mlp", (2048 if n_nerf == 128 else 4096)


BUILDERS = {"vanilla": build_vanilla, "neo360": build_neo360, "pixelnerf": build_pixelnerf,
            "mip360": build_mip360, "mip360_128": lambda dev: build_mip360(dev, 128)}


def cpu_baseline(workload, state, scene, rays_cpu, extra, kw, n):
    """The oracle (CPU restatement of the reference: kind 'port'; oracle == reference is pinned by tests/golden,
    tests/test_oracle_fullsize.py and tests/test_oracle_vs_reference.py) timed up to CPU_REPS times on a bounded sample
    of the same frame on the host cores: for NeO-360 ONE WHOLE reference chunk (1024 rays: BASELINE.md 3),
    thread count from a NeO-360 sweep on the GPU box's host.  No further repetition is started once CPU_BUDGET_S would
    be exceeded, so the default run still finishes in minutes."""
    import oracle
    torch.set_num_threads(min(CPU_THREADS.get(workload, CPU_THREADS_DEFAULT), os.cpu_count() or 1))
    sample = {k: v[:n] for k, v in rays_cpu.items()}
    times = []
    for _ in range(CPU_REPS):
        t0 = time.perf_counter()
        if workload == "vanilla":
            rgb, depth = oracle.vanilla.render_chunked(state, sample, kw["near"], kw["far"], chunk=CHUNK)
        elif workload == "pixelnerf":
            batch = dict(sample)
            batch.update({k: v.cpu() for k, v in extra.items()})
            sc = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in scene.items()}
            rgb, depth = oracle.pixelnerf.render_chunked(state, batch, sc, kw["near"], kw["far"], chunk=CHUNK)
        elif workload.startswith("mip360"):
            from oracle import mip360
            rend, _ = mip360.render(state, sample, kw["train_frac"], kw["near"], kw["far"], num_prop_samples=64,
                                    num_nerf_samples=128 if workload.endswith("128") else 32)
            rgb, depth = rend[-1]["rgb"], torch.zeros(n)
        else:
            batch = dict(sample)
            batch.update({k: v.cpu() for k, v in extra.items()})
            sc = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in scene.items()}
            rgb, depth = oracle.neo360.render_chunked(state, batch, sc, chunk=min(n, CHUNK))
        times.append(time.perf_counter() - t0)
        if sum(times) + times[-1] > CPU_BUDGET_S:
            break
    dt = statistics.median(times)
    base = dict(value=n / dt, unit="rays/s", cores=physical_cores(), threads=torch.get_num_threads(), kind="port",
                threads_choice="best-of-sweep (fastest torch thread count of a sweep on this host type: profiles/r03_cpu_threads_neo360.log, "
                               "profiles/cpu_threads_r01.log; all 128 cores are 10x slower on the gather-bound NeO-360 oracle)",
                sample="first %d rays of the same 640x480 frame as %s, same weights / features, "
                       "torch fp32 CPU oracle (validated equal to the reference: tests/golden, tests/test_oracle_fullsize.py, "
                       "tests/test_oracle_vs_reference.py) on %d of the host's %d physical cores (%d logical); median of %d "
                       "repetition%s, %s s"
                       % (n, "ONE whole reference chunk" if n == CHUNK else ("%d reference chunks" % (n // CHUNK) if n > CHUNK else "one (short) reference chunk"),
                          torch.get_num_threads(), physical_cores(), os.cpu_count() or 1, len(times), "" if len(times) == 1 else "s",
                          "/".join("%.1f" % t for t in times)))
    return base, rgb, depth


def pmc_profile(workload, precision):
    """Summary of the committed rocprofv3 PMC passes of this same command (tools/pmc_bench.sh ->
    profiles/rNN_pmc_<workload>_<precision>.json; newest round wins): HBM bytes per dominant-kernel launch =
    (2 x FETCH_SIZE + WRITE_SIZE) KiB, mean over the launches of a frame (FETCH_SIZE doubled as
    MI355X_MICROARCH.md prescribes for gfx950), MFMA-busy fraction, effective clock.  The summary carries the hash of
    the kernel sources it was taken on (`kernel_source_sha16`, written by tools/pmc_summarize.py); when that is not the
    hash of THIS tree the counter fields are dropped (-> null in the bench line) instead of describing another kernel.
    {} when none is committed."""
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_%s_%s.json" % (workload, precision))))
    if not paths:
        return {}
    with open(paths[-1]) as f:
        full = json.load(f)
    src = os.path.relpath(paths[-1], ROOT)
    have, want = full.get("kernel_source_sha16"), kernel_source_hash(workload)
    if have != want:
        return {"source": src, "stale": "PMC summary %s was taken on kernel sources %s, this tree is %s: counter fields dropped"
                                        % (src, have or "(unstamped)", want)}
    d = full.get("derived", {})
    d["source"] = src
    d["kernel_match"] = full.get("kernel_match")
    return d


class Runner:
    """One workload on this rank: builds the renderer, generates only this rank's ray range, renders, gathers."""

    def __init__(self, workload, precision, dev, world, rank, dist, setup_timing=True):
        from neo360_amd import ops, render, synth
        from neo360_amd.parallel import shard_bounds
        self.ops, self.render, self.dist = ops, render, dist
        self.workload, self.world, self.rank, self.dev = workload, world, rank, dev
        (self.net, self.state, self.extra, self.scene, self.desc, self.kw, kernel, self.cpu_default) = BUILDERS[workload](dev)
        if precision == "auto":
            precision = getattr(self.net, "default_precision", "f32")
        self.precision = precision
        self.split = precision == "f16x3"
        self.net.precision = precision
        self.kernel_name = kernel + ("_h" if self.split else "")
        if workload == "neo360" and self.split and getattr(self.net, "preproject", False):
            self.kernel_name = "k_tp_mlp_hpp" if self.net.preproject == 2 and self.net.preproject is not True else "k_tp_mlp_hp"
        self.c2w = synth.look_at_origin(40.0)
        self.ray_grid = os.environ.get("NEO360_RAY_GRID", "1") != "0"      # frame API's pixel-grid hint (8 x 8 ray patches)
        self.R = H * W
        self.lo, self.hi = shard_bounds(self.R, world, rank, unit=CHUNK)
        self.ctx = self.net._context(dev)
        self._rays = None
        self.scene_setup = None
        if workload == "neo360" and setup_timing:
            self.scene_setup = self._time_scene_setup()

    def _time_scene_setup(self, reps=7):
        """Once-per-scene work that the per-frame numbers do not contain: channels-last re-layout of the feature maps
        (set_scene), weight upload + fragment packing, and the pre-projection of the latent through each of the four
        MLPs' first-layer weights (k_tp_preproject; the 131,072 MACs per point-view the evaluator no longer executes) and -
        pre-projection mode 3, the default - of the three tri-planes through the world columns for the two outside-sphere MLPs.
        Timed with HIP EVENTS on the launch stream, WARM (round 5; the first version differenced host clocks of the process's
        very first calls and so counted code-object loading: 41-46 ms on the builder's boxes, 7 ms in the driver's line, ~5 ms of
        kernels in rocprofv3): one un-timed pass loads every kernel, then `reps` times
            e0 | set_scene + new parameter tensors (-> repack all four MLPs) + a one-chunk render | e1 | the same render | e2
        and set-up = (e1 - e0) - (e2 - e1): the scene / weight epochs changed, so the first render re-runs the re-layout, the
        packing and all ten k_tp_preproject launches; the second is the steady state of the same chunk."""
        sc, net = self.scene, self.net
        tiny = self.shard_rays()
        tiny = {k: (v if k.startswith("src_") else v[:CHUNK]) for k, v in tiny.items()}

        def once(timed):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            ev[0].record()
            net.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], sc["image_wh"])
            ev_mid = torch.cuda.Event(enable_timing=True)
            ev_mid.record()
            net.load_state_dict({k: v.clone() for k, v in self.state.items()})     # fresh tensors: every slot is re-packed
            net(tiny, False, False, 0.0, 0.0, out_depth=True)
            ev[1].record()
            net(tiny, False, False, 0.0, 0.0, out_depth=True)
            ev[2].record()
            torch.cuda.synchronize()
            net.check_flags()
            first, steady = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
            return ev[0].elapsed_time(ev_mid), first, steady

        once(False)                                                                 # loads code objects, grows workspaces
        # The window holds ~150 enqueues and 72 small H2D copies: whatever delays the host thread (another tenant of the box, a
        # page fault) leaves the GPU idle INSIDE the window and can only ADD to it - one builder box gave 93, 95, 7.6, 7.7, 15, 174 ms
        # in one call.  The number of record is therefore the second smallest of the runs (the smallest alone could be a timing
        # glitch; an un-delayed run is reproducible to a few per cent); all runs are in the line.
        # A delay inside the STEADY window would subtract instead (one closing run of round 6 had a run of "0.0"): both windows are
        # picked separately - each can only be inflated - and then differenced.
        runs = [once(True) for _ in range(reps)]
        pick = lambda xs: sorted(xs)[1 if len(xs) > 1 else 0]
        steady = pick([r[2] for r in runs])
        runs = [(r[0], max(0.0, r[1] - steady), r[2]) for r in runs]
        total = pick([r[1] for r in runs])
        import statistics
        return {"total_ms": total, "median_ms": statistics.median(r[1] for r in runs), "runs_ms": [r[1] for r in runs],
                "set_scene_ms": pick([r[0] for r in runs]),
                "one_chunk_steady_ms": steady,
                "method": "HIP events on the launch stream, warm, second smallest of %d runs (host delays only add to the window): "
                          "(set_scene + repack + one-chunk render) - (the same render in the steady state)" % reps,
                "note": "once per scene / per weight update, not part of ms_per_step: channels-last re-layout of 3 tri-planes + latent, "
                        "weight upload + fragment packing, k_tp_preproject (exact fp32 MFMA) x 4 for the latent + x 6 for the tri-planes "
                        "of the two outside-sphere MLPs (pre-projection mode 3)"}

    def shard_rays(self):
        # only this rank's rays are generated, into the previous frame's tensors
        self._rays = self.ops.get_ray_directions_and_rays(H, W, 0.8 * W, self.c2w, ctx=self.ctx,
                                                          ray_range=(self.lo, self.hi), out=self._rays)
        ro, vd, rd, radii = self._rays
        batch = dict(rays_o=ro, viewdirs=vd, rays_d=rd)
        if self.workload.startswith("mip360"):
            batch["radii"] = radii[:, None]
        batch.update(self.extra)
        return batch

    def step(self):
        return self.render.render_frame_sharded(self.net, self.shard_rays(), self.world, self.rank, chunk=CHUNK,
                                                n_rays=self.R, always_gather=self.dist is not None,
                                                image_width=W if self.ray_grid else None, **self.kw)

    def fence(self):
        if self.dist is not None:
            self.dist.barrier()
        torch.cuda.synchronize()

    def timed(self, steps, warmup):
        for _ in range(warmup):
            self.step()
        self.fence()
        self.ctx.set_timing(True)
        # socket power / shader clock sampled from a thread of this process during the timed steps (neo360_amd.telemetry):
        # the split kernels run at the power limit, so the sustained clock belongs next to every throughput number
        from neo360_amd import telemetry
        with telemetry.Sampler(self.dev.index or 0) as tel:
            t0 = time.perf_counter()
            for _ in range(steps):
                frame = self.step()
            self.fence()
            dt = time.perf_counter() - t0
        self.telemetry = tel.summary()
        self.timed_steps = steps
        kern = self.ctx.read_timing()
        self.spans = self.ctx.read_spans()          # every evaluator launch of the timed steps: (ms, kernel, points, flops)
        self.ctx.set_timing(False)
        self.local_dt = dt
        if self.dist is not None:
            tmax = torch.tensor([dt], device=self.dev, dtype=torch.float64)
            self.dist.all_reduce(tmax, op=self.dist.ReduceOp.MAX)
            dt = float(tmax.item())
        return dt, kern, frame

    def chunk_loop(self, frames=2, overlap=True):
        """The same frame driven as the UNCHANGED reference drives the module (render_rays_test, neo360/model.py:861-907):
        300 `forward` calls of 1024 rays, per-ray keys sliced, src_* passed whole, level-1 rgb / depth appended and concatenated
        at the end, then ONE `check_flags()`.  overlap: consecutive calls alternate two side streams and two scratch lanes of
        the context (models.NeRF_TP.overlap_calls, the default); False = every call on the caller's stream (round 5)."""
        net, batch = self.net, self.shard_rays()
        prev = net.overlap_calls
        net.overlap_calls = overlap
        per_ray = ("rays_o", "rays_d", "viewdirs", "radii")
        kw = dict(white_bkgd=False, near=0.2, far=3.0, train_frac=1.0)
        kw.update(self.kw)

        def frame():
            rgb, depth = [], []
            for i in range(0, self.hi - self.lo, CHUNK):
                part = {k: (v[i:i + CHUNK] if k in per_ray else v) for k, v in batch.items()}
                res = self.render._render_once(net, part, CHUNK, kw["white_bkgd"], kw["near"], kw["far"], kw["train_frac"])
                rgb.append(res["rgb"])
                depth.append(res["depth"])
            out = torch.cat(rgb), torch.cat(depth)
            net.check_flags()
            return out
        try:
            frame()
            torch.cuda.synchronize()
            times = []
            for _ in range(frames):                      # frame by frame: the loop is host-paced, a delayed host thread shows as an outlier
                t0 = time.perf_counter()
                out = frame()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            dt = sorted(times)[len(times) // 2] if len(times) > 2 else sum(times) / len(times)
            self.loop_times_ms = [t * 1e3 for t in times]
        finally:
            net.overlap_calls = prev
        return dt, out

    def per_kernel(self):
        """The timed launches grouped by the evaluator that ran (a NeO-360 frame in pre-projection mode 3 = two launches of
        k_tp_mlp_hp, inside the sphere, + two of k_tp_mlp_hpp, outside): launches, mean duration, algorithmic and EXECUTED
        TFLOP/s of each.  Launch order inside a frame: inside coarse, outside coarse, inside fine, outside fine."""
        groups = {}
        for i, (ms, name, pts, fl) in enumerate(getattr(self, "spans", None) or []):
            if name == "unspecified":
                name = self.kernel_name
            g = groups.setdefault(name, dict(launches=0, ms=0.0, points=0.0, flops=0.0, executed=0.0))
            g["launches"] += 1
            g["ms"] += ms
            g["points"] += pts
            g["flops"] += fl
            if self.workload == "neo360" and name in ("k_tp_mlp_hp", "k_tp_mlp_hpp"):
                g["executed"] += pts * executed_flop_per_point_tp_hp(3, outside=bool(i & 1), planes_projected=name == "k_tp_mlp_hpp")
        out = {}
        for name, g in groups.items():
            sec = g["ms"] * 1e-3
            out[name] = {"launches": g["launches"], "avg_launch_ms": g["ms"] / g["launches"], "total_ms": g["ms"],
                         "points_per_launch": g["points"] / g["launches"],
                         "algorithmic_tflops": g["flops"] / sec / 1e12 if sec > 0 else 0.0,
                         "algorithmic_flop_per_launch": g["flops"] / g["launches"]}
            if g["executed"]:
                out[name]["executed_tflops"] = g["executed"] / sec / 1e12
                out[name]["executed_flop_per_launch"] = g["executed"] / g["launches"]
        return out

    def roofline(self, kern):
        kern_ms_all, launches_all, points_all, flops_all = kern
        per = self.per_kernel()
        # the DOMINANT kernel = the one the timed steps spent most time in; its own launches price the roofline
        dom = max(per, key=lambda k: per[k]["total_ms"]) if per else self.kernel_name
        if per:
            self.kernel_name = dom
            kern_ms, launches = per[dom]["total_ms"], per[dom]["launches"]
            points, flops = per[dom]["points_per_launch"] * launches, per[dom]["algorithmic_flop_per_launch"] * launches
        else:
            kern_ms, launches, points, flops = kern_ms_all, launches_all, points_all, flops_all
        achieved = flops / (kern_ms * 1e-3) / 1e12 if kern_ms > 0 else 0.0
        alg_bytes_per_point = 20.0 + {"neo360": 3 * 14336.0, "pixelnerf": 3 * 8192.0}.get(self.workload, 0.0)
        # the path computes on the matrix pipe of its dtype: fp16 MFMA (dense peak 2500) for the split arithmetic,
        # fp32 MFMA (157.3) for the exact kernels.  `frac` = ALGORITHMIC flops (reference formulation) / that peak.
        peak = PEAK_F16_MFMA_TFLOPS if self.split else PEAK_F32_MFMA_TFLOPS
        pmc = pmc_profile(self.workload, self.precision)
        if pmc.get("kernel_match") and dom != pmc["kernel_match"].rstrip("<") and self.workload == "neo360":
            pmc = {"source": pmc.get("source"), "stale": "PMC summary is of kernel %s, the dominant kernel of this run is %s" % (pmc["kernel_match"], dom)}
        avg_ms = kern_ms / max(launches, 1)
        traffic = pmc.get("hbm_bytes_per_launch")
        roof = {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                # `bound` names the roofline the kernel is PRICED against (the contract's enum: "hbm" | "mfma"; the arithmetic runs on
                # the matrix pipe, HBM is at a few per cent).  What actually limits the split evaluators is named here, from the
                # counters and the in-run telemetry: vector-ALU issue + the socket power limit, not the matrix pipe itself.
                "limiter": LIMITER.get(self.workload if self.split else "f32", None),
                "traffic": traffic, "kernel": self.kernel_name, "launches": launches, "avg_launch_ms": avg_ms,
                "algorithmic_flop_per_launch": flops / max(launches, 1), "points_per_launch": points / max(launches, 1),
                "algorithmic_bytes_per_launch": points / max(launches, 1) * alg_bytes_per_point,
                "algorithmic_bytes_definition": ("20 B per point of compulsory I/O" + (
                    " + the reference's NO-REUSE gather volume (3 views x 14,336 B of taps per point, SURVEY.md 8d upper bound): "
                    "this is not an HBM numerator - divided by the launch time it exceeds the HBM peak, because taps are shared in "
                    "L2 / Infinity Cache; every texel once would be 0.56 GB per frame; measured fabric-side bytes are `traffic`"
                    if self.workload in ("neo360", "pixelnerf") else "")),
                # HBM side of the roofline (north_star): PMC bytes of the profiled run / this run's launch time
                "hbm_frac": (traffic / (avg_ms * 1e-3) / PEAK_HBM_BYTES) if traffic and avg_ms > 0 else None,
                "mfma_busy": pmc.get("mfma_busy_frac"), "pmc_source": pmc.get("source"), "pmc_stale": pmc.get("stale"),
                "kernel_source_sha16": kernel_source_hash(self.workload),
                "all_evaluator_launches": {"launches": launches_all, "avg_launch_ms": kern_ms_all / max(launches_all, 1),
                                           "algorithmic_tflops": flops_all / (kern_ms_all * 1e-3) / 1e12 if kern_ms_all > 0 else 0.0},
                "kernels": per}
        tel = getattr(self, "telemetry", None) or {}
        roof.update({k: tel.get(k) for k in ("sclk_mhz_mean", "sclk_mhz_min", "power_w_mean", "power_w_max", "power_limit_w",
                                             "telemetry_samples", "telemetry", "energy_j", "energy_window_s", "power_w_from_energy")})
        if tel.get("energy_j") and getattr(self, "timed_steps", 0):
            # the socket's energy ACCUMULATOR over the timed steps (rsmi_dev_energy_count_get), not power samples x time: joules
            # per frame are what a power-limited part prices a kernel change in (profiles/r06_energy_budget.log)
            roof["energy_j_per_step"] = tel["energy_j"] / self.timed_steps
        if tel.get("sclk_mhz_mean"):
            # the peak is quoted at the 2.4 GHz boost clock; at the clock this run sustained the same pipe peaks lower
            roof["peak_at_measured_clock"] = peak * tel["sclk_mhz_mean"] / PEAK_CLOCK_MHZ
            roof["frac_at_measured_clock"] = achieved / roof["peak_at_measured_clock"]
        if self.split:
            # every algorithmic multiply costs three fp16 products: the ceiling for ALGORITHMIC flops on this arithmetic
            roof["frac_of_split_ceiling"] = achieved / (PEAK_F16_MFMA_TFLOPS / 3.0)
            roof["split_ceiling"] = PEAK_F16_MFMA_TFLOPS / 3.0
        if self.workload == "neo360" and self.split and per.get(dom, {}).get("executed_tflops"):
            # what the matrix pipe really executed in the dominant kernel's launches
            roof["executed_tflops"] = per[dom]["executed_tflops"]
            roof["frac_executed"] = roof["executed_tflops"] / PEAK_F16_MFMA_TFLOPS
            roof["executed_flop_per_point"] = per[dom]["executed_flop_per_launch"] / per[dom]["points_per_launch"]
        if self.workload == "neo360" and not self.split and getattr(self.net, "preproject", False):
            # the exact kernel on projected maps skips the projected stages' MACs: executed = algorithmic - skipped
            pl = self.net.preproject in (2, 3) and self.net.preproject is not True
            # per point: 3 views x (latent [+ planes] pre-projected; bottleneck 16,384 + view layer 0 9,920 moved out of the view loop
            # by linearity) MACs, minus the folded view layer run once per tile (160 x 64), x 2
            skipped = (3 * (131072 + (32768 if pl else 0) + 26304) - 10240) * 2.0
            ex = flops - points * skipped
            roof["executed_tflops"] = ex / (kern_ms * 1e-3) / 1e12 if kern_ms > 0 else 0.0
            roof["frac_executed"] = roof["executed_tflops"] / PEAK_F32_MFMA_TFLOPS
            roof["executed_flop_per_point"] = ex / points if points else 0.0
        roof["peak_definition"] = (
            "dense fp16 MFMA peak (MI355X_MICROARCH.md); frac = algorithmic (reference-formulation) flops / time / peak; "
            "frac_executed = fp16 MFMA flops the kernel really issues (3 products per multiply, padded k-steps, WITHOUT the "
            "latent GEMM that is pre-projected once per scene) / time / peak - the occupancy of the matrix pipe, comparable "
            "with mfma_busy; frac_of_split_ceiling = algorithmic flops / (peak / 3), the ceiling of this arithmetic; the "
            "exact-fp32-MFMA kernel is priced against 157.3 in the exact_f32 record" if self.split else
            "dense fp32 MFMA peak; frac = algorithmic (reference-formulation) flops / time / peak - above 1 is possible because the "
            "latent (and tri-plane) GEMM stages are pre-projected once per scene and not executed per point; frac_executed = the fp32 "
            "MFMA flops really issued / time / peak")
        roof["note"] = ("rank 0's launches, HIP events on the kernel's stream; algorithmic flops = reference formulation MACs x 2 "
                        "(SURVEY.md 8d) whatever the kernel executes; traffic / hbm_frac / mfma_busy from the committed PMC passes "
                        "(profiles/) when their kernel_source_sha16 matches this tree, else null; algorithmic bytes = 4 B t in + "
                        "16 B (rgb,sigma) out per point" +
                        (" + 3 views x 14,336 B of feature taps per point as the reference gathers them (no reuse; SURVEY.md 8d "
                         "upper bound; every texel once would be 560 MB per frame); k_tp_mlp_hp gathers the latent pre-projected "
                         "through the first-layer weights (8,192 -> 4,096 B per point-view, 131,072 of 255,424 MACs per "
                         "point-view not executed per point: they are in scene_setup_ms)" if self.workload == "neo360" else ""))
        return roof


def run_train(args, dev, emit=True):
    """`--workload neo360_train`: the reference's NeO-360 training step on this path (neo360/model.py:697-820: the module's
    randomized forward on a batch of rays, rgb L2 on both levels + 0.01 x eff_distloss on the fine inside / outside weights,
    backward, optimizer step on the four MLPs) at the reference's training batch - 500 rays (opt.py batch_size), 3 source views,
    128 + 256 samples, the bench scene at full map size with the four feature maps as leaves that receive gradients (the stand-in
    for the encoder's outputs).  value = rays/s through whole steps; `steps_per_s` beside it; the CPU leg is the oracle under
    torch autograd on a bounded sample of the same batch."""
    import statistics as st
    from neo360_amd import models, synth, training
    torch.set_grad_enabled(True)
    nv, B = 3, args.train_rays
    net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(dev)
    state = synth.nerf_tp_state(0)
    net.load_state_dict(state)
    sc = synth.scene_features(0, nv, 128, (120, 160), 512, (240, 320), std=0.1)
    maps = [sc[k].to(dev).requires_grad_(True) for k in ("plane_xz", "plane_xy", "plane_yz", "latent")]
    net.set_scene(*maps, (float(W), float(H)))
    from neo360_amd import ops
    ro, vd, rd, _ = ops.get_ray_directions_and_rays(H, W, 0.8 * W, synth.look_at_origin(40.0))
    sel = (torch.arange(B, device=dev) * 601 + 230 * W) % (H * W)
    poses, focal, centre = synth.source_views(nv, W, H)
    batch = dict(rays_o=ro[sel].contiguous(), rays_d=rd[sel].contiguous(), viewdirs=vd[sel].contiguous(), src_poses=poses.to(dev),
                 src_focal=focal.to(dev), src_c=centre.to(dev), src_imgs=torch.zeros(nv, 3, H, W, device=dev))
    target = synth.uniform(5, "train_target", (B, 3), 0.0, 1.0).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    interval = 1.0 / (128 + 1 + 256)

    def step(i):
        opt.zero_grad(set_to_none=True)
        for m in maps:
            m.grad = None
        lv = net(batch, True, False, 0.0, 0.0, out_depth=False, seed=1000 + i)
        loss = sum(((l[0] - target) ** 2).mean() for l in lv)
        loss = loss + 0.01 * (training.eff_distloss(lv[1][1], lv[1][3], interval) + training.eff_distloss(lv[1][2], lv[1][4], interval))
        loss.backward()
        opt.step()
        return loss, lv

    for i in range(args.warmup + 1):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss, lv = step(100 + i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    if emit and args.dump_outputs:
        # the last timed step's loss and per-level rgb, and the four MLPs as its optimizer step left them
        arrays = {"loss": loss.detach(), "rgb_coarse": lv[0][0], "rgb_fine": lv[1][0]}
        arrays.update({"param." + k: v for k, v in net.named_parameters()})
        dump_outputs(args.dump_outputs, arrays)
    phases = None
    if args.full:
        # phases of one step (events): forward, loss + backward, optimizer
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        opt.zero_grad(set_to_none=True)
        ev[0].record()
        lv = net(batch, True, False, 0.0, 0.0, out_depth=False, seed=7)
        ev[1].record()
        l2 = sum(((l[0] - target) ** 2).mean() for l in lv) + 0.01 * (training.eff_distloss(lv[1][1], lv[1][3], interval) + training.eff_distloss(lv[1][2], lv[1][4], interval))
        l2.backward()
        ev[2].record()
        opt.step()
        ev[3].record()
        torch.cuda.synchronize()
        phases = {"forward": ev[0].elapsed_time(ev[1]), "loss_and_backward": ev[1].elapsed_time(ev[2]), "optimizer": ev[2].elapsed_time(ev[3])}
    out = {"metric": "NeO-360 training step: rays/s through forward + loss + backward + optimizer step", "value": B / dt, "unit": "rays/s",
           "steps_per_s": 1.0 / dt, "ms_per_step": dt * 1e3, "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
           "dtype": "f32 (exact fp32 MFMA GEMMs of the training operators)", "data": "synthetic",
           "config": {"workload": "neo360 training step, %d rays, 3 source views, 128 + 256 samples inside + outside the sphere, randomized "
                                  "sampling, full-size feature maps (3x128x120x160 planes, 3x512x240x320 latent) receiving gradients, Adam on the four MLPs" % B,
                      "rays_per_step": B},
           "loss": float(loss.detach())}
    if phases is not None:
        out["phases_ms"] = phases
    # roofline of the step (round 6; VERDICT r5 task 6): the matrix work the training operators EXECUTE per step on the fp32 MFMA
    # pipe (the fused per-row chain kernels, k_sgemm forward / dX, k_dw weight gradients - the library's own GEMMs, texel-space projection included), counted from
    # the operator shapes: per point-view the NeRFPPMLP chain without the 512 latent columns (they are applied once per texel:
    # 4 MLPs x texels x 512 x 256), per point the heads; backward = dX + dW = 2 x forward
    # (round 6: the bottleneck and view layer 0 act on the view means - 26,304 MACs per point-view moved to 26,304 per point)
    pts = B * (129 + 385)
    fwd_mac = pts * nv * ((255424 - 131072 - 26304) + (260800 - 131072 - 26304)) + 2 * pts * (4416 + 26304)
    texels = nv * 240 * 320
    proj_mac = 4 * texels * 512 * 256
    executed = 2.0 * 3.0 * (fwd_mac + proj_mac)
    out["roofline"] = {"bound": "mfma", "achieved": executed / dt / 1e12, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                       "frac": executed / dt / 1e12 / PEAK_F32_MFMA_TFLOPS, "traffic": None,
                       "executed_flop_per_step": executed, "kernel": "k_tp_chain_fwd / _bwd + k_sgemm + k_dw (exact fp32 MFMA) over the whole step",
                       "note": "executed matrix flops of forward + dX + dW per step (operator shapes: %d points x %d views, texel-space "
                               "projection of %d texels for 4 MLPs) / the step's wall time - lookups, scatters, compositing, the "
                               "optimizer and launch gaps are inside that time, so this is the step's matrix-pipe occupancy, not a "
                               "single kernel's" % (2 * pts, nv, texels)}
    # HBM traffic of a step: tools/pmc_train_step.py's stamped summary (two counter-only rocprofv3 passes over this command), attached
    # only when it was taken on this tree's training kernels
    try:
        with open(os.path.join(ROOT, "profiles", "r06_pmc_train_step.json")) as f:
            pm = json.load(f)
        if pm.get("kernel_source_sha16") == kernel_source_hash("neo360_train"):
            out["roofline"]["traffic"] = pm["hbm_GB_per_step"] * 1e9
            out["roofline"]["traffic_note"] = "HBM bytes per step, all kernels (FETCH_SIZE x 2 + WRITE_SIZE, KiB), profiles/r06_pmc_train_step.json"
            out["roofline"]["hbm_frac"] = pm["hbm_GB_per_step"] * 1e9 / dt / PEAK_HBM_BYTES
    except (OSError, KeyError, ValueError):
        pass
    if args.cpu_rays != 0:
        import oracle
        from oracle import training as T
        torch.set_num_threads(min(CPU_THREADS["neo360"], os.cpu_count() or 1))

        def cpu_step(n):
            cb = {k: (v[:n].cpu() if k in ("rays_o", "rays_d", "viewdirs") else v.cpu()) for k, v in batch.items()}
            pp = {k: v.clone().requires_grad_(True) for k, v in state.items()}
            cm = {k: sc[k].clone().requires_grad_(True) for k in ("plane_xz", "plane_xy", "plane_yz", "latent")}
            cm["image_wh"] = (float(W), float(H))
            t0 = time.perf_counter()
            want = oracle.neo360.render(pp, cb, cm, n_coarse=128, n_fine=256, white_bkgd=False, out_depth=False)
            lc = sum(((l[0] - target[:n].cpu()) ** 2).mean() for l in want)
            lc = lc + 0.01 * (T.eff_distloss(want[1][1], want[1][3], interval) + T.eff_distloss(want[1][2], want[1][4], interval))
            lc.backward()
            return time.perf_counter() - t0
        # A CPU step has a cost that does not scale with the rays (dense autograd gradients of the full-size maps): two sample sizes,
        # three repetitions of the larger, a linear fit - the per-ray slope and the fixed part are reported separately and the step
        # at the GPU's batch size is EXTRAPOLATED from them (48 rays x 1 repetition against 500 was not like-for-like)
        n2 = min(B, args.cpu_rays if args.cpu_rays > 0 else 72)
        n1 = max(8, n2 // 3)
        t1 = cpu_step(n1)
        t2s = [cpu_step(n2) for _ in range(3)]
        t2 = sorted(t2s)[1]
        slope = max((t2 - t1) / max(n2 - n1, 1), 1e-9)
        fixed = max(t1 - slope * n1, 0.0)
        step_b = fixed + slope * B
        out["cpu_baseline"] = {"value": B / step_b, "unit": "rays/s", "cores": physical_cores(), "threads": torch.get_num_threads(), "kind": "port",
                               "per_ray_s": slope, "fixed_s_per_step": fixed, "step_s_extrapolated": step_b, "measured": {str(n1): [t1], str(n2): t2s},
                               "sample": "oracle forward (deterministic samples) + the same loss + torch autograd backward on the CPU at %d rays "
                                         "(once) and %d rays (3 repetitions, median); step time = fixed + slope x rays, EXTRAPOLATED to the "
                                         "GPU's %d rays - not a measured 500-ray CPU step" % (n1, n2, B)}
        out["speedup_vs_cpu"] = out["value"] / out["cpu_baseline"]["value"]
        out["speedup_note"] = "GPU step measured at %d rays (randomized sampling) vs the CPU step extrapolated to %d rays (deterministic samples): indicative, not like-for-like" % (B, B)
    if emit:
        print(json.dumps(out))
    return out


class FakeRunner:
    """CPU stand-in for Runner (tests/test_bench_cpu.py: `--fake`, gloo): the same sharding (whole 1024-ray chunks), the same
    barrier / max-over-ranks timing and the same tile all-gather as the GPU path, with a 'renderer' that writes each ray's index
    into its tile - so the launch plumbing of `bench.py --gpus N` (self-spawn, rank environment, rendezvous on 127.0.0.1, the
    assembled frame) is testable without a GPU.  Nothing here is measured."""

    def __init__(self, world, rank, dist):
        from neo360_amd.parallel import gather_tiles, shard_bounds
        self.world, self.rank, self.dist, self.R = world, rank, dist, H * W
        self.lo, self.hi = shard_bounds(self.R, world, rank, unit=CHUNK)
        self._gather = gather_tiles
        self.desc = "fake renderer (CPU plumbing test)"

    def step(self):
        idx = torch.arange(self.lo, self.hi, dtype=torch.float32)
        tile = torch.stack([idx, idx * 0.5, idx * 0.25, idx + 1.0, torch.full_like(idx, float(self.rank))], dim=1)
        return self._gather(tile, self.R, self.world, unit=CHUNK) if self.dist is not None else tile

    def timed(self, steps, warmup):
        for _ in range(warmup):
            self.step()
        if self.dist is not None:
            self.dist.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            frame = self.step()
        if self.dist is not None:
            self.dist.barrier()
        dt = time.perf_counter() - t0
        self.local_dt = dt
        if self.dist is not None:
            tmax = torch.tensor([dt], dtype=torch.float64)
            self.dist.all_reduce(tmax, op=self.dist.ReduceOp.MAX)
            dt = float(tmax.item())
        return dt, None, frame


def _parse_cpulist(text):
    cpus = set()
    for part in text.strip().split(","):
        if not part:
            continue
        a, _, b = part.partition("-")
        cpus.update(range(int(a), int(b or a) + 1))
    return cpus


def bind_to_gpu_numa_node(local_rank, fake=False):
    """One process per GPU: which NUMA node does this rank's GPU hang off - reported in the rank's record - and, only with
    $NEO360_NUMA_BIND=1, pin this rank's host threads to that node's CPUs.  The pinning is OFF by default because it was measured
    to hurt (round 6, tools/gpu_r06j.sh, one MI355X box with 128 of 256 logical CPUs on the GPU's node): frame throughput is
    unchanged (493.5 k vs 492.4 k rays/s) but the once-per-scene set-up window - ~150 enqueues and 72 small pageable
    host-to-device copies - goes from 7.4 ms to 406 ms (every small copy waits ~5 ms for a runtime helper thread that the
    affinity mask moved).  Best effort: returns what was found / done, never fails the run."""
    info = {"numa_node": None, "cpus_bound": None}
    try:
        if fake:
            bdf = os.environ.get("NEO360_FAKE_BDF")            # tests: any PCI device of the box, or nothing
        else:
            pr = torch.cuda.get_device_properties(local_rank)
            bdf = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
        info["pci"] = bdf
        if not bdf:
            return info
        with open("/sys/bus/pci/devices/%s/numa_node" % bdf) as f:
            node = int(f.read().strip())
        info["numa_node"] = node
        if node < 0 or os.environ.get("NEO360_NUMA_BIND", "0") != "1":
            return info
        with open("/sys/devices/system/node/node%d/cpulist" % node) as f:
            cpus = _parse_cpulist(f.read()) & os.sched_getaffinity(0)
        if cpus:
            os.sched_setaffinity(0, cpus)
            info["cpus_bound"] = len(cpus)
    except Exception as e:                                       # no sysfs entry, container without NUMA: say so
        info["numa_note"] = "%s: %s" % (type(e).__name__, e)
    return info


def rank_records(dist, world, rank, local_rank, dev, ms_local, numa):
    """What every rank saw, gathered to all: answers 'did the collective really span N ranks / N distinct GPUs' from the line."""
    if dev is not None:
        pr = torch.cuda.get_device_properties(dev)
        device = {"name": pr.name, "pci_bus_id": getattr(pr, "pci_bus_id", None), "torch_index": dev.index}
    else:
        device = {"name": "cpu (fake renderer)", "pci_bus_id": None, "torch_index": None}
    rec = {"rank": rank, "local_rank": local_rank, "pid": os.getpid(), "ms_per_step": ms_local,
           "world_size_seen": dist.get_world_size() if dist is not None else 1,
           "backend": dist.get_backend() if dist is not None else None, **device, **(numa or {})}
    if dist is None:
        return [rec]
    out = [None] * world
    dist.all_gather_object(out, rec)
    return out


def self_spawn(n, argv):
    """`python bench.py --gpus N` without a launcher (RANK unset): start the N ranks ourselves - one process per GPU, the very
    environment torch.distributed.run would give them (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR = 127.0.0.1 / a free
    MASTER_PORT) - and wait.  Rank 0's JSON line goes to our stdout.  A rank that dies takes the others down (exact PIDs)."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), NEO360_BENCH_SELF_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    alive = list(procs)
    while alive:
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in alive:          # a dead rank leaves the others waiting in a collective: stop them, by PID
                    q.terminate()
        time.sleep(0.05)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=tuple(BUILDERS) + ("neo360_train",), default="neo360")
    ap.add_argument("--train-rays", type=int, default=500, dest="train_rays", help="rays per step of --workload neo360_train (the reference's training batch)")
    ap.add_argument("--precision", choices=("auto", "f32", "f16x3"), default="auto",
                    help="MLP arithmetic: exact fp32 MFMA, or fp16 MFMA with hi/lo-split operands (fp32-equivalent, "
                         "the default of every renderer)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: CPU baseline, scene set-up, chunk loop and (N == 1) the exact fp32 "
                         "kernels, the other configurations and the training step")
    ap.add_argument("--dump-outputs", default=None, dest="dump_outputs", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy")
    ap.add_argument("--cpu-rays", type=int, default=-1, help="rays in the CPU-baseline sample (0 = skip, -1 = default: with --full)")
    ap.add_argument("--others", type=int, default=-1, help="1/0: also time one step of the other BASELINE configs (default: --full and N == 1)")
    ap.add_argument("--setup-timing", type=int, default=-1, dest="setup_timing",
                    help="1/0: the scene_setup_ms measurement (two extra one-chunk renders; counter passes want only the frame's launches; "
                         "default: with --full)")
    ap.add_argument("--exact-f32", type=int, default=-1, dest="exact_f32",
                    help="1/0: also time 2 frames of the same workload on the exact fp32-MFMA kernels (default: as --others)")
    ap.add_argument("--train-step", type=int, default=1, dest="train_step",
                    help="1/0: with the other workloads (N == 1), also time five steps of the NeO-360 training step (`training_step` record)")
    ap.add_argument("--chunk-loop", type=int, default=-1, dest="chunk_loop",
                    help="1/0: also time the frame as the reference's own chunk loop drives the module (300 forward calls; neo360, N = 1; "
                         "default: with --full)")
    ap.add_argument("--fake", action="store_true", help=argparse.SUPPRESS)     # CPU plumbing test: gloo + FakeRunner (tests/test_bench_cpu.py)
    args = ap.parse_args()
    # what only --full runs by default; an explicit 1 / count still turns a single part on
    if args.cpu_rays < 0 and not args.full:
        args.cpu_rays = 0
    if args.setup_timing < 0:
        args.setup_timing = int(args.full)
    if args.chunk_loop < 0:
        args.chunk_loop = int(args.full)

    # one process per GPU.  Under torch.distributed.run the ranks exist already (RANK set); a plain `python bench.py --gpus N`
    # with N > 1 starts them itself - the driver's N = 1 command line with another N must not die on an assertion
    if not args.fake and args.gpus > max(torch.cuda.device_count(), 0):
        sys.exit("bench.py: --gpus %d but this node shows %d GPU%s (torch.cuda.device_count()); nothing was launched"
                 % (args.gpus, torch.cuda.device_count(), "" if torch.cuda.device_count() == 1 else "s"))
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_spawn(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: WORLD_SIZE=%d but --gpus %d: launch one process per GPU (python -m torch.distributed.run "
                 "--nproc-per-node %d ... bench.py --gpus %d), or run `python bench.py --gpus %d` without a launcher"
                 % (world, args.gpus, args.gpus, args.gpus, args.gpus))
    if args.fake:
        dist = None
        if world > 1 or "RANK" in os.environ:
            import torch.distributed as dist
            dist.init_process_group("gloo")
        numa = bind_to_gpu_numa_node(local_rank, fake=True)
        run = FakeRunner(world, rank, dist)
        dt, _, frame = run.timed(args.steps, args.warmup)
        ranks = rank_records(dist, world, rank, local_rank, None, run.local_dt / args.steps * 1e3, numa)
        if rank == 0 and args.dump_outputs:
            dump_outputs(args.dump_outputs, frame_outputs(frame))
        if rank == 0:
            ok = bool(torch.equal(frame[:, 0], torch.arange(run.R, dtype=torch.float32))) if dist is not None else True
            print(json.dumps({"metric": "plumbing test (no measurement)", "fake": True, "n_gpus": world, "steps": args.steps,
                              "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "frame_rows": int(frame.shape[0]), "frame_in_order": ok,
                              "rank_column": sorted(set(frame[:, 4].tolist())) if dist is not None else [0.0],
                              "self_spawned": bool(os.environ.get("NEO360_BENCH_SELF_SPAWNED")), "value": run.R * args.steps / dt,
                              "ranks": ranks}))
        if dist is not None:
            dist.destroy_process_group()
        return
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    numa = bind_to_gpu_numa_node(local_rank)
    if args.workload == "neo360_train":
        if world != 1:
            sys.exit("bench.py: --workload neo360_train is a single-GPU line")
        run_train(args, dev)
        return
    torch.set_grad_enabled(False)
    dist = None
    # one process per GPU over RCCL; a launch under torch.distributed.run with ONE rank (RANK set, world 1) initialises the
    # process group as well, so the collective path of the N-GPU job (barrier, max-reduce, tile all-gather) also runs on a
    # one-GPU box (tools/gpu_r04*.sh keeps that line in profiles/); plain `python bench.py` stays collective-free
    if world > 1 or "RANK" in os.environ:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)

    from neo360_amd import render

    run = Runner(args.workload, args.precision, dev, world, rank, dist, setup_timing=bool(args.setup_timing))
    dt, kern, frame = run.timed(args.steps, args.warmup)
    R = run.R
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, frame_outputs(frame))
    ranks = rank_records(dist, world, rank, local_rank, dev, run.local_dt / args.steps * 1e3, numa)

    if rank == 0:
        out = {
            "metric": "rays/sec (128 samples/ray) + PSNR vs ref, 640x480",
            "value": R * args.steps / dt, "unit": "rays/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None,
            "dtype": "f32 (fp16-MFMA products of hi/lo-split fp32 operands, fp32 accumulate)" if run.split else "f32",
            "data": "synthetic",
            "config": {"workload": run.desc + (", rays sharded by whole 1024-ray chunks + one RCCL all-gather of "
                                               "(rgb,depth,acc) tiles" if world > 1 else ""),
                       "rays_per_frame": R, "parallelism": "ray-shard x%d" % world},
            "roofline": run.roofline(kern),
            # one record per rank, gathered over the process group: the world size each rank saw, its GPU (name, PCI bus), the NUMA
            # node it hangs off (host threads are pinned there only with $NEO360_NUMA_BIND=1: measured harmful, see
            # bind_to_gpu_numa_node) and its OWN time per step (`ms_per_step` above is the max over ranks)
            "ranks": ranks,
        }
        if args.workload == "neo360" and world == 1 and args.chunk_loop:
            # what a run.py user gets without touching the reference's chunk loop (VERDICT r5 task 4)
            dt_o, (rgb_o, depth_o) = run.chunk_loop(5, overlap=True)
            loop_ms = list(run.loop_times_ms)
            dt_s, (rgb_s, depth_s) = run.chunk_loop(2, overlap=False)
            out["chunk_loop"] = {
                "value": R / dt_o, "unit": "rays/s", "ms_per_frame": dt_o * 1e3, "frac_of_headline": (R / dt_o) / out["value"],
                "calls_per_frame": (R + CHUNK - 1) // CHUNK, "rays_per_call": CHUNK, "frames": 5, "frames_ms": loop_ms,
                "statistic": "median of 5 frames timed one by one (the loop is host-paced: 300 Python calls per frame)",
                "serial_calls": {"value": R / dt_s, "ms_per_frame": dt_s * 1e3, "frac_of_headline": (R / dt_s) / out["value"]},
                "bitwise_equal_to_whole_frame_call": bool(torch.equal(rgb_o, frame[:, :3]) and torch.equal(depth_o, frame[:, 3])
                                                          and torch.equal(rgb_s, rgb_o) and torch.equal(depth_s, depth_o)),
                "note": "the same frame as 300 model(chunk) calls of 1024 rays + torch.cat + one check_flags(), as the unchanged "
                        "reference loop issues them (neo360/model.py:861-907); `value`: consecutive calls overlap on two side streams / "
                        "two scratch lanes of the context (the default, models.NeRF_TP.overlap_calls); serial_calls: every call on "
                        "the caller's stream"}
        if run.scene_setup:
            out["scene_setup_ms"] = run.scene_setup["total_ms"]
            out["scene_setup"] = run.scene_setup
        n_cpu = run.cpu_default if args.cpu_rays < 0 else args.cpu_rays
        if world == 1 and n_cpu > 0:
            batch = run.shard_rays()
            n = min(n_cpu, R)
            rays_cpu = {k: batch[k][:n].cpu() for k in ("rays_o", "viewdirs", "rays_d", "radii") if k in batch}
            base, rgb_c, depth_c = cpu_baseline(args.workload, run.state, run.scene, rays_cpu, run.extra, run.kw, n)
            if args.workload == "neo360" and n != CHUNK:
                # NeO-360 results depend on chunk membership: render the same rays as their own chunk
                sub = {k: (v[:n] if k in ("rays_o", "viewdirs", "rays_d") else v) for k, v in batch.items()}
                got = render.render_rays_test(run.net, sub, chunk=n, **run.kw)
                rgb_g, depth_g = got["rgb"].cpu(), got["depth"].cpu()
            else:
                rgb_g, depth_g = frame[:n, :3].cpu(), frame[:n, 3].cpu()
            err = (rgb_g - rgb_c).abs().amax(dim=-1)
            out["cpu_baseline"] = base
            out["parity_vs_cpu"] = {"max_abs_rgb": float(err.max()), "p99_abs_rgb": float(err.quantile(0.99)),
                                    "max_abs_depth": float((depth_g - depth_c).abs().max()),
                                    "psnr_db": render.psnr(rgb_g, rgb_c), "rays": n}
            out["speedup_vs_cpu"] = out["value"] / base["value"]
        others = (world == 1 and args.full) if args.others < 0 else bool(args.others)
        exact = others if args.exact_f32 < 0 else bool(args.exact_f32)
        if exact and world == 1 and run.split:
            # the same workload on the EXACT fp32-MFMA kernels (module.precision = "f32"), 1 warm-up + 2 timed frames:
            # the number priced against the contract's own ceiling (fp32 matrix peak 157.3)
            wl, kw_run = args.workload, run
            run.net.close()
            del run, frame
            torch.cuda.empty_cache()
            r32 = Runner(wl, "f32", dev, 1, 0, None)
            dt32, kern32, f32_ = r32.timed(2, 1)
            roof32 = r32.roofline(kern32)
            out["exact_f32"] = {"value": R * 2 / dt32, "unit": "rays/s", "ms_per_step": dt32 / 2 * 1e3, "steps": 2, "warmup": 1,
                                "dtype": "f32 (v_mfma_f32_32x32x2_f32)", "kernel": roof32["kernel"],
                                "achieved": roof32["achieved"], "peak": roof32["peak"], "unit_roofline": "TFLOP/s",
                                # the roofline FRACTION of this record is the executed one; algorithmic flops / peak exceeds 1 because
                                # the projected stages' MACs are done once per scene (or once per point on the view mean), not per point-view
                                "frac": roof32.get("frac_executed", roof32["frac"]),
                                "algorithmic_over_peak": roof32["frac"], "frac_executed": roof32.get("frac_executed"),
                                "executed_tflops": roof32.get("executed_tflops"),
                                "avg_launch_ms": roof32["avg_launch_ms"], "launches": roof32["launches"],
                                "note": "same algorithm as the headline (projected maps gathered and added), exact fp32 MFMA arithmetic"}
            r32.net.close()
            del r32, f32_
            torch.cuda.empty_cache()
            run = frame = None
        if others and world == 1:
            # the other BASELINE.json single-GPU configurations, 1 warm-up + 2 timed frames each, same code path
            if run is not None:
                run.net.close()
            del run, frame
            torch.cuda.empty_cache()
            out["other_workloads"] = {}
            for wl in ("vanilla", "mip360", "mip360_128"):
                if wl == args.workload:
                    continue
                r2 = Runner(wl, "auto", dev, 1, 0, None)
                dt2, kern2, f2 = r2.timed(2, 1)
                roof = r2.roofline(kern2)
                loop = None
                if args.chunk_loop:
                    dl_o, (lrgb, _) = r2.chunk_loop(1, overlap=True)
                    dl_s, _ = r2.chunk_loop(1, overlap=False)
                    loop = {"value": R / dl_o, "frac_of_frame_call": (R / dl_o) / (R * 2 / dt2), "serial_calls": R / dl_s,
                            "bitwise_equal_to_whole_frame_call": bool(torch.equal(lrgb, f2[:, :3]))}
                out["other_workloads"][wl] = {"value": R * 2 / dt2, "unit": "rays/s", "ms_per_step": dt2 / 2 * 1e3, "steps": 2,
                                              "chunk_loop": loop,
                                              "kernel": roof["kernel"], "achieved_tflops": roof["achieved"],
                                              "roofline_frac": roof["frac"], "peak": roof["peak"],
                                              "frac_of_split_ceiling": roof.get("frac_of_split_ceiling"), "workload": r2.desc}
                r2.net.close()
                del r2, f2
                torch.cuda.empty_cache()
            # the training step of the same model on this path, so that the driver's record carries it too: five
            # 500-ray steps of --workload neo360_train, no CPU leg (bench.py --workload neo360_train is the full line)
            if args.workload == "neo360" and args.train_step:
                import copy
                ta = copy.copy(args)
                ta.steps, ta.warmup, ta.cpu_rays = 5, 2, 0
                try:
                    tr = run_train(ta, dev, emit=False)
                    out["training_step"] = {"ms_per_step": tr["ms_per_step"], "value": tr["value"], "unit": tr["unit"], "steps": 5,
                                            "rays_per_step": tr["config"]["rays_per_step"], "phases_ms": tr.get("phases_ms"),
                                            "matrix_pipe_frac_of_157.3": tr["roofline"]["frac"], "dtype": tr["dtype"],
                                            "workload": tr["config"]["workload"]}
                finally:
                    torch.set_grad_enabled(False)
                torch.cuda.empty_cache()
        out["config"]["launch"] = ("self-spawned ranks (python bench.py --gpus N)" if os.environ.get("NEO360_BENCH_SELF_SPAWNED")
                                   else "torch.distributed.run" if "RANK" in os.environ else "single process")
        if dist is not None:
            out["config"]["collective"] = "RCCL process group of %d rank%s (barrier, max-reduce of the step time, all_gather_into_tensor of the tiles)" % (world, "" if world == 1 else "s")
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
