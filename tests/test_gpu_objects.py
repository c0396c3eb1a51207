"""GPU: object-level rendering of NeRF_TP (`NeRF_TP.render_objects`, neo_tp_render_objects): the two foreground MLPs marched
between a caller-given per-ray interval [near_obj, far_obj], on the rays that have one.

What is checked (scene, boxes and the CPU oracle: tests/object_cases.py, pinned by tests/test_objects_cpu.py):

* parity against the CPU oracle on EVERY hit ray at the project's tolerance (1e-4, no exempt rays), on all five evaluator
  configurations; level 0 directly (its positions are deterministic), level 1 with the oracle evaluated at the GPU's own
  level-1 positions (the project's way of keeping the resampler's discontinuity out of a comparison);
* the compact launches are bitwise the shipped non-compact ones (rebuilt from public stage operators on all rays);
* a hit ray's result does not depend on which other rays hit, nor on whether the caller loops over chunks;
* the edges of the hit rule, the background colour, R == 0; repeatability and overlap neutrality; nothing else changes.
"""
import pytest
import torch

import cases
import object_cases as oc
from conftest import record_parity
from neo360_amd import models, ops, render

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
PER_RAY = ("rays_o", "rays_d", "viewdirs", "near_obj", "far_obj")
OUT = ("rgb", "acc", "depth")


def _net(precision=None, preproject=3, n_coarse=16, n_fine=32):
    net = models.NeRF_TP(num_coarse_samples=n_coarse, num_fine_samples=n_fine, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(oc.state())
    sc = cases.small_scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV),
                  sc["image_wh"], preproject=preproject)
    if precision is not None:
        net.precision = precision
    return net


def _gpu(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _call(net, b, **kw):
    out = net.render_objects(b, return_samples=True, **kw)
    net.check_flags()
    return [[t.clone() for t in lv] for lv in out]


def _ulp(x):
    a = x.abs()
    return torch.nextafter(a, torch.full_like(a, float("inf"))) - a


def _assert_misses(res, miss, white):
    for lv in range(2):
        rgb, acc, depth = res[lv]
        assert bool((rgb[miss] == (1.0 if white else 0.0)).all()), lv
        assert bool((acc[miss] == 0.0).all()) and bool((depth[miss] == 0.0).all()), lv
        assert bool((res[2][lv][miss] == 0.0).all()), lv


def _assert_parity(tag, res, b_cpu, near, far, n_coarse, n_fine, white=True, chunk=None):
    """Every hit ray of both levels against the CPU oracle, level 1 at the GPU's own positions; also the sample rows."""
    t0, t1 = res[2][0].cpu(), res[2][1].cpu()
    want = oc.oracle_render(oc.state(), b_cpu, near, far, n_coarse, n_fine, white_bkgd=white, chunk=chunk, t1=t1)
    hit = want["hit"]
    lo, hi, _ = oc.hit_rule(near.reshape(-1).float(), far.reshape(-1).float())
    assert t0.shape == (hit.shape[0], n_coarse + 1) and t1.shape == (hit.shape[0], n_coarse + 1 + n_fine)
    # level-0 rows: lo (1 - s) + hi s to one ulp; level-1 rows ascending inside [lo, hi]
    assert bool(((t0[hit] - want["t0"][hit]).abs() <= _ulp(want["t0"][hit])).all())
    assert bool((t1[hit][:, 1:] >= t1[hit][:, :-1]).all())
    assert bool((t1[hit] >= lo[hit, None]).all()) and bool((t1[hit] <= hi[hit, None]).all())
    worst = {}
    for lv in range(2):
        for k, got in zip(OUT, res[lv]):
            e = (got.cpu().double() - want["%s%d" % (k, lv)].double()).abs()[hit]
            e = e.reshape(e.shape[0], -1).amax(dim=1)
            worst["%s%d" % (k, lv)] = (float(e.max()), int((e >= TOL).sum()))
    print(tag, {k: "%.2e" % v[0] for k, v in worst.items()})
    record_parity("neo360_objects/" + tag, rays=int(hit.sum()), **{"max_" + k: v[0] for k, v in worst.items()},
                  rays_above_1e4=sum(v[1] for v in worst.values()))
    for k, (mx, n) in worst.items():
        assert n == 0 and mx < TOL, (tag, k, mx, n)
    return hit


# precision x pre-projection mode -> the kernel the two FOREGROUND slots run on
EVALUATORS = [("f16x3", 3, "k_tp_mlp_hp"), ("f16x3", 2, "k_tp_mlp_hpp"), ("f16x3", False, "k_tp_mlp_h"),
              ("f32", 3, "k_tp_mlp"), ("f32", False, "k_tp_mlp")]


@pytest.mark.parametrize("precision,preproject,kernel", EVALUATORS, ids=["%s-pre%d-%s" % (p, int(m), k) for p, m, k in EVALUATORS])
def test_every_hit_ray_matches_the_oracle(precision, preproject, kernel):
    net = _net(precision, preproject)
    b_cpu, mask = oc.batch(96)
    assert int(mask.sum()) == 35 and (35 * 17) % 64 != 0 and (35 * 49) % 64 != 0      # the compact launches end in a partial tile
    gb = _gpu(b_cpu)
    ctx = net._context(torch.device(DEV))
    ctx.set_timing(True)
    try:
        res = _call(net, gb)
        torch.cuda.synchronize()
        launched = [name for _, name, _, _ in ctx.read_spans()]
    finally:
        ctx.set_timing(False)
    # coarse and fine, both COMPACT, on the kernel this case is here for
    assert launched == [kernel, kernel], launched
    assert net.last_object_hits.dtype == torch.int32 and net.last_object_hits.is_cuda and int(net.last_object_hits) == 35
    hit = _assert_parity("%s_pre%d" % (precision, int(preproject)), res, b_cpu, b_cpu["near_obj"], b_cpu["far_obj"], 16, 32)
    assert torch.equal(hit, mask)
    _assert_misses(res, ~mask.to(DEV), True)
    plain = net.render_objects(gb)           # without the sample rows: two levels, the same values
    assert len(plain) == 2 and all(torch.equal(x, y) for lv in range(2) for x, y in zip(plain[lv], res[lv]))


def test_compact_launches_are_bitwise_the_non_compact_evaluators():
    """128 + 256 samples, default mode: every hit ray rebuilt on ALL 96 rays from the public stage operators - the exposed t0 ->
    eval_mlp (slot 0, the shipped k_tp_mlp_hp<3>) -> ops.composite(mode 1, t_far = far_obj) -> ops.resample, then slot 1 ->
    composite.  Missed rays are marched through a dummy interval there and ignored."""
    net = _net(n_coarse=128, n_fine=256)
    b_cpu, mask = oc.batch(96)
    gb = _gpu(b_cpu)
    res = _call(net, gb)
    hit = mask.to(DEV)
    far = torch.where(hit, gb["far_obj"].reshape(-1), torch.full((96,), 0.5, device=DEV))
    dummy = torch.linspace(0.1, 0.5, 129, device=DEV).expand(96, -1)
    t0 = torch.where(hit[:, None], res[2][0], dummy).contiguous()
    c0 = ops.composite(1, net.eval_mlp(0, gb, t0), t0, gb["rays_d"], t_far=far, white_bkgd=True)
    t1 = ops.resample(t0, c0["weights"], 256)
    assert torch.equal(t1[hit], res[2][1][hit])
    c1 = ops.composite(1, net.eval_mlp(1, gb, t1), t1, gb["rays_d"], t_far=far, white_bkgd=True)
    for lv, c in enumerate((c0, c1)):
        for k, got in zip(OUT, res[lv]):
            assert torch.equal(got[hit], c[k][hit]), (lv, k)
    _assert_misses(res, ~hit, True)


def test_a_hit_ray_does_not_depend_on_the_other_rays():
    """300 rays at chunk 128: two whole reference chunks and a short one (quirk Q1 gives a ray a direction that depends on its
    chunk), hits in both 256-ray compaction workgroups."""
    net = _net()
    b_cpu, mask = oc.batch(300)
    gb = _gpu(b_cpu)
    hit = mask.to(DEV)
    full = _call(net, gb, chunk=128)
    assert int(net.last_object_hits) == 114 == int(mask.sum())
    # every second hit ray loses its interval: the remaining hits are bitwise what they were
    drop = torch.zeros_like(hit)
    drop[hit.nonzero().reshape(-1)[::2]] = True
    thin = dict(gb, near_obj=torch.where(drop[:, None], 0.0, gb["near_obj"]), far_obj=torch.where(drop[:, None], 0.0, gb["far_obj"]))
    got = _call(net, thin, chunk=128)
    assert int(net.last_object_hits) == 57
    keep = hit & ~drop
    for lv in range(2):
        for k, x, y in zip(OUT, got[lv], full[lv]):
            assert torch.equal(x[keep], y[keep]), (lv, k)
        assert torch.equal(got[2][lv][keep], full[2][lv][keep])
    _assert_misses(got, ~keep, True)
    # the reference-style loop: three calls of <= 128 rays, each one reference chunk
    parts, hits = [], 0
    for i in range(0, 300, 128):
        part = {k: (v[i:i + 128] if k in PER_RAY else v) for k, v in gb.items()}
        parts.append(net.render_objects(part, return_samples=True))
        hits += int(net.last_object_hits)
    net.check_flags()
    assert hits == 114
    for lv in range(2):
        for j, k in enumerate(OUT):
            assert torch.equal(torch.cat([p[lv][j] for p in parts]), full[lv][j]), (lv, k)
        assert torch.equal(torch.cat([p[2][lv] for p in parts]), full[2][lv])
    frame = render.render_object_rays(net, dict(gb, target=gb["rays_o"]), chunk=128)
    assert torch.equal(frame["rgb"], full[1][0]) and torch.equal(frame["acc"], full[1][1]) and torch.equal(frame["depth"], full[1][2])
    assert frame["target"] is gb["rays_o"] and int(net.last_object_hits) == 114


def test_no_hits_all_hits_and_empty_calls():
    net = _net()
    b_cpu, _ = oc.batch(96)
    gb = _gpu(b_cpu)
    zero = torch.zeros(96, 1, device=DEV)
    for white in (True, False):
        res = _call(net, gb, near_obj=zero, far_obj=zero, white_bkgd=white)
        assert int(net.last_object_hits) == 0
        _assert_misses(res, torch.ones(96, dtype=torch.bool, device=DEV), white)
    assert net._context(torch.device(DEV)).poll_flags() == 0, "the flags word must be clean after a call without hits"
    # every ray between 0.3 and 0.9, bounds given as (B,) arguments in another float dtype
    near, far = torch.full((96,), 0.3, dtype=torch.float64), torch.full((96,), 0.9, dtype=torch.float64)
    res = _call(net, gb, near_obj=near.to(DEV), far_obj=far.to(DEV))
    assert int(net.last_object_hits) == 96
    hit = _assert_parity("all_hits", res, b_cpu, near, far, 16, 32)
    assert bool(hit.all())
    # R == 0
    none = {k: (v[:0] if k in PER_RAY else v) for k, v in gb.items()}
    res = net.render_objects(none, return_samples=True)
    net.check_flags()
    assert int(net.last_object_hits) == 0
    assert [tuple(t.shape) for t in res[0]] == [(0, 3), (0,), (0,)] == [tuple(t.shape) for t in res[1]]
    assert tuple(res[2][0].shape) == (0, 17) and tuple(res[2][1].shape) == (0, 49)


def test_hit_rule_edges_and_background_colour():
    net = _net()
    b_cpu, mask = oc.batch(96)
    gb = _gpu(b_cpu)
    base = _call(net, gb)
    near, far = b_cpu["near_obj"].clone(), b_cpu["far_obj"].clone()
    assert not bool(mask[[0, 5, 17]].any())
    e1, e2, e3, e4 = [i for i in (~mask).nonzero().reshape(-1).tolist() if i not in (0, 5, 17)][:4]       # four more rays without a box
    nan, inf = float("nan"), float("inf")
    near[0], far[0] = nan, 0.9            # NaN near: miss
    near[5], far[5] = 0.6, 0.6            # far <= near: miss
    near[17], far[17] = -0.2, 0.6         # negative near (origin inside a box): hit from 1e-4
    near[e1], far[e1] = 0.3, nan          # NaN far: miss
    near[e2], far[e2] = inf, inf          # infinite bounds: miss
    near[e3], far[e3] = 0.3, inf
    near[e4], far[e4] = 0.7, 0.4          # far < near: miss
    lo, hi, want_hit = oc.hit_rule(near.reshape(-1), far.reshape(-1))
    assert bool(want_hit[17]) and not bool(want_hit[[0, 5, e1, e2, e3, e4]].any()) and int(want_hit.sum()) == 36
    res = _call(net, gb, near_obj=near.to(DEV), far_obj=far.to(DEV))
    assert int(net.last_object_hits) == 36
    _assert_misses(res, ~want_hit.to(DEV), True)
    t0 = res[2][0][17].cpu()
    assert float(t0[0]) == float(torch.tensor(1e-4)) and float(t0[-1]) == float(torch.tensor(0.6)) and bool((t0[1:] > t0[:-1]).all())
    assert 0.0 < float(res[1][1][17]) <= 1.0 and bool(torch.isfinite(res[1][0][17]).all())
    old = mask.to(DEV)
    for lv in range(2):                   # the box hits are untouched by their new neighbours
        for x, y in zip(res[lv], base[lv]):
            assert torch.equal(x[old], y[old])
    _assert_parity("edges", res, b_cpu, near, far, 16, 32)
    # white_bkgd: rgb gains exactly 1 - acc on a hit; a miss is 1 / 0
    black = _call(net, gb, white_bkgd=False)
    hit = mask.to(DEV)
    for lv in range(2):
        (rw, aw, dw), (rb, ab, db) = base[lv], black[lv]
        assert torch.equal(aw, ab) and torch.equal(dw, db) and torch.equal(base[2][lv], black[2][lv])
        want = rb[hit] + (1.0 - ab[hit])[:, None]
        assert bool(((rw[hit] - want).abs() <= _ulp(want)).all()), lv
    _assert_misses(black, ~hit, False)
    _assert_misses(base, ~hit, True)


def test_object_calls_are_repeatable_and_overlap_neutral():
    net = _net()
    gb = _gpu(oc.batch(96)[0])
    a = _call(net, gb)
    b = _call(net, gb)
    assert net.overlap_calls
    net.overlap_calls = False
    c = _call(net, gb)
    net.overlap_calls = True
    for other in (b, c):
        for lv in range(3):
            for x, y in zip(a[lv], other[lv]):
                assert torch.equal(x, y), lv
    # several calls in flight on alternating lanes: each compacts its own rays in its own lane's workspaces
    try:
        outs, counts = [], []
        for i in range(4):
            part = {k: (v[24 * i:] if k in PER_RAY else v) for k, v in gb.items()}
            outs.append(net.render_objects(part, return_samples=True))
            counts.append(net.last_object_hits)
        net.check_flags()
        net.overlap_calls = False
        for i in range(4):
            part = {k: (v[24 * i:] if k in PER_RAY else v) for k, v in gb.items()}
            want = net.render_objects(part, return_samples=True)
            assert int(net.last_object_hits) == int(counts[i])
            for lv in range(3):
                for x, y in zip(outs[i][lv], want[lv]):
                    assert torch.equal(x, y), (i, lv)
        net.check_flags()
    finally:
        net.overlap_calls = True


def test_scope_nothing_else_changes():
    """forward (both out_depth modes) and the culled call return what they returned before an object call on the same module;
    the object call itself has no unit-sphere assertion."""
    net = _net(n_coarse=32, n_fine=64)
    gb = _gpu(oc.batch(96)[0])

    def others():
        out = [net(gb, False, False, 0.0, 0.0, out_depth=True), net(gb, False, False, 0.0, 0.0, out_depth=False)]
        net.cull_background = 1e-2
        try:
            out.append(net(gb, False, False, 0.0, 0.0, out_depth=True))
        finally:
            net.cull_background = None
        net.check_flags()
        return [[t.clone() for t in lv] for o in out for lv in o]
    before = others()
    net.cull_background = 1e-2            # read by forward only
    net.ray_grid = (64, 0)
    try:
        hinted = _call(net, gb)
    finally:
        net.cull_background = None
        net.ray_grid = None
    plain = _call(net, gb)
    for lv in range(3):
        for x, y in zip(hinted[lv], plain[lv]):
            assert torch.equal(x, y)
    after = others()
    for x, y in zip(before, after):
        assert len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y))
    # a ray that misses the unit sphere: forward asserts, the object call does not
    bad = dict(gb)
    bad["rays_o"] = gb["rays_o"].clone()
    bad["rays_o"][3] = torch.tensor([0.0, 0.0, 5.0], device=DEV)
    bad["rays_d"] = gb["rays_d"].clone()
    bad["rays_d"][3] = torch.tensor([1.0, 0.0, 0.0], device=DEV)
    bad["near_obj"] = torch.full((96, 1), 0.3, device=DEV)
    bad["far_obj"] = torch.full((96, 1), 0.9, device=DEV)
    res = _call(net, bad)                 # check_flags inside: nothing to raise
    assert int(net.last_object_hits) == 96 and bool(torch.isfinite(res[1][0]).all())
    assert net._context(torch.device(DEV)).poll_flags() == 0
