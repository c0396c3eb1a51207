"""GPU: every instance of a scene in one call (`NeRF_TP.render_instances`, neo_tp_render_instances) and the per-box intervals it
takes (`ops.sample_rays_in_bbox_list`, neo_aabb_per_box).

The oracle of the per-instance rows is existing code: one `render_objects` call per instance, which the one call must reproduce
BITWISE.  The composite is compared with its torch fp32 restatement (instance_cases.composite) on the call's own per-instance
outputs.  Scene, boxes and the pinned figures the assertions below rely on: tests/instance_cases.py, tests/test_instances_cpu.py.
Everything runs at 16 + 32 samples on 96 or 300 rays.
"""
import pytest
import torch

import cases
import instance_cases as ic
import object_cases as oc
from neo360_amd import models, ops, render
from test_gpu_objects import EVALUATORS

pytestmark = pytest.mark.gpu
DEV = "cuda"
PER_RAY = ("rays_o", "rays_d", "viewdirs")
K7 = len(ic.INSTANCES)


def _net(precision=None, preproject=3):
    net = models.NeRF_TP(num_coarse_samples=ic.N_COARSE, num_fine_samples=ic.N_FINE, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(oc.state())
    sc = cases.small_scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV),
                  sc["image_wh"], preproject=preproject)
    if precision is not None:
        net.precision = precision
    return net


def _scene(n, instances=ic.INSTANCES):
    """GPU rays and the oracle's per-instance bounds (K,n) on the GPU, with the CPU hit mask."""
    gb = {k: v.to(DEV) for k, v in ic.rays(n).items()}
    near, far, hit = ic.bounds(n, instances)
    return gb, near.to(DEV), far.to(DEV), hit


def _call(net, gb, near, far, **kw):
    out = net.render_instances(gb, near, far, **kw)
    net.check_flags()
    inst = None if out["instances"] is None else [[t.clone() for t in lv] for lv in out["instances"]]
    return dict(instances=inst, composite=[[t.clone() for t in lv] for lv in out["composite"]])


def _objects(net, gb, near, far, **kw):
    out = net.render_objects(gb, near_obj=near, far_obj=far, **kw)
    net.check_flags()
    return [[t.clone() for t in lv] for lv in out]


def _flat(res):
    return [t for part in (res["instances"] or [], res["composite"]) for lv in part for t in lv]


def _assert_same(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb)
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert torch.equal(x, y), i


def test_per_box_intervals_are_the_oracles_single_box_calls():
    gb = {k: v.to(DEV) for k, v in ic.rays(300).items()}
    want_near, want_far, want_hit = ic.bounds(300, ic.DISTINCT)
    RTs = oc.rts(*ic.DISTINCT)
    near, far, hit = ops.sample_rays_in_bbox_list(RTs, gb["rays_o"], gb["viewdirs"])
    assert tuple(near.shape) == tuple(far.shape) == (5, 300, 1) and tuple(hit.shape) == (5, 300)
    assert near.dtype == far.dtype == torch.float32 and hit.dtype == torch.bool
    assert torch.equal(near[..., 0].cpu(), want_near) and torch.equal(far[..., 0].cpu(), want_far)
    assert torch.equal(hit.cpu(), want_hit) and hit.sum(dim=1).tolist() == [84, 30, 38, 74, 0]
    per_box = ops.sample_rays_in_bbox(RTs, gb["rays_o"], gb["viewdirs"], return_per_box=True)[3]
    assert torch.equal(hit, per_box.bool())
    assert bool((near[~hit] == 0).all()) and bool((far[~hit] == 0).all())
    # any float dtype of the rays, as sample_rays_in_bbox
    again = ops.sample_rays_in_bbox_list(RTs, gb["rays_o"].double(), gb["viewdirs"].double())
    assert all(torch.equal(x, y) for x, y in zip(again, (near, far, hit)))
    none = ops.sample_rays_in_bbox_list(dict(R=[], T=[], s=[]), gb["rays_o"], gb["viewdirs"])
    assert tuple(none[0].shape) == tuple(none[1].shape) == (0, 300, 1) and tuple(none[2].shape) == (0, 300) and none[2].dtype == torch.bool


@pytest.mark.parametrize("precision,preproject,kernel", EVALUATORS, ids=["%s-pre%d-%s" % (p, int(m), k) for p, m, k in EVALUATORS])
def test_instance_rows_are_bitwise_render_objects(precision, preproject, kernel):
    net = _net(precision, preproject)
    for n, chunk, pairs in ((96, None, 115), (300, 128, 384)):
        gb, near, far, hit = _scene(n)
        for white in (True, False):
            got = _call(net, gb, near, far, white_bkgd=white, chunk=chunk)
            count = net.last_instance_pairs
            assert count.dtype == torch.int32 and count.is_cuda and count.dim() == 0 and int(count) == pairs == int(hit.sum())
            want = {}
            for i, box in enumerate(ic.INSTANCES):
                if id(box) not in want:       # the duplicates are the same call
                    want[id(box)] = _objects(net, gb, near[i], far[i], white_bkgd=white, chunk=chunk)
                    assert int(net.last_object_hits) == int(hit[i].sum())
                for lv in range(2):
                    for k, x, y in zip(("rgb", "acc", "depth"), got["instances"][lv], want[id(box)][lv]):
                        assert x.shape[0] == K7 and torch.equal(x[i], y), (n, white, i, lv, k)
            miss = ~hit.to(DEV)
            for lv in range(2):
                rgb, acc, depth = got["instances"][lv]
                assert bool((rgb[miss] == (1.0 if white else 0.0)).all()) and bool((acc[miss] == 0).all()) and bool((depth[miss] == 0).all())
            # (K,B,1) bounds in another float dtype, and without the per-instance outputs: the same composite
            lean = _call(net, gb, near[:, :, None].double(), far[:, :, None].double(), white_bkgd=white, chunk=chunk, per_instance=False)
            assert lean["instances"] is None
            for lv in range(2):
                assert all(torch.equal(x, y) for x, y in zip(lean["composite"][lv], got["composite"][lv]))


_BASE = {}


def _base(n=96, chunk=None):
    """One module and its white / black results on the seven-instance scene, shared by the tests below (never modified)."""
    key = (n, chunk)
    if key not in _BASE:
        net = _net()
        gb, near, far, hit = _scene(n)
        _BASE[key] = dict(net=net, gb=gb, near=near, far=far, hit=hit,
                          white=_call(net, gb, near, far, white_bkgd=True, chunk=chunk),
                          black=_call(net, gb, near, far, white_bkgd=False, chunk=chunk))
    return _BASE[key]


@pytest.mark.parametrize("n,chunk", [(96, None), (300, 128)])
def test_composite_matches_its_fp32_restatement(n, chunk):
    base = _base(n, chunk)
    near, far, black, white = base["near"], base["far"], base["black"], base["white"]
    K = near.shape[0]
    for lv in range(2):
        p, a, d = black["instances"][lv]
        rgb, acc, depth, ids, order, valid = ic.composite(near, far, p, a, d, white=False)
        g_rgb, g_acc, g_depth, g_ids = black["composite"][lv]
        assert g_ids.dtype == torch.int32 and torch.equal(g_ids, ids), lv
        e_rgb, e_acc, e_depth = float((g_rgb - rgb).abs().max()), float((g_acc - acc).abs().max()), float((g_depth - depth).abs().max())
        print("n %d level %d: |rgb| %.2e |acc| %.2e |depth| %.2e (bounds %.2e, %.2e)" % (n, lv, e_rgb, e_acc, e_depth, K * 2.0 ** -23, K * 2.0 ** -22))
        # at most 2K roundings of values at most 1.001 (rgb, acc); d_i <= far < 2.1 (depth)
        assert e_rgb <= K * 2.0 ** -23 and e_acc <= K * 2.0 ** -23 and e_depth <= K * 2.0 ** -22, lv
        w_rgb, w_acc, w_depth, w_ids = white["composite"][lv]
        assert torch.equal(w_acc, g_acc) and torch.equal(w_depth, g_depth) and torch.equal(w_ids, g_ids)
        assert float((w_rgb - (g_rgb + (1.0 - g_acc)[:, None])).abs().max()) <= 2.0 ** -23, lv
        none = g_ids < 0
        assert torch.equal(none.cpu(), ~base["hit"].any(dim=0))
        assert bool((w_rgb[none] == 1.0).all()) and bool((g_rgb[none] == 0.0).all()) and bool((g_acc[none] == 0).all()) and bool((g_depth[none] == 0).all())
        seen = set(g_ids[~none].tolist())
        assert len(seen) >= 3 and not (seen & {4, 5, 6}), seen      # the empty instance and the later copies never win
        nearest = torch.where(valid[0], order[0].to(torch.int32), torch.full_like(ids, -1))
        assert int((g_ids != nearest).sum()) >= 1, "a map that ignores transmittance would pass"
    if n == 96:       # the oracle's own id map (tests/test_instances_cpu.py): gaps of 3.8e-3 between visibilities, compared exactly
        hist = {int(k): int(v) for k, v in zip(*torch.unique(black["composite"][1][3].cpu(), return_counts=True))}
        assert hist == {-1: 54, 0: 21, 1: 10, 2: 2, 3: 9}, hist


def test_permuting_the_instances_permutes_rows_and_ids():
    base = _base()
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]
    perm = [3, 5, 0, 6, 2, 4, 1]          # new position j holds old instance perm[j]: G A' A G' F D B
    got = _call(net, gb, near[perm], far[perm])
    assert int(net.last_instance_pairs) == 115
    want = base["white"]
    for lv in range(2):
        for x, y in zip(got["instances"][lv], want["instances"][lv]):
            assert torch.equal(x, y[perm]), lv
        for x, y in zip(got["composite"][lv][:3], want["composite"][lv][:3]):
            assert torch.equal(x, y), lv          # ties are exact duplicates: the same values in the same order
        # an old winner's box now wins at the lowest position holding a copy of it
        box_of = [ic.index_of(b) for b in ic.INSTANCES]
        new_pos = {-1: -1}
        for old in range(K7):
            new_pos[old] = min(j for j in range(K7) if box_of[perm[j]] == box_of[old])
        lut = torch.tensor([new_pos[i] for i in range(-1, K7)], dtype=torch.int32, device=DEV)
        assert torch.equal(got["composite"][lv][3], lut[(want["composite"][lv][3] + 1).long()]), lv


def test_dropping_the_empty_instance_changes_nothing_else():
    base = _base()
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]
    keep = [0, 1, 2, 3, 5, 6]
    got = _call(net, gb, near[keep], far[keep])
    assert int(net.last_instance_pairs) == 115
    want = base["white"]
    for lv in range(2):
        for x, y in zip(got["instances"][lv], want["instances"][lv]):
            assert torch.equal(x, y[keep]), lv
        for x, y in zip(got["composite"][lv][:3], want["composite"][lv][:3]):
            assert torch.equal(x, y), lv
        ids = want["composite"][lv][3]
        assert torch.equal(got["composite"][lv][3], torch.where(ids > 4, ids - 1, ids)), lv


def test_edges_no_instances_no_rays_no_hits_and_bad_bounds():
    base = _base()
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]
    for white in (True, False):
        # K = 0
        res = _call(net, gb, near[:0], far[:0], white_bkgd=white)
        assert int(net.last_instance_pairs) == 0
        for lv in range(2):
            assert [tuple(t.shape) for t in res["instances"][lv]] == [(0, 96, 3), (0, 96), (0, 96)]
            rgb, acc, depth, ids = res["composite"][lv]
            assert bool((rgb == (1.0 if white else 0.0)).all()) and bool((acc == 0).all()) and bool((depth == 0).all()) and bool((ids == -1).all())
        # every instance misses
        zero = torch.zeros(3, 96, device=DEV)
        res = _call(net, gb, zero, zero, white_bkgd=white)
        assert int(net.last_instance_pairs) == 0
        for lv in range(2):
            rgb, acc, depth = res["instances"][lv]
            assert bool((rgb == (1.0 if white else 0.0)).all()) and bool((acc == 0).all()) and bool((depth == 0).all())
            rgb, acc, depth, ids = res["composite"][lv]
            assert bool((rgb == (1.0 if white else 0.0)).all()) and bool((acc == 0).all()) and bool((depth == 0).all()) and bool((ids == -1).all())
    assert net._context(torch.device(DEV)).poll_flags() == 0, "the flags word must be clean after calls without hits"
    # B = 0
    none = {k: (v[:0] if k in PER_RAY else v) for k, v in gb.items()}
    res = _call(net, none, near[:, :0], far[:, :0])
    assert int(net.last_instance_pairs) == 0
    for lv in range(2):
        assert [tuple(t.shape) for t in res["instances"][lv]] == [(K7, 0, 3), (K7, 0), (K7, 0)]
        assert [tuple(t.shape) for t in res["composite"][lv]] == [(0, 3), (0,), (0,), (0,)]
    # NaN, inf and reversed bounds are misses; a negative near is a hit from 1e-4 - all as in render_objects
    nan, inf = float("nan"), float("inf")
    n2, f2 = near[[0, 3]].clone(), far[[0, 3]].clone()
    hit_a = base["hit"][0].nonzero().reshape(-1).tolist()
    miss_a = (~base["hit"][0]).nonzero().reshape(-1).tolist()
    n2[0, hit_a[0]] = nan
    f2[0, hit_a[1]] = nan
    f2[0, hit_a[2]] = inf
    n2[0, hit_a[3]], f2[0, hit_a[3]] = far[0, hit_a[3]], near[0, hit_a[3]]       # reversed
    n2[0, hit_a[4]] = f2[0, hit_a[4]]                                           # empty
    n2[0, miss_a[0]], f2[0, miss_a[0]] = inf, inf
    n2[0, miss_a[1]], f2[0, miss_a[1]] = -0.2, 0.6                              # origin inside a box
    lo, hi, want_hit = oc.hit_rule(n2.cpu(), f2.cpu())
    assert not bool(want_hit[0, hit_a[:5] + miss_a[:1]].any()) and bool(want_hit[0, miss_a[1]])
    assert int(want_hit[0].sum()) == 25 - 5 + 1
    res = _call(net, gb, n2, f2)
    assert int(net.last_instance_pairs) == int(want_hit.sum())
    for i in range(2):
        want = _objects(net, gb, n2[i], f2[i])
        for lv in range(2):
            for x, y in zip(res["instances"][lv], want[lv]):
                assert torch.equal(x[i], y), (i, lv)
    m = ~want_hit.to(DEV)
    for lv in range(2):
        rgb, acc, depth = res["instances"][lv]
        assert bool((rgb[m] == 1.0).all()) and bool((acc[m] == 0).all()) and bool((depth[m] == 0).all())
        assert bool(torch.isfinite(res["composite"][lv][0]).all())
    # K = 1: the composite IS the instance; id = 0 exactly where it is visible
    for white in (True, False):
        res = _call(net, gb, near[3:4], far[3:4], white_bkgd=white)
        assert int(net.last_instance_pairs) == 22
        for lv in range(2):
            rgb, acc, depth = res["instances"][lv]
            c_rgb, c_acc, c_depth, ids = res["composite"][lv]
            assert torch.equal(c_rgb, rgb[0]) and torch.equal(c_acc, acc[0]) and torch.equal(c_depth, depth[0])
            assert torch.equal(ids == 0, acc[0] > 0) and torch.equal(ids == -1, ~(acc[0] > 0))
            assert int((ids == 0).sum()) == 22


def test_instance_calls_are_repeatable_chunk_and_overlap_neutral():
    base = _base()
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]
    _assert_same(_call(net, gb, near, far), base["white"])
    assert net.overlap_calls
    net.overlap_calls = False
    try:
        _assert_same(_call(net, gb, near, far), base["white"])
    finally:
        net.overlap_calls = True
    # the reference-style loop: three calls of 32 rays, each one reference chunk, several in flight on alternating lanes
    whole = _call(net, gb, near, far, chunk=32)
    parts, pairs = [], 0
    for i in range(0, 96, 32):
        part = {k: (v[i:i + 32] if k in PER_RAY else v) for k, v in gb.items()}
        parts.append(net.render_instances(part, near[:, i:i + 32], far[:, i:i + 32], chunk=32))
        pairs += int(net.last_instance_pairs)
    net.check_flags()
    assert pairs == 115
    for lv in range(2):
        for j in range(3):
            assert torch.equal(torch.cat([p["instances"][lv][j] for p in parts], dim=1), whole["instances"][lv][j]), (lv, j)
        for j in range(4):
            assert torch.equal(torch.cat([p["composite"][lv][j] for p in parts]), whole["composite"][lv][j]), (lv, j)
    frame = render.render_instance_rays(net, dict(gb, near_inst=near, far_inst=far, target=gb["rays_o"]), chunk=32)
    rgb, acc, depth, ids = whole["composite"][1]
    assert torch.equal(frame["rgb"], rgb) and torch.equal(frame["acc"], acc) and torch.equal(frame["depth"], depth)
    assert torch.equal(frame["instance_id"], ids) and frame["target"] is gb["rays_o"]
    assert all(torch.equal(x, y) for x, y in zip(frame["instances"], whole["instances"][1]))
    # intervals computed from the boxes by the new op: the same frame
    from_boxes = render.render_instance_rays(net, gb, RTs=oc.rts(*ic.INSTANCES), chunk=32)
    assert torch.equal(from_boxes["rgb"], rgb) and torch.equal(from_boxes["instance_id"], ids)


def test_scope_nothing_else_changes():
    """A forward(out_depth=True) and a render_objects issued before and after an instance call are bitwise unchanged; the
    instance call reads neither cull_background nor ray_grid."""
    base = _base()
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]

    def others():
        out = [net(gb, False, False, 0.0, 0.0, out_depth=True), net.render_objects(gb, near_obj=near[0], far_obj=far[0])]
        net.check_flags()
        return [[t.clone() for t in lv] for o in out for lv in o]
    before = others()
    net.cull_background = 1e-2
    net.ray_grid = (32, 0)
    try:
        hinted = _call(net, gb, near, far)
    finally:
        net.cull_background = None
        net.ray_grid = None
    _assert_same(hinted, base["white"])
    after = others()
    for x, y in zip(before, after):
        assert len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y))
