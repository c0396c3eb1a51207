"""GPU: the decomposed render (`NeRF_TP.render_decomposed`, neo_tp_render_decomposed), its kernel on caller rows
(`ops.decompose_rows`) and the frame helper (`render.render_decomposed_rays`).

Scene, boxes, restatements and the pinned content of the fixture: tests/decompose_cases.py, tests/test_decompose_cpu.py.  Whole
renders run at 16 + 32 samples on 96 rays in one chunk or 300 rays in chunks of 128 (a short last chunk).

Bounds.  A slot output is a sum of fp32 products added in a tree whose depth is known: per lane one add per 64-sample round, then
the six steps of the wave butterfly.  Against the same sum in fp64 from the same fp32 rows that is one rounding per product plus
ceil(N/64) + 6 roundings of partial sums, each at most 2^-24 of S_s = sum over the slot of w |x|: (ceil(N/64) + 7) 2^-24 S_s.
Derived, not measured; no case is left out.  The sum over slots against the whole ray's composite has that bound twice, with
S over the whole ray (both sides carry it; the slots' own sum is formed in fp64)."""
import math

import pytest
import torch

import cases
import decompose_cases as dc
import edit_cases as ec
import instance_cases as ic
import object_cases as oc
from neo360_amd import _lib, models, ops, render
from test_gpu_objects import EVALUATORS

pytestmark = pytest.mark.gpu
DEV = "cuda"
PER_RAY = ("rays_o", "rays_d", "viewdirs")
K7 = dc.K7
NAMES = ("rgb", "fg_rgb", "bg_rgb", "fg_acc", "bg_lambda", "depth")
SLOT_KEYS = ("rgb", "acc", "depth")
SHAPES = ((96, None), (300, 128))
# pinned from the run (fine level, 96 rays): the id histogram and the rays whose id differs from render_instances' id.  The fixture's
# density bias of +6 makes the scene a fog that is opaque within its first samples: every instance stands behind it, so the frame's
# id map names nobody, while render_instances - which knows nothing of the scene around the instances - names one on all 42 rays
# that hit a box (21 A, 10 B, 2 F, 9 G).  A positive id in the frame is checked with a box around the camera, below.
ID_HISTOGRAM_96 = {-1: 96}
ID_DIFFERS_FROM_INSTANCES_96 = 42


def _net(precision=None, preproject=3):
    net = models.NeRF_TP(num_coarse_samples=ec.N_COARSE, num_fine_samples=ec.N_FINE, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(ec.state())
    sc = ec.scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV),
                  sc["image_wh"], preproject=preproject)
    if precision is not None:
        net.precision = precision
    return net


def _scene(n):
    gb = {k: v.to(DEV) for k, v in ic.rays(n).items()}
    near, far, hit = ic.bounds(n)
    return gb, near.to(DEV), far.to(DEV), hit


def _forward(net, gb, chunk):
    out = net(gb, False, False, 0.0, 0.0, out_depth=True, chunk=chunk)
    net.check_flags()
    return [[t.clone() for t in lv] for lv in out]


def _copy(x):
    return {k: v.clone() for k, v in x.items()} if isinstance(x, dict) else x.clone()


def _decomposed(net, gb, near, far, **kw):
    out = net.render_decomposed(gb, near, far, **kw)
    net.check_flags()
    res = [[_copy(t) for t in lv] for lv in out[:2]]
    if len(out) > 2:      # return_samples: per level (fg_t, fg_w, bg_s)
        res.append([[t.clone() for t in lv] for lv in out[2]])
    return res


_BASE = {}


def _base(n=96, chunk=None):
    """One default module, its frame and its decomposed frame (both levels, with samples) on the seven-instance scene."""
    key = (n, chunk)
    if key not in _BASE:
        net = _net()
        gb, near, far, hit = _scene(n)
        _BASE[key] = dict(net=net, gb=gb, near=near, far=far, hit=hit, forward=_forward(net, gb, chunk),
                          dec=_decomposed(net, gb, near, far, chunk=chunk, levels=(0, 1), return_samples=True))
    return _BASE[key]


def _flat(res):
    out = []
    for lv in res[:2]:
        for t in lv:
            out += list(t.values()) if isinstance(t, dict) else [t]
    for lv in (res[2] if len(res) > 2 else []):
        out += list(lv)
    return out


# ---- 1. the kernel on caller rows against the restatement ----------------------------------------------------------------------

def _rows_case(R, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.sort(torch.rand(R, N, generator=g) * 1.8 + 0.01, dim=-1).values
    rs = torch.rand(R, N, 4, generator=g) * torch.tensor([1.0, 1.0, 1.0, 30.0]) - torch.tensor([0.001, 0.001, 0.001, 0.0])
    w = torch.rand(R, N, generator=g) * (2.0 / N)
    w[:, ::7] = 0.0                                                    # weights of exactly 0, as behind an opaque sample
    near = torch.rand(K, R, generator=g) * 1.2
    far = near + torch.rand(K, R, generator=g) * 0.8 - 0.1             # some hi <= lo
    nan, inf = float("nan"), float("inf")
    for i in range(K):
        for r in range(R):
            kind = (i * 7 + r * 3 + seed) % 11
            if kind == 0:
                near[i, r] = far[i, r] = 0.0                           # the reference's "no hit" sentinel
            elif kind == 1:
                near[i, r] = nan
            elif kind == 2:
                far[i, r] = nan
            elif kind == 3:
                far[i, r] = inf
            elif kind == 4:
                near[i, r] = -inf
            elif kind == 5:
                near[i, r] = -0.3                                      # origin inside the box: lo = 1e-4
            elif kind == 6:                                            # a sample exactly on lo and one exactly on hi
                a, b = sorted(((i + r) % N, (i * 5 + r + N // 2) % N))
                near[i, r], far[i, r] = t[r, a], (t[r, b] if b > a else t[r, a] + 0.25)
            elif kind == 7:
                near[i, r], far[i, r] = far[i, r].clone(), near[i, r].clone()
    lam = torch.rand(R, generator=g) * 0.6
    return rs, t, w, near, far, lam


def _check_slots(got, want, N, where, S=None, factor=1.0):
    eps = (math.ceil(N / 64) + 7) * 2.0 ** -24 * factor
    worst = 0.0
    for k in SLOT_KEYS:
        scale = want["S_" + k] if S is None else S[k]
        err = (got[k].cpu().double() - want[k]).abs()
        print("%s %s: largest |err| %.3e, largest allowed %.3e" % (where, k, float(err.max()) if err.numel() else 0.0,
                                                                   float((eps * scale).max()) if err.numel() else 0.0))
        assert bool((err <= eps * scale).all()), (where, k, float((err - eps * scale).max()))
        worst = max(worst, float(err.max()) if err.numel() else 0.0)
    return worst


# 200: four rounds, the one register layout of the kernel the issue's sizes do not reach
@pytest.mark.parametrize("N", [5, 64, 65, 200, 385, 1024])
def test_decompose_rows_match_the_restatement(N):
    seen_edge = shared = named = flipped = 0
    for K in (0, 1, 3, 32):
        for R in (1, 4, 5, 96):
            rs, t, w, near, far, lam = _rows_case(R, N, K, N + K + R)
            want = dc.decompose_f64(rs, t, w, near, far)
            g = [x.to(DEV) for x in (rs, t, w, near, far, lam)]
            got = ops.decompose_rows(*g[:5])
            assert [tuple(got[k].shape) for k in ("rgb", "acc", "depth", "id")] == [(K + 1, R, 3), (K + 1, R), (K + 1, R), (R,)]
            assert got["id"].dtype == torch.int32 and all(got[k].dtype == torch.float32 for k in SLOT_KEYS)
            # ownership: exactly zero where the restatement owns nothing
            empty = (want["count"] == 0).to(DEV)
            for k in SLOT_KEYS:
                assert bool((got[k][empty] == 0).all()), (N, K, R, k)
            _check_slots(got, want, N, "N %d K %d R %d" % (N, K, R))
            # the id map is the fp32 rule on the GPU's own masses, without and with bg_lambda
            assert torch.equal(got["id"], dc.id_rule(got["acc"])), (N, K, R)
            with_lam = ops.decompose_rows(*g)
            assert torch.equal(with_lam["id"], dc.id_rule(with_lam["acc"], g[5])), (N, K, R)
            assert all(torch.equal(with_lam[k], got[k]) for k in SLOT_KEYS)
            named += int((got["id"] >= 0).sum())
            flipped += int((with_lam["id"] != got["id"]).sum())
            # (K,R,1) bounds and an (R,1) lambda in another float dtype are the same call
            again = ops.decompose_rows(g[0], g[1], g[2], g[3][:, :, None].double(), g[4][:, :, None].double(), g[5][:, None].double())
            assert all(torch.equal(again[k], with_lam[k]) for k in ("rgb", "acc", "depth", "id"))
            if K:
                inside = ec.inside_mask(t, near, far)
                lo, hi, _ = oc.hit_rule(near, far)
                own = want["own"]
                on_end = inside & ((t[None] == lo[:, :, None]) | (t[None] == hi[:, :, None]))
                seen_edge += int((on_end & (own[None] == torch.arange(K)[:, None, None])).sum())
                shared += int((inside.sum(dim=0) >= 2).sum())
    assert seen_edge >= 2, "owned samples exactly on lo / hi must occur"
    assert shared >= 1, "samples inside more than one interval must occur"
    assert named >= 1 and flipped >= 1, "rays with an id, and rays whose id bg_lambda takes away, must occur"


# ---- 2. bitwise relations on caller rows ------------------------------------------------------------------------------------------

def _composite_rows(R, N, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.sort(torch.rand(R, N, generator=g) * 1.6 + 0.05, dim=-1).values
    d = torch.randn(R, 3, generator=g)
    far = t[:, -1:] + 0.05 + torch.rand(R, 1, generator=g) * 0.2
    rs = torch.rand(R, N, 4, generator=g)
    rs[..., 3] *= torch.rand(R, 1, generator=g) * 60.0 / N            # thin and opaque rays
    return [x.to(DEV) for x in (rs, t, d, far)]


@pytest.mark.parametrize("N", [5, 64, 65, 200, 385, 1024])
def test_a_slot_that_owns_the_ray_is_bitwise_composite(N):
    R = 37
    rs, t, d, far = _composite_rows(R, N, N)
    comp = ops.composite(1, rs, t, d, far)
    w = comp["weights"]
    none = torch.zeros(0, R, device=DEV)
    got = ops.decompose_rows(rs, t, w, none, none, comp["bg_lambda"])
    for k in SLOT_KEYS:
        assert tuple(got[k].shape)[:2] == (1, R) and torch.equal(got[k][0], comp[k]), (N, k)
    assert bool((got["id"] == -1).all())
    # one instance whose interval covers [1e-4, far]; then the same behind a miss and in front of a copy of itself
    cover_n, cover_f = torch.full((1, R), -1.0, device=DEV), far.reshape(1, R) + 1.0
    miss = torch.full((1, R), float("nan"), device=DEV)
    for near, hi, owner in ((cover_n, cover_f, 0), (torch.cat([miss, cover_n, cover_n]), torch.cat([miss, cover_f, cover_f]), 1)):
        got = ops.decompose_rows(rs, t, w, near, hi)
        for k in SLOT_KEYS:
            assert torch.equal(got[k][owner], comp[k]), (N, k, owner)
            others = [s for s in range(near.shape[0] + 1) if s != owner]
            assert bool((got[k][others] == 0).all()), (N, k, owner)
        assert torch.equal(got["id"], torch.where(comp["acc"] > 0, owner, -1).to(torch.int32))
        # with everything outside the sphere added to the (empty) rest the instance still needs the larger share
        lam_id = ops.decompose_rows(rs, t, w, near, hi, comp["bg_lambda"])["id"]
        assert torch.equal(lam_id, torch.where((comp["acc"] > 0) & (comp["acc"] >= comp["bg_lambda"][:, 0]), owner, -1).to(torch.int32))


# ---- 3. the frame render --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,preproject,kernel", EVALUATORS, ids=["%s-pre%d-%s" % (p, int(m), k) for p, m, k in EVALUATORS])
def test_decomposed_frame_is_bitwise_forward(precision, preproject, kernel):
    net = _net(precision, preproject)
    for n, chunk in SHAPES:
        gb, near, far, _ = _scene(n)
        want = _forward(net, gb, chunk)
        for levels, bounds in (((1,), (near, far)), ((0, 1), (near, far)), ((), (near[:0], far[:0])), ((0,), (near[:0], far[:0]))):
            got = _decomposed(net, gb, *bounds, chunk=chunk, levels=levels)
            assert len(got) == 2
            for lv in range(2):
                assert len(got[lv]) == 6 + (lv in levels)
                for k, x, y in zip(NAMES, got[lv], want[lv]):
                    assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (n, lv, k, levels)


@pytest.mark.parametrize("n,chunk", SHAPES)
def test_decomposed_dict_is_the_kernel_on_the_rows_of_the_stage_chain(n, chunk):
    base = _base(n, chunk)
    net, gb, near, far, dec = base["net"], base["gb"], base["near"], base["far"], base["dec"]
    o, d = gb["rays_o"], gb["rays_d"]
    t_far, _ = ops.intersect_sphere(o, d)
    pos = net.sample_positions(gb, chunk)
    net.check_flags()
    for lv in range(2):
        N = ec.N_COARSE + 1 + (ec.N_FINE if lv else 0)
        fg_t = pos[lv][0]
        fg = net.eval_mlp(lv, gb, fg_t, chunk=chunk)
        f = ops.composite(1, fg, fg_t, d, t_far)
        assert torch.equal(dec[2][lv][0], fg_t) and torch.equal(dec[2][lv][1], f["weights"]), lv
        assert torch.equal(dec[lv][1], f["rgb"]) and torch.equal(dec[lv][4], f["bg_lambda"])
        want = ops.decompose_rows(fg, fg_t, f["weights"], near, far, f["bg_lambda"])
        got = dec[lv][6]
        assert tuple(got["rgb"].shape) == (K7 + 1, n, 3)
        for k in ("rgb", "acc", "depth", "id"):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (lv, k)
        # the slots add up to the foreground composite of the frame
        ref = dc.decompose_f64(fg, fg_t, f["weights"], near[:0], far[:0])
        S = {k: ref["S_" + k][0] for k in SLOT_KEYS}
        whole = dict(rgb=dec[lv][1], acc=dec[lv][3], depth=f["depth"])
        summed = {k: got[k].double().sum(dim=0).cpu() for k in SLOT_KEYS}
        _check_slots(whole, summed, N, "%d rays level %d, sum over slots" % (n, lv), S=S, factor=2.0 * (math.ceil(N / 64) + 6) / (math.ceil(N / 64) + 7))
        # the duplicates and the empty instance own nothing; the owning slots are the restatement's
        cpu = dc.decompose_f64(fg, fg_t, f["weights"], near, far)
        assert bool((got["acc"][[ic.D, 5, 6]] == 0).all()) and bool((got["rgb"][[ic.D, 5, 6]] == 0).all())
        assert bool((got["acc"][(cpu["count"] == 0).to(DEV)] == 0).all())
        _check_slots(got, cpu, N, "%d rays level %d" % (n, lv))
        print("%d rays level %d: rays on which A, B, F, G hold weight: %s" % (n, lv, (got["acc"][:4] > 0).sum(dim=-1).tolist()))


def _permuted(res, perm):
    idx = list(perm) + [len(perm)]
    return {k: (v[idx] if k != "id" else v) for k, v in res.items()}


def test_permuting_the_list_permutes_the_slots_and_dropping_d_changes_nothing_else():
    base = _base()
    net, gb, near, far, dec = base["net"], base["gb"], base["near"], base["far"], base["dec"]
    # A and G swapped: slot s of the new list is instance perm[s] of the old one
    perm = [ic.G, ic.B, ic.F, ic.A, ic.D, 5, 6]
    swapped = _decomposed(net, gb, near[perm], far[perm], levels=(0, 1))
    for lv in range(2):
        fg_t = dec[2][lv][0]
        inside = ec.inside_mask(fg_t, near, far)
        shared_rays = (inside[:5].sum(dim=0) >= 2).any(dim=-1)          # rays with a sample inside two distinct boxes
        old, new = dec[lv][6], swapped[lv][6]
        for k in SLOT_KEYS:
            assert torch.equal(new[k][K7], old[k][K7]), (lv, k)         # the rest does not depend on the order
            for s, i in enumerate(perm):
                assert torch.equal(new[k][s][~shared_rays], old[k][i][~shared_rays]), (lv, k, s)
        assert 0 < int(shared_rays.sum()) < 96
        moved = (new["acc"][0] != old["acc"][ic.G]) | (new["acc"][3] != old["acc"][ic.A])
        assert bool((moved <= shared_rays).all()) and int(moved.sum()) > 0, lv
        # G first takes the shared samples from A
        assert bool((new["acc"][0][moved] >= old["acc"][ic.G][moved]).all()) and bool((new["acc"][3][moved] <= old["acc"][ic.A][moved]).all())
    # dropping D: the other slots, the rest and the id map (renumbered) stay
    keep = [ic.A, ic.B, ic.F, ic.G, 5, 6]
    dropped = _decomposed(net, gb, near[keep], far[keep], levels=(0, 1))
    renumber = torch.tensor([0, 1, 2, 3, -1, 4, 5, -1], dtype=torch.int32, device=DEV)       # old id -> new id; index 7 stands for -1
    for lv in range(2):
        old, new = dec[lv][6], dropped[lv][6]
        for k in SLOT_KEYS:
            assert torch.equal(new[k], old[k][keep + [K7]]), (lv, k)
        assert not bool((old["id"] == ic.D).any())
        assert torch.equal(new["id"], renumber[torch.where(old["id"] < 0, 7, old["id"]).long()])
        for x, y in zip(dropped[lv][:6], dec[lv][:6]):
            assert torch.equal(x, y)


# ---- 4. the frame helper ------------------------------------------------------------------------------------------------------------

def test_decomposed_frames():
    base = _base(300, 128)
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]
    RTs = oc.rts(*ic.INSTANCES)
    batch = dict(gb, near_inst=near, far_inst=far, target=gb["rays_o"])
    frame = render.render_rays_test(net, gb, chunk=128)
    fine = base["dec"][1]
    for b, kw, K in ((batch, {}, K7), (gb, dict(RTs=RTs), K7), (gb, {}, 0)):
        out = render.render_decomposed_rays(net, b, chunk=128, **kw)
        assert torch.equal(out["rgb"], frame["rgb"]) and torch.equal(out["depth"], frame["depth"]) and torch.equal(out["acc"], frame["acc"])
        assert torch.equal(out["fg_rgb"], frame["fg_rgb"]) and torch.equal(out["bg_rgb"], frame["bg_rgb"])
        assert [tuple(out[k].shape) for k in ("layer_rgb", "layer_acc", "layer_depth", "instance_id")] == [(K + 1, 300, 3), (K + 1, 300), (K + 1, 300), (300,)]
        if K == 0:          # the rest layer is the frame: fg + lambda bg, the merge's own two operations
            assert torch.equal(out["layer_rgb"][0], out["rgb"]) and torch.equal(out["layer_acc"][0], out["acc"])
            assert bool((out["instance_id"] == -1).all())
        else:
            assert torch.equal(out["layer_rgb"][:K7], fine[6]["rgb"][:K7]) and torch.equal(out["layer_acc"], fine[6]["acc"])
            assert torch.equal(out["layer_rgb"][K7], fine[6]["rgb"][K7] + fine[4] * fine[2])
            assert torch.equal(out["instance_id"], fine[6]["id"])
            seen = fine[6]["acc"] > 0
            assert bool((out["layer_depth"][~seen] == 0).all()) and 0 < int(seen[:K7].sum())
            assert torch.equal(out["layer_depth"][seen], fine[6]["depth"][seen] / fine[6]["acc"][seen])
            # a slot's expected ray parameter lies inside its interval (up to rounding)
            lo = torch.clamp(near, min=1e-4)
            inst = seen[:K7]
            assert bool((out["layer_depth"][:K7][inst] >= lo[inst] * (1 - 1e-5)).all()) and bool((out["layer_depth"][:K7][inst] <= far[inst] * (1 + 1e-5)).all())
            # the layers add up to the frame
            err = float((out["layer_rgb"].double().sum(dim=0) - out["rgb"].double()).abs().max())
            print("300 rays: sum of the layers against the frame, largest |err| %.3e" % err)
            # 49 samples: the sum over slots is within 2 * 7 * 2^-24 S of fg_rgb, S = sum w |c| <= 1.002; the frame and the rest
            # layer each add lambda * bg_rgb to their side with two roundings of values below 2.1
            assert err <= 14 * 2.0 ** -24 * 1.002 + 4 * 2.0 ** -24 * 2.1
    assert out.get("target") is None and render.render_decomposed_rays(net, batch, chunk=128)["target"] is gb["rays_o"]
    with pytest.raises(TypeError):
        render.render_decomposed_rays(models.NeRF().to(DEV), gb)


# ---- 5. the id map against the instance composite ------------------------------------------------------------------------------------

def test_id_map_against_the_instance_composite():
    base = _base()
    net, gb, near, far, hit = base["net"], base["gb"], base["near"], base["far"], base["hit"]
    ids = base["dec"][1][6]["id"].cpu()
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (96,)
    _, _, rule_hit = oc.hit_rule(near.cpu(), far.cpu())
    has = ids >= 0
    assert bool(rule_hit[ids[has].long(), torch.nonzero(has)[:, 0]].all()), "an id names an instance the ray hits"
    assert bool((ids[~rule_hit.any(dim=0)] == -1).all()) and int((~rule_hit.any(dim=0)).sum()) == 54
    assert not bool(((ids == ic.D) | (ids >= 5)).any()), "the empty instance and the duplicates are never visible"
    histogram = {int(v): int((ids == v).sum()) for v in ids.unique()}
    inst = net.render_instances(gb, near, far, white_bkgd=False)["composite"][1][3].cpu()
    net.check_flags()
    differs = int((inst != ids).sum())
    print("id histogram %r; differs from render_instances' id on %d of 96 rays (its histogram: %r)"
          % (histogram, differs, {int(v): int((inst == v).sum()) for v in inst.unique()}))
    assert histogram == ID_HISTOGRAM_96
    assert differs == ID_DIFFERS_FROM_INSTANCES_96
    # where they differ the scene occludes (the frame says -1 or another instance holds more of the ray's weight)
    assert bool(((ids == -1) | (inst >= 0))[inst != ids].all())
    acc = base["dec"][1][6]["acc"]
    lam = base["dec"][1][4][:, 0]
    print("largest share of a ray held by A, B, F, G: %s; smallest rest + bg_lambda on those rays: %s"
          % ([round(float(acc[i].max()), 4) for i in range(4)], [round(float((acc[K7] + lam)[acc[i].argmax()]), 4) for i in range(4)]))
    # an instance that does hold its rays: a box around the camera in front of the list, on every second ray.  It owns every
    # sample there, so it is named exactly where the foreground outweighs what leaves the sphere, and the rows of the frame say where
    odd = (torch.arange(96, device=DEV) % 2 == 1)
    front_n = torch.where(odd, -1.0, float("nan")).to(DEV)[None]
    front_f = torch.full((1, 96), 10.0, device=DEV)
    got = _decomposed(net, gb, torch.cat([front_n, near]), torch.cat([front_f, far]))[1]
    fg_acc, d = got[3], got[6]
    assert torch.equal(d["acc"][0][odd], fg_acc[odd]) and torch.equal(d["rgb"][0][odd], got[1][odd]) and bool((d["acc"][0][~odd] == 0).all())
    assert bool((d["acc"][1:][:, odd] == 0).all())
    want = torch.where(odd & (fg_acc > 0) & (fg_acc >= lam), 0, -1).to(torch.int32)
    assert torch.equal(d["id"][odd], want[odd]) and int((want == 0).sum()) >= 24
    shifted = torch.where(base["dec"][1][6]["id"] >= 0, base["dec"][1][6]["id"] + 1, -1).to(torch.int32)
    assert torch.equal(d["id"][~odd], shifted[~odd])


# ---- 6. edges, determinism, scope -------------------------------------------------------------------------------------------------

def test_edges_and_bad_arguments():
    base = _base()
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]
    none = {k: (v[:0] if k in PER_RAY else v) for k, v in gb.items()}
    out = _decomposed(net, none, near[:, :0], far[:, :0], levels=(0, 1), return_samples=True)
    assert [tuple(t.shape) for t in out[1][:6]] == [(0, 3), (0, 3), (0, 3), (0,), (0, 1), (0,)]
    assert [tuple(out[1][6][k].shape) for k in ("rgb", "acc", "depth", "id")] == [(K7 + 1, 0, 3), (K7 + 1, 0), (K7 + 1, 0), (0,)]
    assert [tuple(t.shape) for t in out[2][1]] == [(0, 49)] * 3
    z = ops.decompose_rows(torch.zeros(0, 9, 4, device=DEV), torch.zeros(0, 9, device=DEV), torch.zeros(0, 9, device=DEV), near[:, :0], far[:, :0])
    assert tuple(z["rgb"].shape) == (K7 + 1, 0, 3) and tuple(z["id"].shape) == (0,)
    big = near[:1].expand(33, -1)
    rs, t = torch.zeros(96, 9, 4, device=DEV), torch.rand(96, 9, device=DEV)
    for call in (lambda: net.render_decomposed(gb, big, big), lambda: ops.decompose_rows(rs, t, t, big, big),
                 lambda: net.render_decomposed(gb, near[:, :-1], far), lambda: net.render_decomposed(gb, near, far.long()),
                 lambda: net.render_decomposed(gb, near.cpu(), far.cpu()), lambda: net.render_decomposed(gb, near[:3], far[:4]),
                 lambda: net.render_decomposed(gb, near, far, levels=(2,)), lambda: net.render_decomposed(gb, near, far, levels=(True,)),
                 lambda: ops.decompose_rows(rs[:, :8], t, t, near, far), lambda: ops.decompose_rows(rs, t, t[:, :8], near, far),
                 lambda: ops.decompose_rows(rs, t, t, near[:, :95], far[:, :95]), lambda: ops.decompose_rows(rs, t, t.long(), near, far),
                 lambda: ops.decompose_rows(rs, t.cpu(), t, near, far), lambda: ops.decompose_rows(rs, t, t.cpu(), near, far),
                 lambda: ops.decompose_rows(rs, t, t, near.cpu(), far.cpu()), lambda: ops.decompose_rows(rs, t, t, near, far, torch.zeros(95, device=DEV)),
                 lambda: ops.decompose_rows(rs, t, t, near, far, torch.zeros(96)),
                 lambda: ops.decompose_rows(torch.zeros(2, 1025, 4, device=DEV), torch.zeros(2, 1025, device=DEV), torch.zeros(2, 1025, device=DEV), near[:, :2], far[:, :2]),
                 lambda: ops.decompose_rows(torch.zeros(2, 0, 4, device=DEV), torch.zeros(2, 0, device=DEV), torch.zeros(2, 0, device=DEV), near[:, :2], far[:, :2])):
        with pytest.raises(ValueError):
            call()
    # the library refuses the same counts on its own
    c = net._context(torch.device(DEV))
    o = _lib.TpDecomposedOut(None, None, None, None)
    p = rs.data_ptr()
    assert c.lib.neo_tp_decompose_rows(c.handle, p, p, p, p, p, 33, 96, 9, None, _lib.ctypes.byref(o), c.stream()) != 0
    assert c.lib.neo_tp_decompose_rows(c.handle, p, p, p, p, p, 7, 2, 1025, None, _lib.ctypes.byref(o), c.stream()) != 0
    assert c.lib.neo_tp_decompose_rows(c.handle, p, p, p, p, p, 7, 2, 0, None, _lib.ctypes.byref(o), c.stream()) != 0
    assert c.lib.neo_tp_decompose_rows(c.handle, p, p, p, p, p, 7, 96, 9, None, _lib.ctypes.byref(o), c.stream()) == 0      # every output NULL
    assert c.poll_flags() == 0
    # a ray that misses the unit sphere still raises, as in forward
    miss = dict(gb, rays_o=gb["rays_o"].clone(), rays_d=gb["rays_d"].clone())
    miss["rays_o"][5] = torch.tensor([0.0, 0.0, 5.0], device=DEV)
    miss["rays_d"][5] = torch.tensor([1.0, 0.0, 0.0], device=DEV)
    net.render_decomposed(miss, near, far)
    with pytest.raises(AssertionError):
        net.check_flags()
    with pytest.raises(AssertionError):
        render.render_decomposed_rays(net, dict(miss, near_inst=near, far_inst=far))
    net.check_flags()


def test_decomposed_calls_are_repeatable_chunk_and_overlap_neutral_and_synchronise_nothing():
    base = _base()
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]
    kw = dict(levels=(0, 1), return_samples=True)
    again = _decomposed(net, gb, near, far, **kw)
    assert all(torch.equal(x, y) for x, y in zip(_flat(again), _flat(base["dec"])))
    assert net.overlap_calls
    net.overlap_calls = False
    try:
        off = _decomposed(net, gb, near, far, **kw)
    finally:
        net.overlap_calls = True
    assert all(torch.equal(x, y) for x, y in zip(_flat(off), _flat(base["dec"])))
    # the reference-style loop: three calls of 32 rays, each one reference chunk, in flight on alternating lanes; no blocking wait
    whole = _decomposed(net, gb, near, far, chunk=32, **kw)
    ctx = net._context(torch.device(DEV))
    before = ctx.sync_count()
    parts = []
    for i in range(0, 96, 32):
        part = {k: (v[i:i + 32] if k in PER_RAY else v) for k, v in gb.items()}
        parts.append(net.render_decomposed(part, near[:, i:i + 32], far[:, i:i + 32], chunk=32, **kw))
    assert ctx.sync_count() == before, "a decomposed call blocked on the device"
    net.check_flags()
    for lv in range(2):
        for j in range(6):
            assert torch.equal(torch.cat([p[lv][j] for p in parts]), whole[lv][j]), (lv, j)
        for k in SLOT_KEYS:
            assert torch.equal(torch.cat([p[lv][6][k] for p in parts], dim=1), whole[lv][6][k]), (lv, k)
        assert torch.equal(torch.cat([p[lv][6]["id"] for p in parts]), whole[lv][6]["id"]), lv
        for j in range(3):
            assert torch.equal(torch.cat([p[2][lv][j] for p in parts]), whole[2][lv][j]), (lv, j)


def test_scope_nothing_else_changes():
    """forward, render_objects, render_instances and render_edited issued before and after decomposed calls are bitwise unchanged;
    the decomposed call reads neither cull_background nor compute_extras."""
    base = _base()
    net, gb, near, far = base["net"], base["gb"], base["near"], base["far"]
    scale = [0.0, 0.3, 1.0, 1.0, 1.0, 1.0, 1.0]

    def others():
        inst = net.render_instances(gb, near, far)
        out = [net(gb, False, False, 0.0, 0.0, out_depth=True), net.render_objects(gb, near_obj=near[0], far_obj=far[0]),
               inst["instances"], inst["composite"], net.render_edited(gb, near, far, density_scale=scale)]
        net.check_flags()
        return [[t.clone() for t in lv] for o in out for lv in o]
    before = others()
    net.cull_background = 1e-2
    try:
        culled = _decomposed(net, gb, near, far, levels=(0, 1), return_samples=True)
    finally:
        net.cull_background = None
    net.compute_extras = True
    try:
        extras = _decomposed(net, gb, near, far, levels=(0, 1), return_samples=True)
    finally:
        net.compute_extras = False
    for res in (culled, extras):
        assert len(res[0]) == len(res[1]) == 7
        assert all(torch.equal(x, y) for x, y in zip(_flat(res), _flat(base["dec"])))
    after = others()
    for x, y in zip(before, after):
        assert len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y))
