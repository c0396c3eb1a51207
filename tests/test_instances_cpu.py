"""CPU: the host side of the instance render (NeRF_TP.render_instances, neo_tp_render_instances, neo_aabb_per_box) and the scene
the GPU tests of it (tests/test_gpu_instances.py) stand on.

The scene is pinned to the REFERENCE arithmetic, not to the code under test: hit counts come from the CPU oracle's single-box
calls, opacities from object_cases.oracle_render at 16 + 32 samples, and the id map from the composite recurrence restated in
torch (instance_cases.composite) on the oracle's own level-1 results."""
import os
import re

import pytest
import torch

import instance_cases as ic
import object_cases as oc
from conftest import ROOT
from neo360_amd import _lib, models, ops, render


def _header():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(bare, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
    assert m, "%s is not declared in include/neo360_hip.h" % name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_header_declares_and_ctypes_binds_the_instance_entry_points():
    text, bare = _header()
    obj, inst = _params(bare, "neo_tp_render_objects"), _params(bare, "neo_tp_render_instances")
    # neo_tp_render_objects' arguments with the (K, R) bounds, K in front of R, and its own output struct
    assert inst[:4] == obj[:4]
    assert inst[4:7] == ["const float* near_inst", "const float* far_inst", "int K"]
    assert inst[7:17] == obj[6:16]
    assert inst[17:19] == ["const neo_tp_instance_out* level0", "const neo_tp_instance_out* level1"]
    assert inst[19] == "int* pairs_out" and inst[20] == obj[-1] and len(inst) == 21
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*neo_tp_instance_out\s*;", bare)
    fields = ["rgb", "acc", "depth", "comp_rgb", "comp_acc", "comp_depth", "instance_id"]
    assert m and re.findall(r"(?:float|int)\s*\*\s*(\w+)\s*;", m.group(1)) == fields
    assert [n for n, _ in _lib.TpInstanceOut._fields_] == fields
    res, args = _lib.SIGNATURES["neo_tp_render_instances"]
    res0, args0 = _lib.SIGNATURES["neo_tp_render_objects"]
    assert res is res0 and len(args) == len(inst)
    assert args[:6] == args0[:6] and args[6] is _lib._i and args[7:17] == args0[6:16]
    assert args[17] == args[18] == _lib.ctypes.POINTER(_lib.TpInstanceOut) and args[19] is _lib._vp and args[20] is args0[-1]
    # the per-box intervals: neo_aabb_multi's inputs, per-box float32 near / far and the uint8 mask
    multi, per_box = _params(bare, "neo_aabb_multi"), _params(bare, "neo_aabb_per_box")
    assert per_box[:7] == multi[:7] and per_box[7:] == ["float* near", "float* far", "uint8_t* hit", "void* stream"]
    assert len(_lib.SIGNATURES["neo_aabb_per_box"][1]) == len(per_box)
    assert _lib.SIGNATURES["neo_aabb_per_box"][1][:7] == _lib.SIGNATURES["neo_aabb_multi"][1][:7]
    # the hit rule and the composite recurrence are stated where the entry point is declared
    comment = text[:text.index("} neo_tp_instance_out;")].rsplit("typedef struct", 1)[0].rsplit("/*", 1)[1]
    flat = re.sub(r"[\s*]+", " ", comment)
    for phrase in ("HIT RULE", "lo = max(near_inst, 1e-4)", "hi = far_inst", "both bounds are finite and hi > lo",
                   "NaN bound makes the pair a miss", "COMPOSITE RECURRENCE", "ascending lo, ties to the lower instance index",
                   "T = 1, rgb = depth = acc = 0, best = 0, id = -1", "v = T a_i; rgb += T p_i; depth += T d_i; acc += v;",
                   "if v > best then best = v, id = i; T = T (1 - a_i)", "if white_bkgd: rgb += 1 - acc",
                   "density inside an overlap counts twice", "K WINDOWS of at most R rows"):
        assert phrase in flat, phrase
    lib = _lib.load()
    assert hasattr(lib, "neo_tp_render_instances") and hasattr(lib, "neo_aabb_per_box")


def test_render_instances_validates_bounds_and_rejects_cpu_tensors():
    net = models.NeRF_TP(num_coarse_samples=8, num_fine_samples=8)
    assert net.last_instance_pairs is None
    b = ic.rays(96)
    near, far, _ = ic.bounds(96)
    assert tuple(near.shape) == (7, 96)
    for bad in (near[:, :-1], near.reshape(-1), near.t(), near[:, :, None].expand(-1, -1, 2), near[None], torch.zeros(()),
                near[:1].expand(33, -1)):
        with pytest.raises(ValueError):
            net.render_instances(b, bad, far)
        with pytest.raises(ValueError):
            net.render_instances(b, near, bad)
    with pytest.raises(ValueError):
        net.render_instances(b, near[:3], far[:4])                 # differing instance counts
    with pytest.raises(ValueError):
        net.render_instances(b, near.long(), far)
    with pytest.raises(ValueError):
        net.render_instances(b, near, far.tolist())
    with pytest.raises(ValueError):
        net.render_instances(b, near.to("meta"), far.to("meta"))   # not on the rays' device
    with pytest.raises(TypeError):
        net.render_instances(b)                                    # the bounds are required arguments
    # well-formed bounds in both shapes and any float dtype, 0 and 32 instances included: CPU tensors are refused as everywhere
    for n, f in ((near, far), (near[:, :, None].double(), far[:, :, None].half()), (near[:0], far[:0]),
                 (near[:1].expand(32, -1), far[:1].expand(32, -1))):
        with pytest.raises(_lib.NeoError):
            net.render_instances(b, n, f)
        with pytest.raises(_lib.NeoError):
            net.render_instances(b, n, f, per_instance=False)
    with pytest.raises(_lib.NeoError):
        render.render_instance_rays(net, dict(b, near_inst=near, far_inst=far))
    with pytest.raises(_lib.NeoError):
        render.render_instance_rays(net, b, RTs=oc.rts(*ic.INSTANCES))
    with pytest.raises(_lib.NeoError):
        ops.sample_rays_in_bbox_list(oc.rts(*ic.INSTANCES), b["rays_o"], b["viewdirs"])
    with pytest.raises(ValueError):
        render.render_instance_rays(net, b)                        # no intervals anywhere
    with pytest.raises(TypeError):
        render.render_instance_rays(models.NeRF(), b)
    assert net.last_instance_pairs is None, "a refused call leaves no count behind"


PINS = {96: dict(per_box=[25, 10, 11, 22, 0], met=[54, 25, 8, 9], pairs=115, a_and_g=(10, 7)),
        300: dict(per_box=[84, 30, 38, 74, 0], met=[168, 70, 30, 32], pairs=384, a_and_g=(32, 26))}


@pytest.mark.parametrize("n", [96, 300])
def test_oracle_hit_counts_of_the_instance_scene(n):
    pin = PINS[n]
    near, far, hit = ic.bounds(n, ic.DISTINCT)
    lo, hi, rule = oc.hit_rule(near, far)
    assert torch.equal(rule, hit), "the hit rule is the reference's mask on the reference's own per-box bounds"
    assert hit.sum(dim=1).tolist() == pin["per_box"]
    met = hit.sum(dim=0)
    assert [int((met == k).sum()) for k in range(4)] == pin["met"] and int(met.max()) == 3
    near7, far7, hit7 = ic.bounds(n)
    assert int(hit7.sum()) == pin["pairs"] > n, "more pairs than rays: at least two non-empty windows"
    assert torch.equal(near7[5], near7[0]) and torch.equal(far7[6], far7[3]) and not bool(hit7[4].any())
    both = hit[ic.A] & hit[ic.G]
    assert (int((both & (lo[ic.A] < lo[ic.G])).sum()), int((both & (lo[ic.G] < lo[ic.A])).sum())) == pin["a_and_g"]
    if n == 96:
        for other in (ic.A, ic.G):      # F is in front of whatever it shares a ray with: both depth orders occur across the scene
            shared = hit[ic.F] & hit[other]
            assert int(shared.sum()) == 9 and bool((lo[ic.F][shared] < lo[other][shared]).all())
    else:
        blocks = torch.unique(hit7.reshape(-1).nonzero().reshape(-1) // 256)
        assert len(blocks) >= 2, "the hit pairs span several 256-element compaction workgroups"


def test_oracle_opacities_and_id_map_of_the_instance_scene():
    """Level-1 acc over the hits (two significant digits), and the composite recurrence on the oracle's own level-1 results at 96
    rays: the id histogram, the rays whose winner is not their nearest instance, and the smallest gap between the two largest
    visibilities of a ray - far above any rounding, so the GPU id map is compared exactly."""
    o = ic.oracle_instances(96)
    hit = o["hit"]
    for box, lo_pin, hi_pin in ((ic.A, 0.061, 0.893), (ic.F, 0.043, 0.328), (ic.G, 0.043, 0.677)):
        acc = o["acc1"][box][hit[box]]
        print("level-1 acc of box %s: %.4f .. %.4f" % (ic.NAMES[box], float(acc.min()), float(acc.max())))
        assert abs(float(acc.min()) - lo_pin) <= 1e-3 and abs(float(acc.max()) - hi_pin) <= 1e-3, ic.NAMES[box]
    idx = [ic.index_of(b) for b in ic.INSTANCES]
    near, far = o["near"][idx], o["far"][idx]
    p, a, d = o["rgb1"][idx], o["acc1"][idx], o["depth1"][idx]
    rgb, acc, depth, ids, order, valid = ic.composite(near, far, p, a, d, white=False)
    hist = {int(k): int(v) for k, v in zip(*torch.unique(ids, return_counts=True))}
    assert hist == {-1: 54, 0: 21, 1: 10, 2: 2, 3: 9}, hist
    nearest = torch.where(valid[0], order[0].to(torch.int32), torch.full_like(ids, -1))
    assert int((ids != nearest).sum()) == 12, "rays whose most visible instance is not their nearest one"
    # visibilities v = T a of every (instance, ray) in the ray's order; the gap between the two largest of a ray with >= 2 hits
    cols = torch.arange(96)
    T = torch.ones(96)
    vis = torch.zeros(7, 96)
    for s in range(7):
        i = order[s]
        ai = torch.where(valid[s], a[i, cols], torch.zeros(96))
        vis[s] = T * ai
        T = T * (1.0 - ai)
    top = torch.sort(vis, dim=0, descending=True).values
    many = valid.sum(dim=0) >= 2
    gap = float((top[0] - top[1])[many].min())
    print("smallest gap between the two largest visibilities: %.2e" % gap)
    assert abs(gap - 3.8e-3) <= 1e-4
    assert bool((acc <= 1.0 + 1e-6).all()) and bool((acc[ids < 0] == 0).all())
