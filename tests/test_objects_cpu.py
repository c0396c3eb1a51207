"""CPU: the host side of the object render (NeRF_TP.render_objects, neo_tp_render_objects) and the scene the GPU tests of it
(tests/test_gpu_objects.py) stand on.

The scene is pinned to the REFERENCE arithmetic, not to the code under test: the CPU oracle (tests/object_cases.py: the existing
oracle functions composed with the object interval in place of the sphere interval) must show the hit counts and the spread of
accumulated opacity the GPU tests were designed around."""
import os
import re

import pytest
import torch

import object_cases as oc
from conftest import ROOT
from neo360_amd import _lib, models, render


def test_header_declares_and_ctypes_binds_the_object_render():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
        assert m, "%s is not declared in include/neo360_hip.h" % name
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    plain, obj = params("neo_tp_render"), params("neo_tp_render_objects")
    # neo_tp_render's arguments with the two bounds behind viewdirs, its own output struct and the device hit count
    assert obj[:4] == plain[:4]
    assert obj[4:6] == ["const float* near_obj", "const float* far_obj"]
    assert obj[6:16] == plain[4:14]
    assert obj[16:18] == ["const neo_tp_object_out* level0", "const neo_tp_object_out* level1"]
    assert obj[18] == "int* hits_out" and obj[19] == plain[-1] and len(obj) == 20
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*neo_tp_object_out\s*;", bare)
    assert m and re.findall(r"float\s*\*\s*(\w+)\s*;", m.group(1)) == ["rgb", "acc", "depth", "tvals"]
    assert [n for n, _ in _lib.TpObjectOut._fields_] == ["rgb", "acc", "depth", "tvals"]
    res, args = _lib.SIGNATURES["neo_tp_render_objects"]
    res0, args0 = _lib.SIGNATURES["neo_tp_render"]
    assert res is res0 and len(args) == len(obj)
    assert args[:4] == args0[:4] and args[4] is _lib._vp and args[5] is _lib._vp and args[6:16] == args0[4:14]
    assert args[16] == args[17] == _lib.ctypes.POINTER(_lib.TpObjectOut) and args[18] is _lib._vp and args[19] is args0[-1]
    # the hit rule is stated where the entry point is declared
    comment = text[:text.index("typedef struct { float* rgb; float* acc; float* depth; float* tvals; } neo_tp_object_out")].rsplit("/*", 1)[1]
    flat = re.sub(r"[\s*]+", " ", comment)
    for phrase in ("HIT RULE", "lo = max(near_obj, 1e-4)", "hi = far_obj", "both bounds are finite and hi > lo", "NaN bound makes the ray a miss"):
        assert phrase in flat, phrase


def test_render_objects_validates_bounds_and_rejects_cpu_tensors():
    net = models.NeRF_TP(num_coarse_samples=8, num_fine_samples=8)
    assert net.last_object_hits is None
    b, _ = oc.batch(96)
    rays = {k: v for k, v in b.items() if k not in ("near_obj", "far_obj")}
    near, far = b["near_obj"], b["far_obj"]
    with pytest.raises(ValueError):
        net.render_objects(rays)                                  # no bounds anywhere
    with pytest.raises(ValueError):
        net.render_objects(rays, near_obj=near)                   # one of them
    with pytest.raises(ValueError):
        net.render_objects(dict(rays, near_obj=near), far_obj=None)
    for bad in (near[:-1], near.reshape(1, -1), near.expand(-1, 2), near.reshape(-1, 1, 1), torch.zeros(())):
        with pytest.raises(ValueError):
            net.render_objects(rays, near_obj=bad, far_obj=far)
        with pytest.raises(ValueError):
            net.render_objects(rays, near_obj=near, far_obj=bad)
    with pytest.raises(ValueError):
        net.render_objects(rays, near_obj=near.long(), far_obj=far)
    with pytest.raises(ValueError):
        net.render_objects(rays, near_obj=near.reshape(-1).tolist(), far_obj=far)
    # well-formed bounds in both shapes, any float dtype, from the batch or as arguments: CPU tensors are refused as everywhere
    for kw in (dict(near_obj=near, far_obj=far), dict(near_obj=near.reshape(-1).double(), far_obj=far.reshape(-1).half())):
        with pytest.raises(_lib.NeoError):
            net.render_objects(rays, **kw)
    with pytest.raises(_lib.NeoError):
        net.render_objects(b)
    with pytest.raises(_lib.NeoError):
        render.render_object_rays(net, b)
    with pytest.raises(TypeError):
        render.render_object_rays(models.NeRF(), b)
    assert net.last_object_hits is None, "a refused call leaves no count behind"


def test_oracle_hit_counts_of_the_test_scene():
    for n, hits in ((96, 35), (300, 114)):
        b, mask = oc.batch(n)
        near, far = b["near_obj"].reshape(-1), b["far_obj"].reshape(-1)
        lo, hi, hit = oc.hit_rule(near, far)
        assert torch.equal(hit, mask), "the hit rule is the reference's mask on the reference's own bounds"
        assert int(hit.sum()) == hits
        assert 0.2 <= float(hit.float().mean()) <= 0.8, "a mixed frame"
        assert bool((far[hit] > near[hit]).all()) and bool((near[~hit] == 0).all()) and bool((far[~hit] == 0).all())
        assert 0.42 <= float(near[hit].min()) and float(near[hit].max()) <= 0.82
    hit = oc.batch(300)[1]
    assert bool(hit[:256].any()) and bool(hit[256:].any()), "hits in both 256-ray compaction workgroups"
    a, bb = oc.batch(96, oc.BOX_A)[1], oc.batch(96, oc.BOX_B)[1]
    assert int(a.sum()) == 25 and int(bb.sum()) == 10 and not bool((a & bb).any())         # 0.26 and 0.10 of 96
    frame = oc.frame_batch()[1]
    assert abs(float(frame.float().mean()) - 0.377) <= 5e-4
    # rays 0, 5 and 17 miss both boxes: the GPU edge test gives them bounds of its own
    m96 = oc.batch(96)[1]
    assert not bool(m96[[0, 5, 17]].any())


def test_oracle_opacity_spread_of_the_test_scene():
    """At 16 + 32 samples the level-1 acc over the 35 hits spans 0.061 .. 0.893: neither empty nor saturated, so a wrong interval,
    a wrong last delta or a wrong composite shows.  Two significant digits."""
    b, mask = oc.batch(96)
    o = oc.oracle_render(oc.state(), b, b["near_obj"], b["far_obj"], 16, 32)
    acc = o["acc1"][mask]
    print("level-1 acc over the hits: %.4f .. %.4f; level 0: %.4f .. %.4f"
          % (float(acc.min()), float(acc.max()), float(o["acc0"][mask].min()), float(o["acc0"][mask].max())))
    assert abs(float(acc.min()) - 0.061) <= 1e-3 and abs(float(acc.max()) - 0.893) <= 1e-3
    # white background: rgb = sum w c + (1 - acc); depth inside the interval scaled by acc
    near, far = b["near_obj"].reshape(-1)[mask], b["far_obj"].reshape(-1)[mask]
    d = o["depth1"][mask]
    assert bool((d >= near * acc - 1e-5).all()) and bool((d <= far * acc + 1e-5).all())
    black = oc.oracle_render(oc.state(), b, b["near_obj"], b["far_obj"], 16, 32, white_bkgd=False, t1=o["t1"])
    assert torch.allclose(o["rgb1"][mask], black["rgb1"][mask] + (1.0 - acc)[:, None], atol=1e-6)
