"""CPU: the restatements the edited-render tests stand on (tests/edit_cases.py), the pinned content of their fixture, the C ABI
declarations and the host-side validation of `ops.edit_rgbsigma`, `ops.composite_layers`, `NeRF_TP.render_edited`,
`render.instance_layers` and `render.render_edited_rays` as far as it runs without a device."""
import os
import re

import numpy as np
import pytest
import torch

import edit_cases as ec
import instance_cases as ic
import object_cases as oc
import oracle
from conftest import ROOT
from neo360_amd import _lib, models, ops, render


def test_oracle_render_edited_without_edits_is_the_oracle_render():
    b = ic.rays(96)
    near, far, _ = ic.bounds(96)
    want = oracle.neo360.render(ec.state(), b, ec.scene(), ec.N_COARSE, ec.N_FINE, out_depth=True)
    for kw in (dict(), dict(scale=[1.0] * ec.K7, tint=[[1.0, 1.0, 1.0]] * ec.K7)):
        got, extra = ec.oracle_render_edited(ec.state(), b, ec.scene(), near, far, keep=True, **kw)
        for lv in range(2):
            assert len(got[lv]) == len(want[lv]) == 6
            for i, (x, y) in enumerate(zip(got[lv], want[lv])):
                assert x.dtype == y.dtype and torch.equal(x, y), (lv, i)
            assert torch.equal(extra[lv]["fg_rows"], extra[lv]["fg_raw"])
    # given level-1 positions are used as they are
    given = (extra[1]["fg_t"], extra[1]["bg_s"])
    again = ec.oracle_render_edited(ec.state(), b, ec.scene(), near, far, fine_samples=given)
    assert all(torch.equal(x, y) for x, y in zip(again[1], want[1]))
    # and an edit changes the rays it touches only: A removed
    scale = [0.0] + [1.0] * (ec.K7 - 1)
    cut, extra = ec.oracle_render_edited(ec.state(), b, ec.scene(), near[:1], far[:1], scale=scale[:1], keep=True)
    hit_a = ic.bounds(96)[2][0]
    for lv in range(2):
        changed = (cut[lv][0] != want[lv][0]).any(dim=-1)
        assert bool(changed.any()) and not bool((changed & ~hit_a).any()), lv
        inside = ec.inside_mask(extra[lv]["fg_t"], near[:1], far[:1])[0]
        assert bool((extra[lv]["fg_w"][inside] == 0).all()), lv


def test_layer_restatement_without_layers_is_the_oracle_composite():
    g = torch.Generator().manual_seed(5)
    for N in (5, 64, 65, 385):
        R = 7
        rs = torch.rand(R, N, 4, generator=g)
        rs[..., 3] = rs[..., 3] * 40.0
        t = torch.sort(torch.rand(R, N, generator=g) * 1.5 + 0.01, dim=-1).values
        d = torch.randn(R, 3, generator=g)
        far = t[:, -1:] + 0.1
        got = ec.composite_layers_f64(rs, t, d, far)
        rgb, acc, w, lam, depth = oracle.compositing.neo_composite(rs[..., :3].double(), rs[..., 3:].double(), t.double(), d.double(), True,
                                                                  far.double())
        assert torch.equal(got["rgb"], rgb) and torch.equal(got["acc"], acc) and torch.equal(got["depth"], depth), N
        assert torch.equal(got["weights"], w) and torch.equal(got["bg_lambda"], lam), N
        assert tuple(got["visibility"].shape) == (0, R)
        # layers that are all invalid: the same numbers, zero visibility
        layers = dict(key=torch.tensor([[float("nan")] * R, [float("inf")] * R, [0.5] * R]), rgb=torch.ones(3, R, 3),
                      acc=torch.tensor([[0.5] * R, [0.5] * R, [0.0] * R]), depth=torch.ones(3, R))
        same = ec.composite_layers_f64(rs, t, d, far, layers)
        assert all(torch.equal(same[k], got[k]) for k in ("rgb", "acc", "depth", "weights", "bg_lambda")), N
        assert bool((same["visibility"] == 0).all())
    # one opaque layer in front of everything: the scene vanishes behind it
    layers = dict(key=torch.zeros(1, R), rgb=torch.full((1, R, 3), 0.25), acc=torch.ones(1, R), depth=torch.full((1, R), 0.125))
    front = ec.composite_layers_f64(rs, t, d, far, layers)
    assert bool((front["rgb"] == 0.25).all()) and bool((front["acc"] == 1).all()) and bool((front["depth"] == 0.125).all())
    assert bool((front["bg_lambda"] == 0).all()) and bool((front["visibility"] == 1).all())
    assert torch.equal(front["weights"], got["weights"]), "the scene weights do not see the layers"
    # one half-transparent layer behind everything: the scene in front is untouched, the layer is seen through S_end
    layers = dict(key=torch.full((1, R), 9.0), rgb=torch.full((1, R, 3), 0.5), acc=torch.full((1, R), 0.5), depth=torch.ones(1, R))
    back = ec.composite_layers_f64(rs, t, d, far, layers)
    s_end = got["bg_lambda"][:, 0]
    assert torch.equal(back["visibility"][0], s_end * 0.5) and torch.equal(back["bg_lambda"][:, 0], s_end * 0.5)
    assert torch.equal(back["acc"], got["acc"] + s_end * 0.5)


PINS = {96: dict(samples=96 * 17, inside=[45, 13, 6, 30, 0, 45, 30], two=54, three=21, fine_only=(30, 115), no_hit=54),
        300: dict(samples=300 * 17, inside=[151, 45, 16, 92, 0, 151, 92], two=177, three=66, fine_only=(98, 384), no_hit=168)}


@pytest.mark.parametrize("n", [96, 300])
def test_fixture_counts_of_the_edit_scene(n):
    pin = PINS[n]
    lv0 = ec.oracle_level0(n)
    fg_t, near, far, hit = lv0["fg_t"], lv0["near"], lv0["far"], lv0["hit"]
    assert fg_t.numel() == pin["samples"]
    inside = ec.inside_mask(fg_t, near, far)
    assert inside.sum(dim=(1, 2)).tolist() == pin["inside"]
    per_sample = inside.sum(dim=0)
    assert int((per_sample >= 2).sum()) == pin["two"] and int((per_sample >= 3).sum()) == pin["three"]
    empty = hit & ~inside.any(dim=2)
    assert (int(empty.sum()), int(hit.sum())) == pin["fine_only"], "hit pairs that only the fine level's samples fall into"
    assert int((~hit.any(dim=0)).sum()) == pin["no_hit"]
    # no sample sits within rounding of an interval end: its inside / outside decision is the same on CPU and GPU rows
    lo, hi, rule = oc.hit_rule(near, far)
    assert torch.equal(rule, hit)
    gap = torch.minimum((fg_t[None] - lo[:, :, None]).abs(), (fg_t[None] - hi[:, :, None]).abs())[hit]
    print("closest level-0 sample to an interval end (%d rays): %.2e" % (n, float(gap.min())))
    assert float(gap.min()) >= 2.0e-5 and float(gap.min()) > 100 * float(np.spacing(np.float32(fg_t.max())))


def _header():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(bare, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
    assert m, "%s is not declared in include/neo360_hip.h" % name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_header_declares_and_ctypes_binds_the_edit_entry_points():
    text, bare = _header()
    for name in ("neo_tp_edit_rows", "neo_composite_layers", "neo_tp_render_edited"):
        assert len(_lib.SIGNATURES[name][1]) == len(_params(bare, name)), name
        assert hasattr(_lib.load(), name)
    for struct, cls in (("neo_tp_layers", _lib.TpLayers), ("neo_tp_edit_samples", _lib.TpEditSamples)):
        m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % struct, bare)
        assert m and re.findall(r"float\s*\*\s*(\w+)\s*;", m.group(1)) == [n for n, _ in cls._fields_], struct
    flat = re.sub(r"[\s*]+", " ", text)
    for phrase in ("EDIT RULE", "lo <= t_j && t_j <= hi", "a sample inside no interval is not written", "LAYER RECURRENCE",
                   "ascending key, ties to the lower index", "keep_l = max(1 - a_l, 0) in fp32", "j_l = the first sample with t_j >= key_l",
                   "A layer is a slab at its key, not a merged medium"):
        assert phrase in flat, phrase


def test_edit_entry_points_validate_on_the_host():
    net = models.NeRF_TP(num_coarse_samples=8, num_fine_samples=8)
    b = ic.rays(96)
    near, far, _ = ic.bounds(96)
    K = near.shape[0]
    # the host tables: right length, finite, >= 0
    assert ops.edit_table(K) == (None, None)
    scale, tint = ops.edit_table(2, [0.0, 2.5], torch.tensor([[1.0, 0.5, 0.0], [2.0, 1.0, 1.0]]))
    assert list(scale) == [0.0, 2.5] and list(tint) == [1.0, 0.5, 0.0, 2.0, 1.0, 1.0]
    for kw in (dict(density_scale=[1.0] * (K - 1)), dict(density_scale=[1.0] * (K - 1) + [-0.5]), dict(density_scale=[float("nan")] * K),
               dict(density_scale=[float("inf")] * K), dict(tint=[[1.0, 1.0, 1.0]] * (K + 1)), dict(tint=[[1.0, 1.0]] * K),
               dict(tint=[[1.0, -1.0, 1.0]] * K), dict(tint=[[1.0, float("nan"), 1.0]] * K), dict(density_scale=torch.ones(K, device="meta"))):
        with pytest.raises(ValueError):
            net.render_edited(b, near, far, **kw)
        with pytest.raises(ValueError):
            ops.edit_rgbsigma(torch.zeros(96, 9, 4), torch.zeros(96, 9), near, far, **kw)
    # the bounds, as render_instances validates them
    for bad in (near[:, :-1], near.reshape(-1), near.t(), near[None], near[:1].expand(33, -1), near.long()):
        with pytest.raises(ValueError):
            net.render_edited(b, bad, far)
        with pytest.raises(ValueError):
            net.render_edited(b, near, bad)
    with pytest.raises(ValueError):
        net.render_edited(b, near[:3], far[:4])
    with pytest.raises(ValueError):
        net.render_edited(b, near.to("meta"), far.to("meta"))
    # the layers
    good = dict(key=torch.zeros(2, 96), rgb=torch.zeros(2, 96, 3), acc=torch.zeros(2, 96), depth=torch.zeros(2, 96))
    for bad in (dict(good, rgb=torch.zeros(2, 96)), dict(good, acc=torch.zeros(3, 96)), dict(good, key=torch.zeros(2, 95)),
                {k: v for k, v in good.items() if k != "depth"}, dict(good, depth=torch.zeros(2, 96, dtype=torch.long)),
                dict(good, acc=torch.zeros(2, 96, device="meta")), [good],
                dict(key=torch.zeros(33, 96), rgb=torch.zeros(33, 96, 3), acc=torch.zeros(33, 96), depth=torch.zeros(33, 96))):
        with pytest.raises(ValueError):
            net.render_edited(b, near, far, layers=bad)
    # well-formed calls reach the device check: CPU tensors are refused as everywhere
    for kw in (dict(), dict(density_scale=[0.0] * K, tint=[[2.0, 0.5, 1.0]] * K), dict(layers=good), dict(return_samples=True)):
        with pytest.raises(_lib.NeoError):
            net.render_edited(b, near, far, **kw)
    with pytest.raises(_lib.NeoError):
        net.render_edited(b, near[:0], far[:0])
    with pytest.raises(_lib.NeoError):
        ops.edit_rgbsigma(torch.zeros(96, 9, 4), torch.zeros(96, 9), near, far)
    with pytest.raises(ValueError):
        ops.edit_rgbsigma(torch.zeros(96, 9, 3), torch.zeros(96, 9), near, far)
    doc = models.NeRF_TP.render_edited.__doc__
    assert "cull_background" in doc and "compute_extras" in doc


def test_moves_must_be_rigid_and_leave_the_moved_instance_alone():
    net = models.NeRF_TP(num_coarse_samples=8, num_fine_samples=8)
    b = ic.rays(96)
    RTs = oc.rts(*ic.INSTANCES)
    eye = np.eye(4)
    shear, scaled, mirror, bent = np.eye(4), np.eye(4), np.eye(4), np.eye(4)
    shear[0, 1] = 0.1
    scaled[:3, :3] *= 1.01
    mirror[0, 0] = -1.0
    bent[3, 0] = 0.1
    for bad in (shear, scaled, mirror, bent, np.eye(3), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            render.instance_layers(net, b, RTs, {0: bad})
        with pytest.raises(ValueError):
            render.render_edited_rays(net, b, RTs=RTs, moves={0: bad})
    for index in (-1, 7, "0", 1.0):
        with pytest.raises(ValueError):
            render.instance_layers(net, b, RTs, {index: eye})
    near, far, _ = ic.bounds(96)
    batch = dict(b, near_inst=near, far_inst=far)
    with pytest.raises(ValueError):
        render.render_edited_rays(net, batch, moves={0: eye})                                  # moves need the boxes
    with pytest.raises(ValueError):
        render.render_edited_rays(net, batch, RTs=RTs, moves={0: eye}, density_scale=[0.5] + [1.0] * 6)
    with pytest.raises(ValueError):
        render.render_edited_rays(net, batch, RTs=RTs, moves={3: eye}, tint=[[1.0, 1.0, 1.0]] * 3 + [[2.0, 1.0, 1.0]] + [[1.0, 1.0, 1.0]] * 3)
    with pytest.raises(ValueError):
        render.render_edited_rays(net, batch, RTs=oc.rts(*ic.DISTINCT))                        # 5 boxes, 7 intervals
    with pytest.raises(ValueError):
        render.render_edited_rays(net, batch, on_range="ignore")
    with pytest.raises(TypeError):
        render.render_edited_rays(models.NeRF(), batch)
    with pytest.raises(TypeError):
        render.instance_layers(models.NeRF(), b, RTs, {0: eye})
    # well-formed: the device check is what stops a CPU batch
    with pytest.raises(_lib.NeoError):
        render.render_edited_rays(net, batch, density_scale=[0.0] + [1.0] * 6)
    rot = np.eye(4)
    c, s = np.cos(0.3), np.sin(0.3)
    rot[:2, :2] = [[c, -s], [s, c]]
    rot[:3, 3] = [0.1, -0.2, 0.05]
    with pytest.raises(_lib.NeoError):
        render.instance_layers(net, b, RTs, {0: rot})
