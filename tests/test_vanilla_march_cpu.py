"""CPU: the restatements of the vanilla marching-frame tests (tests/vanilla_march_cases.py), the conditions on their inputs, the
a-priori bound on the oracle, the host-side validation of the new module and its ABI declarations.  Nothing here needs a device.

The BOX KEEP RULE is stated twice, in fp32 (what the kernel computes) and in fp64 from the same fp32 inputs and the same fp32
scale.  The two may disagree only where (x - lo) scale lies within the fp32 roundings of an integer; vc.near_face_box leaves
those samples out, and they are at most 1 % of the samples of every input the GPU tests classify, so the exclusion cannot hide a
failure."""
import os
import re

import pytest
import torch

from conftest import ROOT
import occupancy_cases as oc
import vanilla_march_cases as vc
from neo360_amd import _lib, marching, models

GRIDS = (8, 32, 256)
STOPPING = tuple(c for c in vc.COUNTS if vc.n_level(c)[1] > vc.SEGMENT)


def _level0(counts, n):
    b = vc.rays(n)
    t0 = torch.linspace(0.0, 1.0, counts[0] + 1)
    t0 = vc.NEAR * (1.0 - t0) + vc.FAR * t0
    return b, t0[None, :].expand(n, -1).contiguous()


@pytest.mark.parametrize("G", GRIDS)
def test_fp32_and_fp64_box_keep_rules_agree_away_from_faces(G):
    grid = vc.mixed(G)
    seen_in = seen_out = 0
    for box in (vc.BOX, vc.SMALL):
        for counts in vc.COUNTS:
            b, t0 = _level0(counts, 257)
            o, d = b["rays_o"], b["viewdirs"]
            face = vc.near_face_box(box, o, d, t0, G)
            assert int(face.sum()) <= 0.01 * face.numel(), (G, box, counts, int(face.sum()))
            for clip in (False, True):
                k32 = vc.keep_rule_box(grid, box, o, d, t0, clip, torch.float32)
                k64 = vc.keep_rule_box(grid, box, o, d, t0, clip, torch.float64)
                assert k32.dtype == torch.bool and tuple(k32.shape) == tuple(t0.shape)
                assert torch.equal(k32[~face], k64[~face]), (G, box, counts, clip)
            c = vc.cell_box(oc.positions(o, d, t0), box, G)
            inside = ((c >= 0) & (c < G)).all(dim=-1)
            seen_in += int(inside.sum())
            seen_out += int((~inside).sum())
            assert bool(vc.keep_rule_box(grid, box, o, d, t0, False)[~inside].all()), "outside without clip: kept"
            assert not bool(vc.keep_rule_box(grid, box, o, d, t0, True)[~inside].any()), "outside with clip: skipped"
    assert seen_in > 1000 and seen_out > 1000, "the boxes hold samples and lose samples"


def test_box_cells_outside_rule_and_non_finite_positions():
    box = ((-1.0, 0.0, 2.0), (1.0, 4.0, 3.0))
    x = torch.tensor([[-1.0, 0.0, 2.0], [0.999, 3.999, 2.999], [1.0, 1.0, 2.5], [0.0, -0.001, 2.5], [0.0, 1.0, 3.0], [-0.75, 0.5, 2.125]])
    assert vc.cell_box(x, box, 8).tolist() == [[0, 0, 0], [7, 7, 7], [8, 2, 4], [4, -1, 4], [4, 2, 8], [1, 1, 1]]
    grid = oc.zeros(8)
    grid[1, 1, 1] = grid[0, 0, 0] = True
    zero = torch.zeros(6, 3)
    t = torch.zeros(6, 1)
    assert vc.keep_rule_box(grid, box, x, zero, t, False).reshape(-1).tolist() == [True, False, True, True, True, True]
    assert vc.keep_rule_box(grid, box, x, zero, t, True).reshape(-1).tolist() == [True, False, False, False, False, True]
    assert bool(vc.keep_rule_box(None, None, x, zero, t, True).all()), "no grid keeps everything"
    wild = torch.tensor([[float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0], [50.0, 50.0, 50.0]])
    got = vc.keep_rule_box(oc.zeros(8), box, wild, torch.zeros(3, 3), torch.zeros(3, 1), True).reshape(-1).tolist()
    assert got == [True, True, False], "a non-finite coordinate is kept even with clip; a finite far point is outside"
    assert not bool(vc.keep_rule_box(oc.ones(8), vc.FAR_AWAY, *[vc.rays(65)[k] for k in ("rays_o", "viewdirs")],
                                     _level0((64, 128), 65)[1], True).any()), "FAR_AWAY holds no sample"


@pytest.mark.parametrize("counts", STOPPING, ids=lambda c: "%d+%d" % c)
def test_the_inputs_mix_stopped_and_never_stopped_rays(counts):
    N1 = vc.n_level(counts)[1]
    for n in vc.RAYS:
        if n < 63 or (counts == (64, 128) and n > 65):
            continue
        _, _, extra = vc.oracle_frames(counts, n)
        stop = extra[1]["stop"]
        assert bool((extra[0]["stop"] == vc.n_level(counts)[0]).all()), "level 0 does not follow the rule without coarse"
        stopped, never = int((stop < N1).sum()), int((stop == N1).sum())
        print("%s, %d rays: %d stop before N1 = %d, %d never stop" % (counts, n, stopped, N1, never))
        assert 4 * stopped >= n and 4 * never >= n, (counts, n, stopped, never)
        assert set(stop.tolist()) <= set(range(64, N1, 64)) | {N1}
        # the fp32 and the fp64 statement of the rule agree outside the rays within tc.NEAR_TOL * eps of a boundary
        stop64, _ = vc.stops(extra[1]["T64"], vc.EPS, vc.SEGMENT)
        near = vc.near_threshold(extra[1]["T64"], vc.EPS, vc.SEGMENT)
        assert torch.equal(stop[~near], stop64[~near]) and int(near.sum()) <= max(1, n // 50)


def test_zero_rows_leave_the_product_alone_and_a_nan_marches_on():
    t = torch.linspace(0.2, 3.0, 130)[None, :].expand(3, -1).contiguous()
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 2.0, 0.0], [1.0, 1.0, 1.0]])
    sigma = torch.zeros(3, 130)
    T = vc.transmittance0(sigma, t, d)
    assert bool((T == 1).all()), "alpha(0 * delta) = 0, also for the last delta 1e10, and 1.0f + 1e-10f == 1.0f"
    sigma[0, 5] = float("nan")
    sigma[1, :] = 50.0
    stop, trans = vc.stops(vc.transmittance0(sigma, t, d), 0.5, 64)
    assert stop.tolist() == [130, 64, 130] and bool(torch.isnan(trans[0])) and float(trans[2]) == 1.0
    # |rays_d| scales every interval: twice the norm, the square of the transmittance (up to the 1e-10 terms)
    s1 = torch.full((1, 130), 0.7)
    T1 = vc.transmittance0(s1, t[:1], torch.tensor([[0.0, 0.0, 1.0]]), torch.float64)
    T2 = vc.transmittance0(s1, t[:1], torch.tensor([[0.0, 2.0, 0.0]]), torch.float64)
    assert torch.allclose(T2[:, :-1], T1[:, :-1] ** 2, rtol=1e-6)


@pytest.mark.parametrize("white", (False, True), ids=("black", "white"))
@pytest.mark.parametrize("counts", STOPPING, ids=lambda c: "%d+%d" % c)
def test_the_bound_holds_on_the_oracle(counts, white):
    """include/neo360_hip.h, VANILLA MARCHING FRAME, BOUND: against the same frame at eps = 0 with the same grid, level 1."""
    n = 65 if counts == (64, 128) else 257
    N1 = vc.n_level(counts)[1]
    seen = 0
    for eps in (1e-2, 1e-3):
        for occ in (None, vc.mixed(32)):
            plain, got, extra = vc.oracle_frames(counts, n, eps, occ=occ, box=vc.BOX if occ is not None else None, white_bkgd=white)
            stop = extra[1]["stop"]
            stopped = stop < N1
            trans = vc.stops(extra[1]["T"], eps, vc.SEGMENT)[1]
            for i in range(3):
                assert torch.equal(got[0][i], plain[0][i]), "level 0 is identical"
                assert torch.equal(got[1][i][~stopped], plain[1][i][~stopped]), "a ray that never stops is unchanged"
            if not bool(stopped.any()):
                continue
            seen += int(stopped.sum())
            assert bool((trans[stopped] < eps).all())
            d_rgb = (got[1][0] - plain[1][0]).abs().max(dim=-1).values
            d_depth = (got[1][2] - plain[1][2]).abs()
            print("%s eps %g grid %s white %s: %d stopped, max |rgb change| / trans %.4f, max |depth change| / (far trans) %.4f"
                  % (counts, eps, occ is not None, white, int(stopped.sum()), float((d_rgb / trans)[stopped].max()),
                     float((d_depth / (vc.FAR * trans))[stopped].max())))
            assert bool((d_rgb[stopped] <= 1.003 * trans[stopped]).all())
            assert bool((d_depth[stopped] <= 1.001 * vc.FAR * trans[stopped]).all())
    assert seen > 0


def _header():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(bare, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
    assert m, "%s is not declared in include/neo360_hip.h" % name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_header_declares_and_ctypes_binds_the_entry_points():
    text, bare = _header()
    for name in ("neo_vanilla_mlp_compact", "neo_vanilla_set_occupancy", "neo_vanilla_set_march_window", "neo_vanilla_occupancy_keep",
                 "neo_occupancy_from_sigma_box", "neo_vanilla_termination_stops", "neo_vanilla_render_marching"):
        assert len(_lib.SIGNATURES[name][1]) == len(_params(bare, name)), name
        assert hasattr(_lib.load(), name)
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*neo_vanilla_march_samples\s*;", bare)
    fields = [f.split("*")[-1].strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in _lib.VanillaMarchSamples._fields_] == ["t", "w", "keep", "stop", "rows"]
    assert _lib.SIGNATURES["neo_vanilla_render_marching"][1][:10] == _lib.SIGNATURES["neo_vanilla_render"][1][:10]
    assert _lib.load().neo_abi_version() == 1
    for phrase in ("VANILLA MARCHING FRAME", "BOX KEEP RULE", "MODE-0 STOP RULE", "1.003", "1 - c"):
        assert phrase in text, phrase


def test_the_module_is_a_nerf_with_the_same_state_and_validates_on_the_host():
    net = marching.MarchingNeRF(num_coarse_samples=7, num_fine_samples=64)
    plain = models.NeRF(num_coarse_samples=7, num_fine_samples=64)
    assert list(net.state_dict().keys()) == list(plain.state_dict().keys())
    net.load_state_dict(vc.state((7, 64)))
    assert net.occupancy is None and net.occupancy_box is None and net.last_march_kept is None
    good = oc.ones(8)
    for bad in (good.float(), good.to(torch.uint8), good[0], good[:, :, :4], torch.ones(24, 24, 24, dtype=torch.bool), [[[True]]], "grid"):
        with pytest.raises(ValueError):
            net.set_occupancy(bad, vc.BOX)
    for bad in (None, ((0, 0, 0),), ((0, 0), (1, 1)), ((0, 0, 0), (1, 1, 0)), ((0, 0, 0), (1, float("inf"), 1)),
                ((0, float("nan"), 0), (1, 1, 1)), ((1, 1, 1), (0, 0, 0)), "box", ((0, 0, "a"), (1, 1, 1))):
        with pytest.raises(ValueError):
            net.set_occupancy(good, bad)
        with pytest.raises(ValueError):
            net.build_occupancy(bad, 8, 0.5)
    for kw in (dict(resolution=12), dict(probes=0), dict(probes=5), dict(dilate=-1), dict(dilate=5), dict(sigma_threshold=float("nan")),
               dict(sigma_threshold="x")):
        args = dict(resolution=8, sigma_threshold=0.5, probes=2, dilate=1)
        args.update(kw)
        with pytest.raises(ValueError):
            net.build_occupancy(vc.BOX, **args)
    b = vc.rays(5)
    for eps in (-0.1, 1.0, float("nan"), "x", True):
        with pytest.raises(ValueError):
            net.render_marching(b, eps, False, vc.NEAR, vc.FAR)
        with pytest.raises(ValueError):
            marching.render_marching_rays(net, b, eps)
    for segment in (0, 32, 65, -64, 64.0):
        with pytest.raises(ValueError):
            net.render_marching(b, 0.1, False, vc.NEAR, vc.FAR, segment=segment)
    with pytest.raises(ValueError):
        marching.render_marching_rays(net, b, 0.1, chunk=0)
    with pytest.raises(TypeError):
        marching.render_marching_rays(plain, b, 0.1)
    # CPU tensors are refused by name, shapes and dtypes before any device is touched
    o, d, t = b["rays_o"], b["viewdirs"], torch.zeros(5, 4)
    with pytest.raises(ValueError, match="rays_o is on cpu"):
        net.render_marching(b, 0.1, False, vc.NEAR, vc.FAR)
    with pytest.raises(ValueError, match="rays_o is on cpu"):
        marching.occupancy_keep_box(good, vc.BOX, o, d, t)
    with pytest.raises(ValueError, match="rays_o must have shape"):
        marching.occupancy_keep_box(good, vc.BOX, o[:, :2], d, t)
    with pytest.raises(ValueError, match="rays_o must be a floating-point"):
        marching.occupancy_keep_box(good, vc.BOX, o.long(), d, t)
    with pytest.raises(ValueError):
        marching.occupancy_keep_box(good, None, o, d, t)
    with pytest.raises(ValueError, match="t is on cpu"):
        marching.termination_stops_vanilla(torch.zeros(5, 4, 4), t, d, 0.1)
    with pytest.raises(ValueError):
        marching.termination_stops_vanilla(torch.zeros(5, 4, 4), t, d, 1.5)
    with pytest.raises(ValueError, match="sigma must have shape"):
        marching.occupancy_from_sigma_box(torch.zeros(8, 8, 8), 8, 0.5)
    with pytest.raises(ValueError, match="rays_o is on cpu"):
        marching.eval_points(net, 0, o, d, t[:, 0], torch.zeros((), dtype=torch.int32))
    with pytest.raises(ValueError):
        marching.eval_points(net, 2, o, d, t[:, 0], torch.zeros((), dtype=torch.int32))
    with pytest.raises(TypeError):
        marching.eval_points("net", 0, o, d, t[:, 0], torch.zeros((), dtype=torch.int32))
    c, lo, ld = marching.occupancy_lattice_box(vc.BOX, 8, 2)
    assert tuple(c.shape) == (16,) and tuple(lo.shape) == tuple(ld.shape) == (256, 3)
    assert abs(float(c[0]) - (vc.BOX[0][2] + 0.5 * (vc.BOX[1][2] - vc.BOX[0][2]) / 16)) < 1e-6 and bool((lo[:, 2] == 0).all())
