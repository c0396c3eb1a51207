"""CPU: the conditions on the inputs of the PixelNeRF marching-frame tests (tests/pix_march_cases.py), asserted on the oracle alone,
the oracle's direction tiling, the host-side validation of the new module and its ABI declarations.  Nothing here needs a device."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
import cases
import occupancy_cases as oc
import pix_march_cases as pc
from neo360_amd import _lib, marching, models

_C2CTYPES = (
    (r"^(const\s+)?neo_vanilla_march_samples\s*\*$", ctypes.POINTER(_lib.VanillaMarchSamples)),
    (r"^const\s+float\s*\*$", None),        # a device pointer (c_void_p) or a host table (POINTER(c_float)): decided by name below
    (r"^.*\*$", ctypes.c_void_p),
    (r"^int$", ctypes.c_int),
    (r"^float$", ctypes.c_float),
)
_HOST_FLOAT_TABLES = ("lo", "hi", "src_poses")


def _header():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(bare, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
    assert m, "%s is not declared in include/neo360_hip.h" % name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        mm = re.match(r"^(.*?)(\w+)$", p)
        out.append((mm.group(1).strip(), mm.group(2)))
    return out


def _ctype(ctype, name):
    for pattern, t in _C2CTYPES:
        if re.match(pattern, ctype):
            if t is None:
                return ctypes.POINTER(ctypes.c_float) if name in _HOST_FLOAT_TABLES else ctypes.c_void_p
            return t
    raise AssertionError("no ctypes type for %r" % ctype)


def test_header_and_ctypes_table_agree_parameter_for_parameter():
    text, bare = _header()
    for name in ("neo_pix_set_occupancy", "neo_pix_set_march_window", "neo_pix_mlp_compact", "neo_pix_render_marching"):
        restype, argtypes = _lib.SIGNATURES[name]
        params = _params(bare, name)
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for i, ((ctype, pname), got) in enumerate(zip(params, argtypes)):
            assert got is _ctype(ctype, pname) or (got.__name__ == _ctype(ctype, pname).__name__), (name, i, ctype, pname, got)
        assert hasattr(_lib.load(), name), name
    sig = _lib.SIGNATURES
    assert sig["neo_pix_render_marching"][1][:16] == sig["neo_pix_render"][1][:16], "neo_pix_render's arguments come first"
    assert sig["neo_pix_render_marching"][1][16:] == sig["neo_vanilla_render_marching"][1][10:], "then eps .. kept as in the vanilla frame"
    assert sig["neo_pix_set_occupancy"] == sig["neo_vanilla_set_occupancy"] and sig["neo_pix_set_march_window"] == sig["neo_vanilla_set_march_window"]
    assert [n for _, n in _params(bare, "neo_pix_mlp_compact")][:8] == ["ctx", "slot", "rays_o", "rays_d", "viewdirs", "t", "cap", "count_dev"]
    assert _lib.load().neo_abi_version() == 1
    for phrase in ("PIXELNERF MARCHING FRAME", "quirk-Q1", "1.003", "1.001"):
        assert phrase in text, phrase


def test_the_module_is_a_pixelnerf_with_the_same_state_and_validates_on_the_host():
    net = marching.MarchingPixelNeRF(num_coarse_samples=7, num_fine_samples=64, num_src_views=cases.NV)
    plain = models.PixelNeRF(num_coarse_samples=7, num_fine_samples=64, num_src_views=cases.NV)
    assert list(net.state_dict().keys()) == list(plain.state_dict().keys())
    net.load_state_dict(pc.state((7, 64)))
    assert net.occupancy is None and net.occupancy_box is None and net.last_march_kept is None and net.march_window is None
    assert type(net).forward is models.PixelNeRF.forward and type(net).eval_mlp is models.PixelNeRF.eval_mlp
    b = pc.rays(5)
    good = oc.ones(8)
    for bad in (good.float(), good.to(torch.uint8), good[0], good[:, :, :4], torch.ones(24, 24, 24, dtype=torch.bool), [[[True]]], "grid"):
        with pytest.raises(ValueError):
            net.set_occupancy(bad, pc.BOX)
    for bad in (None, ((0, 0, 0),), ((0, 0), (1, 1)), ((0, 0, 0), (1, 1, 0)), ((0, 0, 0), (1, float("inf"), 1)),
                ((0, float("nan"), 0), (1, 1, 1)), ((1, 1, 1), (0, 0, 0)), "box", ((0, 0, "a"), (1, 1, 1))):
        with pytest.raises(ValueError):
            net.set_occupancy(good, bad)
        with pytest.raises(ValueError):
            net.build_occupancy(b, bad, 8, 0.5)
    for kw in (dict(resolution=12), dict(probes=0), dict(probes=5), dict(dilate=-1), dict(dilate=5), dict(sigma_threshold=float("nan")),
               dict(sigma_threshold="x")):
        args = dict(resolution=8, sigma_threshold=0.5, probes=2, dilate=1)
        args.update(kw)
        with pytest.raises(ValueError):
            net.build_occupancy(b, pc.BOX, **args)
    for eps in (-0.1, 1.0, float("nan"), "x", True):
        with pytest.raises(ValueError):
            net.render_marching(b, eps, False, pc.NEAR, pc.FAR)
        with pytest.raises(ValueError):
            marching.render_marching_rays(net, b, eps)
    for segment in (0, 32, 65, -64, 64.0):
        with pytest.raises(ValueError):
            net.render_marching(b, 0.1, False, pc.NEAR, pc.FAR, segment=segment)
    for chunk in (0, -3, 2.0, True):
        with pytest.raises(ValueError):
            net.render_marching(b, 0.1, False, pc.NEAR, pc.FAR, chunk=chunk)
        with pytest.raises(ValueError):
            marching.render_marching_rays(net, b, 0.1, chunk=chunk)
    for other in (plain, models.NeRF(), "net"):
        with pytest.raises(TypeError):
            marching.render_marching_rays(other, b, 0.1)
    # CPU tensors are refused by name, shapes and dtypes before any device is touched
    with pytest.raises(ValueError, match="rays_o is on cpu"):
        net.render_marching(b, 0.1, False, pc.NEAR, pc.FAR)
    with pytest.raises(ValueError, match="rays_d must have shape"):
        marching.render_marching_rays(net, dict(b, rays_d=b["rays_d"][:, :2]), 0.1)
    with pytest.raises(ValueError, match="viewdirs must be a floating-point"):
        marching.render_marching_rays(net, dict(b, viewdirs=b["viewdirs"].long()), 0.1)
    t, count = torch.zeros(5), torch.zeros((), dtype=torch.int32)
    with pytest.raises(ValueError, match="rays_o is on cpu"):
        marching.eval_points_pix(net, 0, b, t, count)
    with pytest.raises(ValueError):
        marching.eval_points_pix(net, 2, b, t, count)
    with pytest.raises(TypeError):
        marching.eval_points_pix(models.NeRF(), 0, b, t, count)
    with pytest.raises(TypeError):
        marching.eval_points_pix("net", 0, b, t, count)


@pytest.mark.parametrize("counts", pc.STOPPING, ids=lambda c: "%d+%d" % c)
def test_the_inputs_mix_stopped_and_never_stopped_rays(counts):
    """Condition (a): at eps = 1e-2, for every R >= 63, at least a quarter of the rays stop before N1 and at least a quarter never
    stop - on the unmasked oracle frame, or, for the pair that has no robust bias there (63 + 64), on the frame masked by the mixed
    grid of pc.STOP_GRID, whose zero rows spread the rays' transmittances."""
    N = pc.n_level(counts)
    arm = pc.STOP_GRID[counts]
    for n in pc.RAYS:
        if n < 63:
            continue
        _, extra = pc.oracle_frame(counts, n) if arm is None else pc.oracle_frame(counts, n, pc.EPS, *arm)
        stop = extra[1]["stop"]
        assert bool((extra[0]["stop"] == N[0]).all()), "level 0 does not follow the rule without coarse"
        stopped, never = int((stop < N[1]).sum()), int((stop == N[1]).sum())
        print("%s, %d rays: %d stop before N1 = %d, %d never stop" % (counts, n, stopped, N[1], never))
        assert 4 * stopped >= n and 4 * never >= n, (counts, n, stopped, never)
        assert set(stop.tolist()) <= set(range(64, N[1], 64)) | {N[1]}
        # the fp32 and the fp64 statement of the rule agree outside the rays within the restatement's tolerance of a boundary
        stop64, _ = pc.stops(extra[1]["T64"], pc.EPS, pc.SEGMENT)
        near = pc.vc.near_threshold(extra[1]["T64"], pc.EPS, pc.SEGMENT)
        assert torch.equal(stop[~near], stop64[~near]) and int(near.sum()) <= max(1, n // 50)


@pytest.mark.parametrize("G", (8, 32))
@pytest.mark.parametrize("counts", pc.COUNTS, ids=lambda c: "%d+%d" % c)
def test_the_mixed_grid_keeps_and_skips_at_both_levels_of_the_masked_frame(counts, G):
    """Condition (b): BOX, mixed(G), clip=True - at each level of the MASKED oracle frame at least 15 % of the samples are kept and
    at least 5 % are skipped."""
    for n in (65, 257):
        _, extra = pc.oracle_frame(counts, n, pc.EPS, G)
        for lv in range(2):
            share = float(extra[lv]["keep"].float().mean())
            print("%s G %d, %d rays, level %d: %.3f of the samples kept" % (counts, G, n, lv, share))
            assert 0.15 <= share <= 0.95, (counts, G, n, lv, share)
            assert bool((extra[lv]["rows"][~extra[lv]["keep"]] == 0).all())


@pytest.mark.parametrize("chunk", (None, 64))
def test_the_oracles_direction_of_a_masked_row_is_the_dense_rows(chunk):
    """A row of the masked frame is the DENSE launch's row: evaluated on its own, as one point that is its own ray and carries the
    direction pc.q1_index names (what the compact launch is given), it reproduces the row of the dense evaluation bit for bit - so
    zeroing rows AFTER the dense evaluation (pc.oracle_render_marching) and evaluating only the kept ones agree."""
    counts = (7, 64)
    n, N = 65, 8
    b = pc.rays(n)
    params = pc.state(counts)
    t, _ = pc.oracle.sampling.vanilla_level0(b["rays_o"], b["rays_d"], counts[0], pc.NEAR, pc.FAR)
    dense = torch.cat([pc.oracle_rows(params, "coarse_mlp.", pc.part(b, i, i + (chunk or n)), t[i:i + (chunk or n)])
                       for i in range(0, n, chunk or n)])
    q1 = pc.q1_index(n, N, chunk)
    assert q1.min() >= 0 and q1.max() < n and not torch.equal(q1, torch.arange(n)[:, None].expand(n, N))
    if chunk:
        assert int(q1[64].min()) == 64 == int(q1[64].max()), "a chunk of one ray sees its own direction"
        assert int(q1[:64].max()) == 63
    keep = pc.keep_rule_box(pc.mixed(8), pc.BOX, b["rays_o"], b["rays_d"], t, True)
    bs, js = torch.nonzero(keep, as_tuple=True)
    assert 0 < bs.numel() < keep.numel()
    points = dict(b, rays_o=b["rays_o"][bs], rays_d=b["rays_d"][bs], viewdirs=b["viewdirs"][q1[bs, js]])
    alone = pc.oracle_rows(params, "coarse_mlp.", points, t[bs, js][:, None])[:, 0]
    assert torch.allclose(alone, dense[bs, js], rtol=0, atol=1e-6), float((alone - dense[bs, js]).abs().max())
    wrong = dict(points, viewdirs=b["viewdirs"][bs])
    off = pc.oracle_rows(params, "coarse_mlp.", wrong, t[bs, js][:, None])[:, 0]
    assert float((off[:, :3] - dense[bs, js][:, :3]).abs().max()) > 1e-4, "the ray's own direction is another colour"
    assert torch.allclose(off[:, 3], dense[bs, js][:, 3], rtol=0, atol=1e-6), "and the same density"
