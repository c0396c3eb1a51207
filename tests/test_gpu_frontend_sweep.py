"""GPU: the kernels that make the evaluators' inputs - ray generation, the three slab tests, the sphere exit, the level-0 samplers,
neo_tp_train_points, neo_mip_encode, the activation op with its backward, and the grid-stride loops - against fp64 truths, case by
case of tests/frontend_cases.py: ray and point counts on the edges of a block, designed degenerate rows, bounds per entry (the
table's conditions are checked on the CPU by test_frontend_cases_cpu.py).  The slab tests are bit for bit against an exact-FMA
restatement of the kernels' box-frame transform, which is row-independent where numpy's own product is not.  Every case lands in
the parity report under frontend_sweep/<kernel>/<case>."""
import numpy as np
import pytest
import torch

import cases
import frontend_cases as F
from conftest import record_parity
from neo360_amd import ops, training
from neo360_amd.context import get_context
from oracle import mip360
from oracle import training as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _record(kernel, case, checks):
    record_parity("frontend_sweep/%s/%s" % (kernel, case), **F.summarize(checks))
    F.assert_inside(checks, (kernel, case))


def _exact(kernel, case, **counts):
    """A bit-for-bit case: what was compared, for the report."""
    record_parity("frontend_sweep/%s/%s" % (kernel, case), bit_for_bit=True, **counts)


def _flags():
    return get_context(torch.device(DEV)).poll_flags()


# ---- 1. ray generation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", F.RAYGEN_FRAMES)
def test_raygen_frames(H, W):
    """Frames down to the radii rule's minimum (H = 3), one column, ray counts around a block of 256; a long lens; the identity
    rotation and a translation of 1e3.  Origins exact, directions and radii per entry."""
    for fx in F.RAYGEN_FOCALS:
        for pi in range(5):
            focal, pose, ref64, ref32 = F.raygen_case(H, W, fx, pi)
            ro, vd, rd, rad = ops.get_ray_directions_and_rays(H, W, focal, pose)
            assert ro.shape == (H * W, 3) and rad.shape == (H * W,)
            got = dict(rays_o=ro.cpu(), viewdirs=vd.cpu(), rays_d=rd.cpu(), radii=rad.cpu())
            assert torch.equal(got["viewdirs"], got["rays_d"])
            _record("raygen", "%dx%d_f%gW_pose%d" % (H, W, fx, pi), F.raygen_checks(got, ref64, ref32))


def test_raygen_ranges_equal_the_full_frame():
    H, W = F.RAYGEN_RANGE_FRAME
    for fx in F.RAYGEN_FOCALS:
        focal, pose, _, _ = F.raygen_case(H, W, fx, 1)
        full = ops.get_ray_directions_and_rays(H, W, focal, pose)
        for lo, hi in F.RAYGEN_RANGES:
            part = ops.get_ray_directions_and_rays(H, W, focal, pose, ray_range=(lo, hi))
            for a, b in zip(part, full):
                assert a.shape[0] == hi - lo and torch.equal(a, b[lo:hi]), (fx, lo, hi)
        _exact("raygen", "%dx%d_f%gW_ranges" % (H, W, fx), ranges=len(F.RAYGEN_RANGES))


# ---- 2. slab tests -----------------------------------------------------------------------------------------------------------------
def _slab_rays(R):
    o, d = F.slab_rays()
    return torch.from_numpy(o[:R].copy()).to(DEV), torch.from_numpy(d[:R].copy()).to(DEV)


@pytest.mark.parametrize("n_boxes", sorted(F.SLAB_SETS))
def test_slab_box_sets_bit_for_bit(n_boxes):
    """neo_aabb_multi and neo_aabb_per_box on prefixes of the 513 designed + ordinary rays (1 ray .. two blocks and one) against the
    exact-FMA restatement: per-box hits, merged near / far / mask, every box's own near / far / hit; and each box's rows equal the
    merged call with that box alone."""
    names = F.SLAB_SETS[n_boxes]
    RTs = F.slab_rts(names)
    for R in F.SLAB_COUNTS:
        o, d = _slab_rays(R)
        tr = F.slab_truth(n_boxes, R)
        near, far, mask, per_box = ops.sample_rays_in_bbox(RTs, o, d, return_per_box=True)
        assert near.shape == far.shape == mask.shape == (R, 1) and per_box.shape == (n_boxes, R)
        assert torch.equal(near.cpu(), tr["near"]) and torch.equal(far.cpu(), tr["far"]) and torch.equal(mask.cpu(), tr["mask"]), (n_boxes, R)
        n2, f2, m2 = ops.sample_rays_in_bbox(RTs, o, d)
        assert torch.equal(n2, near) and torch.equal(f2, far) and torch.equal(m2, mask)
        ln, lf, lh = ops.sample_rays_in_bbox_list(RTs, o, d)
        assert ln.shape == lf.shape == (n_boxes, R, 1) and lh.shape == (n_boxes, R)
        for b, name in enumerate(names):
            p = tr["per_box"][b]
            assert torch.equal(per_box[b].cpu().bool(), p["hit_mask"]), (n_boxes, R, name)
            assert torch.equal(lh[b].cpu(), p["hit_mask"]) and torch.equal(ln[b].cpu(), p["near"]) and torch.equal(lf[b].cpu(), p["far"]), (n_boxes, R, name)
            alone = ops.sample_rays_in_bbox(F.slab_rts((name,)), o, d)
            assert torch.equal(alone[0], ln[b]) and torch.equal(alone[1], lf[b]), (n_boxes, R, name)
            # the merge calls near == 0.0f "no hit": the face-origin ray is hit by the slab test and masked out by the merge
            assert torch.equal(alone[2].cpu(), (p["near"] != 0) & (p["far"] != 0))
        _exact("slab", "boxes%d_R%d" % (n_boxes, R), boxes=n_boxes, rays=R, hits=int(tr["mask"].sum()))


def test_slab_single_box_entry_on_pretransformed_rays():
    """neo_aabb_intersect on the restatement's box-frame rays: fp64 tmin, tmax and the hit of every pool box, bit for bit."""
    for name, (_, _, s) in F.slab_pool().items():
        tr = F.slab_box_truth(name)
        for R in F.SLAB_COUNTS:
            hit, tmin, tmax = ops.bbox_intersection_batch(s, torch.from_numpy(tr["o"][:R].copy()).to(DEV), torch.from_numpy(tr["d"][:R].copy()).to(DEV))
            assert np.array_equal(hit.cpu().numpy().astype(np.float64), tr["hit"][:R]), (name, R)
            assert np.array_equal(tmin.cpu().numpy(), tr["tmin"][:R]) and np.array_equal(tmax.cpu().numpy(), tr["tmax"][:R]), (name, R)
        _exact("slab", "single_box_%s" % name, rays=F.SLAB_RAYS, hits=int(tr["hit"].sum()))


# ---- 3. sphere exit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", F.SPHERE_SCALES)
def test_sphere_exit(scale):
    """Mask exact against fp64, NaN where the oracle's formula is NaN, far per entry; direction lengths 1e-3 .. 1e3."""
    for R in F.SPHERE_COUNTS:
        for misses in (True, False):
            (o, d), ref64, ref32 = F.sphere_case(R, scale, misses)
            far, ok = ops.intersect_sphere(o.to(DEV), d.to(DEV), check=False)
            flagged = bool(_flags() & 1)                              # read and cleared: nothing is left behind for the next call
            assert flagged == bool((~ref64[1]).any()), (R, scale, misses)
            assert far.shape == (R, 1) and ok.shape == (R,)
            _record("sphere", "R%d_len%g_%s" % (R, scale, "misses" if misses else "clean"), F.sphere_checks(far, ok, ref64, ref32))


def test_sphere_check_raises_if_and_only_if_the_call_holds_a_miss():
    for R in F.SPHERE_COUNTS:
        (o, d), ref64, _ = F.sphere_case(R, 1.3, True)
        if bool((~ref64[1]).any()):
            with pytest.raises(AssertionError):
                ops.intersect_sphere(o.to(DEV), d.to(DEV))
        else:
            ops.intersect_sphere(o.to(DEV), d.to(DEV))
        (o, d), _, _ = F.sphere_case(R, 1.3, False)
        _, ok = ops.intersect_sphere(o.to(DEV), d.to(DEV))           # the next clean call does not raise
        assert bool(ok.all())


# ---- 4. level-0 rows ---------------------------------------------------------------------------------------------------------------
def _level0(R, n, randomized):
    far, u, ref64, ref32 = F.level0_case(R, n, randomized)
    if not randomized:
        fg, bg = training.sample_level0(far.to(DEV), n)
    else:
        drawn = [training.rand_uniform(F.L0_SEED + n, s, R, n + 1) for s in F.L0_STREAMS]
        for a, s in zip(drawn, F.L0_STREAMS):
            assert torch.equal(a.cpu(), T.philox_uniform(F.L0_SEED + n, s, R, n + 1)), ("rand_uniform is not philox_uniform", R, n, s)
        u_fg, u_bg = (F.level0_designed_draws(a.cpu()).to(DEV) for a in drawn)
        assert torch.equal(u_fg.cpu(), u[0]) and torch.equal(u_bg.cpu(), u[1])
        fg, bg = training.sample_level0(far.to(DEV), n, u_fg, u_bg)
    assert fg.shape == bg.shape == (R, n + 1)
    return far, fg.cpu(), bg.cpu(), ref64, ref32


@pytest.mark.parametrize("n", F.L0_N)
def test_level0_rows(n):
    """Both forms at the entry's limits (3, 1023) and around a 64-wide round, 1 / 5 / 257 rays, a constant row (far == near), the
    draws u = 0 and u = 1 - 2^-24."""
    for R in F.L0_R:
        for randomized in (False, True):
            far, fg, bg, ref64, ref32 = _level0(R, n, randomized)
            if randomized:
                order = F.level0_order(fg, bg, far)
                assert all(order.values()), (R, n, order)
            else:
                assert bool((bg == bg[:1]).all()), "the deterministic outside row differs between rays"
            _record("level0_rand" if randomized else "level0", "n%d_R%d" % (n, R), F.level0_checks(fg, bg, far, ref64, ref32))


# ---- 5. train_points ---------------------------------------------------------------------------------------------------------------
def _points(region, inp, rows=None):
    o, d, t, far, poses = inp
    cut = (lambda x: x[:rows].contiguous()) if rows is not None else (lambda x: x)
    look, x = training.train_points(None, region, cut(o).to(DEV), cut(d).to(DEV), cut(t).to(DEV), cut(far).to(DEV) if region else None,
                                    poses.to(DEV))
    return look.cpu(), x.cpu()


@pytest.mark.parametrize("region", [0, 1])
def test_train_points(region):
    """Lookup points and per-view encodings, entry by entry: P = 1 .. 1584 points (one partial block of 64 .. 24 full and a partial
    one), one and three views, a row from t = 0 to t = far inside, s from 1 to 0 and a near-radial ray outside; every octave held to
    its own bound instead of octave 9's."""
    for R, N in F.POINT_SHAPES:
        for NV in F.POINT_NV:
            inp, ref64, ref32 = F.point_case(region, R, N, NV)
            look, x = _points(region, inp)
            assert look.shape == (R * N, 3) and x.shape == (NV, R * N, 84 if region else 63)
            _record("train_points", "region%d_R%d_N%d_NV%d" % (region, R, N, NV), F.point_checks(region, look, x, ref64, ref32))
    assert (_flags() & 1) == 0


@pytest.mark.parametrize("region", [0, 1])
def test_train_points_rows_do_not_depend_on_the_ray_count(region):
    R, N = F.POINT_SHAPES[-1]
    inp, _, _ = F.point_case(region, R, N, cases.NV)
    look, x = _points(region, inp)
    for r in (1, 3, 5):
        pl, px = _points(region, inp, rows=r)
        assert torch.equal(pl, look[:r * N]) and torch.equal(px, x[:, :r * N]), (region, r)
    _exact("train_points", "region%d_row_independence" % region, ray_counts=3)


def test_train_points_radial_ray_and_missing_ray():
    """An exactly radial ray (alone in its call): the reference's rotation axis is 0 / 0, the three spatial coordinates are NaN, the
    inverse radius and the lookup point are finite - the oracle's pattern.  A ray that misses the sphere raises flag bit 1."""
    o, d, s, far = F.radial_inputs()
    poses = F.point_case(1, 1, 1, cases.NV)[0][4]
    look, x = _points(1, (o, d, s, far, poses))
    ref64, ref32 = (F.points_oracle(1, o, d, s, far, poses, dt) for dt in (torch.float64, torch.float32))
    assert bool(torch.isfinite(look).all()) and F.radial_nan_pattern(x) and F.radial_nan_pattern(ref64[1])
    _record("train_points", "region1_radial_ray", F.radial_checks(look, x, ref64, ref32))
    assert (_flags() & 1) == 0                                          # NaN coordinates are not a missed sphere
    o = torch.tensor([[0.0, 0.0, 3.0]])
    _points(1, (o, torch.tensor([[1.0, 0.0, 0.0]]), s, far, poses))
    assert (_flags() & 1) == 1
    assert (_flags() & 1) == 0


# ---- 6. mip_encode -----------------------------------------------------------------------------------------------------------------
def _mip_encode(R, n):
    (o, d, rad, t), ref64, ref32 = F.mip_case(R, n)
    got = training.mip_encode(o.to(DEV), d.to(DEV), rad.to(DEV), t.to(DEV), mip360.icosahedron_basis().to(DEV)).cpu()
    assert got.shape == (R * n, 504)
    return got, ref64, ref32


def test_mip_encode_rows():
    """P = 1 .. 72 rows in blocks of 8 (the partial last block clamps its row and leaves the feature loop early); a zero-width
    interval, intervals from 0 to 1e6, means one ulp either side of the contraction's branch, radii 0 and 1, |d| 0.5 and 2.  The rule
    of test_encode_rows_match_the_oracle per (row, octave): 2e-6 + 2 x THAT row's fp32-vs-fp64 noise at THAT octave, and at most
    2e-5 on the first 63 features.

    What this found: with the row's Gaussian, its contraction and the lift onto the basis in fp32, 25 of the table's 2400
    (row, octave) pairs were over their bound, all at octaves 7 .. 11, the worst by 3.7 x (case (2, 33), row 8, octave 10: error
    3.9e-5, the oracle's own 4.3e-6, bound 1.07e-5).  Octave k multiplies the error of a lifted mean by 2^k; the kernel's means were
    as good as the fp32 oracle's (per octave its largest error was 0.80 .. 1.34 of the oracle's over a case), but one (row, octave)
    of the oracle is one sample of that rounding, and where the oracle's sample is small no other fp32 evaluation is inside twice
    it.  k_mip_encode now carries the row set-up and the arguments of the sine and the exponential in float64 (mip_train.hip:
    mip_row_gaussian, sin_of_double); every pair uses at most 0.05 of its bound (errors <= 1.2e-7 at every octave)."""
    for R, n in F.MIP_SHAPES:
        got, ref64, ref32 = _mip_encode(R, n)
        share, _, _ = F.mip_shares(got, ref64, ref32)
        record_parity("frontend_sweep/mip_encode/R%d_n%d" % (R, n), pairs=share.numel(), pairs_over=int((share > 1.0).sum()))
        _record("mip_encode", "R%d_n%d" % (R, n), F.mip_checks(got, ref64, ref32))


# ---- 7. activate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", F.ACT_P)
def test_activate_forward_and_backward(P):
    """Saturated colours (+-100), the density argument exactly at the softplus threshold 20 and one ulp either side, +-100 and 0;
    the noise given, absent, and scaled by 0; point counts around a block of 256."""
    for kind in F.ACT_NOISE:
        (raw_rgb, raw_sigma, noise, scale, up), ref64, ref32 = F.activate_case(P, kind)
        with torch.enable_grad():
            a, b = raw_rgb.to(DEV).requires_grad_(True), raw_sigma.to(DEV).requires_grad_(True)
            out = training.activate(a, b, noise.to(DEV) if noise is not None else None, scale)
            ga, gb = torch.autograd.grad((out * up.to(DEV)).sum(), [a, b])
        assert out.shape == (P, 4) and ga.shape == (P, 3) and gb.shape == (P, 1)
        got = dict(out=out.detach().cpu(), g_rgb=ga.cpu(), g_sigma=gb.cpu())
        _record("activate", "P%d_noise_%s" % (P, kind), F.activate_checks(got, ref64, ref32))


# ---- 8. the grid-stride loops ------------------------------------------------------------------------------------------------------
def test_pos_enc_grid_stride():
    """8193 blocks' worth of features on a grid capped at 8192: the second trip of k_pos_enc's loop."""
    x, ref64, ref32 = F.pos_enc_big_case()
    _record("pos_enc", "rows%d_grid_stride" % F.PE_BIG[0], F.pos_enc_checks(ops.pos_enc(x.to(DEV), 0, 10), ref64, ref32))


def test_rand_uniform_grid_stride():
    rows, cols = F.UNIFORM_BIG
    got = training.rand_uniform(F.UNIFORM_SEED, F.UNIFORM_STREAM, rows, cols).cpu()
    assert torch.equal(got, T.philox_uniform(F.UNIFORM_SEED, F.UNIFORM_STREAM, rows, cols))
    _exact("rand_uniform", "%dx%d_grid_stride" % (rows, cols), values=rows * cols)


def test_level0_grid_stride():
    R, n = F.L0_BIG
    for randomized in (False, True):
        far, fg, bg, ref64, ref32 = _level0(R, n, randomized)
        if randomized:
            assert all(F.level0_order(fg, bg, far).values())
        _record("level0_rand" if randomized else "level0", "n%d_R%d_grid_stride" % (n, R), F.level0_checks(fg, bg, far, ref64, ref32))
