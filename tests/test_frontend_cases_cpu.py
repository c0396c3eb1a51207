"""CPU: the case table of tests/frontend_cases.py is one on which the reference's own arithmetic passes.

For every case the GPU sweep (tests/test_gpu_frontend_sweep.py) runs: the fp64 truth is finite outside the stated NaN rows, the
fp32 oracle - the reference's arithmetic - stays inside the per-entry bounds with the fp64 truth as truth, the exact-FMA
restatement of the slab kernels' box-frame transform is tied to the oracle and to the golden, and the noise term of a bound
matters only where the table says it may."""
import numpy as np
import pytest
import torch

import cases
import frontend_cases as F
import oracle
from oracle import training as T


def _finite(*xs):
    return all(bool(torch.isfinite(v).all()) for x in xs for v in (x.values() if isinstance(x, dict) else x if isinstance(x, (tuple, list)) else [x]))


# ---- ray generation --------------------------------------------------------------------------------------------------------------------
def test_raygen_cases_fp32_oracle_inside_bounds():
    used = {}
    for H, W, fx, pi in F.raygen_table():
        focal, pose, ref64, ref32 = F.raygen_case(H, W, fx, pi)
        assert _finite(ref64, ref32) and ref64["radii"].shape == (H * W,), (H, W, fx, pi)
        checks = F.raygen_checks(ref32, ref64, ref32)
        F.oracle_inside(checks, ("raygen", H, W, fx, pi))
        # the noise term of the radii bound is what the cancellation of two fp32 directions gives: a few ulp of the largest
        # un-normalised direction component (3e-8 on the golden test's frames, where that component is below 1)
        cap = 4 * 1.2e-7 * max(1.0, max(H, W) / focal)
        assert float((ref32["radii"].double() - ref64["radii"]).abs().max()) < cap, (H, W, fx, pi)
        for k, v in checks.items():
            used[k] = max(used.get(k, 0.0), v["fp32_ratio"])
    print("raygen: largest share of a bound the fp32 oracle uses:", {k: "%.2f" % v for k, v in used.items()})


# ---- slab tests ------------------------------------------------------------------------------------------------------------------------
def test_slab_designed_rows_are_what_the_docstring_says():
    tr = {k: v for k, v in F.slab_box_truth("A").items()}
    hit, tmin, tmax = tr["hit"], tr["tmin"], tr["tmax"]
    assert hit[:6].tolist() == [1.0] * 6                                           # zero components, +0.0 and -0.0, each axis alone
    assert np.array_equal(tmin[0:6:2], tmin[1:6:2]) and np.array_equal(tmax[0:6:2], tmax[1:6:2])
    assert hit[6] == 0.0 and hit[8] == 0.0 and hit[10] == 0.0                      # inside, behind, parallel and outside
    assert hit[7] == 1.0 and tmin[7] == 0.0 and tmax[7] > 0.0                      # on the face: accepted, near rounds to the sentinel
    assert hit[9] == 1.0 and tmin[9] == tmax[9] == 0.75                            # the graze: lo == a_hi exactly
    assert hit[11] == 1.0 and tmin[11] == 0.75 and tmax[11] == 1.25                # corner to corner
    assert hit[12] == 1.0 and 0.9e6 < tmin[12] < tmax[12] < 1.1e6                  # the far origin
    assert float(F.slab_box_truth("miss")["hit"].sum()) == 0.0                     # a box no ray meets
    x, y = F.slab_box_truth("X"), F.slab_box_truth("Y")
    both = (x["hit"] > 0) & (y["hit"] > 0)
    assert int(both.sum()) > 50 and bool((y["tmin"][both] < x["tmin"][both]).all())   # the box listed second is the nearer one
    one = F.slab_truth(1, F.SLAB_RAYS)
    assert bool(one["per_box"][0]["hit_mask"][7]) and not bool(one["mask"][7])     # hit by the slab test, "no hit" for the merge
    for n in F.SLAB_SETS:
        m = F.slab_truth(n, F.SLAB_RAYS)
        assert bool(torch.isfinite(m["near"]).all() and torch.isfinite(m["far"]).all())
        assert 0 < int(m["mask"].sum()) < F.SLAB_RAYS or n == 1


def test_slab_restatement_is_the_oracle_on_the_513_ray_calls():
    o, d = F.slab_rays()
    for n, names in F.SLAB_SETS.items():
        near, far, mask, hits = oracle.rays.sample_rays_in_bbox(F.slab_rts(names), o, d)
        tr = F.slab_truth(n, F.SLAB_RAYS)
        assert torch.equal(near, tr["near"]) and torch.equal(far, tr["far"]) and torch.equal(mask, tr["mask"]), n
        for b, h in enumerate(hits):
            assert torch.equal(h, tr["per_box"][b]["hit_mask"]), (n, b)
    for name, (rot, tran, s) in F.slab_pool().items():
        tr = F.slab_box_truth(name)
        no, nd = oracle.rays.rays_to_box_frame(o, d, F.box_from_world(rot, tran))
        hit, tmin, tmax = oracle.rays.aabb_slab_batch(s, no, nd)
        assert np.array_equal(hit, tr["hit"]) and np.array_equal(tmin, tr["tmin"]) and np.array_equal(tmax, tr["tmax"]), name


def test_slab_restatement_is_the_golden_on_the_golden_inputs(golden):
    g = golden("g2_aabb")
    RTs, o, d = cases.oriented_box_cases()
    per = [F.slab_box_exact(o, d, r, t, s) for r, t, s in zip(RTs["R"], RTs["T"], RTs["s"])]
    for bi, p in enumerate(per):
        assert torch.equal(p["hit_mask"].to(torch.uint8), g["ob_hit%d" % bi]), bi
    near, far, mask = oracle.rays.merge_boxes([p["near"] for p in per], [p["far"] for p in per])
    assert torch.equal(near, g["ob_near"]) and torch.equal(far, g["ob_far"]) and torch.equal(mask.to(torch.uint8), g["ob_mask"])


def test_numpy_product_per_ray_count_is_recorded():
    """numpy's own product is row-dependent: which ray counts of the table it reproduces the exact-FMA order on is recorded (and
    printed for docs/frontend_sweep.md); the restatement is the truth either way.  The 513-ray call is asserted above."""
    rec = {R: F.numpy_product_agrees(R) for R in F.SLAB_COUNTS}
    print("numpy product == exact-FMA restatement, per ray count and box:", {R: [k for k, v in a.items() if not v] or "all" for R, a in rec.items()})
    assert all(rec[F.SLAB_RAYS].values())


# ---- sphere exit -----------------------------------------------------------------------------------------------------------------------
def test_sphere_cases_masks_agree_and_fp32_oracle_inside_bounds():
    used = 0.0
    for R in F.SPHERE_COUNTS:
        for scale in F.SPHERE_SCALES:
            for misses in (True, False):
                (o, d), ref64, ref32 = F.sphere_case(R, scale, misses)
                assert torch.equal(ref32[1], ref64[1]), (R, scale, "the fp32 oracle's mask is not the fp64 one: change the margins")
                want_miss = [i for i in F.SPHERE_MISS_ROWS if i < R] if misses else []
                assert (~ref64[1].reshape(-1)).nonzero().flatten().tolist() == want_miss, (R, scale)
                assert bool(torch.isfinite(ref64[0][ref64[1]]).all()) and bool(torch.isnan(ref64[0][~ref64[1]]).all())
                checks = F.sphere_checks(ref32[0], ref32[1], ref64, ref32)
                F.oracle_inside(checks, ("sphere", R, scale, misses))
                used = max(used, checks["far"]["fp32_ratio"])
                if not misses:                  # the local restatement IS the oracle where the oracle's assertion lets it run
                    far, ok = oracle.rays.sphere_exit_depth(o, d)
                    assert torch.equal(far, ref32[0]) and torch.equal(ok, ref32[1])
    print("sphere: largest share of the bound the fp32 oracle uses: %.2f" % used)


# ---- level-0 rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("randomized", [False, True])
def test_level0_cases_fp32_oracle_inside_bounds(randomized):
    used = {}
    for n in F.L0_N:
        for R in F.L0_R:
            far, u, ref64, ref32 = F.level0_case(R, n, randomized)
            assert _finite(ref64, ref32), (R, n)
            checks = F.level0_checks(ref32[0], ref32[1], far, ref64, ref32)
            F.oracle_inside(checks, ("level0", R, n, randomized))
            assert torch.equal(ref32[1][0], ref32[1][-1]) or randomized             # the deterministic outside row is the same for every ray
            order = F.level0_order(ref32[0], ref32[1], far)
            assert all(order.values()), (R, n, order)
            assert all(F.level0_order(ref64[0], ref64[1], far).values())
            if randomized and R >= 5:
                assert float(u[0][2].max()) == 0.0 and float(u[1][3].min()) == F.U_TOP
            for k, v in checks.items():
                used[k] = max(used.get(k, 0.0), v["fp32_ratio"])
    print("level0 randomized=%s: largest share of a bound the fp32 oracle uses:" % randomized, {k: "%.2f" % v for k, v in used.items()})


# ---- train_points ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", [0, 1])
def test_point_cases_fp32_oracle_inside_bounds(region):
    used = {}
    for R, N in F.POINT_SHAPES:
        for NV in F.POINT_NV:
            inp, ref64, ref32 = F.point_case(region, R, N, NV)
            assert _finite(ref64, ref32), (region, R, N, NV)
            assert ref64[1].shape == (NV, R * N, 84 if region else 63)
            checks = F.point_checks(region, ref32[0], ref32[1], ref64, ref32)
            F.oracle_inside(checks, ("train_points", region, R, N, NV))
            # Where the noise term matters.  The fp32 oracle forms the shifted-sine argument as fl32(2^k x + pi/2): half an ulp of an
            # argument of up to 2^9 x 1.7, 0.3 of the octave's plain constant at every octave, on every row (the kernels form it the
            # same way).  So "3 x noise exceeds the plain bound on the near-radial rows only" does not hold (docs/frontend_sweep.md,
            # Deviations); what holds and is asserted: outside the near-radial ray the noise stays below the plain constant - the
            # reference's arithmetic passes WITHOUT the noise term, and no bound is lifted to more than four times its constant.
            _, _, share = F.point_bounds(region, ref64[0], ref64[1], ref32[1])
            other = torch.ones(R * N, dtype=torch.bool)
            if region == 1 and R > F.NEAR_RADIAL_ROW:
                other[F.NEAR_RADIAL_ROW * N:(F.NEAR_RADIAL_ROW + 1) * N] = False
            assert float(share[other].max()) < 1.0, (region, R, N, NV, float(share[other].max()))
            used["noise / plain, ordinary rows"] = max(used.get("noise / plain, ordinary rows", 0.0), float(share[other].max()))
            if not bool(other.all()):
                used["noise / plain, near-radial ray"] = max(used.get("noise / plain, near-radial ray", 0.0), float(share[~other].max()))
            t = inp[2]
            if region == 0 and R > F.FULL_SPAN_ROW:
                assert float(t[F.FULL_SPAN_ROW, 0]) == 0.0 and float(t[F.FULL_SPAN_ROW, -1]) == float(inp[3][F.FULL_SPAN_ROW])
            if region == 1 and N > 1:
                assert float(t[:, 0].min()) == 1.0 and float(t[:, -1].max()) == 0.0
            for k, v in checks.items():
                used[k] = max(used.get(k, 0.0), v["fp32_ratio"])
    print("train_points region %d: largest share of a bound the fp32 oracle uses:" % region, {k: "%.2f" % v for k, v in used.items()})


def test_radial_ray_nan_pattern_of_the_oracle():
    o, d, s, far = F.radial_inputs()
    poses = F.point_case(1, 1, 1, cases.NV)[0][4]
    for dtype in (torch.float32, torch.float64):
        look, x = F.points_oracle(1, o, d, s, far, poses, dtype)
        p4 = oracle.sampling.inverted_sphere_points(o.to(dtype), d.to(dtype), s.to(dtype))
        assert bool(torch.isnan(p4[..., :3]).all()) and bool(torch.isfinite(p4[..., 3]).all())
        assert bool(torch.isfinite(look).all()) and F.radial_nan_pattern(x)


# ---- mip_encode ------------------------------------------------------------------------------------------------------------------------
def test_mip_cases_fp32_oracle_inside_bounds():
    used = {}
    for R, n in F.MIP_SHAPES:
        (o, d, rad, t), ref64, ref32 = F.mip_case(R, n)
        assert _finite(ref64, ref32) and ref64.shape == (R * n, 504), (R, n)
        checks = F.mip_checks(ref32, ref64, ref32)
        F.oracle_inside(checks, ("mip_encode", R, n))
        if R >= 9:
            assert float(rad[1]) == 0.0 and float(rad[2]) == 1.0 and float(t[5, n // 2 + 1]) == float(t[5, n // 2])
            assert abs(float(d[3].norm()) - 0.5) < 1e-6 and abs(float(d[4].norm()) - 2.0) < 1e-6
            means, _ = F.mip360.conical_frustum_gaussians(t, o, d, rad)
            assert float(means[7, 0, 2]) == float(np.float32(F.ONE_IN)) and float(means[8, 0, 2]) == float(np.float32(F.ONE_OUT))
            assert float((means[7, 0] ** 2).sum()) <= 1.0 < float((means[8, 0] ** 2).sum())
        for k, v in checks.items():
            used[k] = max(used.get(k, 0.0), v["fp32"])
    print("mip_encode: largest fp32-oracle error:", {k: "%.2e" % v for k, v in used.items()})
    low = max(float((F.mip_case(R, n)[2].double() - F.mip_case(R, n)[1])[:, :63].abs().max()) for R, n in F.MIP_SHAPES)
    assert low < 0.1 * F.MIP_LOW                      # the first 63 features are well conditioned on these kinds of rows (8.9e-7)


# ---- activate --------------------------------------------------------------------------------------------------------------------------
def test_activate_cases_fp32_oracle_inside_bounds():
    used = {}
    for P in F.ACT_P:
        for kind in F.ACT_NOISE:
            inp, ref64, ref32 = F.activate_case(P, kind)
            assert _finite(ref64, ref32), (P, kind)
            checks = F.activate_checks(ref32, ref64, ref32)
            F.oracle_inside(checks, ("activate", P, kind))
            raw_rgb, raw_sigma, noise, scale, _ = inp
            m = min(P, len(F.ACT_DENSITY_ARG))
            arg = raw_sigma[:m, 0] + (noise[:m] * scale if noise is not None else 0.0) + (-1.0)        # fp32, as the kernel forms it
            assert arg.tolist() == [float(np.float32(v)) for v in F.ACT_DENSITY_ARG[:m]], (P, kind)
            k = min(3 * P, len(F.ACT_COLOUR))
            assert raw_rgb.reshape(-1)[:k].tolist() == [float(np.float32(v)) for v in F.ACT_COLOUR[:k]]
            for q, v in checks.items():
                used[q] = max(used.get(q, 0.0), v["fp32_ratio"])
    print("activate: largest share of a bound the fp32 oracle uses:", {k: "%.2f" % v for k, v in used.items()})


# ---- the grid-stride cases -------------------------------------------------------------------------------------------------------------
def test_grid_stride_cases_are_over_the_caps_and_the_oracle_inside_bounds():
    assert (F.PE_BIG[0] * 63 + 255) // 256 == 8193 and (F.UNIFORM_BIG[0] * F.UNIFORM_BIG[1] + 255) // 256 > 16384
    assert (F.L0_BIG[0] * (F.L0_BIG[1] + 1) + 255) // 256 > 16384
    x, ref64, ref32 = F.pos_enc_big_case()
    assert _finite(ref64, ref32)
    F.oracle_inside(F.pos_enc_checks(ref32, ref64, ref32), "pos_enc big")
    u = T.philox_uniform(F.UNIFORM_SEED, F.UNIFORM_STREAM, 64, F.UNIFORM_BIG[1])
    assert 0.0 <= float(u.min()) and float(u.max()) <= F.U_TOP
    for randomized in (False, True):
        far, _, ref64, ref32 = F.level0_case(F.L0_BIG[0], F.L0_BIG[1], randomized)
        F.oracle_inside(F.level0_checks(ref32[0], ref32[1], far, ref64, ref32), ("level0 big", randomized))


# ---- what the per-octave bounds see that one bound per tensor did not ------------------------------------------------------------------
def test_planted_low_octave_errors_are_caught():
    """An error of 1e-4 at octave 3 of one mip_encode row passes `2 x noise + 2e-6` with the noise taken over all twelve octaves, and
    an error of 2e-5 at octave 0 of one train_points row passes `max_abs < 1e-4`; the per-octave bounds reject both, and accept
    the fp32 oracle."""
    _, ref64, ref32 = F.mip_case(9, 8)
    planted = ref64.clone()
    planted[11, 3 * 21 + 5] += 1e-4
    assert float((planted - ref64).abs().max()) <= 2.0 * float((ref32.double() - ref64).abs().max()) + 2e-6      # the earlier expression
    assert F.mip_checks(planted, ref64, ref32)["enc"]["ratio"] > 10.0
    assert F.mip_checks(ref32, ref64, ref32)["enc"]["ratio"] <= 1.0
    for region, width in ((0, 3), (1, 4)):
        _, r64, r32 = F.point_case(region, 5, 13, cases.NV)
        planted = r64[1].clone()
        planted[1, 40, width + 1] += 2e-5                                                       # sin(2^0 y) of one point in one view
        assert float((planted - r64[1]).abs().max()) < F.OCTAVE9[region]                          # the earlier expression
        assert F.point_checks(region, r64[0], planted, r64, r32)["x_enc"]["ratio"] > 3.0
        assert F.point_checks(region, r32[0], r32[1], r64, r32)["x_enc"]["ratio"] <= 1.0
