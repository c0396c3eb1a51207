"""CPU: the case table of tests/alongray_cases.py is one on which the reference's own arithmetic passes.

For every case the GPU sweep (tests/test_gpu_alongray_sweep.py) runs: every fp64 reference value and gradient is finite, and the
fp32 oracle - the reference's arithmetic - stays inside the per-entry bounds with the fp64 oracle as truth.  A case that failed
this was replaced in the table (the reasons are written at its builder), never exempted.  The planted-error tests show what the
per-entry bounds see that one bound per tensor did not."""
import pytest
import torch

import alongray_cases as A


def _finite(*refs):
    return all(bool(torch.isfinite(v).all()) for r in refs for v in (r.values() if isinstance(r, dict) else [r]))


# ---- compositing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.COMPOSITE_MODES)
def test_compositing_cases_fp32_oracle_inside_bounds(mode):
    used = {}
    for m, N, white in A.composite_table():
        if m != mode:
            continue
        inp, ref64, ref32 = A.composite_case(m, N, white)
        assert _finite(ref64, ref32), (m, N, white)
        checks = A.composite_checks(ref32, m, ref64, ref32)
        A.assert_inside({k: dict(v, ratio=v["fp32_ratio"]) for k, v in checks.items()}, ("compositing", m, N, white))
        # the noise term of the sentinel bound: needed by one ray of the nine at most (the spike row)
        _, lifted = A.sigma_grad_bounds(m, ref64["g_sigma"], ref32["g_sigma"])
        assert int(lifted.sum()) <= A.MAX_LIFTED_RAYS, (m, N, white, lifted.nonzero().flatten().tolist())
        assert not bool(lifted.any()) or lifted.nonzero().flatten().tolist() == [2], (m, N, white)
        for k, v in checks.items():
            used[k] = max(used.get(k, 0.0), v["fp32_ratio"])
    print("mode", mode, "largest share of a bound the fp32 oracle uses:", {k: "%.2f" % v for k, v in used.items()})


@pytest.mark.parametrize("mode", A.COMPOSITE_MODES)
def test_compositing_ray_count_cases_fp32_oracle_inside_bounds(mode):
    for R in A.RAY_COUNTS:
        inp, ref64, ref32 = A.composite_case(mode, A.COMPOSITE_MID_N, False, R, False)
        assert _finite(ref64, ref32)
        checks = A.composite_checks(ref32, mode, ref64, ref32)
        A.assert_inside({k: dict(v, ratio=v["fp32_ratio"]) for k, v in checks.items()}, ("compositing", mode, R))


@pytest.mark.parametrize("which", [("rgb",), ("weights",), ("lam",)])
def test_compositing_partial_losses_fp32_oracle_inside_bounds(which):
    for mode in A.COMPOSITE_MODES:
        if which == ("lam",) and mode != 1:
            continue
        inp, ref64, ref32 = A.composite_case(mode, 65, True, A.R_DEG, True, which)
        assert _finite(ref64, ref32)
        checks = A.composite_checks(dict(g_rgb=ref32["g_rgb"], g_sigma=ref32["g_sigma"]), mode, ref64, ref32)
        A.assert_inside({k: dict(v, ratio=v["fp32_ratio"]) for k, v in checks.items()}, ("partial loss", which, mode))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("white", [False, True])
def test_planted_density_gradient_error_is_caught(mode, white):
    """cases.composite_case() in modes 0 and 2 holds one entry of 1e10 G (ray 0 is empty, its last interval the 1e10 sentinel).  The
    bound `2e-5 * max(1, max|g|)` then lets every other entry be wrong by 1e5; the per-entry bounds do not."""
    inp, ref64, ref32 = A.composite_case(mode, 129, white, 64, True, None, True)
    g64 = ref64["g_sigma"]
    assert float(g64[0, -1].abs()) > 1e9 and float(g64[:, :-1].abs().max()) < 1.0        # the table of the issue
    assert A.sigma_grad_inside(ref32["g_sigma"], mode, g64, ref32["g_sigma"])            # the reference's arithmetic passes
    for ray, i in ((5, 17), (0, 64), (63, 127), (1, 0)):
        planted = g64.clone()
        planted[ray, i] += 1e-3
        assert A.old_sigma_grad_check(planted - g64, g64), "the old expression accepts the planted error"
        assert not A.sigma_grad_inside(planted, mode, g64, ref32["g_sigma"]), "the per-entry bounds reject it"
    # an error in a sentinel entry the size of its own rounding is still accepted, one of 1e-3 of the entry is not
    planted = g64.clone()
    planted[0, -1] *= 1.0 + 1e-6
    assert A.sigma_grad_inside(planted, mode, g64, ref32["g_sigma"])
    planted[0, -1] = g64[0, -1] * (1.0 + 1e-3)
    assert not A.sigma_grad_inside(planted, mode, g64, ref32["g_sigma"])


def test_mode_1_bound_is_unchanged_in_kind():
    """Mode 1 has no sentinel: every entry is held to 2e-5 x max(1, largest entry), as before."""
    inp, ref64, ref32 = A.composite_case(1, 129, False, 64, True, None, True)
    bound, lifted = A.sigma_grad_bounds(1, ref64["g_sigma"], ref32["g_sigma"])
    assert not bool(lifted.any()) and float(bound.min()) == float(bound.max()) == A.G_SIGMA * A.scale_of(ref64["g_sigma"])


# ---- distortion loss -------------------------------------------------------------------------------------------------------------
def test_distloss_cases_fp32_oracle_inside_bounds():
    for N in A.DISTLOSS_N:
        inp, ref64, ref32 = A.distloss_case(N)
        assert _finite(ref64, ref32), N
        checks = A.distloss_checks(ref32, ref64, ref32)
        A.assert_inside(checks, ("distloss", N))
        # the prefix-sum form is the pairwise definition
        brute = A.T.distloss_bruteforce(inp["w"].double(), inp["m"].double(), inp["interval"])
        assert abs(float(brute) - float(ref64["loss"])) < 1e-12
    for R in A.RAY_COUNTS:
        inp, ref64, ref32 = A.distloss_case(A.DISTLOSS_MID_N, R, False)
        A.assert_inside(A.distloss_checks(ref32, ref64, ref32), ("distloss", R))


def test_planted_distloss_gradient_error_is_caught():
    for N in (65, 385):
        inp, ref64, ref32 = A.distloss_case(N)
        planted = dict(loss=ref64["loss"], g_w=ref64["g_w"].clone())
        planted["g_w"][4, N // 3] += 1e-4
        assert A.distloss_checks(planted, ref64, ref32)["g_w"]["ratio"] > 1.0


# ---- inverse-CDF resampling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_prev,n_new", A.RESAMPLE_SHAPES)
@pytest.mark.parametrize("randomized", [False, True])
def test_resample_cases_fp32_oracle_inside_bounds(n_prev, n_new, randomized):
    for descending in (False, True):
        inp, ref64, ref32 = A.resample_case(n_prev, n_new, descending)
        if randomized:
            u = A.resample_draws(inp, A.R_DEG, n_new)
            ref64 = A.resample_oracle(inp["t_prev"], inp["w"], u, torch.float64)
            ref32 = A.resample_oracle(inp["t_prev"], inp["w"], u, torch.float32)
        assert _finite(ref64, ref32)
        as_returned = torch.flip(ref32, dims=[-1]) if descending else ref32
        A.resample_invariants(as_returned, inp["t_prev"], n_new, descending)
        A.assert_inside(A.resample_checks(as_returned, inp, None, descending, ref64, ref32), ("resample", n_prev, n_new, descending))
        if descending:
            # how many rows the reference determines: the strict 1e-4 applies to those.  Up to 65 previous samples at least two
            # thirds; beyond, the count is what it is (the per-entry evidence at those sizes is the ascending case of the same shape)
            well = int(A.descending_well_determined(ref64, ref32).sum())
            print("descending (%d, %d) %s: %d of %d rows determined to 1e-5" % (n_prev, n_new, "randomized" if randomized else
                                                                                  "deterministic", well, A.R_DEG))
            if n_prev <= 65:
                assert 3 * well >= 2 * A.R_DEG, (n_prev, n_new, well)


def test_resample_ray_count_cases_fp32_oracle_inside_bounds():
    n_prev, n_new = A.RESAMPLE_MID
    for R in A.RAY_COUNTS:
        for descending in (False, True):
            inp, ref64, ref32 = A.resample_case(n_prev, n_new, descending, R, False)
            as_returned = torch.flip(ref32, dims=[-1]) if descending else ref32
            A.resample_invariants(as_returned, inp["t_prev"], n_new, descending)
            A.assert_inside(A.resample_checks(as_returned, inp, None, descending, ref64, ref32, well_from=0), ("resample", R, descending))


def test_resample_invariants_notice_a_lost_sample():
    inp, ref64, ref32 = A.resample_case(64, 192, False)
    A.resample_invariants(ref32, inp["t_prev"], 192, False)
    broken = ref32.clone()
    j = int((broken[5] == inp["t_prev"][5, 7]).nonzero()[0])
    broken[5, j] = torch.nextafter(broken[5, j], torch.tensor(2.0))          # a previous sample one ulp off: still sorted
    with pytest.raises(AssertionError):
        A.resample_invariants(broken, inp["t_prev"], 192, False)


# ---- Mip-NeRF 360 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dilate", [True, False])
def test_mip_resample_cases_fp32_oracle_inside_bounds(dilate):
    table = [c for c in A.mip_resample_table() if c[2] == dilate]
    if dilate:
        table += [A.MIP_RESAMPLE_MID]
    for n_prev, n, d in table:
        for randomized in (False, True):
            inp, ref64, ref32 = A.mip_resample_case(n_prev, n, d, randomized)
            assert _finite(ref64, ref32), (n_prev, n, d, randomized)
            A.assert_inside(A.mip_resample_checks(ref32, A.mip_tdist_of(ref32), ref64, ref32), ("mip resample", n_prev, n, d, randomized))
    n_prev, n, d = A.MIP_RESAMPLE_MID
    if dilate == d:
        for R in A.RAY_COUNTS:
            inp, ref64, ref32 = A.mip_resample_case(n_prev, n, d, True, R, False)
            A.assert_inside(A.mip_resample_checks(ref32, A.mip_tdist_of(ref32), ref64, ref32), ("mip resample", R))


def test_mip_composite_cases_fp32_oracle_inside_bounds():
    for n in A.MIP_COMPOSITE_N:
        for bg in (0.0, 1.0):
            inp, ref64, ref32 = A.mip_composite_case(n, bg)
            assert _finite(ref64, ref32), (n, bg)
            A.assert_inside(A.mip_composite_checks(ref32, ref64, ref32), ("mip composite", n, bg))
    for R in A.RAY_COUNTS:
        inp, ref64, ref32 = A.mip_composite_case(A.MIP_COMPOSITE_MID_N, 1.0, R, False)
        A.assert_inside(A.mip_composite_checks(ref32, ref64, ref32), ("mip composite", R))
    for which in (("weights",), ("rgb",)):
        inp, ref64, ref32 = A.mip_composite_case(65, 1.0, A.R_DEG, True, which)
        assert _finite(ref64, ref32)
        A.assert_inside(A.mip_composite_checks(ref32, ref64, ref32), ("mip composite", which))
