"""CPU: the case table of tests/mip_extras_cases.py for the Mip-NeRF 360 extras.  Its restatement of the reference's helpers equals the
reference's own results (tests/golden/g13_mip_extras.npz, written by tests/golden/make_mip_extras.py), the table's condition holds,
a row without weight returns t_n, the backward formula equals fp64 autograd wherever autograd is defined, and the public boundary
(header, ctypes table, CPU tensors refused, the module attribute) is in place."""
import os
import re

import pytest
import torch

import mip_extras_cases as M
from conftest import ROOT

FIXTURE = "g13_mip_extras"


def test_restatement_equals_the_reference_fixture(golden):
    """fp64 percentiles of every stored case to 1e-12 (x the tensor's scale); the builders reproduce the stored inputs bit for bit,
    so the GPU sweep runs on exactly what the reference was run on."""
    g = golden(FIXTURE)
    for family, n, convention, u in M.fixture_cases():
        stored, pct64, pct32 = M.fixture_case(g, family, n, convention, u)
        inp = M.inputs(family, n)
        assert torch.equal(stored["edges"], M.kernel_edges(inp, family, convention)[0]), (family, n, convention)
        assert torch.equal(stored["w"], inp["w"]), (family, n, convention)
        mine = M.evaluate(inp, family, convention, u, torch.float64)["pct"]
        assert mine.dtype == pct64.dtype == torch.float64 and mine.shape == pct64.shape
        err = float((mine - pct64).abs().max())
        assert err <= 1e-12 * M.scale_of(pct64), (family, n, convention, err)
        assert bool(torch.isfinite(pct32).all())


def test_reference_fp32_percentiles_against_the_bound(golden):
    """For information, asserted as found: the reference's OWN fp32 percentiles, as stored (n <= 129), stay inside the bound."""
    g = golden(FIXTURE)
    worst = 0.0
    for family, n, convention, u in M.fixture_cases():
        _, pct64, pct32 = M.fixture_case(g, family, n, convention, u)
        c = M.worst_entry(pct32, pct64, M.DISTLOSS * M.scale_of(pct64), pct32)
        worst = max(worst, c["ratio"])
    assert worst <= 1.0, worst


def test_condition_of_the_table():
    """Random family: every quantile at least KNOT_MARGIN from every fp64 knot, in every case of the table.  Grid family: every
    knot is a multiple of 1 / 4096 below 2^11, so fp32 and fp64 prefix sums are exact in any order."""
    seen = set()
    for family, n, convention, R, u in M.table():
        if (family, n, R, u) in seen:
            continue
        seen.add((family, n, R, u))
        inp = M.inputs(family, n, R)
        assert bool((inp["edges"][:, 1:] >= inp["edges"][:, :-1]).all()) and bool((inp["w"] >= 0).all())
        if family == "random":
            d = M.knot_distance(inp, u)
            assert d >= M.KNOT_MARGIN, (family, n, R, d)
        else:
            k = inp["w"].double() * 4096
            assert bool((k == k.round()).all()) and float(k.sum(-1).max()) < 2 ** 23
            assert torch.equal(torch.cumsum(inp["w"], -1).double(), torch.cumsum(inp["w"].double(), -1))
    assert len(seen) == 2 * (len(M.NS) + len(M.RAY_COUNTS)) + 1


def test_table_shape_and_references():
    """Every case has finite fp64 references of the right shapes; the degenerate rows are what the docstring says; the grid family
    has ties, zero weights and rows on both sides of the clip."""
    for family, n, convention, R, u in M.table():
        inp, ref64, ref32 = M.case(family, n, convention, R, u)
        assert ref64["acc"].shape == (R,) and ref64["mean"].shape == (R,) and ref64["pct"].shape == (R, len(u))
        assert ref64["g_w"].shape == (R, n)
        assert all(v.dtype == torch.float64 and bool(torch.isfinite(v).all()) for v in ref64.values())
        assert bool((ref64["pct"][:, 1:] >= ref64["pct"][:, :-1]).all())          # ascending quantiles, ascending distances
        M.assert_inside(M.checks(ref32, ref64, ref32, M.FP32_INSIDE), ("fp32 restatement", family, n, convention, R))
    w = M.inputs("random", 128)["w"].double()
    assert float(w[0].abs().max()) == 0 and float(w[1].max()) == 1 and abs(float(w[2].sum()) - 1.7) < 1e-5
    assert abs(float(w[3].sum()) - 0.3) < 1e-5 and float(w[4, 1::2].abs().max()) == 0
    g = M.inputs("grid", 128)
    assert bool((g["edges"][:, 1:] == g["edges"][:, :-1]).any()) and bool((g["w"] == 0).any())
    sums = g["w"].double().sum(-1)
    assert float(sums.min()) < 1 < float(sums.max()) + 0.5


def test_a_row_without_weight_returns_the_far_edge():
    for convention in M.CONVENTIONS:
        for n in (1, 64, 1024):
            inp, ref64, _ = M.case("random", n, convention)
            t_n = M.kernel_edges(inp, "random", convention)[0][0, -1].double()
            t_n = M.s_to_t(t_n) if convention == "sdist" else t_n
            assert float(ref64["acc"][0]) == 0.0 and float(ref64["mean"][0]) == float(t_n)
            assert torch.equal(ref64["g_w"][0], inp["g_acc"][0].double().expand(n))      # the second term is 0 by contract
    assert abs(float(M.s_to_t(torch.tensor(1.0, dtype=torch.float64))) - M.FAR) < 1e-12


def test_backward_formula_equals_autograd_where_autograd_is_defined():
    """fp64 autograd of the restatement (through the clip) on every row with acc > 0, every case of the table; NaN exactly on the
    rows without weight, where the contract defines the second term as 0."""
    for family, n, convention, R, u in M.table():
        inp, ref64, _ = M.case(family, n, convention, R, u)
        auto = M.autograd_g_w(inp, family, convention)
        has = ref64["acc"] > 0
        assert bool(torch.isnan(auto[~has]).all())
        err = float((auto[has] - ref64["g_w"][has]).abs().max()) if bool(has.any()) else 0.0
        assert err <= 1e-12 * M.scale_of(ref64["g_w"]), (family, n, convention, R, err)


def test_planted_errors_are_caught():
    """A bracket one knot off, a renormalised cumulative weight and a mean without the clip each leave the bound."""
    for family in M.FAMILIES:
        inp, ref64, ref32 = M.case(family, 65, "sdist")
        shifted = M.evaluate(inp, family, "sdist", M.U3, torch.float64,
                             interp=lambda x, xp, fp: M.sorted_interp(x, torch.roll(xp, 1, -1), fp))
        assert M.checks(shifted, ref64, ref32, ("pct",))["pct"]["ratio"] > 1.0
        renorm = M.evaluate(inp, family, "sdist", M.U3, torch.float64,
                            integrate=lambda w: M.integrate_weights(w / w.sum(-1, keepdim=True).clamp(min=1e-30)))
        assert M.checks(renorm, ref64, ref32, ("pct",))["pct"]["ratio"] > 1.0
    inp, ref64, ref32 = M.case("random", 65, "sdist")
    wrong = ref64["mean"].clone()
    wrong[0] = 0.0                      # nan_to_num's default for the row without weight
    assert M.checks(dict(ref64, mean=wrong), ref64, ref32, ("mean",))["mean"]["ratio"] > 1.0


NEW_SYMBOLS = ("neo_mip_extras", "neo_mip_extras_backward")


def test_entry_points_declared_and_bound():
    from neo360_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neo360_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(neo_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["neo_mip_extras"][1]) == 13
    assert len(_lib.SIGNATURES["neo_mip_extras_backward"][1]) == 11


def test_cpu_tensors_are_refused_and_the_attribute_defaults_to_off():
    """No fallback: CPU tensors raise NeoError before anything is looked up in the library."""
    from neo360_amd import _lib, models, ops, training
    inp = M.inputs("grid", 3)
    with pytest.raises(_lib.NeoError):
        ops.mip_extras(inp["edges"], inp["w"])
    with pytest.raises(_lib.NeoError):
        training.mip_expected_distance(inp["edges"], inp["w"])
    with torch.enable_grad():
        with pytest.raises(ValueError, match="edges"):
            training.mip_expected_distance(inp["edges"].clone().requires_grad_(True), inp["w"])
    assert models.MipNeRF360.compute_extras is False


def test_restatement_against_the_reference_live():
    """Where the reference tree is present: its functions, run here, against the restatement on every case of the table."""
    import _ref_loader
    if not _ref_loader.reference_available():
        pytest.skip("reference tree not present")
    H = _ref_loader.load("models.mipnerf360.helper")
    _, warp = H.construct_ray_warps(M.NEAR, M.FAR)
    for family, n, convention, R, u in M.table():
        inp, ref64, _ = M.case(family, n, convention, R, u)
        live = M.evaluate(inp, family, convention, u, torch.float64, interp=H.sorted_interp, integrate=H.integrate_weights, warp=warp)
        err = float((live["pct"] - ref64["pct"]).abs().max())
        assert err <= 1e-12 * M.scale_of(ref64["pct"]), (family, n, convention, R, err)
