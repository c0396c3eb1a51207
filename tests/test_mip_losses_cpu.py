"""CPU: the case table of tests/mip_loss_cases.py for Mip-NeRF 360's interlevel and distortion losses.  Its restatement of the
reference's two helpers equals the reference's own results (tests/golden/g12_mip_losses.npz, written by
tests/golden/make_mip_losses.py), fp32 arithmetic stays inside the table's bounds where the table says it does, planted errors are
caught, and the public boundary (header, ctypes table, CPU tensors refused) is in place."""
import os
import re

import pytest
import torch

import mip_loss_cases as M
from conftest import ROOT

FIXTURE = "g12_mip_losses"


def _fixture_cases():
    return [(f, n, ne) for f in M.FAMILIES for (n, ne) in M.FIXTURE_SHAPES]


def test_restatement_equals_the_reference_fixture(golden):
    """fp64, every output and gradient of every stored case to 1e-12 (x the tensor's scale); the builders reproduce the stored inputs
    bit for bit, so the GPU sweep runs on exactly what the reference was run on."""
    g = golden(FIXTURE)
    for family, N, Ne in _fixture_cases():
        inp, ref64, _ = M.fixture_case(g, family, N, Ne)
        built = M.inputs(family, N, Ne)
        for k in M.INPUTS:
            assert torch.equal(inp[k], built[k]), (family, N, Ne, k)
        mine = M.evaluate(inp, torch.float64)
        for k in M.OUTPUTS:
            assert mine[k].dtype == ref64[k].dtype == torch.float64
            err = float((mine[k] - ref64[k]).abs().max())
            assert err <= 1e-12 * M.scale_of(ref64[k]), (family, N, Ne, k, err)


def test_reference_fp32_results_against_the_bounds(golden):
    """The reference's OWN fp32 run, as stored: inside the bounds on the grid family and, on the random family, for the loss values, the
    distortion loss and its gradient.  Its fp32 lossfun_outer gradients leave them on the random family (the ill-conditioning the
    native kernels remove by keeping their prefix sums in fp64): that is the finding, so it is asserted too."""
    g = golden(FIXTURE)
    worst_outer_grad = 0.0
    for family, N, Ne in _fixture_cases():
        _, ref64, ref32 = M.fixture_case(g, family, N, Ne)
        M.assert_inside(M.checks(ref32, ref64, ref32, M.FP32_INSIDE[family]), ("reference fp32", family, N, Ne))
        if family == "random":
            c = M.checks(ref32, ref64, ref32, ("g_w", "g_w_env"))
            worst_outer_grad = max(worst_outer_grad, c["g_w"]["ratio"], c["g_w_env"]["ratio"])
    assert worst_outer_grad > 100.0, worst_outer_grad


def test_fp32_restatement_inside_bounds():
    """All 24 nine-row cases and the ray-count cases, finite fp64 references included."""
    todo = [(f, n, ne, M.R_CASE) for f, n, ne in M.table()] + [(f,) + M.MID_SHAPE + (r,) for f in M.FAMILIES for r in M.RAY_COUNTS]
    for family, N, Ne, R in todo:
        inp, ref64, ref32 = M.case(family, N, Ne, R)
        assert all(bool(torch.isfinite(v).all()) for v in ref64.values())
        assert ref64["loss"].shape == (R, N) and ref64["g_w_env"].shape == (R, Ne) and ref64["dist"].shape == (R,)
        M.assert_inside(M.checks(ref32, ref64, ref32, M.FP32_INSIDE[family]), (family, N, Ne, R))
        if family == "random" and R == M.R_CASE:
            # row 2: the envelope dominates everywhere
            assert float(ref64["loss"][2].abs().max()) == 0.0 and float(ref64["g_w"][2].abs().max()) == 0.0
            assert float(ref64["g_w_env"][2].abs().max()) == 0.0


def test_some_intervals_are_active_in_every_family():
    """The loss is not identically zero on the table: a share of the fine intervals exceeds its envelope in both families."""
    for family in M.FAMILIES:
        _, ref64, _ = M.case(family, 128, 64)
        assert 0.05 < float((ref64["loss"] > 0).double().mean()) < 0.95


@pytest.mark.parametrize("family", M.FAMILIES)
def test_planted_errors_are_caught(family):
    """One lo index off by one, and g_w_env shifted by one bin, each leave the bounds."""
    for (N, Ne) in ((32, 64), (65, 63), (129, 257)):
        inp, ref64, ref32 = M.case(family, N, Ne)
        t, te, we = inp["t"].double(), inp["t_env"].double(), inp["w_env"].double()
        lo, hi = M.bracket(t, te)
        # the interval whose left bin carries the most envelope weight among those with a positive loss
        left = torch.gather(we, -1, lo[..., :-1].clamp(max=Ne - 1)) * (ref64["loss"] > 0) * (lo[..., :-1] < Ne)
        r, i = divmod(int(left.reshape(-1).argmax()), N)
        assert float(left[r, i]) > 1e-4
        lo2 = lo.clone()
        lo2[r, i] += 1
        planted = M.evaluate(inp, torch.float64, outer=lambda a, b, c, d: M.lossfun_outer(a, b, c, d, (lo2, hi)))
        c = M.checks(planted, ref64, ref32, ("loss", "g_w", "g_w_env"))
        assert c["loss"]["ratio"] > 1.0 and c["g_w_env"]["ratio"] > 1.0, (family, N, Ne, c)
        shifted = dict(ref64, g_w_env=torch.roll(ref64["g_w_env"], 1, -1))
        assert M.checks(shifted, ref64, ref32, ("g_w_env",))["g_w_env"]["ratio"] > 1.0, (family, N, Ne)


def test_interlevel_and_distortion_losses_of_a_history():
    """model.py:725-741 restated: the last level is detached for the interlevel loss (no gradient reaches it from there), the
    proposal levels get one, and the distortion loss reaches only the last level."""
    inp = M.inputs("random", 32, 64)
    with torch.enable_grad():
        hist = [dict(sdist=inp["t_env"].double(), weights=inp["w_env"].double().requires_grad_(True)) for _ in range(2)]
        hist.append(dict(sdist=inp["t"].double(), weights=inp["w"].double().requires_grad_(True)))
        ws = [h["weights"] for h in hist]
        g_inter = torch.autograd.grad(M.interlevel_loss(hist), ws, allow_unused=True)
        g_dist = torch.autograd.grad(M.distortion_loss(hist), ws, allow_unused=True)
    assert g_inter[2] is None and float(g_inter[0].abs().max()) > 0 and torch.equal(g_inter[0], g_inter[1])
    assert g_dist[0] is None and g_dist[1] is None and float(g_dist[2].abs().max()) > 0
    want = 2 * M.lossfun_outer(inp["t"].double(), inp["w"].double(), inp["t_env"].double(), inp["w_env"].double()).mean()
    assert abs(float(M.interlevel_loss(hist)) - float(want)) < 1e-15


NEW_SYMBOLS = ("neo_mip_lossfun_outer", "neo_mip_lossfun_outer_backward", "neo_mip_lossfun_distortion")


def test_entry_points_declared_and_bound():
    from neo360_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neo360_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(neo_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["neo_mip_lossfun_outer"][1]) == 10
    assert len(_lib.SIGNATURES["neo_mip_lossfun_outer_backward"][1]) == 12
    assert len(_lib.SIGNATURES["neo_mip_lossfun_distortion"][1]) == 8


def test_cpu_tensors_are_refused():
    """No fallback: CPU tensors raise NeoError before anything is looked up in the library."""
    from neo360_amd import _lib, training
    inp = M.inputs("grid", 3, 2)
    with pytest.raises(_lib.NeoError):
        training.lossfun_outer(inp["t"], inp["w"], inp["t_env"], inp["w_env"])
    with pytest.raises(_lib.NeoError):
        training.lossfun_distortion(inp["t"], inp["w"])
    with torch.enable_grad():
        with pytest.raises(ValueError):
            training.lossfun_distortion(inp["t"].clone().requires_grad_(True), inp["w"])
        with pytest.raises(ValueError):
            training.lossfun_outer(inp["t"], inp["w"], inp["t_env"].clone().requires_grad_(True), inp["w_env"])


def test_restatement_against_the_reference_live():
    """Where the reference tree is present: its two functions, run here, against the restatement on every case of the table."""
    import _ref_loader
    if not _ref_loader.reference_available():
        pytest.skip("reference tree not present")
    H = _ref_loader.load("models.mipnerf360.helper")
    for family, N, Ne in M.table():
        inp, ref64, _ = M.case(family, N, Ne)
        live = M.evaluate(inp, torch.float64, outer=H.lossfun_outer, distortion=H.lossfun_distortion)
        for k in M.OUTPUTS:
            err = float((live[k] - ref64[k]).abs().max())
            assert err <= 1e-12 * M.scale_of(ref64[k]), (family, N, Ne, k, err)
