"""CPU: the NeO-360 extras' restatement (tests/tp_extras_cases.py) in closed form, the conditions of its case table, and the
presence of the feature at every layer that can be looked at without a device: the two header symbols and their ctypes rows,
ops.tp_extras, NeRF_TP.compute_extras / extras_quantiles."""
import math
import os
import re

import pytest
import torch

import tp_extras_cases as T
from conftest import ROOT


# ---- 1. the feature exists -------------------------------------------------------------------------------------------------------
def test_the_feature_exists_at_every_layer():
    from neo360_amd import _lib, models, ops
    header = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("neo_tp_extras", "neo_tp_render_extras"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "neo_tp_extras_out" in header
    assert [n for n, _ in _lib.TpExtrasOut._fields_] == ["opacity", "disparity", "dist_pct"]
    # neo_tp_render_extras = the arguments of neo_tp_render + (u, n_u, extras0, extras1) in front of the stream
    assert len(_lib.SIGNATURES["neo_tp_render_extras"][1]) == len(_lib.SIGNATURES["neo_tp_render"][1]) + 4
    assert _lib.SIGNATURES["neo_tp_render_extras"][1][:-5] == _lib.SIGNATURES["neo_tp_render"][1][:-1]
    assert len(_lib.SIGNATURES["neo_tp_extras"][1]) == 17
    assert callable(ops.tp_extras)
    assert models.NeRF_TP.compute_extras is False
    assert tuple(models.NeRF_TP.extras_quantiles) == (0.05, 0.5, 0.95)
    assert os.path.exists(os.path.join(ROOT, "neo-360_amd", "csrc", "tp_extras.hip"))


def test_the_operator_refuses_what_it_cannot_take_before_any_device_call():
    """Only some of the outside arguments, a CPU tensor: ValueError from the host checks (no library call is reached)."""
    from neo360_amd import ops
    inp = T.inputs("grid", 3)
    kw = T.kernel_kwargs(inp, "two", "cpu")
    with pytest.raises(ValueError, match="device"):
        ops.tp_extras(**kw)


# ---- 2. closed forms -------------------------------------------------------------------------------------------------------------
def _ray(o, d):
    return torch.tensor([o], dtype=torch.float64), torch.tensor([d], dtype=torch.float64)


def test_tau_of_one_is_the_sphere_exit():
    """|o + tau(1) d| = 1 with tau(1) beyond the nearest point, for every ray of both families, to 1e-12; tau(0) = +inf."""
    for family in T.FAMILIES:
        for n in (1, 64):
            inp = T.inputs(family, n)
            o, d = inp["rays_o"].double(), inp["rays_d"].double()
            geom = T.ray_geometry(o, d)
            t1 = T.tau(torch.ones(o.shape[0], 1, dtype=torch.float64), geom)[:, 0]
            assert float(((o + t1[:, None] * d).norm(dim=-1) - 1.0).abs().max()) < 1e-12
            assert bool((t1 > geom[0]).all())
            # the closed form of the reference's intersect_sphere (neo360/helper.py:253-273): d1 + sqrt(1 - |p|^2) / |d|
            assert float((t1 - (geom[0] + torch.sqrt(1.0 - geom[1]) / geom[2])).abs().max()) < 1e-12
            assert float((t1.float() - inp["far"]).abs().max()) <= 2.4e-7 * float(t1.max())
            assert bool(torch.isinf(T.tau(torch.zeros(o.shape[0], 1, dtype=torch.float64), geom)).all())
    o, d = _ray((0.0, 0.0, 0.0), (0.0, 0.0, 2.0))
    assert float(T.tau(torch.tensor([[0.25]], dtype=torch.float64), T.ray_geometry(o, d))) == 2.0      # radius 4 at t = 4 / |d|


def test_one_opaque_inside_interval_puts_the_median_at_its_middle():
    inp = dict(rays_o=torch.tensor([[0.0, 0.0, 0.0]]), rays_d=torch.tensor([[0.0, 2.0, 0.0]]), far=torch.tensor([0.5]),
               fg_t=torch.tensor([[0.125]]), fg_w=torch.tensor([[1.0]]))
    out = T.evaluate(inp, "inside", (0.0, 0.5, 0.75, 1.0))
    assert out["pct"].tolist() == [[0.125, 0.3125, 0.40625, T.INF]]
    assert float(out["opacity"]) == 1.0 and float(out["disparity"]) == (8.0 + 2.0) / 2
    assert out["at_knot"].tolist() == [[True, False, False, False]]


def test_a_two_interval_outside_ray_by_hand():
    """o = 0, d = (0, 0, 2): tau(s) = 1 / (2 s).  Inside: one interval [1/4, 1/2] with mass 1/4.  Outside, lambda = 1/2: s from 1 to 1/2
    with weight 1/2 (mass 1/4), s from 1/2 to 0 with weight 1 (mass 1/2).  Knots 0, 1/4, 1/2, 1."""
    inp = dict(rays_o=torch.zeros(1, 3), rays_d=torch.tensor([[0.0, 0.0, 2.0]]), far=torch.tensor([0.5]), fg_t=torch.tensor([[0.25]]),
               fg_w=torch.tensor([[0.25]]), bg_s=torch.tensor([[1.0, 0.5]]).reshape(1, 2), bg_w=torch.tensor([[0.5, 1.0]]),
               lam=torch.tensor([0.5]))
    inp["fg_t"] = torch.tensor([[0.25, 0.5]])            # two inside samples, the second one a zero-width, zero-mass interval at far
    inp["fg_w"] = torch.tensor([[0.25, 0.0]])
    out = T.evaluate(inp, "two", (0.125, 0.25, 0.375, 0.5, 0.75, 1.0))
    # 1/8: half way through the inside interval; 1/4: the knot shared by the zero-mass interval and the first outside one -> its
    # first edge tau(1) = 1/2; 3/8: s = 3/4 -> 2/3; 1/2: tau(1/2) = 1; 3/4: s = 1/4 -> 2; 1: the ray leaves
    want = [0.375, 0.5, 1.0 / (2 * 0.75), 1.0, 2.0, T.INF]
    assert out["pct"][0].tolist() == want
    assert out["at_knot"][0].tolist() == [False, True, False, True, False, False]
    assert float(out["opacity"]) == 1.0
    # 1/4 (4 + 2) / 2 inside, 1/4 (2 + 1) / 2 and 1/2 (1 + 0) / 2 outside
    assert float(out["disparity"]) == 0.75 + 0.375 + 0.25
    inside = T.evaluate(inp, "inside", (0.125, 0.25))
    assert inside["pct"][0].tolist() == [0.375, T.INF] and float(inside["opacity"]) == 0.25


def test_grid_rows_meet_knots_exactly():
    """Row 0's median meets the run of tied knots that crosses the sphere and lands on the last outside edge; row 1's stays inside and
    lands on the last inside sample; 0 and 1 among the eight quantiles take the first interval with mass and +inf."""
    for n in T.NS:
        inp, ref = T.case("grid", n, "two")
        h = T.histogram(inp, "two")
        assert bool(ref["at_knot"][0, 1]) and float(ref["pct"][0, 1]) == float(h["a"][0, 2 * n - 1])
        assert math.isfinite(float(ref["pct"][0, 1])) and float(ref["pct"][0, 1]) == float(ref["pct"][0, 1].float())
        inp, ref = T.case("grid", n, "inside")
        assert float(ref["pct"][0, 1]) == T.INF
        if n > 1:
            assert bool(ref["at_knot"][1, 1]) and float(ref["pct"][1, 1]) == float(inp["fg_t"][1, n - 1])
    family, n = T.U8_CASE
    for form in T.FORMS:
        inp, ref = T.case(family, n, form, T.R_CASE, T.U8)
        assert bool(ref["at_knot"][:, 0].all())
        assert int(ref["at_knot"].sum()) > T.R_CASE
        total = ref["opacity"]
        assert torch.equal(torch.isinf(ref["pct"][:, -1]), total <= 1.0)


# ---- 3. conditions of the table --------------------------------------------------------------------------------------------------
def test_table_shape():
    rows = T.table()
    assert len(rows) == len(set(rows)) == 2 * 2 * len(T.NS) + 2 * 2 * len(T.RAY_COUNTS) + 2
    assert {r[2] for r in rows} == set(T.FORMS) and {r[1] for r in rows if r[3] == T.R_CASE and r[4] == T.U3} == set(T.NS)


@pytest.mark.parametrize("family,n,form,R,u", T.table(), ids=lambda v: None)
def test_conditions_of_every_case(family, n, form, R, u):
    inp, ref = T.case(family, n, form, R, u)
    # the inputs are what the contract takes: fp32, origins inside the sphere, no unit directions, ascending / descending rows
    assert all(v.dtype == torch.float32 for v in inp.values())
    assert bool((inp["rays_o"].norm(dim=-1) < 1).all())
    dn = inp["rays_d"].norm(dim=-1)
    assert bool(((dn >= 0.5) & (dn <= 2.0)).all()) and not bool((dn == 1.0).any())
    assert bool((inp["fg_t"][:, 1:] >= inp["fg_t"][:, :-1]).all()) and bool((inp["fg_t"][:, -1] <= inp["far"]).all())
    assert bool((inp["bg_s"][:, 1:] <= inp["bg_s"][:, :-1]).all()) and bool((inp["bg_s"] >= 0).all()) and bool((inp["bg_s"] <= 1).all())
    assert float(T.ray_geometry(inp["rays_o"].double(), inp["rays_d"].double())[1].min()) == 0.0 or R < 7
    if family == "random":
        assert T.knot_distance(inp, form, u) >= T.KNOT_MARGIN
    # front to back against pairwise: the same infinite entries, every finite one within a tenth of the bound
    other = T.evaluate(inp, form, u, pairwise=True)
    T.assert_inside(T.checks(other, ref, T.case_id(family, n, form, R, u), share=0.1), T.case_id(family, n, form, R, u))
    if family == "grid":               # every knot is exact: the two orders agree bit for bit
        assert torch.equal(T.knots(T.histogram(inp, form), True), T.knots(T.histogram(inp, form), False))
        assert torch.equal(other["pct"], ref["pct"]) and torch.equal(other["opacity"], ref["opacity"])


def test_the_degenerate_rows_are_what_they_claim():
    for n in T.NS:
        inp, ref = T.case("random", n, "two")
        assert float(ref["opacity"][0]) == 0.0 and float(ref["disparity"][0]) == 0.0 and bool(torch.isinf(ref["pct"][0]).all())
        assert float(inp["lam"][1]) == 0.0 and bool(torch.isfinite(ref["pct"][1]).all())
        assert bool(torch.isinf(ref["pct"][2]).all()) and float(ref["opacity"][2]) == 1.0 and float(ref["disparity"][2]) == 0.0
        assert abs(float(ref["opacity"][4]) - 0.3) < 1e-6 and torch.isinf(ref["pct"][4]).tolist() == [False, True, True]
        assert float(T.ray_geometry(inp["rays_o"].double(), inp["rays_d"].double())[1][6]) == 0.0
        if n > 1:
            assert float(inp["bg_s"][3, -1]) == 2.0 ** -10 and float(inp["bg_s"][7, -1]) == 0.0
            assert bool(torch.isfinite(ref["pct"][3]).all())
        rest = [r for r in range(T.R_CASE) if r not in (0, 2, 4, 7)]      # row 7's last interval is [0, 0] in inverse radius: +inf
        assert bool(torch.isfinite(ref["pct"][rest]).all()), n
