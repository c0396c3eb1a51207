"""GPU: the Mip-NeRF 360 extras (ops.mip_extras / training.mip_expected_distance over neo_mip_extras / neo_mip_extras_backward, and
MipNeRF360.compute_extras) against the fp64 restatement of tests/mip_extras_cases.py, entry by entry at DISTLOSS x max(1, largest
|fp64 value| of the tensor): every case of the table in both families and both edge conventions, rows that do not depend on their
neighbours, bitwise repeatability, the NULL outputs and the limits of the C entry points, and the attribute on the small synthetic
module: off - nothing changes; on - five more keys per level, the same histograms bit for bit, a real depth column in the frame,
and gradients from distance_mean to every MLP on the operator chain."""
import pytest
import torch

import cases
import mip_extras_cases as M
from conftest import record_parity
from neo360_amd import _lib, models, ops, render, synth, training
from neo360_amd.context import get_context, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXTRA_KEYS = ("acc", "distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95")


def _record(case, checks):
    record_parity("mip_extras/%s" % case, **M.summarize(checks))
    M.assert_inside(checks, case)


def _run(inp, family, convention, u=M.U3, rows=None):
    """The four outputs of a case through the Python operators; acc and mean are those of mip_expected_distance (under autograd),
    and must be ops.mip_extras' own bit for bit.  rows = (a, b): rays [a, b) only."""
    edges, near, far = M.kernel_edges(inp, family, convention)
    a, b = rows if rows is not None else (0, inp["w"].shape[0])
    g = lambda x: x[a:b].contiguous().to(DEV)
    e, w0 = g(edges), g(inp["w"])
    acc0, mean0, pct = ops.mip_extras(e, w0, u, near, far)
    with torch.enable_grad():
        w = w0.clone().requires_grad_(True)
        acc, mean = training.mip_expected_distance(e, w, near, far)
        (g_w,) = torch.autograd.grad((acc * g(inp["g_acc"]) + mean * g(inp["g_mean"])).sum(), [w])
    assert torch.equal(acc.detach(), acc0) and torch.equal(mean.detach(), mean0)
    return dict(acc=acc0.cpu(), mean=mean0.cpu(), pct=pct.cpu(), g_w=g_w.cpu())


# ---- 1. the sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("convention", M.CONVENTIONS)
@pytest.mark.parametrize("n", M.NS, ids=lambda n: "n%d" % n)
@pytest.mark.parametrize("family", M.FAMILIES)
def test_sweep_forward_and_backward(family, n, convention):
    """Every entry of acc, distance_mean, the percentiles and g_w; no entry exempted, no noise term."""
    inp, ref64, ref32 = M.case(family, n, convention)
    got = _run(inp, family, convention)
    assert got["pct"].shape == ref64["pct"].shape and got["mean"].shape == ref64["mean"].shape
    _record(M.case_id(family, n, convention), M.checks(got, ref64, ref32))
    if family == "random":             # row 0 carries no weight: the far edge, and the second gradient term is 0 by contract
        assert float(got["acc"][0]) == 0.0 and float(got["mean"][0]) == float(ref64["mean"][0].float())
        assert torch.equal(got["g_w"][0], inp["g_acc"][0].expand(n))


@pytest.mark.parametrize("convention", M.CONVENTIONS)
def test_eight_quantiles_with_both_ends(convention):
    family, n = M.U8_CASE
    inp, ref64, ref32 = M.case(family, n, convention, M.R_CASE, M.U8)
    got = _run(inp, family, convention, M.U8)
    _record(M.case_id(family, n, convention, M.R_CASE, M.U8), M.checks(got, ref64, ref32))
    three = _run(inp, family, convention)                      # a quantile does not depend on which others share the call
    assert torch.equal(got["pct"][:, [1, 3, 5]], three["pct"])


# ---- 2. ray counts and row independence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", M.FAMILIES)
def test_ray_counts_and_row_independence(family):
    for convention in M.CONVENTIONS:
        for R in M.RAY_COUNTS:
            inp, ref64, ref32 = M.case(family, M.MID_N, convention, R)
            _record(M.case_id(family, M.MID_N, convention, R), M.checks(_run(inp, family, convention), ref64, ref32))
        for n in (65, 1024):
            inp, _, _ = M.case(family, n, convention)
            full = _run(inp, family, convention)
            for a, b in ((0, 1), (0, 3), (2, 5), (4, 9), (8, 9)):
                part = _run(inp, family, convention, rows=(a, b))
                for k, v in part.items():
                    assert torch.equal(v, full[k][a:b]), (family, convention, n, a, b, k)


# ---- 3. repeatability ------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit():
    for family, n, convention in (("random", 129, "sdist"), ("random", 1023, "metric"), ("grid", 1024, "sdist")):
        inp, _, _ = M.case(family, n, convention)
        first, second = _run(inp, family, convention), _run(inp, family, convention)
        for k in M.OUTPUTS:
            assert torch.equal(first[k], second[k]), (family, n, convention, k)


# ---- 4. the C entry points: NULL outputs and rejects -----------------------------------------------------------------------------
def _raw(c, inp, family, convention, want=(True, True, True), want_up=(True, True)):
    edges, near, far = M.kernel_edges(inp, family, convention)
    e, w, ga, gm = (x.to(DEV) for x in (edges, inp["w"], inp["g_acc"], inp["g_mean"]))
    R, n = w.shape
    u = M.quantiles(M.U3).to(DEV)
    acc, mean, pct, g_w = (torch.full(s, -7.0, device=DEV) for s in ((R,), (R,), (R, 3), (R, n)))
    _lib.check(c.lib.neo_mip_extras(c.handle, ptr(e), ptr(w), R, n, near, far, ptr(u), 3, ptr(acc) if want[0] else None,
                                    ptr(mean) if want[1] else None, ptr(pct) if want[2] else None, c.stream()))
    _lib.check(c.lib.neo_mip_extras_backward(c.handle, ptr(e), ptr(w), R, n, near, far, ptr(ga) if want_up[0] else None,
                                             ptr(gm) if want_up[1] else None, ptr(g_w), c.stream()))
    return dict(acc=acc.cpu(), mean=mean.cpu(), pct=pct.cpu(), g_w=g_w.cpu())


def test_null_outputs():
    """Any output of the forward may be NULL: the others are the full call's bit for bit and the absent one is not written.  A NULL
    upstream pointer of the backward stands for zeros."""
    c = get_context(torch.device(DEV))
    for family, n, convention in (("random", 65, "sdist"), ("grid", 129, "metric")):
        inp, ref64, ref32 = M.case(family, n, convention)
        full = _raw(c, inp, family, convention)
        _record(M.case_id(family, n, convention) + "_entry_points", M.checks(full, ref64, ref32))
        for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, False, False)):
            part = _raw(c, inp, family, convention, want)
            for k, present in zip(("acc", "mean", "pct"), want):
                assert torch.equal(part[k], full[k]) if present else bool((part[k] == -7.0).all()), (family, k, want)
        t = M.kernel_edges(inp, family, convention)[0].double()
        t = M.s_to_t(t) if convention == "sdist" else t
        zero = torch.zeros_like(inp["g_acc"]).double()
        for want_up in ((True, False), (False, True), (False, False)):
            got = _raw(c, inp, family, convention, want_up=want_up)["g_w"]
            ref = M.backward_formula(t, inp["w"].double(), inp["g_acc"].double() if want_up[0] else zero,
                                     inp["g_mean"].double() if want_up[1] else zero)
            M.assert_inside({"g_w": M.worst_entry(got, ref, M.DISTLOSS * M.scale_of(ref))}, (family, n, convention, want_up))


def test_argument_rejects():
    """n = 0, n = 1025, n_u = -1, n_u = 9, exactly one of near / far zero, a negative ray count, a NULL required pointer: a negative
    status with a message, the outputs untouched."""
    c = get_context(torch.device(DEV))
    R = 5
    e = torch.sort(torch.rand(R, 1026, device=DEV), dim=-1).values
    w, up = torch.rand(R, 1025, device=DEV), torch.rand(R, device=DEV)
    u = torch.linspace(0, 1, 9, device=DEV)
    out = [torch.full(s, -7.0, device=DEV) for s in ((R,), (R,), (R, 9), (R, 1025))]
    lib, h, s = c.lib, c.handle, c.stream()

    def fwd(n=64, near=0.2, far=3.0, n_u=3, R=R, e=e, w=w, u=u):
        return lib.neo_mip_extras(h, ptr(e), ptr(w), R, n, near, far, ptr(u), n_u, ptr(out[0]), ptr(out[1]), ptr(out[2]), s)

    def bwd(n=64, near=0.2, far=3.0, R=R, e=e, w=w, g_w=out[3]):
        return lib.neo_mip_extras_backward(h, ptr(e), ptr(w), R, n, near, far, ptr(up), ptr(up), ptr(g_w), s)

    def refused(rc):
        torch.cuda.synchronize()
        assert rc < 0 and lib.neo_last_error(), rc
        assert all(bool((o == -7.0).all()) for o in out)

    for n in (0, 1025):
        refused(fwd(n=n))
        refused(bwd(n=n))
    for n_u in (-1, 9):
        refused(fwd(n_u=n_u))
    for near, far in ((0.0, 3.0), (0.2, 0.0), (-0.2, 3.0)):
        refused(fwd(near=near, far=far))
        refused(bwd(near=near, far=far))
    refused(fwd(R=-1))
    refused(bwd(R=-1))
    refused(fwd(e=None))
    refused(fwd(w=None))
    refused(fwd(u=None))
    refused(bwd(e=None))
    refused(bwd(g_w=None))
    # no rays: nothing to do
    assert fwd(R=0, e=None, w=None) == 0 and bwd(R=0, e=None, w=None, g_w=None) == 0
    with pytest.raises(_lib.NeoError, match="n <= 1024"):
        ops.mip_extras(e, w)
    with pytest.raises(_lib.NeoError, match="n_u <= 8"):
        ops.mip_extras(e[:, :65].contiguous(), w[:, :64].contiguous(), u)
    with pytest.raises(ValueError, match="one more entry"):
        ops.mip_extras(e, w[:, :64].contiguous())
    # leading dimensions are the caller's
    inp, _, _ = M.case("random", 64, "sdist")
    acc, mean, pct = ops.mip_extras(inp["edges"].to(DEV).reshape(3, 3, -1), inp["w"].to(DEV).reshape(3, 3, -1), near=M.NEAR, far=M.FAR)
    flat = ops.mip_extras(inp["edges"].to(DEV), inp["w"].to(DEV), near=M.NEAR, far=M.FAR)
    assert acc.shape == (3, 3) and mean.shape == (3, 3) and pct.shape == (3, 3, 3) and torch.equal(pct.reshape(9, 3), flat[2])


# ---- 5. the module ---------------------------------------------------------------------------------------------------------------
NEAR, FAR = 0.2, 3.0


def _net(counts=(64, 32), gain=0.5):
    net = models.MipNeRF360(num_prop_samples=counts[0], num_nerf_samples=counts[1]).to(DEV)
    net.load_state_dict(synth.mip360_state(0, weight_gain=gain))
    return net


def _rays(R):
    return {k: v.to(DEV) for k, v in cases.mip_rays(R).items()}


@pytest.fixture(scope="module")
def plain_and_extras():
    """One call of 160 rays without the attribute and one with it, on the same module."""
    net, rays = _net(), _rays(160)
    assert net.compute_extras is False
    plain = net(rays, 1.0, False, False, NEAR, FAR)
    frame0 = render.render_rays_test(net, rays, near=NEAR, far=FAR)
    net.compute_extras = True
    try:
        extra = net(rays, 1.0, False, False, NEAR, FAR)
        frame1 = render.render_rays_test(net, rays, near=NEAR, far=FAR)
    finally:
        net.compute_extras = False
    return net, rays, plain, extra, frame0, frame1


def test_attribute_off_changes_nothing(plain_and_extras):
    _, _, (rend, hist), _, frame0, _ = plain_and_extras
    assert all(sorted(r) == ["rgb"] for r in rend) and len(rend) == 3
    assert sorted(frame0) == ["acc", "depth", "rgb"] and float(frame0["depth"].abs().max()) == 0.0
    assert torch.equal(frame0["acc"], hist[-1]["weights"].sum(-1))


def test_attribute_on_adds_the_five_keys_at_every_level(plain_and_extras):
    """... equal to ops.mip_extras on the level's own sdist / weights bit for bit, with rgb, sdist and weights those of the call
    without extras; and against the fp64 restatement on CPU copies of the level's histogram."""
    _, _, (rend0, hist0), (rend, hist), _, _ = plain_and_extras
    for lv in range(3):
        assert sorted(rend[lv]) == sorted(EXTRA_KEYS + ("rgb",))
        assert torch.equal(rend[lv]["rgb"], rend0[lv]["rgb"])
        for k in ("sdist", "weights", "density", "rgb"):
            assert torch.equal(hist[lv][k], hist0[lv][k]), (lv, k)
        acc, mean, pct = ops.mip_extras(hist[lv]["sdist"], hist[lv]["weights"], near=NEAR, far=FAR)
        got = dict(acc=rend[lv]["acc"], mean=rend[lv]["distance_mean"],
                   pct=torch.stack([rend[lv]["distance_percentile_5"], rend[lv]["distance_median"], rend[lv]["distance_percentile_95"]], -1))
        for k, v in dict(acc=acc, mean=mean, pct=pct).items():
            assert torch.equal(got[k], v), (lv, k)
        t = M.s_to_t(hist[lv]["sdist"].cpu().double())
        w = hist[lv]["weights"].cpu().double()
        ref_acc, ref_mean = M.acc_and_mean(t, w)
        ref = dict(acc=ref_acc, mean=ref_mean, pct=M.sorted_interp(M.quantiles(M.U3).double().expand(w.shape[0], 3), M.integrate_weights(w), t))
        _record("module_level%d" % lv, {k: M.worst_entry(got[k], ref[k], M.DISTLOSS * M.scale_of(ref[k])) for k in ref})


def test_frame_carries_a_real_depth(plain_and_extras):
    _, _, _, (rend, hist), frame0, frame1 = plain_and_extras
    assert torch.equal(frame1["rgb"], frame0["rgb"])
    assert torch.equal(frame1["depth"], rend[-1]["distance_mean"]) and torch.equal(frame1["acc"], rend[-1]["acc"])
    for k in EXTRA_KEYS[2:]:
        assert torch.equal(frame1[k], rend[-1][k]), k
    t_near, t_far = (M.s_to_t(hist[-1]["sdist"][:, i].cpu().double()).float() for i in (0, -1))
    depth = frame1["depth"].cpu()
    assert bool((depth >= t_near).all()) and bool((depth <= t_far).all()) and float(depth.std()) > 0
    assert bool((frame1["distance_percentile_5"] <= frame1["distance_median"]).all())
    assert bool((frame1["distance_median"] <= frame1["distance_percentile_95"]).all())


def test_sharded_frame_and_overlapped_chunk_loop(plain_and_extras):
    """render_frame_sharded's (R, 5) tile carries the depth column; a loop of chunk calls in flight on alternating lanes returns
    each chunk's histograms and extras bitwise as the same calls one at a time, and rgb / sdist / weights as without extras."""
    net, rays, (rend0, hist0), _, _, frame1 = plain_and_extras
    net.compute_extras = True
    try:
        tile = render.render_frame_sharded(net, rays, 1, 0, chunk=64, near=NEAR, far=FAR)
        assert tile.shape == (160, 5) and torch.equal(tile[:, 3], frame1["depth"]) and torch.equal(tile[:, 4], frame1["acc"])
        assert net.overlap_calls
        parts = [{k: v[40 * i:40 * (i + 1)] for k, v in rays.items()} for i in range(4)]
        outs = [net(p, 1.0, False, False, NEAR, FAR) for p in parts]
        net.check_flags()
        net.overlap_calls = False
        for i, p in enumerate(parts):
            rend, hist = net(p, 1.0, False, False, NEAR, FAR)
            for lv in range(3):
                for k in EXTRA_KEYS + ("rgb",):
                    assert torch.equal(outs[i][0][lv][k], rend[lv][k]), (i, lv, k)
                for k in ("sdist", "weights"):
                    assert torch.equal(outs[i][1][lv][k], hist[lv][k]), (i, lv, k)
                    assert torch.equal(hist[lv][k], hist0[lv][k][40 * i:40 * (i + 1)]), (i, lv, k)
                assert torch.equal(rend[lv]["rgb"], rend0[lv]["rgb"][40 * i:40 * (i + 1)]), (i, lv)
    finally:
        net.compute_extras = False
        net.overlap_calls = True


def test_operator_chain_carries_gradients_from_the_expected_distance():
    """mip_render_train with the attribute: the five keys at every level, acc / distance_mean attached to the graph, the percentiles
    detached; a loss on every level's distance_mean reaches every parameter of all three MLPs with finite, non-zero gradients."""
    R = 96
    net = _net((16, 8), gain=0.25)
    net.compute_extras = True
    rays = _rays(R)
    with torch.enable_grad():
        for p in net.parameters():
            p.requires_grad_(True)
        rend, hist = net(rays, 0.5, True, True, NEAR, FAR, seed=13)
        for lv in range(3):
            assert sorted(rend[lv]) == sorted(EXTRA_KEYS + ("rgb",))
            assert rend[lv]["acc"].requires_grad and rend[lv]["distance_mean"].requires_grad
            assert not any(rend[lv][k].requires_grad for k in EXTRA_KEYS[2:])
            acc, mean, pct = ops.mip_extras(hist[lv]["sdist"], hist[lv]["weights"].detach(), near=NEAR, far=FAR)
            assert torch.equal(rend[lv]["distance_mean"].detach(), mean) and torch.equal(rend[lv]["distance_median"], pct[:, 1])
        sum(r["distance_mean"].mean() for r in rend).backward()
    for lvl in range(3):
        for name, p in net.mlps[lvl].named_parameters():
            if name.split(".")[0] in ("bottleneck_layer", "views_linear", "rgb_layer"):
                # the NeRF MLP's colour branch: a distance depends on the densities only, its gradient there is exactly zero
                assert p.grad is None or float(p.grad.abs().max()) == 0, (lvl, name)
                continue
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (lvl, name)
    net.compute_extras = False
    rend, _ = net(rays, 0.5, True, True, NEAR, FAR, seed=13)
    assert all(sorted(r) == ["rgb"] for r in rend)
