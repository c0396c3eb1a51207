"""GPU: Mip-NeRF 360's interlevel and distortion losses (training.lossfun_outer / lossfun_distortion over neo_mip_lossfun_outer,
neo_mip_lossfun_outer_backward and neo_mip_lossfun_distortion) against the fp64 restatement of tests/mip_loss_cases.py, entry by
entry at DISTLOSS x max(1, largest |fp64 value| of the tensor): every shape of the table in both input families, ray counts that
leave one, two and three waves of a block idle, rows that do not depend on their neighbours, bitwise repeatability, the NULL outputs
and the limits of the C entry points, and the losses of training_step on the histograms mip_render_train returns."""
import pytest
import torch

import cases
import mip_loss_cases as M
from conftest import record_parity
from neo360_amd import _lib, models, synth, training
from neo360_amd.context import get_context, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _record(case, checks):
    record_parity("mip_losses/%s" % case, **M.summarize(checks))
    M.assert_inside(checks, case)


def _run(inp, rows=None):
    """The five outputs of a case through the Python operators under autograd; rows = (a, b): rays [a, b) only."""
    a, b = rows if rows is not None else (0, inp["w"].shape[0])
    g = lambda k: inp[k][a:b].contiguous().to(DEV)
    with torch.enable_grad():
        w, we = g("w").requires_grad_(True), g("w_env").requires_grad_(True)
        loss = training.lossfun_outer(g("t"), w, g("t_env"), we)
        g_w, g_we = torch.autograd.grad((loss * g("up")).sum(), [w, we])
        dist = training.lossfun_distortion(g("t"), w)
        (g_dist,) = torch.autograd.grad((dist * g("up_dist")).sum(), [w])
    return dict(loss=loss.detach().cpu(), g_w=g_w.cpu(), g_w_env=g_we.cpu(), dist=dist.detach().cpu(), g_dist=g_dist.cpu())


# ---- 1. the sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "N%d_Ne%d" % s)
@pytest.mark.parametrize("family", M.FAMILIES)
def test_sweep_forward_and_backward(family, shape):
    """Every entry of loss, g_w, g_w_env, the distortion loss and its gradient; no entry exempted, no noise term."""
    inp, ref64, ref32 = M.case(family, *shape)
    got = _run(inp)
    assert got["loss"].shape == ref64["loss"].shape and got["dist"].shape == ref64["dist"].shape
    _record(M.case_id(family, *shape), M.checks(got, ref64, ref32))
    if family == "random":             # row 2: an envelope that dominates everywhere - exact zeros
        assert float(got["loss"][2].abs().max()) == 0.0 and float(got["g_w"][2].abs().max()) == 0.0
        assert float(got["g_w_env"][2].abs().max()) == 0.0


# ---- 2. ray counts and row independence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", M.FAMILIES)
def test_ray_counts_and_row_independence(family):
    N, Ne = M.MID_SHAPE
    for R in M.RAY_COUNTS:
        inp, ref64, ref32 = M.case(family, N, Ne, R)
        _record(M.case_id(family, N, Ne, R), M.checks(_run(inp), ref64, ref32))
    for (n, ne) in ((65, 63), (1024, 1024)):
        inp, _, _ = M.case(family, n, ne)
        full = _run(inp)
        for a, b in ((0, 1), (0, 3), (2, 5), (4, 9), (8, 9)):
            part = _run(inp, (a, b))
            for k, v in part.items():
                assert torch.equal(v, full[k][a:b]), (family, n, ne, a, b, k)


# ---- 3. repeatability ------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit():
    for family, N, Ne in (("random", 385, 64), ("random", 64, 385), ("grid", 1024, 1024)):
        inp, _, _ = M.case(family, N, Ne)
        first, second = _run(inp), _run(inp)
        for k in M.OUTPUTS:
            assert torch.equal(first[k], second[k]), (family, N, Ne, k)


# ---- 4. the C entry points: NULL outputs and rejects -----------------------------------------------------------------------------
def _raw(c, inp, N, Ne, R, want_w=True, want_we=True, want_grad=True):
    t, w, te, we, up = (inp[k].to(DEV) for k in ("t", "w", "t_env", "w_env", "up"))
    loss, g_w, g_we = (torch.full(s, -7.0, device=DEV) for s in ((R, N), (R, N), (R, Ne)))
    dist, g_dist = torch.full((R,), -7.0, device=DEV), torch.full((R, N), -7.0, device=DEV)
    _lib.check(c.lib.neo_mip_lossfun_outer(c.handle, ptr(t), ptr(w), ptr(te), ptr(we), R, N, Ne, ptr(loss), c.stream()))
    _lib.check(c.lib.neo_mip_lossfun_outer_backward(c.handle, ptr(t), ptr(w), ptr(te), ptr(we), ptr(up), R, N, Ne,
                                                    ptr(g_w) if want_w else None, ptr(g_we) if want_we else None, c.stream()))
    _lib.check(c.lib.neo_mip_lossfun_distortion(c.handle, ptr(t), ptr(w), R, N, ptr(dist), ptr(g_dist) if want_grad else None, c.stream()))
    return dict(loss=loss.cpu(), g_w=g_w.cpu(), g_w_env=g_we.cpu(), dist=dist.cpu(), g_dist=g_dist.cpu())


def test_null_outputs():
    """Either gradient of the backward, and the distortion gradient, may be NULL: the other outputs are the full call's bit for bit and
    the absent one is not written."""
    c = get_context(torch.device(DEV))
    for family, N, Ne in (("random", 65, 63), ("grid", 129, 257)):
        inp, ref64, ref32 = M.case(family, N, Ne)
        R = M.R_CASE
        full = _raw(c, inp, N, Ne, R)
        wanted = dict(full, g_dist=full["g_dist"] * inp["up_dist"][:, None])      # the entry point returns the unit gradient
        _record(M.case_id(family, N, Ne) + "_entry_points", M.checks(wanted, ref64, ref32))
        for want_w, want_we, want_grad in ((False, True, False), (True, False, True)):
            part = _raw(c, inp, N, Ne, R, want_w, want_we, want_grad)
            for k, present in (("g_w", want_w), ("g_w_env", want_we), ("g_dist", want_grad)):
                assert torch.equal(part[k], full[k]) if present else bool((part[k] == -7.0).all()), (family, k, present)
            assert torch.equal(part["loss"], full["loss"]) and torch.equal(part["dist"], full["dist"])


def test_argument_rejects():
    """N = 0, N = 1025 (Ne likewise), a NULL required pointer: a negative status with a message, nothing launched."""
    c = get_context(torch.device(DEV))
    R = 5
    t, te = (torch.sort(torch.rand(R, 1026, device=DEV), dim=-1).values for _ in range(2))
    w, we, up = (torch.rand(R, 1025, device=DEV) for _ in range(3))
    out = [torch.full((R, 1025), -7.0, device=DEV) for _ in range(3)]
    lib, h, s = c.lib, c.handle, c.stream()

    def refused(rc):
        torch.cuda.synchronize()
        assert rc < 0 and lib.neo_last_error(), rc
        assert all(bool((o == -7.0).all()) for o in out)

    for N, Ne in ((0, 64), (1025, 64), (64, 0), (64, 1025)):
        refused(lib.neo_mip_lossfun_outer(h, ptr(t), ptr(w), ptr(te), ptr(we), R, N, Ne, ptr(out[0]), s))
        refused(lib.neo_mip_lossfun_outer_backward(h, ptr(t), ptr(w), ptr(te), ptr(we), ptr(up), R, N, Ne, ptr(out[0]), ptr(out[1]), s))
    for N in (0, 1025):
        refused(lib.neo_mip_lossfun_distortion(h, ptr(t), ptr(w), R, N, ptr(out[0]), ptr(out[1]), s))
    refused(lib.neo_mip_lossfun_outer(h, ptr(t), ptr(w), ptr(te), ptr(we), -1, 64, 64, ptr(out[0]), s))
    # a NULL required pointer
    refused(lib.neo_mip_lossfun_outer(h, ptr(t), None, ptr(te), ptr(we), R, 64, 64, ptr(out[0]), s))
    refused(lib.neo_mip_lossfun_outer(h, ptr(t), ptr(w), ptr(te), ptr(we), R, 64, 64, None, s))
    refused(lib.neo_mip_lossfun_outer_backward(h, ptr(t), ptr(w), ptr(te), ptr(we), None, R, 64, 64, ptr(out[0]), ptr(out[1]), s))
    refused(lib.neo_mip_lossfun_outer_backward(h, ptr(t), ptr(w), ptr(te), ptr(we), ptr(up), R, 64, 64, None, None, s))
    refused(lib.neo_mip_lossfun_distortion(h, None, ptr(w), R, 64, ptr(out[0]), ptr(out[1]), s))
    refused(lib.neo_mip_lossfun_distortion(h, ptr(t), ptr(w), R, 64, None, ptr(out[1]), s))
    # no rays: nothing to do, as neo_distloss
    for rc in (lib.neo_mip_lossfun_outer(h, None, None, None, None, 0, 64, 64, None, s),
               lib.neo_mip_lossfun_outer_backward(h, None, None, None, None, None, 0, 64, 64, None, None, s),
               lib.neo_mip_lossfun_distortion(h, None, None, 0, 64, None, None, s)):
        assert rc == 0
    with pytest.raises(_lib.NeoError, match="N, Ne <= 1024"):
        training.lossfun_outer(t, w, te[:, :65].contiguous(), we[:, :64].contiguous())
    with pytest.raises(_lib.NeoError, match="N <= 1024"):
        training.lossfun_distortion(t, w)


# ---- 5. edges carry no gradient --------------------------------------------------------------------------------------------------
def test_edges_that_require_grad_are_refused():
    inp, _, _ = M.case("random", 32, 64)
    t, w, te, we = (inp[k].to(DEV) for k in ("t", "w", "t_env", "w_env"))
    with torch.enable_grad():
        with pytest.raises(ValueError, match="edges"):
            training.lossfun_outer(t.clone().requires_grad_(True), w, te, we)
        with pytest.raises(ValueError, match="edges"):
            training.lossfun_outer(t, w, te.clone().requires_grad_(True), we)
        with pytest.raises(ValueError, match="edges"):
            training.lossfun_distortion(t.clone().requires_grad_(True), w)
    # leading dimensions are the caller's
    loss = training.lossfun_outer(t.reshape(3, 3, -1), w.reshape(3, 3, -1), te.reshape(3, 3, -1), we.reshape(3, 3, -1))
    dist = training.lossfun_distortion(t.reshape(3, 3, -1), w.reshape(3, 3, -1))
    assert loss.shape == (3, 3, 32) and dist.shape == (3, 3)
    assert torch.equal(loss.reshape(9, 32), training.lossfun_outer(t, w, te, we))


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def _net(counts=(16, 8)):
    net = models.MipNeRF360(num_prop_samples=counts[0], num_nerf_samples=counts[1]).to(DEV)
    net.load_state_dict(synth.mip360_state(0, weight_gain=0.25))
    return net


def test_training_loss_on_the_histograms_of_the_training_call():
    """mip_render_train on 96 randomized rays, then mip_training_loss: the loss and its gradients with respect to every level's
    weights and the final colour against the fp64 restatement applied to CPU copies of the library's own history tensors (the detach
    of the last level, the means and the multipliers, without the MLPs' ReLU-kink noise).  Then the interlevel term alone through the
    whole chain: every parameter of both proposal MLPs receives a finite, non-zero gradient, the NeRF MLP none."""
    R = 96
    net = _net((16, 8))
    rays = {k: v.to(DEV) for k, v in cases.mip_rays(R).items()}
    target = synth.uniform(93, "mip_target", (R, 3), 0.0, 1.0)
    with torch.enable_grad():
        for p in net.parameters():
            p.requires_grad_(True)
        rend, hist = training.mip_render_train(net, rays, 0.5, True, 0.2, 3.0, seed=13)
        loss, terms = training.mip_training_loss(rend, hist, target.to(DEV))
        wrt = [h["weights"] for h in hist] + [rend[-1]["rgb"]]
        got = torch.autograd.grad(loss, wrt, retain_graph=True)
        hist_c = [dict(sdist=h["sdist"].detach().cpu().double(), weights=h["weights"].detach().cpu().double().requires_grad_(True))
                  for h in hist]
        rgb_c = rend[-1]["rgb"].detach().cpu().double().requires_grad_(True)
        loss_c = M.training_loss(rgb_c, hist_c, target.double())
        want = torch.autograd.grad(loss_c, [h["weights"] for h in hist_c] + [rgb_c])
        inter_c, dist_c = float(M.interlevel_loss(hist_c).detach()), float(M.distortion_loss(hist_c).detach())
    assert not hist[0]["sdist"].requires_grad and inter_c > 0 and dist_c > 0
    names = ["g_weights_level%d" % l for l in range(3)] + ["g_rgb"]
    ref = dict(zip(names, want), loss=loss_c.detach().reshape(1), interlevel=torch.tensor([inter_c]), distortion=torch.tensor([dist_c]))
    res = dict(zip(names, got), loss=loss.detach().reshape(1), interlevel=terms["interlevel"].detach().reshape(1),
               distortion=terms["distortion"].detach().reshape(1))
    checks = {k: M.worst_entry(res[k], ref[k], M.DISTLOSS * M.scale_of(ref[k])) for k in ref}
    _record("training_loss_R%d" % R, checks)
    with torch.enable_grad():
        training.mip_interlevel_loss(hist).backward()
    for lvl in (0, 1):
        for name, p in net.mlps[lvl].named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (lvl, name)
    for name, p in net.mlps[2].named_parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0, name
