"""GPU: results the host-side machinery around the kernels could lose without an error.

* plane gradients of a training call, whose lookups share one set of gradient buffers (training.gather_planes(..., shared)):
  partial backward passes over a retained graph, other gradient terms on the planes, several calls in one loss;
* device assertion bits raised by one lane of overlapped calls while another lane reads and clears the flag word;
* the activation-tape layout of the projected training chains when neo_train_chain_mode changes between a forward and its
  backward.
"""
import pytest
import torch

import cases
import oracle
from conftest import max_abs
from neo360_amd import _lib, models, render, synth, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
PER_RAY = ("rays_o", "rays_d", "viewdirs")
MAPS = ("plane_xz", "plane_xy", "plane_yz", "latent")


def _tp_net(scene, n_coarse=16, n_fine=24):
    net = models.NeRF_TP(num_coarse_samples=n_coarse, num_fine_samples=n_fine, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(synth.nerf_tp_state(0))
    net.set_scene(*(scene[k].to(DEV) for k in MAPS), scene["image_wh"])
    return net


def _batch(n):
    return {k: v.to(DEV) for k, v in cases.neo_batch(cases.strided_rays(n)).items()}


# ---- A: shared plane-gradient buffers ------------------------------------------------------------------------------------------

_GATHER_CASES = {
    # name: (lookups in pass 1 or None, lookups of the final pass, direct term on the planes, two shared groups)
    "all": (None, (0, 1, 2, 3), False, False),
    "two_of_four": (None, (2, 3), False, False),
    "retained_then_all": ((2, 3), (0, 1, 2, 3), False, False),
    "all_plus_direct_term": (None, (0, 1, 2, 3), True, False),
    "two_groups": (None, (0, 1, 2, 3), False, True),
}


@pytest.mark.parametrize("case", list(_GATHER_CASES))
def test_shared_plane_gradients_match_fp64_autograd(case):
    """gather_planes with one `shared` dict and four lookups at different points against fp64 autograd through the oracle's
    triplane_features: the loss reaches all / some of the lookups, a partial pass runs first over the retained graph, the planes
    get a gradient of their own, or two groups share the planes in one loss."""
    first, final, direct, two_groups = _GATHER_CASES[case]
    sc = cases.small_scene()
    net = _tp_net(sc)
    batch = cases.neo_batch(cases.strided_rays(8))
    gbatch = {k: v.to(DEV) for k, v in batch.items()}
    pts = [synth.uniform(40 + i, "shared_pts", (37 + 11 * i, 3), -1.4, 1.4) for i in range(4)]
    gen = torch.Generator().manual_seed(7)
    ups = [torch.randn(cases.NV * p.shape[0], 128, generator=gen, dtype=torch.float64) for p in pts]
    with torch.enable_grad():
        cm = [sc[k].clone().double().requires_grad_(True) for k in MAPS[:3]]
        poses = batch["src_poses"].double()

        def ref_loss(which, scale=1.0):
            return sum(scale * (oracle.gather.triplane_features(pts[i].double(), *cm, poses).reshape(-1, 128) * ups[i]).sum()
                       for i in which)

        gm = [sc[k].to(DEV).clone().requires_grad_(True) for k in MAPS[:3]]
        latent = sc["latent"].to(DEV)
        net.set_scene(*gm, latent, sc["image_wh"])
        fp = net._scene_src
        groups = [{}, {}] if two_groups else [{}]
        outs = [[training.gather_planes(net, pts[i].to(DEV), *gm, latent, gbatch, shared=sh) for i in range(4)] for sh in groups]
        assert net._scene_src is fp, "a lookup through the shared-gradient sink uploaded the scene again"

        def gpu_loss(which):
            return sum(s * (outs[j][i] * ups[i].float().to(DEV)).sum() for j, s in enumerate((1.0, 0.5)[:len(groups)]) for i in which)

        if first is not None:
            g1 = torch.autograd.grad(gpu_loss(first), gm, retain_graph=True)
            kept = [t.clone() for t in g1]
            w1 = torch.autograd.grad(ref_loss(first), cm)
        loss = gpu_loss(final)
        want = ref_loss(final) + (ref_loss(final, 0.5) if two_groups else 0.0)
        if direct:
            loss = loss + 0.1 * sum((p ** 2).sum() for p in gm)
            want = want + 0.1 * sum((p ** 2).sum() for p in cm)
        g = torch.autograd.grad(loss, gm)
        w = torch.autograd.grad(want, cm)
    for a, b in zip(g, w):
        assert a.shape == b.shape and max_abs(a, b) < 1e-5 * max(1.0, float(b.abs().max())), case
    if first is not None:
        for a, b, k in zip(g1, w1, kept):
            assert max_abs(a, b) < 1e-5 * max(1.0, float(b.abs().max())), case
            assert torch.equal(a, k), "pass 2 changed the gradient pass 1 returned"


def _train_grads(projected, losses, sc, batches, into_grad=False):
    """Gradients of the four maps of a NeRF_TP training call (train_shared_grads on) under the loss `losses` builds from the
    calls' outputs.  losses(outs) -> list of (loss, retain) run in order; returns the gradients of each pass."""
    net = models.NeRF_TP(num_coarse_samples=16, num_fine_samples=24, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(synth.nerf_tp_state(0))
    net.train_projected = projected
    net.train_shared_grads = True
    maps = [sc[k].to(DEV).clone().requires_grad_(True) for k in MAPS]
    res = []
    with torch.enable_grad():
        net.set_scene(*maps, sc["image_wh"])
        fp = net._scene_src
        for p in net.parameters():
            p.requires_grad_(True)
        outs = [net(b, True, False, 0.0, 0.0, out_depth=False, seed=5 + i, chunk=32) for i, b in enumerate(batches)]
        assert net._scene_src is fp, "the training call uploaded the scene again"
        for loss, retain in losses(outs, maps):
            if into_grad:
                for m in maps:
                    m.grad = None
                loss.backward(retain_graph=retain)
                res.append([m.grad.detach().clone() for m in maps])
            else:
                res.append([t.detach() for t in torch.autograd.grad(loss, maps, retain_graph=retain)])
    return res


def _close(a_list, b_list, label):
    for nm, a, b in zip(MAPS, a_list, b_list):
        rel = float((a - b).norm()) / (float(a.norm()) + 1e-20)
        assert rel < 2e-3 and float(b.abs().max()) > 0.0, (label, nm, rel)


def test_training_call_fine_only_retained_then_full():
    sc = cases.small_scene()
    gb = _batch(64)
    target = synth.uniform(23, "chunk_target", (64, 3), 0.0, 1.0).to(DEV)
    mse = lambda lv: ((lv[0] - target) ** 2).mean()
    losses = lambda outs, maps: [(mse(outs[0][1]), True), (mse(outs[0][0]) + mse(outs[0][1]), False)]
    ref = _train_grads(False, losses, sc, [gb])
    got = _train_grads(True, losses, sc, [gb])
    _close(ref[0], got[0], "fine-only pass")
    _close(ref[1], got[1], "full pass after the retained one")


def test_training_call_with_a_regulariser_on_the_planes():
    sc = cases.small_scene()
    gb = _batch(64)
    target = synth.uniform(23, "chunk_target", (64, 3), 0.0, 1.0).to(DEV)
    losses = lambda outs, maps: [(sum(((lv[0] - target) ** 2).mean() for lv in outs[0])
                                  + 1e-3 * sum((m ** 2).mean() for m in maps[:3]), False)]
    _close(_train_grads(False, losses, sc, [gb])[0], _train_grads(True, losses, sc, [gb])[0], "rgb + regulariser")


@pytest.mark.parametrize("into_grad", [False, True])
def test_two_training_calls_in_one_loss(into_grad):
    sc = cases.small_scene()
    b1, b2 = _batch(96), _batch(96)
    b2 = {k: (v[48:] if k in PER_RAY else v) for k, v in b2.items()}
    b1 = {k: (v[:48] if k in PER_RAY else v) for k, v in b1.items()}
    target = synth.uniform(23, "chunk_target", (48, 3), 0.0, 1.0).to(DEV)
    losses = lambda outs, maps: [(sum(((lv[0] - target) ** 2).mean() for o in outs for lv in o), False)]
    _close(_train_grads(False, losses, sc, [b1, b2], into_grad)[0], _train_grads(True, losses, sc, [b1, b2], into_grad)[0],
           "two calls, into_grad=%s" % into_grad)


# ---- B: flag bits raised while overlapped calls read the word ------------------------------------------------------------------

def _bad(batch, i):
    """Ray i misses the unit sphere (the reference's assertion, neo360/helper.py)."""
    b = dict(batch)
    b["rays_o"], b["rays_d"] = batch["rays_o"].clone(), batch["rays_d"].clone()
    b["rays_o"][i] = torch.tensor([0.0, 0.0, 5.0], device=DEV)
    b["rays_d"][i] = torch.tensor([1.0, 0.0, 0.0], device=DEV)
    return b


CHUNK, NCHUNK = 64, 24


def _loop(net, batch):
    for i in range(0, batch["rays_o"].shape[0], CHUNK):
        net({k: (v[i:i + CHUNK] if k in PER_RAY else v) for k, v in batch.items()}, False, False, 0.0, 0.0, out_depth=True)


@pytest.mark.parametrize("poll", ["deferred", "immediate"])
@pytest.mark.parametrize("k", [0, NCHUNK // 2, NCHUNK - 1])
def test_sphere_miss_in_one_overlapped_chunk_is_reported(k, poll):
    """One ray of chunk k misses the sphere in a loop of 24 overlapped calls (two lanes): the loop followed by check_flags() and
    render_rays_test must both raise the reference's AssertionError, whichever lane chunk k ran on."""
    sc = cases.small_scene()
    net = _tp_net(sc)
    net.poll_flags = poll
    assert net.overlap_calls
    batch = _bad(_batch(CHUNK * NCHUNK), k * CHUNK + 17)
    with torch.no_grad():
        with pytest.raises(AssertionError):
            _loop(net, batch)
            net.check_flags()
        # the loop stopped where the miss was raised; reads still in flight may hold the bit again (a call sets it from more than
        # one kernel, and another lane's read can take it in between): drain them, then the word must be clean
        try:
            net.check_flags()
        except AssertionError:
            pass
        net.check_flags()
        with pytest.raises(AssertionError):
            render.render_rays_test(net, batch, chunk=CHUNK)
        net.check_flags()


def test_range_guard_under_overlap_rerenders_exactly():
    """A scene beyond the fp16 range, rendered in more chunks than there are lanes: render_rays_test reports the guard and
    returns the exact kernels' frame, bitwise."""
    sc = dict(cases.small_scene())
    sc["latent"] = sc["latent"] * 1.0e6
    batch = _batch(CHUNK * NCHUNK)
    exact = _tp_net(sc)
    exact.precision = "f32"
    with torch.no_grad():
        want = render.render_rays_test(exact, batch, chunk=CHUNK)
        net = _tp_net(sc)
        with pytest.warns(RuntimeWarning, match="re-rendered on the exact fp32 kernels"):
            got = render.render_rays_test(net, batch, chunk=CHUNK)
    assert got["precision_used"] == "f32"
    for k in ("rgb", "depth", "acc", "fg_rgb", "bg_rgb"):
        assert torch.equal(got[k], want[k]), k


# ---- C: tape layout recorded by the forward ------------------------------------------------------------------------------------

def _toggled(fn, params, inputs, up, fwd_mode, bwd_mode):
    """Forward under chain mode fwd_mode, backward after switching to bwd_mode."""
    lib = _lib.load()
    old = lib.neo_train_chain_mode(-1)
    try:
        with torch.enable_grad():
            for p in params:
                p.requires_grad_(True)
            ins = [t.clone().requires_grad_(True) for t in inputs]
            lib.neo_train_chain_mode(fwd_mode)
            rgb, sigma = fn(ins)
            lib.neo_train_chain_mode(bwd_mode)
            grads = torch.autograd.grad((rgb * up[0]).sum() + (sigma * up[1]).sum(), ins + params)
    finally:
        lib.neo_train_chain_mode(old)
    return rgb.detach(), sigma.detach(), grads


def _same_as_untoggled(fn, params, inputs, up):
    """Toggled pair against the same-mode pair, within the bounds of test_gpu_host_r6.py::
    test_fused_training_chain_equals_the_layer_by_layer_chain (the weight gradients' split-K partials are summed atomically, so
    two runs of one mode need not be bitwise equal).  A backward reading the other layout's tape is off by O(1)."""
    for fwd in (1, 0):
        want = _toggled(fn, params, inputs, up, fwd, fwd)
        got = _toggled(fn, params, inputs, up, fwd, 1 - fwd)
        for a, b in zip(got[:2], want[:2]):
            assert max_abs(a, b) <= 5e-6 * max(1.0, float(b.abs().max()))
        for i, (a, b) in enumerate(zip(got[2], want[2])):
            err, ref = max_abs(a, b), max(float(b.abs().max()), 1e-6)
            assert err <= 2e-5 * ref, ("forward mode", fwd, "gradient", i, err, ref)


@pytest.mark.parametrize("rows_p,nv,input_ch", [(37, 2, 3), (777, 3, 4), (777, 2, 3), (37, 3, 4)])
def test_nerfpp_chain_mode_switch_between_forward_and_backward(rows_p, nv, input_ch):
    """nerfpp_mlp_projected: a forward in one chain mode and its backward after neo_train_chain_mode switched give bitwise the
    outputs and gradients (18 parameters, world, pre) of the same-mode pair - the backward reads the layout the forward wrote."""
    mlp = models.NeRFPPMLP(0, 10, 4, input_ch=input_ch, num_src_views=nv).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(rows_p + nv)
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(torch.randn(p.shape, device=DEV, generator=g) * (0.15 if p.dim() == 2 else 0.05))
    P = rows_p
    x_enc = torch.randn(nv, P, 21 * input_ch, device=DEV, generator=g)
    cond = torch.randn(nv * P, 27, device=DEV, generator=g)
    world = torch.randn(nv * P, 128, device=DEV, generator=g) * 0.5
    pre = torch.randn(nv * P, 256, device=DEV, generator=g) * 0.5
    up = (torch.randn(P, 3, device=DEV, generator=g), torch.randn(P, 1, device=DEV, generator=g))
    layers = mlp.ordered_layers()
    params = [l.weight for l in layers] + [l.bias for l in layers]
    _same_as_untoggled(lambda ins: training.nerfpp_mlp_projected(mlp, x_enc, cond, ins[0], ins[1], nv), params, [world, pre], up)


@pytest.mark.parametrize("P,nv", [(37, 2), (777, 3)])
def test_pixel_chain_mode_switch_between_forward_and_backward(P, nv):
    """The same for PixelNeRF's projected chain (pixel_mlp_fused): 18 parameter gradients and the gradient of `pre`."""
    net = models.PixelNeRF(num_src_views=nv, num_coarse_samples=16, num_fine_samples=24).to(DEV)
    net.load_state_dict(synth.pixelnerf_state(0))
    mlp = net.fine_mlp
    g = torch.Generator(device=DEV).manual_seed(P)
    x_enc = torch.randn(nv, P, 63, device=DEV, generator=g)
    cond = torch.randn(nv * P, 27, device=DEV, generator=g)
    pre = torch.randn(nv * P, 128, device=DEV, generator=g) * 0.5
    up = (torch.randn(P, 3, device=DEV, generator=g), torch.randn(P, 1, device=DEV, generator=g))
    layers = mlp.ordered_layers()
    params = [l.weight for l in layers] + [l.bias for l in layers]
    _same_as_untoggled(lambda ins: training.pixel_mlp_fused(mlp, x_enc, cond, ins[0], nv), params, [pre], up)
