"""GPU: the exact-fp32 pillar stage (csrc/pillar_f32.hip) and GridEncoder's range-guard retry.

precision "f32" against the reference's fixture and the oracle; power-of-two scale invariance of the new kernel (an exact,
derived condition: tests/pillar_scale_cases.py, shown on the CPU by test_pillar_scale_cases_cpu.py); the retry on a latent
beyond the fp16 range (per call, no latch) and on a packed weight (latched until the parameters change); training under "f32"
and through a retried call; NeRF_TP with an un-normalised encoder attached renders a frame instead of raising;
$NEO360_PRECISION; the full 64^3 x 3 size."""
import warnings

import pytest
import torch

import cases
import oracle
import pillar_scale_cases as P
from conftest import max_abs, record_parity
from neo360_amd import _lib, encoder, models, render, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID = (12, 10, 8)
SEED_G = 11                       # cotangents of the floor-plans, as in test_gpu_encoder_training.py


def _views():
    poses, focal, centre = synth.source_views(cases.NV, *cases.IMG_WH)
    return poses.to(DEV), focal.to(DEV), centre.to(DEV)


def _enc(grid, params, precision=None):
    enc = encoder.GridEncoder(grid_size=grid).to(DEV)
    missing = enc.load_state_dict(params, strict=False)
    assert not missing.unexpected_keys
    enc.precision = precision
    return enc


def _plans(enc, latent, image_wh):
    return enc.floorplans(latent.to(DEV), *_views(), image_wh)


def _flags(enc):
    (ctx,) = enc._ctx_cache.values()
    return ctx.poll_flags()


# ---- 1, 2, 8: precision "f32" against the fixture and the oracle --------------------------------------------------------------
def _check_fixture(got, g, tag):
    worst = {"values": 0.0, "sums": 0.0, "squares": 0.0}
    for name, fp in zip(("yz", "xz", "xy"), got):
        fp = fp.cpu()
        e = (max_abs(fp[..., ::4], g["fp_" + name]), max_abs(fp.double().sum(-1), g["sum_" + name]),
             max_abs((fp.double() ** 2).sum(-1), g["sq_" + name]))
        print(tag, name, "values %.3g  channel sums %.3g  squared sums %.3g" % e)
        for k, v in zip(worst, e):
            worst[k] = max(worst[k], v)
    record_parity(tag, **worst)
    # the bounds of test_gpu_encoder.py::test_floorplans_vs_reference_fixture
    assert worst["values"] < 2e-5 and worst["sums"] < 2e-3 and worst["squares"] < 2e-3, worst


def test_f32_floorplans_vs_reference_fixture(golden):
    sc = cases.small_scene()
    enc = _enc(GRID, synth.pillar_state(0), "f32")
    got = _plans(enc, sc["latent"], sc["image_wh"])
    assert enc.last_precision_used == "f32" and _flags(enc) == 0
    _check_fixture(got, golden("g9_pillar"), "pillar_f32/fixture_g9")


def test_env_precision_f32(golden, monkeypatch):
    monkeypatch.setenv("NEO360_PRECISION", "f32")
    sc = cases.small_scene()
    enc = _enc(GRID, synth.pillar_state(0))
    got = _plans(enc, sc["latent"], sc["image_wh"])
    assert enc.last_precision_used == "f32"
    _check_fixture(got, golden("g9_pillar"), "pillar_f32/fixture_g9_env")
    monkeypatch.delenv("NEO360_PRECISION")
    want = _plans(_enc(GRID, synth.pillar_state(0), "f32"), sc["latent"], sc["image_wh"])
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("grid", [(16, 16, 16), (5, 7, 3), (64, 4, 9)])
def test_f32_floorplans_vs_oracle_other_grids(grid):
    torch.set_num_threads(8)
    sc = cases.small_scene(seed=19)
    params = synth.pillar_state(2)
    got = _plans(_enc(grid, params, "f32"), sc["latent"], sc["image_wh"])
    poses, focal, centre = synth.source_views(cases.NV, *cases.IMG_WH)
    want = oracle.pillar.floorplans(params, sc["latent"], sc["image_wh"], poses, focal, centre, grid)
    worst = 0.0
    for a, b in zip(got, want):
        assert a.shape == b.shape
        worst = max(worst, max_abs(a, b))
    print("f32 vs oracle, grid", grid, "max |difference| %.3g" % worst)
    record_parity("pillar_f32/oracle_%dx%dx%d" % grid, max_abs=worst)
    assert worst < 2e-5


# ---- 3: scale invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(12, 10, 8), (5, 7, 3)])
def test_f32_scale_invariance(grid):
    """Case L through the exact kernels: every product and partial sum is the unscaled one times a power of two or unchanged, so
    the floor-plans are bitwise the same.  No tolerance."""
    sc = cases.small_scene()
    params = synth.pillar_state(0)
    p2, lat2, _ = P.case_l(params, sc["latent"])
    want = _plans(_enc(grid, params, "f32"), sc["latent"], sc["image_wh"])
    got = _plans(_enc(grid, p2, "f32"), lat2, sc["image_wh"])
    for name, a, b in zip(("yz", "xz", "xy"), got, want):
        assert torch.equal(a, b), (name, max_abs(a, b))


# ---- 4: retry on the latent -------------------------------------------------------------------------------------------------------
def test_retry_on_latent_is_per_call():
    sc = cases.small_scene()
    params = synth.pillar_state(0)
    p2, lat2, _ = P.case_l(params, sc["latent"])
    enc = _enc(GRID, p2)
    enc.on_range = "raise"
    with pytest.raises(_lib.NeoRangeError):
        _plans(enc, lat2, sc["image_wh"])
    enc.on_range = "retry_f32"
    want = _plans(_enc(GRID, p2, "f32"), lat2, sc["image_wh"])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = _plans(enc, lat2, sc["image_wh"])
        again = _plans(enc, lat2, sc["image_wh"])
    assert len([w for w in seen if issubclass(w.category, RuntimeWarning)]) == 1, [str(w.message) for w in seen]
    for a, b, c in zip(got, again, want):
        assert torch.equal(a, c) and torch.equal(b, c)
    assert enc.last_precision_used == "f32" and enc._range_latch is None
    assert _flags(enc) == 0                          # nothing left over for a later call
    # an in-range call afterwards runs on the split kernels again
    enc.load_state_dict(params, strict=False)
    back = _plans(enc, sc["latent"], sc["image_wh"])
    fresh = _plans(_enc(GRID, params), sc["latent"], sc["image_wh"])
    for a, b in zip(back, fresh):
        assert torch.equal(a, b)
    assert enc.last_precision_used == "f16x3" and _flags(enc) == 0


# ---- 5: static latch ---------------------------------------------------------------------------------------------------------------
def test_static_operand_latches_until_parameters_change():
    sc = cases.small_scene()
    params = synth.pillar_state(0)
    p2, lat2, _ = P.case_w(params, sc["latent"])
    enc = _enc(GRID, p2)
    want = _plans(_enc(GRID, p2, "f32"), lat2, sc["image_wh"])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        first = _plans(enc, lat2, sc["image_wh"])
        assert enc.last_precision_used == "f32" and enc._range_latch == enc.operands_key()
        second = _plans(enc, lat2, sc["image_wh"])
    assert len([w for w in seen if issubclass(w.category, RuntimeWarning)]) == 1
    assert enc.last_precision_used == "f32"
    for a, b, c in zip(first, second, want):
        assert torch.equal(a, c) and torch.equal(b, c)
    # the scaled weights are an exact rescaling: the exact kernels return the unscaled encoder's f32 plans
    plain = _plans(_enc(GRID, params, "f32"), sc["latent"], sc["image_wh"])
    for a, b in zip(first, plain):
        assert torch.equal(a, b)
    enc.load_state_dict(params, strict=False)
    back = _plans(enc, sc["latent"], sc["image_wh"])
    assert enc._range_latch is None and enc.last_precision_used == "f16x3" and _flags(enc) == 0
    fresh = _plans(_enc(GRID, params), sc["latent"], sc["image_wh"])
    for a, b in zip(back, fresh):
        assert torch.equal(a, b)


# ---- 6: training ------------------------------------------------------------------------------------------------------------------
def _names():
    layers = ["depth_fc.common_branch.0", "depth_fc.common_branch.2", "depth_fc.depth_encoder"]
    for ax in ("xz", "yz", "xy"):
        layers += ["pillar_aggregator_%s.0" % ax, "pillar_aggregator_%s.2" % ax]
    return [l + ".weight" for l in layers] + [l + ".bias" for l in layers]


NAMES = _names()
# a scorer head's bias shifts every score of a pillar alike: its exact gradient is zero (|g| <= 1e-4 instead of a relative bound)
HEAD_BIAS = {"pillar_aggregator_%s.2.bias" % ax for ax in ("xz", "yz", "xy")}


def _cotangents(grid, nv=cases.NV):
    G0, G1, G2 = grid
    shapes = {"yz": (nv, G1, G2, 512), "xz": (nv, G0, G2, 512), "xy": (nv, G0, G1, 512)}
    return [synth.normal(SEED_G, "pillar_grad_" + k, shapes[k], 1.0) for k in ("yz", "xz", "xy")]


def _library_grads(enc, latent, image_wh, cot):
    with torch.enable_grad():
        lat = latent.to(DEV).clone().requires_grad_(True)
        pd = dict(enc.named_parameters())
        fps = enc.floorplans_train(lat, *_views(), image_wh)
        loss = sum((a * g.to(DEV)).sum() for a, g in zip(fps, cot))
        gr = torch.autograd.grad(loss, [pd[n] for n in NAMES] + [lat])
    return fps, dict(zip(NAMES + ["latent"], gr))


def _oracle_grads(params, sc, grid, cot, dtype, tape=None):
    """fp32 / fp64 autograd of oracle.pillar.floorplans; with `tape` (h1, h2, L, scores xz, yz, xy of a library forward) every
    layer's value - and the ReLUs' activation pattern - is the library's own while the gradient flows through the layer: the
    exact gradient at the library's intermediates (the `fwd` term of the yardstick)."""
    import torch.nn.functional as F
    from oracle import gather
    torch.set_num_threads(8)
    poses, focal, centre = (t.to(dtype) for t in synth.source_views(cases.NV, *cases.IMG_WH))
    with torch.enable_grad():
        pp = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
        lat = sc["latent"].to(dtype).clone().requires_grad_(True)
        if tape is None:
            fps = oracle.pillar.floorplans(pp, lat, sc["image_wh"], poses, focal, centre, grid)
        else:
            nv = cases.NV
            G0, G1, G2 = grid
            wg = oracle.pillar.world_grid(grid).to(dtype)
            cam = gather.world_to_camera(wg, poses)
            mask = cam[:, :, 2] < 1e-3
            dirs = wg[None] - poses[:, None, :3, -1]
            dirs = dirs / torch.norm(dirs + 1e-9, dim=-1)[:, :, None]
            dirs = dirs * mask[:, :, None]
            uv = -cam[..., :2] / (cam[..., 2:] + 1e-9)
            uv = uv * torch.stack([focal[0], -focal[0]]) + centre[0]
            Hf, Wf = lat.shape[-2:]
            scale = gather.latent_scaling(Hf, Wf).to(dtype) / torch.tensor([float(sc["image_wh"][0]), float(sc["image_wh"][1])], dtype=dtype)
            feat = F.grid_sample(lat, (uv * scale - 1.0).unsqueeze(2), align_corners=True, mode="bilinear", padding_mode="zeros")[:, :, :, 0]
            x = torch.cat([feat, cam.permute(0, 2, 1), dirs.permute(0, 2, 1)], dim=1).permute(0, 2, 1)
            lin = lambda name, t: F.linear(t, pp[name + ".weight"], pp[name + ".bias"])
            sub = lambda y, i: y + (tape[i].to(dtype).reshape(y.shape) - y).detach()
            act = lambda y, i: sub(y * (tape[i].to(dtype).reshape(y.shape) > 0), i)
            h = act(lin("depth_fc.common_branch.0", x), 0)
            h = act(lin("depth_fc.common_branch.2", h), 1)
            L = sub(lin("depth_fc.depth_encoder", h), 2).reshape(nv, G0, G1, G2, -1)
            w3 = wg.reshape(1, G0, G1, G2, 3).expand(nv, -1, -1, -1, -1)
            score = lambda ax, coord, i: sub(lin("pillar_aggregator_%s.2" % ax, torch.relu(lin(
                "pillar_aggregator_%s.0" % ax, torch.cat([L, w3[..., coord:coord + 1]], dim=-1)))), 3 + i)
            w_yz = torch.softmax(score("yz", 0, 1), dim=1)
            w_xz = torch.softmax(score("xz", 1, 0), dim=2)
            w_xy = torch.softmax(score("xy", 2, 2), dim=3)
            fps = (L * w_yz).sum(1), (L * w_xz).sum(2), (L * w_xy).sum(3)
        loss = sum((a * g.to(dtype)).sum() for a, g in zip(fps, cot))
        gr = torch.autograd.grad(loss, [pp[n] for n in NAMES] + [lat])
    return dict(zip(NAMES + ["latent"], gr))


def _tape_parts(fp, grid, nv=cases.NV):
    tape = fp.grad_fn.tape
    M = nv * grid[0] * grid[1] * grid[2]
    parts = [tape[i * M * 512:(i + 1) * M * 512].reshape(M, 512) for i in range(3)]
    return [t.detach().cpu() for t in parts + [tape[3 * M * 512 + a * M:3 * M * 512 + (a + 1) * M] for a in range(3)]]


def _rel(x, ref):
    x, ref = x.double().cpu(), ref.double().cpu()
    return float(x.abs().max()) / (float(ref.abs().max()) + 1e-30), float(x.norm()) / (float(ref.norm()) + 1e-30)


def test_f32_train_forward_is_floorplans():
    sc = cases.small_scene(seed=19)
    enc = _enc(GRID, synth.pillar_state(2), "f32")
    want = _plans(enc, sc["latent"], sc["image_wh"])
    with torch.enable_grad():
        got = enc.floorplans_train(sc["latent"].to(DEV).clone().requires_grad_(True), *_views(), sc["image_wh"])
    for a, b in zip(got, want):
        assert a.requires_grad and torch.equal(a.detach(), b)
    assert enc.last_precision_used == "f32"


@pytest.mark.parametrize("grid", [(12, 10, 8), (64, 4, 9)])
def test_f32_gradients_vs_fp64_oracle(grid):
    """The yardstick of test_gpu_encoder_training.py::test_gradients_vs_fp64_oracle under precision "f32": per tensor, relative
    max and relative L2 of (library - fp64) within 1.5 x what the fp32 oracle misses fp64 by + the forward's own part `fwd` (fp64
    backward at the library's tape vs plain fp64) + 2e-5; then the derivative alone, library vs fp64-at-the-tape, to 1e-5 relative
    L2.  `fwd` is now the exact forward's own and is recorded.  It is NOT near zero on these inputs (MI355X: largest relative L2
    2.1e-3 at (12, 10, 8), on the latent; 1.6e-3 at (64, 4, 9), on pillar_aggregator_xy.0.bias; 6e-6 on the g11 fixture's inputs):
    fp32 intermediates sit ~1e-7 from fp64's, and among ~3 M ReLU units of a forward that still leaves the odd unit on the other
    side of its kink - one flipped unit of depth_fc moves the latent's gradient in four texels by a whole term."""
    sc = cases.small_scene(seed=19)
    params = synth.pillar_state(2)
    enc = _enc(grid, params, "f32")
    cot = _cotangents(grid)
    fps, lib = _library_grads(enc, sc["latent"], sc["image_wh"], cot)
    g64 = _oracle_grads(params, sc, grid, cot, torch.float64)
    g32 = _oracle_grads(params, sc, grid, cot, torch.float32)
    gt = _oracle_grads(params, sc, grid, cot, torch.float64, tape=_tape_parts(fps[0], grid))
    fwd_max, fwd_l2, fwd_at = 0.0, 0.0, None
    for n in NAMES + ["latent"]:
        a, b, r = lib[n], g64[n], g32[n]
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), n
        if n in HEAD_BIAS:
            assert float(a.abs().max()) <= 1e-4, (n, float(a[0]))
            continue
        mine, ref, fwd = _rel(a.cpu().double() - b, b), _rel(r.double() - b, b), _rel(gt[n] - b, b)
        if fwd[1] > fwd_l2:
            fwd_at = n
        fwd_max, fwd_l2 = max(fwd_max, fwd[0]), max(fwd_l2, fwd[1])
        assert mine[0] <= 1.5 * ref[0] + fwd[0] + 2e-5 and mine[1] <= 1.5 * ref[1] + fwd[1] + 2e-5, (n, mine, ref, fwd)
    print("grid", grid, "largest fwd term: rel max %.3g, rel L2 %.3g (%s)" % (fwd_max, fwd_l2, fwd_at))
    record_parity("pillar_f32/grad_fwd_term_%dx%dx%d" % grid, rel_max=fwd_max, rel_l2=fwd_l2, tensor=fwd_at)
    for n in NAMES + ["latent"]:
        if n not in HEAD_BIAS:
            mine = _rel(lib[n].cpu().double() - gt[n], gt[n])
            assert mine[1] <= 1e-5, (n, mine)


def test_f32_gradients_vs_reference_fixture(golden):
    """The yardstick of test_gradients_vs_reference_fixture (g11_pillar_grad, grid (12, 10, 8)) under precision "f32": per stored
    quantity, relative L2 to the reference within 1.5 x fp64 autograd's + the forward's part + 2e-5."""
    g = golden("g11_pillar_grad")
    sc = cases.small_scene()
    params = synth.pillar_state(0)
    enc = _enc(GRID, params, "f32")
    cot = _cotangents(GRID)
    fps, lib = _library_grads(enc, sc["latent"], sc["image_wh"], cot)
    g64 = _oracle_grads(params, sc, GRID, cot, torch.float64)
    gt = _oracle_grads(params, sc, GRID, cot, torch.float64, tape=_tape_parts(fps[0], GRID))
    rl2 = lambda x, ref: float((x - ref).norm()) / (float(ref.norm()) + 1e-30)
    fwd_worst = [0.0]

    def check(what, f, want):
        a, b, t = f(lib[what[0]].cpu().double()), f(g64[what[0]]), f(gt[what[0]])
        want = torch.as_tensor(want).double()
        fwd_worst[0] = max(fwd_worst[0], rl2(t, b))
        assert rl2(a, want) <= 1.5 * rl2(b, want) + rl2(t, b) + 2e-5, (what, rl2(a, want), rl2(b, want), rl2(t, b))

    for n in NAMES:
        key = n.replace(".", "_")
        if lib[n].dim() == 2:
            check((n, "rows"), lambda x: x[::32], g["rows_" + key])
            check((n, "sum"), lambda x: x.sum(1), g["sum_" + key])
            check((n, "sq"), lambda x: (x ** 2).sum(1), g["sq_" + key])
        elif n in HEAD_BIAS:
            assert float(lib[n].abs().max()) <= 1e-4, n
        else:
            check((n,), lambda x: x, g[key])
    check(("latent",), lambda x: x.reshape(-1)[::389], g["latent_strided"])
    print("g11: largest fwd term (rel L2) %.3g" % fwd_worst[0])
    record_parity("pillar_f32/grad_fwd_term_g11", rel_l2=fwd_worst[0])


def test_retried_autograd_call_is_the_f32_run():
    """Default precision, case L: the differentiable forward trips on the latent, runs again on the exact kernels into the same tape,
    and the backward of that tape gives the gradients of an explicit "f32" run: floor-plans, tape and the 18 parameter gradients
    bitwise (fixed-order reductions).  The latent's gradient is scattered with atomics (csrc/pillar_train.hip step 4) and repeats to
    rounding only, between ANY two runs: it is held to the 1e-6 relative L2 of test_repeatable_and_retained_graph."""
    sc = cases.small_scene()
    p2, lat2, _ = P.case_l(synth.pillar_state(0), sc["latent"])
    cot = _cotangents(GRID)
    exact = _enc(GRID, p2, "f32")
    fps_e, want = _library_grads(exact, lat2, sc["image_wh"], cot)
    enc = _enc(GRID, p2)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        fps, got = _library_grads(enc, lat2, sc["image_wh"], cot)
    assert len([w for w in seen if issubclass(w.category, RuntimeWarning)]) == 1
    assert enc.last_precision_used == "f32" and enc._range_latch is None and _flags(enc) == 0
    for a, b in zip(fps, fps_e):
        assert torch.equal(a.detach(), b.detach())
    assert torch.equal(fps[0].grad_fn.tape, fps_e[0].grad_fn.tape)
    for n in NAMES:
        assert torch.equal(got[n], want[n]), n
    assert _rel(got["latent"] - want["latent"], want["latent"])[1] <= 1e-6
    enc.on_range = "raise"
    with pytest.raises(_lib.NeoRangeError):
        _library_grads(enc, lat2, sc["image_wh"], cot)


# ---- 7: end to end -----------------------------------------------------------------------------------------------------------------
class _Spatial(torch.nn.Module):
    """Stands in for the ResNet: emits a fixed latent."""

    def __init__(self, latent):
        super().__init__()
        self.fixed = latent

    def forward(self, images):
        self.latent = self.fixed.to(images.device).contiguous()
        return self.latent


def _attached(pillar, latent, decoder, precision, preproject, convs=None, grid=(8, 8, 8)):
    enc = encoder.GridEncoder(spatial_encoder=_Spatial(latent), grid_size=grid).to(DEV)
    enc.load_state_dict(pillar, strict=False)
    if convs is not None:           # the floor-plan conv nets are initialised from torch's generator: both nets hold the same ones
        enc.load_state_dict(convs, strict=False)
    enc.precision = precision
    enc.eval()
    net = models.NeRF_TP(num_coarse_samples=16, num_fine_samples=24, num_src_views=cases.NV, encoder=enc).to(DEV)
    net.load_state_dict(decoder, strict=False)
    net.precision = precision
    if preproject is not None:
        net.preproject = preproject
    return net


@pytest.fixture
def _deterministic_convs():
    """The floor-plan conv nets (PyTorch / MIOpen, not part of this library) do not repeat bitwise by default: two runs of the same
    encoder differ by 1e-8 in the planes (|planes| <= 0.05), which the samplers turn into up to 9e-7 of depth - the whole 1e-6 the
    comparison below allows.  Their deterministic algorithms take that out: what is left to compare is this library's path."""
    prev = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = prev


def _render_pair(preproject):
    """(frame of the un-normalised encoder + compensated decoder at default precision, the unscaled all-"f32" frame, net)."""
    sc = cases.small_scene()
    params = synth.pillar_state(0)
    p2, lat2, _ = P.case_l(params, sc["latent"])
    batch = {k: v.to(DEV) for k, v in cases.neo_batch(cases.strided_rays(64)).items()}
    ref = _attached(params, sc["latent"], synth.nerf_tp_state(0), "f32", preproject)
    convs = {k: v for k, v in ref.encoder.state_dict().items() if k.startswith("floorplan_convnet")}
    net = _attached(p2, lat2, P.decoder_compensated(synth.nerf_tp_state(0)), None, preproject, convs)
    want = render.render_rays_test(ref, batch, chunk=64, near=0.0, far=0.0)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = render.render_rays_test(net, batch, chunk=64, near=0.0, far=0.0)      # parent: NeoRangeError out of _ensure_scene
    assert [w for w in seen if issubclass(w.category, RuntimeWarning)]
    assert net.encoder_runs == 1 and net.encoder.last_precision_used == "f32"
    assert bool(torch.isfinite(got["rgb"]).all()) and bool(torch.isfinite(got["depth"]).all())
    return got, want, net


def test_unnormalised_encoder_renders_a_frame(_deterministic_convs):
    """The decoder gathers the latent itself (preproject off: the reference's operation order), so the 3.2e5 latent is an operand
    of ITS split arithmetic too: the encoder resolves its own trip, then render_rays_test's retry resolves the decoder's."""
    got, want, net = _render_pair(False)
    assert got["precision_used"] == "f32" and net.last_precision_used == "f32"
    e_rgb, e_depth = max_abs(got["rgb"], want["rgb"]), max_abs(got["depth"], want["depth"])
    print("end to end: max |rgb difference| %.3g, max |depth difference| %.3g" % (e_rgb, e_depth))
    assert e_rgb <= 1e-6 and e_depth <= 1e-6        # the bound of test_state_dict_layout_and_integration between equivalent paths


def test_unnormalised_encoder_with_the_default_preprojection(_deterministic_convs):
    """With the default pre-projection the decoder's split kernels never see the latent itself (it goes through the first-layer
    columns on exact fp32 MFMA first, and the compensated columns bring it back in range): the decoder does not trip, the frame is
    a split-arithmetic frame.  What must hold: no exception, one encoder run, and the house end-to-end tolerance (1e-4, the bound
    of the smoke run and of conftest.check_vs_reference_noise) to the all-"f32" frame."""
    got, want, net = _render_pair(None)
    assert "precision_used" not in got and net.last_precision_used == "f16x3"
    e_rgb, e_depth = max_abs(got["rgb"], want["rgb"]), max_abs(got["depth"], want["depth"])
    print("end to end, pre-projected: max |rgb difference| %.3g, max |depth difference| %.3g" % (e_rgb, e_depth))
    assert e_rgb < 1e-4 and e_depth < 1e-4


# ---- 9: full size ------------------------------------------------------------------------------------------------------------------
def test_f32_full_size_runs_and_agrees_with_split():
    """64^3 x 3 views: finite, two runs bitwise equal, and within 4e-5 of the split result (2e-5 + 2e-5: each arithmetic's bound
    against the oracle, triangle inequality)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    latent = torch.randn(3, 512, 60, 80, device=DEV, generator=g) * 0.3
    poses, focal, centre = (t.to(DEV) for t in synth.source_views(3, 640, 480))
    params = synth.pillar_state(0)
    enc = _enc((64, 64, 64), params, "f32")
    a = enc.floorplans(latent, poses, focal, centre, (640.0, 480.0))
    b = enc.floorplans(latent, poses, focal, centre, (640.0, 480.0))
    split = _enc((64, 64, 64), params).floorplans(latent, poses, focal, centre, (640.0, 480.0))
    worst = 0.0
    for x, y, z in zip(a, b, split):
        assert x.shape == (3, 64, 64, 512) and bool(torch.isfinite(x).all()) and torch.equal(x, y)
        worst = max(worst, float((x - z).abs().max()))
    print("full size: max |f32 - split| %.3g" % worst)
    record_parity("pillar_f32/full_size_vs_split", max_abs=worst)
    assert worst < 4e-5
