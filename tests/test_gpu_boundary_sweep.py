"""GPU half of the boundary sweep (docs/boundary_sweep.md): every record of tests/boundary_cases.py is called with each layout
variant of each tensor argument and must return - outputs, and for the differentiable entries gradients - BITWISE what the dense
fp32 call returns (the conversion is exact, so there is no tolerance), leaving the caller's tensors untouched; with each mismatch
variant it must raise on the host, naming an argument, and leave the module as it was.  The backward functions are run with
expanded, sliced, misaligned, fp64 and absent cotangents, and module state (scene, weights, occupancy grid) is installed from
strided and fp64 tensors.

Every tensor of a mismatch case is a leading view of an allocation as large as the largest extent the case implies
(tests/test_boundary_cases_cpu.py asserts that), so a missing check reads memory this test owns and shows as "did not raise"."""
import re

import pytest
import torch

import boundary_cases as B
import cases
from neo360_amd import _lib, encoder, models, ops, render, synth, training

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RECORDS = sorted(B.RECORDS)


class Env:
    ops, training, render = ops, training, render


@pytest.fixture(scope="module")
def env():
    """The package's modules and ONE instance per model class, shared by every case."""
    e = Env()
    e.dev = DEV
    e.c2w = synth.look_at_origin(40.0)
    e.src = {k: v.to(DEV) for k, v in cases.neo_batch({}).items()}
    e.scene = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in cases.small_scene().items()}   # kept alive: weak references
    st = synth.nerf_tp_state(0)
    for k in ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias"):
        st[k] = st[k] + 6.0             # visible opacity on a short march (object_cases.BIAS)
    e.tp = models.NeRF_TP(num_coarse_samples=B.N_COARSE, num_fine_samples=B.N_FINE, num_src_views=cases.NV).to(DEV)
    e.tp.load_state_dict(st)
    e.tp_state = st
    _set_scene(e)
    e.nerf = models.NeRF().to(DEV)
    e.nerf.load_state_dict(synth.vanilla_state(0))
    e.pix = models.PixelNeRF(num_src_views=cases.NV).to(DEV)
    e.pix.load_state_dict(synth.pixelnerf_state(0))
    e.pix.set_scene(e.scene["latent"], e.scene["image_wh"])
    e.mip = models.MipNeRF360(num_prop_samples=B.MIP_COUNTS[0], num_nerf_samples=B.MIP_COUNTS[1]).to(DEV)
    e.mip.load_state_dict(synth.mip360_state(0, weight_gain=0.5))
    e.enc = encoder.GridEncoder(grid_size=B.PILLAR_GRID).to(DEV)
    assert not e.enc.load_state_dict(synth.pillar_state(0), strict=False).unexpected_keys
    torch.manual_seed(0)                # the floor-plan convolutions keep their seeded default initialisation
    e.enc_full = encoder.GridEncoder(spatial_encoder=_FixedLatent(e.scene["latent"]), grid_size=B.PILLAR_GRID).to(DEV)
    assert not e.enc_full.load_state_dict(synth.pillar_state(0), strict=False).unexpected_keys
    return e


class _FixedLatent(torch.nn.Module):
    """Stands in for the ResNet of a GridEncoder: emits the scene's latent."""

    def __init__(self, latent):
        super().__init__()
        self.fixed = latent

    def forward(self, images):
        self.latent = self.fixed
        return self.latent


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is not an assertion: once the device reports one, nothing more of this file is started on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit("the device reported an error, stopping: %s" % err, returncode=3)


def _set_scene(e):
    sc = e.scene
    e.tp.set_scene(sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], sc["latent"], sc["image_wh"])
    e.tp.set_occupancy(B.base()["occ"])


# ---- comparisons ------------------------------------------------------------------------------------------------------------------

def _bits(t):
    t = t.detach()
    if t.is_floating_point():
        return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t.contiguous()


def assert_same(got, want, what):
    """Two nested results hold the same tensors, bit for bit (NaN payloads and the sign of zero included)."""
    a, b = B.flatten(got), B.flatten(want)
    assert len(a) == len(b) and len(a) > 0, what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i, x.shape, y.shape, x.dtype, y.dtype)
        assert torch.equal(_bits(x), _bits(y)), (what, "output %d" % i, float((x.double() - y.double()).abs().max()) if x.numel() else 0.0)


def _snapshot(T):
    return {k: (v.clone(), v.stride(), v.data_ptr(), v._version) for k, v in T.items() if v is not None}


def assert_untouched(T, snap, what):
    for k, (copy, stride, ptr, version) in snap.items():
        v = T[k]
        assert v.stride() == stride and v.data_ptr() == ptr and v._version == version, (what, k)
        assert torch.equal(_bits(v.contiguous()), _bits(copy.contiguous())), (what, k)


def _run(rec, env, T, grads=False):
    """The record's call on T -> (outputs, input gradients in the order of rec.grad).  The leaves are detached views of T's
    tensors: same memory, same strides, same offset."""
    if rec.chain is not None:
        # a training driver: the module call with autograd on takes the operator chain.  Returned with the outputs: the gradient
        # of every parameter of the module except those the record names (accumulated in no fixed order: boundary_cases)
        attr, unordered = rec.chain
        net = getattr(env, attr)
        net.zero_grad(set_to_none=True)
        with torch.enable_grad():
            out = rec.call(env, T)
            rec.scalar(out).backward()
        grads_ = [p.grad.clone() for k, p in net.named_parameters() if p.grad is not None and not k.endswith(unordered or ("\0",))]
        assert len(grads_) >= 8, len(grads_)
        _drop_grads(env)
        return [o.detach() for o in B.flatten(out)], grads_
    if not (grads and rec.grad):
        with torch.no_grad():
            return rec.call(env, T), []
    with torch.enable_grad():
        leaves = dict(T)
        for k in rec.grad:
            leaves[k] = T[k].detach().requires_grad_(True)
        out = rec.call(env, leaves)
        rec.scalar(out).backward()
    _drop_grads(env)            # an operator on a module's weights (the projections) also left gradients on them
    return out, [leaves[k].grad for k in rec.grad]


def _drop_grads(env):
    for net in (env.nerf, env.tp, env.pix, env.mip, env.enc, env.enc_full):
        net.zero_grad(set_to_none=True)
    for t in env.scene.values():
        if isinstance(t, torch.Tensor):
            t.grad = None


def assert_same_grads(got, want, what):
    assert len(got) == len(want)
    for i, (g, d) in enumerate(zip(got, want)):
        if g is None and d is not None:         # no path from the used outputs to this input: autograd's None stands for zeros
            assert not bool(d.any()), (what, i)
            continue
        assert g is not None and d is not None and g.shape == d.shape, (what, i)
        assert torch.equal(_bits(g), _bits(d.to(g.dtype))), (what, "gradient %d" % i)       # exact: the values are the fp32 call's


# ---- layout neutrality --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RECORDS)
def test_layout_neutrality(env, name):
    rec = B.RECORDS[name]
    ran = 0
    for cid, who, layout, T, twin in B.layout_variants(rec, DEV):
        if who != "together" and rec.arg(who).role == "output":
            # a caller-owned output is written through: anything but the dense aligned fp32 tensor is refused, nothing is written
            snap = _snapshot(T)
            with pytest.raises(ValueError, match="out"):
                rec.call(env, T)
            torch.cuda.synchronize()
            assert_untouched(T, snap, cid)
            ran += 1
            continue
        has = B.LAYOUTS[layout][1]
        assert all(has(T[k]) for k in ([who] if who != "together" else [k for k in rec.together if T[k] is not twin[k]])), cid
        snap = _snapshot(T)
        want, want_g = _run(rec, env, twin, grads=True)
        got, got_g = _run(rec, env, T, grads=True)
        assert_same(got, want, cid)
        assert_same_grads(got_g, want_g, cid)
        torch.cuda.synchronize()
        assert_untouched(T, snap, cid)
        ran += 1
    assert ran >= 3 * len(rec.args), (name, ran)


def test_raygen_writes_the_callers_dense_tensors(env):
    rec = B.RECORDS["ops.get_ray_directions_and_rays[out]"]
    T = {k: v.to(DEV) for k, v in rec.build().items()}
    fresh = ops.get_ray_directions_and_rays(4, 8, 6.4, env.c2w, ray_range=(5, 5 + B.R))
    got = rec.call(env, T)
    assert all(a is b for a, b in zip(got, (T["out_rays_o"], T["out_viewdirs"], T["out_rays_d"], T["out_radii"])))
    assert_same(got, fresh, "out=")


# ---- mismatches -----------------------------------------------------------------------------------------------------------------------

def _said(name):
    """What a message calls an argument: its name (without the table's out_ prefix); the grid of the occupancy calls by its noun."""
    return "occupancy grid" if name == "occ" else name[4:] if name.startswith("out_") else name


def _names_it(msg, name):
    return re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(_said(name)), msg) is not None


@pytest.mark.parametrize("name", RECORDS)
def test_mismatches_are_refused_on_the_host(env, name):
    rec = B.RECORDS[name]
    dense = {k: (v.to(DEV) if v is not None else None) for k, v in rec.build().items()}
    before = _run(rec, env, dense)[0]
    before = [t.clone() for t in B.flatten(before)]         # a caller-owned output is overwritten by the next valid call
    ran = 0
    for cid, who, kind, T in B.mismatch_variants(rec, DEV):
        snap = _snapshot(T)
        allowed = (ValueError, TypeError, _lib.NeoError) if kind == "cpu" else (ValueError, TypeError)
        with pytest.raises(allowed) as e:
            _run(rec, env, T)
        msg = str(e.value)
        # the message names the argument - or, in the cases boundary_cases.NAMED_INSTEAD lists one by one, the tensor of the pair
        # that the check is made on (the varied argument is the one that defines the size, the other one is found not to fit it)
        other = B.NAMED_INSTEAD.get(cid)
        assert _names_it(msg, who) or (other is not None and _names_it(msg, other)), (cid, other, msg)
        torch.cuda.synchronize()
        assert_untouched(T, snap, cid)
        # nothing was left half set up and no flag latched: the next valid call is the earlier one, bit for bit
        assert_same(_run(rec, env, dense)[0], before, cid + " -> next valid call")
        ran += 1
    assert ran >= len(rec.args), (name, ran)


# ---- cotangents -----------------------------------------------------------------------------------------------------------------------

DIFFERENTIABLE = [n for n in RECORDS if B.RECORDS[n].grad]


def _forward(rec, env):
    dense = {k: (v.to(DEV) if v is not None else None) for k, v in rec.build().items()}
    leaves = dict(dense)
    for k in rec.grad:
        leaves[k] = dense[k].detach().requires_grad_(True)
    outs = [o for o in B.flatten(rec.call(env, leaves)) if o.is_floating_point() and o.requires_grad]
    return outs, [leaves[k] for k in rec.grad]


def _grads(rec, env, make):
    """Input gradients of a fresh forward for the cotangents make(i, output) (None: that output is not used)."""
    with torch.enable_grad():
        outs, leaves = _forward(rec, env)
        gs = [make(i, o) for i, o in enumerate(outs)]
        used = [(o, g) for o, g in zip(outs, gs) if g is not None]
        return torch.autograd.grad([o for o, _ in used], leaves, [g for _, g in used], allow_unused=True)


def _cot(i, o):
    return B.q(0.25 + torch.rand(tuple(o.shape), generator=torch.Generator().manual_seed(200 + i))).to(o.device)


@pytest.mark.parametrize("name", DIFFERENTIABLE)
def test_cotangent_layouts(env, name):
    rec = B.RECORDS[name]
    dense = _grads(rec, env, _cot)
    assert all(g is not None for g in dense)
    for layout in ("column_slice", "misaligned", "float64"):
        def make(i, o, layout=layout):
            if o.dim() == 0 and layout == "column_slice":       # a scalar loss has no columns
                return _cot(i, o)
            v = B.LAYOUTS[layout][0](_cot(i, o))
            assert B.LAYOUTS[layout][1](v)
            return v
        assert_same_grads(_grads(rec, env, make), dense, "%s/%s" % (name, layout))
    # .sum().backward(): autograd hands the backward an expanded scalar
    ones = _grads(rec, env, lambda i, o: torch.ones_like(o))
    with torch.enable_grad():
        outs, leaves = _forward(rec, env)
        total = sum(o.sum() for o in outs)
        expanded = torch.autograd.grad(total, leaves, allow_unused=True)
    assert_same_grads(expanded, ones, name + "/expanded")
    # an output nobody used: None (or whatever autograd materialises for it) equals a dense zero cotangent
    first = _grads(rec, env, lambda i, o: _cot(i, o) if i == 0 else None)
    zeros = _grads(rec, env, lambda i, o: _cot(i, o) if i == 0 else torch.zeros_like(o))
    assert_same_grads(first, zeros, name + "/unused")


# ---- module state ---------------------------------------------------------------------------------------------------------------------

def _tp_frame(env):
    T = {k: v.to(DEV) for k, v in B.RECORDS["models.NeRF_TP.forward[eval]"].build().items()}
    with torch.no_grad():
        return env.tp(dict(env.src, **T), False, False, 0.0, 0.0, out_depth=True), env.tp.render_skipping(dict(env.src, **T))


def _channels_last_view(x):
    """An NCHW view of a channels-last allocation: what `.permute(0, 3, 1, 2)` of a feature map is."""
    v = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not v.is_contiguous() and torch.equal(v, x)
    return v


def test_set_scene_from_permuted_and_fp64_maps(env):
    want = _tp_frame(env)
    keys = ("plane_xz", "plane_xy", "plane_yz", "latent")
    try:
        for what, make in (("permuted", _channels_last_view), ("fp64", lambda x: x.double()), ("misaligned", B.LAYOUTS["misaligned"][0])):
            maps = [make(env.scene[k]) for k in keys]
            snap = _snapshot(dict(zip(keys, maps)))
            env.tp.set_scene(*maps, env.scene["image_wh"])
            env.tp.set_occupancy(B.base()["occ"])
            assert_same(_tp_frame(env), want, what)
            assert_untouched(dict(zip(keys, maps)), snap, what)
            # the cache rule is the caller's tensor objects at their versions, not the converted copies
            assert env.tp.scene_matches(maps), what
            maps[0].add_(1.0)
            assert not env.tp.scene_matches(maps), what + ": an in-place edit of the caller's plane went unnoticed"
    finally:
        _set_scene(env)
    assert_same(_tp_frame(env), want, "dense scene again")


def test_set_scene_mismatches_leave_no_scene_behind(env):
    """A refused set_scene raises on the host, naming the map.  As for every failed upload (tests/test_gpu_host_r4.py) the module
    then holds NO scene - no tensor set matches, a render says so - rather than a half-installed one, and the next valid set_scene
    renders bitwise what it rendered before."""
    want = _tp_frame(env)
    sc = env.scene
    good = [sc[k] for k in ("plane_xz", "plane_xy", "plane_yz", "latent")]
    big = [torch.zeros(2 * (t.numel() // t.shape[0] + t.numel()), device=DEV) for t in good]     # room for one more view, row or column

    def view(i, shape, dtype=torch.float32):
        n = 1
        for e in shape:
            n *= e
        return big[i][:n].view(shape).to(dtype) if dtype != torch.float32 else big[i][:n].view(shape)

    NVv, C, H, W = good[1].shape
    bad = [(1, "plane_xy", view(1, (NVv, C, H, W - 1))), (1, "plane_xy", view(1, (NVv, C, H + 1, W))), (2, "plane_yz", view(2, (NVv, C, H * W))),
           (2, "plane_yz", view(2, (NVv + 1, C, H, W))), (3, "latent", view(3, (NVv - 1,) + tuple(good[3].shape[1:]))),
           (3, "latent", view(3, tuple(good[3].shape), torch.int32)), (0, "plane_xz", view(0, (NVv, C, H, W, 1))),
           (1, "plane_xy", good[1].cpu()), (3, "latent", None)]
    try:
        for i, name, t in bad:
            maps = list(good)
            maps[i] = t
            with pytest.raises((ValueError, TypeError)) as e:
                env.tp.set_scene(*maps, sc["image_wh"])
            assert name in str(e.value) or (i == 0 and "plane" in str(e.value)), str(e.value)
            assert not env.tp.scene_matches(good) and not env.tp.scene_matches(maps)
            with pytest.raises(_lib.NeoError, match="no scene features"):
                _tp_frame(env)
            _set_scene(env)
            assert_same(_tp_frame(env), want, "after a refused set_scene (%s)" % name)
    finally:
        _set_scene(env)


def test_pixelnerf_set_scene_layouts(env):
    rec = B.RECORDS["models.PixelNeRF.forward"]
    T = {k: v.to(DEV) for k, v in rec.build().items()}
    want = _run(rec, env, T)[0]
    try:
        for what, make in (("permuted", _channels_last_view), ("fp64", lambda x: x.double()), ("misaligned", B.LAYOUTS["misaligned"][0])):
            latent = make(env.scene["latent"])
            env.pix.set_scene(latent, env.scene["image_wh"])
            assert_same(_run(rec, env, T)[0], want, what)
        for bad in (env.scene["latent"][0], env.scene["latent"].int(), env.scene["latent"].cpu()):
            with pytest.raises(ValueError, match="latent"):
                env.pix.set_scene(bad, env.scene["image_wh"])
            assert_same(_run(rec, env, T)[0], want, "after a refused set_scene")
    finally:
        env.pix.set_scene(env.scene["latent"], env.scene["image_wh"])


WEIGHTS = {      # model class -> (record of its frame call, the module in env, its state dict)
    "NeRF": ("models.NeRF.forward", "nerf", lambda env: synth.vanilla_state(0)),
    "NeRF_TP": ("models.NeRF_TP.forward[eval]", "tp", lambda env: env.tp_state),
    "PixelNeRF": ("models.PixelNeRF.forward", "pix", lambda env: synth.pixelnerf_state(0)),
    "MipNeRF360": ("models.MipNeRF360.forward", "mip", lambda env: synth.mip360_state(0, weight_gain=0.5)),
    "GridEncoder": ("encoder.GridEncoder.floorplans", "enc", lambda env: synth.pillar_state(0)),      # the 18 tensors of the pillar stage
}


@pytest.mark.parametrize("cls", sorted(WEIGHTS))
def test_load_state_dict_from_transposed_and_fp64_weights(env, cls):
    """Each class packs its weights through its own upload path (`_upload` / `_upload_extra`): fed from transposed-storage and
    fp64 state dicts the renders are bitwise the dense upload's, and an in-place edit of the parameters reaches the device copy."""
    name, attr, state_of = WEIGHTS[cls]
    rec, net, state = B.RECORDS[name], getattr(env, attr), state_of(env)
    T = {k: v.to(DEV) for k, v in rec.build().items()}
    want = B.flatten(_run(rec, env, T)[0])
    try:
        for what, make in (("transposed", lambda v: v.t().contiguous().t() if v.dim() == 2 else v), ("fp64", lambda v: v.double()),
                           ("misaligned", lambda v: B.LAYOUTS["misaligned"][0](v) if v.is_floating_point() and v.dim() else v)):
            net.load_state_dict({k: make(v.to(DEV)) for k, v in state.items()}, strict=cls != "GridEncoder")
            assert_same(_run(rec, env, T)[0], want, "%s/%s" % (cls, what))
        # the packed device copy follows the parameters' versions: an in-place edit is seen, and undone by the next load
        with torch.no_grad():
            for k, p in net.named_parameters():
                if k.endswith("bias") and k in state:
                    p.add_(0.25)
        moved = B.flatten(_run(rec, env, T)[0])
        assert any(not torch.equal(a, b) for a, b in zip(moved, want)), "an in-place edit of the parameters did not reach the device copy"
    finally:
        net.load_state_dict(state, strict=cls != "GridEncoder")
    assert_same(_run(rec, env, T)[0], want, cls + ": weights loaded again")


def test_occupancy_grid_from_strided_bool_tensors_and_uint8_refused(env):
    want = _tp_frame(env)
    occ = B.base()["occ"].to(DEV)
    wide = torch.zeros(B.G, B.G, B.G + 3, dtype=torch.bool, device=DEV)
    wide[..., 1:-2] = occ
    strided = wide[..., 1:-2]
    assert not strided.is_contiguous()
    try:
        for what, grid in (("strided", strided), ("transposed", occ.permute(2, 1, 0).contiguous().permute(2, 1, 0)), ("cpu", occ.cpu())):
            snap = _snapshot(dict(grid=grid))
            env.tp.set_occupancy(grid)
            assert torch.equal(env.tp.occupancy, occ)
            assert_same(_tp_frame(env), want, what)
            assert_untouched(dict(grid=grid), snap, what)
        # set_occupancy documents a bool grid: uint8 (and a float one) is refused, and the installed grid stays
        for bad in (occ.to(torch.uint8), occ.float(), occ[..., :-1]):
            with pytest.raises(ValueError, match="occupancy grid"):
                env.tp.set_occupancy(bad)
            assert torch.equal(env.tp.occupancy, occ)
            assert_same(_tp_frame(env), want, "after a refused grid")
    finally:
        env.tp.set_occupancy(B.base()["occ"])
