"""CPU: what the host code between torch.autograd and the native MLP chains checks before it touches the library - the exception
type and full message of every shape check of the five public wrappers (validation runs before the device check, so CPU tensors
reach it) - and the weight sync shared by the four renderers, against a stub context."""
import pytest
import torch

from neo360_amd import _lib, models, training

NV, P = 3, 5


def _tp(projected):
    mlp = models.NeRFPPMLP(input_ch=3, num_src_views=NV)
    args = dict(x_enc=torch.zeros(NV, P, 63), cond_rows=torch.zeros(NV * P, 27), world_feat=torch.zeros(NV * P, 128))
    args["pre" if projected else "local_feat"] = torch.zeros(NV * P, 256 if projected else 512)
    fn = training.nerfpp_mlp_projected if projected else training.nerfpp_mlp
    return mlp, args, lambda m, a: fn(m, nv=NV, **a)


def _vanilla():
    return (models.NeRFMLP(), dict(x_enc=torch.zeros(2, 3, 63), dir_enc=torch.zeros(2, 27)), lambda m, a: training.nerf_mlp(m, **a))


def _pix():
    args = dict(x_enc=torch.zeros(NV, P, 63), cond_rows=torch.zeros(NV * P, 27), pre=torch.zeros(NV * P, 128))
    return models.PixelNeRFMLP(), args, lambda m, a: training.pixel_mlp_fused(m, nv=NV, **a)


def _mip():
    args = dict(x0=torch.zeros(4 * 6, 504), d_enc=torch.zeros(4, 27))
    return models.MipNeRF360MLP(4, 256), args, lambda m, a: training.mip_mlp_fused(m, n=6, **a)


WRAPPERS = {"nerfpp_mlp": lambda: _tp(False), "nerfpp_mlp_projected": lambda: _tp(True), "nerf_mlp": _vanilla,
            "pixel_mlp_fused": _pix, "mip_mlp_fused": _mip}

# wrapper -> case -> (exception type, full message); case = the argument given a wrong last dimension (`name:width`),
# `weight:i` / `bias:i` = layer i of ordered_layers() with one dimension off, `ok` = correct shapes on the CPU.  Recorded from
# the code as it was before the shared helpers existed.
EXPECTED = {
    "nerfpp_mlp": {
        "x_enc:60": (ValueError, "x_enc must be (NV, P, 63), got (3, 5, 60)"),
        "cond_rows:24": (ValueError, "cond_rows must be (NV*P, 27) = (15, 27), got (15, 24)"),
        "world_feat:125": (ValueError, "world_feat must be (NV*P, 128) = (15, 128), got (15, 125)"),
        "local_feat:509": (ValueError, "local_feat must be (NV*P, 512) = (15, 512), got (15, 509)"),
        "weight:2": (ValueError, "NeRFPPMLP layer 2: weight (128, 129) / bias (128,), expected (128, 128) / (128,)"),
        "weight:0": (ValueError, "NeRFPPMLP layer 0: weight (128, 704) / bias (128,), expected (128, 703) / (128,)"),
        "bias:1": (ValueError, "NeRFPPMLP layer 1: weight (128, 128) / bias (129,), expected (128, 128) / (128,)"),
        "bias:last": (ValueError, "NeRFPPMLP layer 8: weight (3, 64) / bias (4,), expected (3, 64) / (3,)"),
        "local_feat:509&weight:2": (ValueError, "local_feat must be (NV*P, 512) = (15, 512), got (15, 509)"),
        "ok": (_lib.NeoError, "x_enc is on cpu: the neo360_amd path runs only on a ROCm device (there is no CPU fallback)"),
    },
    "nerfpp_mlp_projected": {
        "x_enc:60": (ValueError, "x_enc must be (NV, P, 63), got (3, 5, 60)"),
        "cond_rows:24": (ValueError, "cond_rows must be (NV*P, 27) = (15, 27), got (15, 24)"),
        "world_feat:125": (ValueError, "world_feat must be (NV*P, 128) = (15, 128), got (15, 125)"),
        "pre:253": (ValueError, "pre must be (NV*P, 256) = (15, 256), got (15, 253)"),
        "weight:2": (ValueError, "layer 2: weight (128, 129) / bias (128,), expected (128, 128) / (128,)"),
        "weight:0": (ValueError, "layer 0: weight (128, 704) / bias (128,), expected (128, 703) / (128,)"),
        "bias:1": (ValueError, "layer 1: weight (128, 128) / bias (129,), expected (128, 128) / (128,)"),
        "bias:last": (ValueError, "layer 8: weight (3, 64) / bias (4,), expected (3, 64) / (3,)"),
        "pre:253&weight:2": (ValueError, "pre must be (NV*P, 256) = (15, 256), got (15, 253)"),
        "ok": (_lib.NeoError, "x_enc is on cpu: the neo360_amd path runs only on a ROCm device (there is no CPU fallback)"),
    },
    "nerf_mlp": {
        "x_enc:60": (ValueError, "x_enc must be (B, N, 63) and dir_enc (B, 27), got (2, 3, 60) / (2, 27)"),
        "dir_enc:24": (ValueError, "x_enc must be (B, N, 63) and dir_enc (B, 27), got (2, 3, 63) / (2, 24)"),
        "weight:2": (ValueError, "NeRFMLP layer 2: weight (256, 257) / bias (256,), expected (256, 256) / (256,)"),
        "weight:0": (ValueError, "NeRFMLP layer 0: weight (256, 64) / bias (256,), expected (256, 63) / (256,)"),
        "bias:1": (ValueError, "NeRFMLP layer 1: weight (256, 256) / bias (257,), expected (256, 256) / (256,)"),
        "bias:last": (ValueError, "NeRFMLP layer 11: weight (3, 128) / bias (4,), expected (3, 128) / (3,)"),
        "dir_enc:24&weight:2": (ValueError, "x_enc must be (B, N, 63) and dir_enc (B, 27), got (2, 3, 63) / (2, 24)"),
        "ok": (_lib.NeoError, "x_enc is on cpu: the neo360_amd path runs only on a ROCm device (there is no CPU fallback)"),
    },
    "pixel_mlp_fused": {
        "x_enc:60": (ValueError, "x_enc must be (NV, P, 63), got (3, 5, 60)"),
        "cond_rows:24": (ValueError, "cond_rows must be (NV*P, 27) = (15, 27), got (15, 24)"),
        "pre:125": (ValueError, "pre must be (NV*P, 128) = (15, 128), got (15, 125)"),
        "weight:2": (ValueError, "PixelNeRF MLP layer 2: weight (128, 129) / bias (128,), expected (128, 128) / (128,)"),
        "weight:0": (ValueError, "PixelNeRF MLP layer 0: weight (128, 576) / bias (128,), expected (128, 575) / (128,)"),
        "bias:1": (ValueError, "PixelNeRF MLP layer 1: weight (128, 128) / bias (129,), expected (128, 128) / (128,)"),
        "bias:last": (ValueError, "PixelNeRF MLP layer 8: weight (3, 128) / bias (4,), expected (3, 128) / (3,)"),
        "pre:125&weight:2": (ValueError, "pre must be (NV*P, 128) = (15, 128), got (15, 125)"),
        "ok": (_lib.NeoError, "x_enc is on cpu: the neo360_amd path runs only on a ROCm device (there is no CPU fallback)"),
    },
    "mip_mlp_fused": {
        "x0:501": (ValueError, "x0 must be (R n, 504) with n = 6, got (24, 501)"),
        "d_enc:24": (ValueError, "d_enc must be (R, 27) = (4, 27), got (4, 24)"),
        "weight:2": (ValueError, "Mip-NeRF 360 MLP layer 2: weight (256, 257) / bias (256,), expected (256, 256) / (256,)"),
        "weight:0": (ValueError, "Mip-NeRF 360 MLP layer 0: weight (256, 505) / bias (256,), expected (256, 504) / (256,)"),
        "bias:1": (ValueError, "Mip-NeRF 360 MLP layer 1: weight (256, 256) / bias (257,), expected (256, 256) / (256,)"),
        "bias:last": (ValueError, "Mip-NeRF 360 MLP layer 7: weight (3, 128) / bias (4,), expected (3, 128) / (3,)"),
        "d_enc:24&weight:2": (ValueError, "d_enc must be (R, 27) = (4, 27), got (4, 24)"),
        "ok": (_lib.NeoError, "x0 is on cpu: the neo360_amd path runs only on a ROCm device (there is no CPU fallback)"),
    },
}


def _case_names(wrapper):
    _, args, _ = WRAPPERS[wrapper]()
    names = ["%s:%d" % (k, v.shape[-1] - 3) for k, v in args.items()]
    return names + ["weight:2", "weight:0", "bias:1", "bias:last", names[-1] + "&weight:2", "ok"]       # a&b: inputs are judged first


def run_case(wrapper, case):
    mlp, args, call = WRAPPERS[wrapper]()
    for part in case.split("&"):
        kind, _, what = part.partition(":")
        if kind in ("weight", "bias"):
            layer = mlp.ordered_layers()[-1 if what == "last" else int(what)]
            old = getattr(layer, kind)
            setattr(layer, kind, torch.nn.Parameter(torch.zeros(*old.shape[:-1], old.shape[-1] + 1)))
        elif kind != "ok":
            args[kind] = torch.zeros(*args[kind].shape[:-1], int(what))
    return call(mlp, args)


@pytest.mark.parametrize("wrapper,case", [(w, c) for w in WRAPPERS for c in _case_names(w)])
def test_wrapper_validation_messages(wrapper, case):
    exc, msg = EXPECTED[wrapper][case]
    with pytest.raises(exc) as e:
        run_case(wrapper, case)
    assert type(e.value) is exc and str(e.value) == msg


# ---- the weight sync of the renderers, against a context that only records ---------------------------------------------------

class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("neo_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


class _StubContext:
    handle = "handle"

    def __init__(self):
        self.uploaded = {}
        self.lib = _RecordingLib()

    def stream(self):
        return "stream"


def _tp_lead(mlp):
    return (mlp.input_ch,)


def _mip_lead(mlp):
    return (mlp.netwidth, mlp.netdepth, 0 if mlp.disable_rgb else 1)


# renderer -> (key in ctx.uploaded, upload function, its MLPs, arguments between the slot and the tables, has the basis pointer behind them)
SYNCS = {
    "NeRF": (lambda: models.NeRF(), "vanilla", "neo_vanilla_upload_mlp", lambda m: (m.coarse_mlp, m.fine_mlp), lambda mlp: (), False),
    "NeRF_TP": (lambda: models.NeRF_TP(), "tp", "neo_tp_upload_mlp",
                lambda m: (m.fg_coarse_mlp, m.fg_fine_mlp, m.bg_coarse_mlp, m.bg_fine_mlp), _tp_lead, False),
    "PixelNeRF": (lambda: models.PixelNeRF(), "pix", "neo_pix_upload_mlp", lambda m: (m.coarse_mlp, m.fine_mlp), lambda mlp: (), False),
    "MipNeRF360": (lambda: models.MipNeRF360(), "mip", "neo_mip_upload_mlp", lambda m: tuple(m.mlps), _mip_lead, True),
}


def _expected_upload(fn, slot, mlp, lead, basis):
    layers = mlp.ordered_layers()
    tail = (mlp.pos_basis_t.data_ptr(),) if basis else ()
    return (fn, "handle", slot, *lead(mlp), [l.weight.data_ptr() for l in layers], [l.bias.data_ptr() for l in layers], *tail, "stream")


def _normalised(call):
    """A recorded call with its pointer tables as lists and its tensor pointers as integers."""
    name, args = call
    return (name, *[list(a) if hasattr(a, "_length_") else a.value if hasattr(a, "value") else a for a in args])


@pytest.mark.parametrize("renderer", list(SYNCS))
def test_weight_sync_uploads_what_changed_and_nothing_else(renderer, monkeypatch):
    make, kind, fn, mlps_of, lead, basis = SYNCS[renderer]
    monkeypatch.setattr(models, "f32", lambda t, name="tensor": t.float().contiguous())       # the device check is not the subject
    net, ctx = make(), _StubContext()
    mlps = mlps_of(net)
    net._sync_weights(ctx)
    assert [_normalised(c) for c in ctx.lib.calls] == [_expected_upload(fn, s, m, lead, basis) for s, m in enumerate(mlps)]
    assert sorted(ctx.uploaded) == [(kind, s) for s in range(len(mlps))]
    if renderer == "NeRF_TP":
        assert [c[1][2] for c in ctx.lib.calls] == [3, 3, 4, 4]
    if renderer == "MipNeRF360":
        assert [c[1][2:5] for c in ctx.lib.calls] == [(256, 4, 0), (256, 4, 0), (1024, 8, 1)]
    net._sync_weights(ctx)
    assert len(ctx.lib.calls) == len(mlps)                      # nothing changed: nothing uploaded
    last = len(mlps) - 1
    with torch.no_grad():
        mlps[last].ordered_layers()[1].bias.add_(1.0)          # in place: same address, new version
    net._sync_weights(ctx)
    assert [_normalised(c) for c in ctx.lib.calls[len(mlps):]] == [_expected_upload(fn, last, mlps[last], lead, basis)]
    with torch.no_grad():                                       # a new tensor at another address (load_state_dict(assign=True), .to())
        mlps[0].ordered_layers()[0].weight = torch.nn.Parameter(mlps[0].ordered_layers()[0].weight.detach().clone())
    net._sync_weights(ctx)
    assert [_normalised(c) for c in ctx.lib.calls[len(mlps) + 1:]] == [_expected_upload(fn, 0, mlps[0], lead, basis)]
    if basis:                                                   # the basis is uploaded with the weights: it is part of the fingerprint
        mlps[1].pos_basis_t.mul_(1.0)
        net._sync_weights(ctx)
        assert [_normalised(c) for c in ctx.lib.calls[len(mlps) + 2:]] == [_expected_upload(fn, 1, mlps[1], lead, basis)]
    n = len(ctx.lib.calls)
    net._sync_weights(ctx)
    assert len(ctx.lib.calls) == n


def test_mode_setter_calls_the_library_only_on_a_change():
    ctx = _StubContext()
    for mode in (3, 3, 0, 0, 3):
        models._HipModule._set_mode(ctx, "_preproject", "neo_tp_set_preproject", mode)
    assert ctx.lib.calls == [("neo_tp_set_preproject", ("handle", 3)), ("neo_tp_set_preproject", ("handle", 0)),
                             ("neo_tp_set_preproject", ("handle", 3))]
    assert ctx._preproject == 3
    models._HipModule._set_mode(ctx, "_pix_preproject", "neo_pix_set_preproject", True)       # PixelNeRF caches the bool, sends the int
    assert ctx.lib.calls[-1] == ("neo_pix_set_preproject", ("handle", 1)) and ctx._pix_preproject is True
