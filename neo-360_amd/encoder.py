"""Scene encoder with the pillar stage on the HIP library.

`GridEncoder` mirrors models/neo360/encoder_tp_fusion_conv.py:282-597: same constructor role, `forward(images, poses,
focal, c)` -> (scene_grid_xz, scene_grid_xy, scene_grid_yz), same state_dict keys (`depth_fc.*`,
`pillar_aggregator_{xz,yz,xy}.*`, `floorplan_convnet_{xy,yz,xz}.*`, `spatial_encoder.*`).  What runs where:

  spatial_encoder        the caller's image CNN (the reference's ResNet-34 SpatialEncoder): PyTorch, out of scope
  pillar stage           world grid -> per cell-view [latent | camera xyz | direction] -> depth_fc -> three axis scorers ->
                         softmax-weighted sums = three floor-plans: ONE library call, 1.58 MMAC per cell-view x 786,432
                         cell-views, the part the reference pays 300 x per frame.  Two arithmetics, as on the renderers:
                         "f16x3" (default; csrc/pillar.hip, fp16 MFMA on hi/lo-split operands) and "f32" (csrc/pillar_f32.hip,
                         exact fp32 MFMA) - `precision` / $NEO360_PRECISION choose
  floorplan_convnet_*    the reference's 2-D conv stacks on 64 x 64 floor-plans: PyTorch (MIOpen), once per scene

Attach it to `models.NeRF_TP(encoder=GridEncoder(spatial_encoder=...))`: the module runs it once per distinct src_imgs.
The encoder's `precision` and `on_range` are its own: `NeRF_TP.precision` does not propagate to an attached encoder
($NEO360_PRECISION sets both).

Range guard: a latent texel or a pillar weight at or beyond 65504 cannot be split into fp16 planes.  `on_range = "retry_f32"`
(default; the names are render.render_rays_test's): the same call runs again on the exact kernels into the same output and
tape buffers, a RuntimeWarning says so once per module, `last_precision_used` names the arithmetic of the last call, and when
the operand that left the range is a packed weight (`NeoRangeError.static_operand`) the module is latched to "f32" until its
parameters change (`operands_key()`); a trip on the latent is per call and does not latch.  `on_range = "raise"`: the
NeoRangeError goes to the caller.  An un-normalised encoder therefore never turns a frame into an exception.

Training: with autograd on and a pillar parameter or the latent requiring grad, `forward` runs the pillar stage as a
`torch.autograd.Function` (`_PillarStage`): the same forward kernels in the same arithmetic (bitwise the floor-plans of
`floorplans`) writing their activations to a tape, and a native backward on exact fp32 MFMA (csrc/pillar_train.hip) that returns the
gradients of all nine depth_fc / pillar_aggregator layers (weights and biases) and of the latent.  `differentiable`
(None = automatic, True / False = always / never) overrides the choice, as on the renderers.  No gradient reaches the poses,
focal length or principal point (the reference's cameras are data).
"""
import ctypes
import os
import warnings

import torch
import torch.nn as nn

from . import _lib
from .context import f32, ptr, ptr_table
from .context import dense
from .models import _HipModule, _fingerprint


def _kaiming(m):
    """init_weights_kaiming (encoder_tp_fusion_conv.py:255-260): applies to nn.Linear only."""
    if type(m) == nn.Linear:
        nn.init.kaiming_normal_(m.weight)
        nn.init.uniform_(m.bias, -1e-3, 1e-3)


class DepthPillarEncoder(nn.Module):
    """encoder_tp_fusion_conv.py:263-279 (parameter container; evaluated by the library)."""

    def __init__(self, inp_ch, LS):
        super().__init__()
        self.common_branch = nn.Sequential(nn.Linear(inp_ch, LS), nn.ReLU(inplace=True), nn.Linear(LS, LS), nn.ReLU(inplace=True))
        self.depth_encoder = nn.Linear(LS, LS)
        self.common_branch.apply(_kaiming)
        self.depth_encoder.apply(_kaiming)


def _floorplan_convnet():
    """encoder_tp_fusion_conv.py:375-397 (identical for xy / yz / xz)."""
    return nn.Sequential(
        nn.Conv2d(512, 256, 3, stride=2, padding=1), nn.BatchNorm2d(256), nn.ReLU(inplace=True),
        nn.Conv2d(256, 128, 3, stride=2, padding=1), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
        nn.Conv2d(128, 128, 3, stride=1, padding=1), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
        nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True),
        nn.Conv2d(128, 128, 3, padding=1), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
        nn.Upsample(size=(120, 160), mode="bilinear", align_corners=True),
        nn.Conv2d(128, 128, 3, padding=1))


class GridEncoder(_HipModule):
    LATENT = 512

    def __init__(self, spatial_encoder=None, grid_size=(64, 64, 64), encoder_type="resnet"):
        super().__init__()
        self.grid_size = [int(g) for g in grid_size]
        self.encoder_type = encoder_type
        self.side_lengths = [1, 1, 1]
        if spatial_encoder is not None:
            self.spatial_encoder = spatial_encoder
        self.latent_size = LS = self.LATENT
        self.depth_fc = DepthPillarEncoder(LS + 3 + 3, LS)
        mk = lambda: nn.Sequential(nn.Linear(LS + 1, LS), nn.ReLU(inplace=True), nn.Linear(LS, 1))
        self.pillar_aggregator_xz, self.pillar_aggregator_yz, self.pillar_aggregator_xy = mk(), mk(), mk()
        self.floorplan_convnet_xy, self.floorplan_convnet_yz, self.floorplan_convnet_xz = (_floorplan_convnet() for _ in range(3))
        for m in (self.pillar_aggregator_xz, self.pillar_aggregator_yz, self.pillar_aggregator_xy, self.floorplan_convnet_xy,
                  self.floorplan_convnet_yz, self.floorplan_convnet_xz):
            m.apply(_kaiming)

    # what a tripped range guard of the split arithmetic does: "retry_f32" = the call runs again on the exact fp32 kernels,
    # "raise" = the NeoRangeError goes to the caller (the names of render.render_rays_test's argument)
    on_range = "retry_f32"

    def _wanted_precision(self):
        return self.precision or os.environ.get("NEO360_PRECISION", self.default_precision)

    def _context(self, device, exact=False):
        """exact: this one call runs on the fp32 kernels whatever `precision` says (the next plain call sets it back)."""
        ctx = super()._context(device)
        if exact and ctx._precision != "f32":
            ctx.set_precision("f32")
            ctx._precision = "f32"
        return ctx

    def _run_pillar(self, device, call):
        """One pillar-stage library call, `call(ctx)`, behind the range-guard policy of `on_range`; a retry calls it again with
        the same buffers.  Returns the context the last call ran on."""
        if self.on_range not in ("retry_f32", "raise"):
            raise ValueError("on_range must be 'retry_f32' or 'raise', got %r" % (self.on_range,))
        want = self._wanted_precision()
        retry = self.on_range == "retry_f32" and want != "f32" and bool(self.poll_flags)
        exact = False
        if retry and self._range_latch is not None:
            if self._range_latch == self.operands_key():
                exact = True                 # the packed weights that tripped are still the ones in use: no failed attempt first
            else:
                self._range_latch = None     # parameters changed: the split arithmetic gets another chance
        ctx = self._context(device, exact)
        self._sync_weights(ctx)
        call(ctx)
        used = "f32" if exact else want
        if self.poll_flags:
            try:
                self._raise_flags(ctx.poll_flags())
            except _lib.NeoRangeError as err:
                if not retry or exact:
                    raise
                if not getattr(self, "_warned_range_downgrade", False):
                    self._warned_range_downgrade = True
                    warnings.warn("%s: an operand of the pillar stage left the fp16 range of the split arithmetic (precision "
                                  "'f16x3'); this call (and any later one that trips the guard) runs again on the exact fp32 "
                                  "kernels (~2x slower). Set encoder.precision = 'f32' to skip the failed attempt."
                                  % type(self).__name__, RuntimeWarning, stacklevel=3)
                if getattr(err, "static_operand", False):
                    self._range_latch = self.operands_key()
                ctx = self._context(device, True)
                call(ctx)
                self._raise_flags(ctx.poll_flags())      # the exact kernels raise nothing: the word is clean for the next call
                used = "f32"
        self.last_precision_used = used
        return ctx

    def ordered_layers(self):
        """Upload order fixed by include/neo360_hip.h (neo_enc_upload)."""
        agg = []
        for m in (self.pillar_aggregator_xz, self.pillar_aggregator_yz, self.pillar_aggregator_xy):
            agg += [m[0], m[2]]
        return [self.depth_fc.common_branch[0], self.depth_fc.common_branch[2], self.depth_fc.depth_encoder] + agg

    def _sync_weights(self, ctx):
        layers = self.ordered_layers()
        ws = [f32(l.weight.detach(), "weight") for l in layers]
        bs = [f32(l.bias.detach(), "bias") for l in layers]
        fp = _fingerprint(ws + bs)
        if ctx.uploaded.get("enc") == fp:
            return
        _lib.check(ctx.lib.neo_enc_upload(ctx.handle, ptr_table(ws), ptr_table(bs), ctx.stream()))
        ctx.uploaded["enc"] = fp

    @torch.no_grad()
    def floorplans(self, latent, poses, focal, c, image_wh):
        """The pillar stage alone: latent (NV,512,Hf,Wf), poses (NV,4,4) c2w, focal (NV,), c (NV,2) (view 0's are used
        for every view, encoder_tp_fusion_conv.py:491-493), image_wh = (W,H) of the encoded images.  The latent defines NV; the
        cameras are checked against it (ValueError) and read on the host; any float dtype, any strides.  Returns the
        channels-last floor-plans (yz (NV,G1,G2,512), xz (NV,G0,G2,512), xy (NV,G0,G1,512))."""
        latent = _pillar_inputs(latent, poses, focal, c)
        dev = latent.device
        NV, C, Hf, Wf = latent.shape
        if C != self.LATENT:
            raise _lib.NeoError("the pillar stage is specialised for the reference's 512-channel latent")
        G0, G1, G2 = self.grid_size
        host = poses.detach().float().cpu().contiguous()
        host_poses = (ctypes.c_float * (16 * NV))(*host.reshape(-1).tolist())
        f0 = float(focal[0])
        cx, cy = (float(x) for x in c[0])
        yz = torch.empty(NV, G1, G2, 512, device=dev)
        xz = torch.empty(NV, G0, G2, 512, device=dev)
        xy = torch.empty(NV, G0, G1, 512, device=dev)
        self._run_pillar(dev, lambda ctx: _lib.check(ctx.lib.neo_enc_floorplans(
            ctx.handle, ptr(latent), NV, Hf, Wf, float(image_wh[0]), float(image_wh[1]), host_poses, f0, cx, cy, G0, G1, G2,
            ptr(yz), ptr(xz), ptr(xy), ctx.stream())))
        return yz, xz, xy

    def _pillar_params(self):
        """The pillar stage's parameters in the library's order: the nine weights, then the nine biases."""
        layers = self.ordered_layers()
        return [l.weight for l in layers] + [l.bias for l in layers]

    def _pillar_grad(self, latent):
        """Whether `forward` takes the differentiable pillar stage (`differentiable` overrides the automatic rule)."""
        if self.differentiable is not None:
            return bool(self.differentiable)
        return torch.is_grad_enabled() and (latent.requires_grad or any(p.requires_grad for p in self._pillar_params()))

    def floorplans_train(self, latent, poses, focal, c, image_wh):
        """`floorplans` under autograd: same arguments, same (bitwise) floor-plans, differentiable with respect to the latent
        and the nine depth_fc / pillar_aggregator layers.  Keeps a tape of 3 x 512 + 3 floats per cell-view (4.7 GB at 64^3 x 3
        views) until the backward."""
        return _PillarStage.apply(self, (poses, focal, c, image_wh), latent, *self._pillar_params())

    def forward(self, images, poses, focal, c):
        """GridEncoder.forward (encoder_tp_fusion_conv.py:472-597): images (NV,3,H,W) -> three (NV,128,120,160) planes
        in the reference's return order (xz, xy, yz).  Leaves the pixel-aligned latent in `spatial_encoder.latent`."""
        images = dense(images, "images", (None, None, None, None))      # any float dtype, any strides; the cameras: floorplans
        NV, _, H, W = images.shape
        self.spatial_encoder(images)
        latent = self.spatial_encoder.latent
        if self._pillar_grad(latent):
            yz, xz, xy = self.floorplans_train(latent, poses, focal, c, (W, H))
        else:
            yz, xz, xy = self.floorplans(latent, poses, focal, c, (W, H))
        nchw = lambda t: t.permute(0, 3, 1, 2)
        return self.floorplan_convnet_xz(nchw(xz)), self.floorplan_convnet_xy(nchw(xy)), self.floorplan_convnet_yz(nchw(yz))


def _pillar_inputs(latent, poses, focal, c):
    """The tensor contract of the pillar stage: latent (NV,C,Hf,Wf) on the device defines NV (any float dtype, any strides);
    poses (NV,4,4), focal (NV,) and c (NV,2) are read on the host and may live anywhere.  Returns the latent as the library reads it."""
    latent = dense(latent, "latent", (None, None, None, None))
    nv = latent.shape[0]
    for name, t, shape in (("poses", poses, (nv, 4, 4)), ("focal", focal, (nv,)), ("c", c, (nv, 2))):
        dense(t, name, shape, on_device=False)
    return latent


def _camera_args(poses, focal, c):
    nv = poses.shape[0]
    host = poses.detach().float().cpu().contiguous()
    host_poses = (ctypes.c_float * (16 * nv))(*host.reshape(-1).tolist())
    cx, cy = (float(x) for x in c[0])
    return host_poses, float(focal[0]), cx, cy


class _PillarStage(torch.autograd.Function):
    """The pillar stage under autograd.  Inputs: the encoder, the camera tuple (poses, focal, c, image_wh: no gradient), the
    latent (NV,512,Hf,Wf) and the 18 tensors of `GridEncoder._pillar_params`; outputs the channels-last floor-plans
    (yz, xz, xy).  The tape (h1, h2, L, scores) lives in the autograd context; the backward only reads it, so a retained
    graph differentiates again to the same gradients."""

    @staticmethod
    def forward(ctx_, enc, cams, latent, *params):
        poses, focal, c, image_wh = cams
        latent32 = _pillar_inputs(latent.detach(), poses, focal, c)
        dev = latent32.device
        NV, C, Hf, Wf = latent32.shape
        if C != enc.LATENT:
            raise _lib.NeoError("the pillar stage is specialised for the reference's 512-channel latent")
        G0, G1, G2 = enc.grid_size
        host_poses, f0, cx, cy = _camera_args(poses, focal, c)
        tape = torch.empty(int(_lib.load().neo_enc_train_tape_floats(NV, G0, G1, G2)), device=dev)
        yz = torch.empty(NV, G1, G2, 512, device=dev)
        xz = torch.empty(NV, G0, G2, 512, device=dev)
        xy = torch.empty(NV, G0, G1, 512, device=dev)
        geo = (NV, Hf, Wf, float(image_wh[0]), float(image_wh[1]))
        # a retry after a tripped range guard rewrites the same tape and floor-plans; the tape layout is the same in both arithmetics
        enc._run_pillar(dev, lambda ctx: _lib.check(ctx.lib.neo_enc_floorplans_train(
            ctx.handle, ptr(latent32), *geo, host_poses, f0, cx, cy, G0, G1, G2, ptr(tape), ptr(yz), ptr(xz), ptr(xy), ctx.stream())))
        ctx_.enc, ctx_.tape = enc, tape
        ctx_.args = (geo, host_poses, f0, cx, cy, (G0, G1, G2))
        ctx_.save_for_backward(latent, *params)
        return yz, xz, xy

    @staticmethod
    def backward(ctx_, g_yz, g_xz, g_xy):
        latent, *params = ctx_.saved_tensors
        geo, host_poses, f0, cx, cy, (G0, G1, G2) = ctx_.args
        latent = f32(latent.detach(), "latent")
        dev = latent.device
        ctx = ctx_.enc._context(dev)
        NV = geo[0]
        grads = []
        for g, shape in ((g_yz, (NV, G1, G2, 512)), (g_xz, (NV, G0, G2, 512)), (g_xy, (NV, G0, G1, 512))):
            grads.append(torch.zeros(shape, device=dev) if g is None else f32(g, "floor-plan gradient"))
        ws = [f32(p.detach(), "weight") for p in params[:9]]
        bs = [f32(p.detach(), "bias") for p in params[9:]]
        gw = [torch.zeros_like(w) for w in ws]
        gb = [torch.zeros_like(b) for b in bs]
        g_lat = torch.zeros_like(latent) if ctx_.needs_input_grad[2] else None
        _lib.check(ctx.lib.neo_enc_floorplans_backward(ctx.handle, ptr_table(ws), ptr_table(bs), ptr(latent), *geo, host_poses,
                                                       f0, cx, cy, G0, G1, G2, ptr(ctx_.tape), ptr(grads[0]), ptr(grads[1]),
                                                       ptr(grads[2]), ptr_table(gw), ptr_table(gb), ptr(g_lat), ctx.stream()))
        out = [g if need else None for g, need in zip(gw + gb, ctx_.needs_input_grad[3:])]
        return (None, None, g_lat, *out)
