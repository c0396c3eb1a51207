"""Drop-in renderer modules: same constructor arguments, `forward` signatures,
return tuples and `state_dict` keys as the reference's renderer nn.Modules, so
they slot in under the reference's Lit* systems / run.py unchanged (SURVEY.md
§8b).  The parameters are ordinary nn.Linear containers; all arithmetic happens
in the HIP library.

  NeRF      <-> models/vanilla_nerf/model.py:128-216
  NeRF_TP   <-> models/neo360/model.py:162-581 (decoder half; scene features
                come from `set_scene`, or from an attached encoder module)

Inference path only (`randomized=False`, no autograd), as SURVEY.md §8b scopes it.
"""
import ctypes
import math
import os
import warnings
import weakref

import torch
import torch.nn as nn

from . import _lib, ops
from .context import CallOverlap, dense, f32, new_context, ptr, ptr_table
from .context import radii_shapes as _radii_shapes, ray_rows as _ray_rows


def _xavier_linear(n_in, n_out, xavier=True):
    layer = nn.Linear(n_in, n_out)
    if xavier:
        nn.init.xavier_uniform_(layer.weight)
    return layer


def _sample_rows(t, name, rays_o):
    """Caller sample positions (B,N) of a stage-level call: they define N, the rays define B."""
    return dense(t, name, (rays_o.shape[0], None), device=rays_o.device)


def _fingerprint(tensors):
    return tuple((t.data_ptr(), t._version, t.device) for t in tensors)


class _SceneKey:
    """Identity of the inputs an attached encoder was last run on.  Holds STRONG references to the source tensors
    (so the allocator cannot hand their addresses to a later batch) and compares them with `is` + `_version`,
    plus a fingerprint of the encoder's parameters / buffers and its training flag: a new `src_imgs` tensor, an
    in-place edit, `load_state_dict`, an optimizer step or `.train()` all force a re-encode."""

    def __init__(self, tensors, encoder):
        self.tensors = tuple(tensors)
        self.versions = tuple(t._version for t in self.tensors)
        self.enc = self._enc_fp(encoder)

    @staticmethod
    def _enc_fp(encoder):
        if not isinstance(encoder, nn.Module):
            return None
        items = list(encoder.parameters()) + list(encoder.buffers())
        return (encoder.training, tuple((id(t), t.data_ptr(), t._version) for t in items))

    def matches(self, tensors, encoder):
        tensors = tuple(tensors)
        return (len(tensors) == len(self.tensors) and all(a is b for a, b in zip(tensors, self.tensors))
                and tuple(t._version for t in tensors) == self.versions and self._enc_fp(encoder) == self.enc)


class NeRFMLP(nn.Module):
    """Parameter container with the layout of vanilla_nerf/model.py:44-98:
    pts_linears.0..7 (256 wide, skip concat feeds index 5), views_linear.0,
    bottleneck_layer, density_layer, rgb_layer.  Initialisers as the reference
    (xavier_uniform_ on every weight except views_linear.0, default biases)."""

    def __init__(self, min_deg_point=0, max_deg_point=10, deg_view=4, netdepth=8, netwidth=256,
                 netdepth_condition=1, netwidth_condition=128, skip_layer=4, input_ch=3, input_ch_view=3,
                 num_rgb_channels=3, num_density_channels=1):
        super().__init__()
        if (netdepth, netwidth, netdepth_condition, netwidth_condition, skip_layer, input_ch, input_ch_view,
                num_rgb_channels, num_density_channels, min_deg_point, max_deg_point, deg_view) != (
                8, 256, 1, 128, 4, 3, 3, 3, 1, 0, 10, 4):
            raise NotImplementedError("the HIP kernel is specialised for the reference's default NeRFMLP shape")
        pos = ((max_deg_point - min_deg_point) * 2 + 1) * input_ch
        view = (deg_view * 2 + 1) * input_ch_view
        layers = [_xavier_linear(pos, netwidth)]
        for idx in range(netdepth - 1):
            layers.append(_xavier_linear(netwidth + pos if (idx % skip_layer == 0 and idx > 0) else netwidth, netwidth))
        self.pts_linears = nn.ModuleList(layers)
        self.views_linear = nn.ModuleList([_xavier_linear(netwidth + view, netwidth_condition, xavier=False)])
        self.bottleneck_layer = _xavier_linear(netwidth, netwidth)
        self.density_layer = _xavier_linear(netwidth, num_density_channels)
        self.rgb_layer = _xavier_linear(netwidth_condition, num_rgb_channels)

    def ordered_layers(self):
        """Upload order fixed by include/neo360_hip.h (neo_vanilla_upload_mlp)."""
        return list(self.pts_linears) + [self.views_linear[0], self.bottleneck_layer, self.density_layer, self.rgb_layer]


class _HipModule(nn.Module):
    """Shared plumbing: one private library context per module and device,
    parameters re-packed on the device whenever they change."""

    def __init__(self):
        super().__init__()
        self._ctx_cache = {}

    # MLP GEMM arithmetic: "f16x3" = fp16 matrix cores on hi/lo-split fp32 operands (fp32-equivalent,
    # ~3x faster), "f32" = exact fp32 MFMA.  None -> $NEO360_PRECISION or the class default.
    precision = None
    default_precision = "f16x3"
    # The device assertion word (bit 0: the unit-sphere assertion of NeRF_TP, bit 1: the range guard of the split-fp16
    # arithmetic, bit 2 beside it: the operand was a static one - a packed weight beyond either end of the range, a feature map) is read WITHOUT synchronising by default (no sync inside the call):
    #   "deferred"  (default) every call enqueues a read-and-clear of the word behind its kernels; reads that have
    #               completed are looked at when the NEXT call on this module starts, and all of them in
    #               `check_flags()` (which waits) - render.render_rays_test calls it before returning a frame, and a
    #               caller running its own chunk loop calls `model.check_flags()` once before it consumes the results;
    #   "immediate" / True   one stream synchronisation + read after every call: the exception is raised by the very
    #               call that tripped it, exactly like the reference's assert (300 syncs per frame under a chunk loop);
    #   "never" / False   no reads at all; `check_flags()` reads the word on demand.
    poll_flags = "deferred"

    def _flag_mode(self):
        m = self.poll_flags
        if m is True or m == "immediate":
            return "immediate"
        if m is False or m is None or m == "never":
            return "never"
        if m == "deferred":
            return "deferred"
        raise ValueError("poll_flags must be 'deferred', 'immediate' (True) or 'never' (False), got %r" % (m,))

    def check_flags(self):
        """Wait for every outstanding read of the assertion word and raise what it reports (AssertionError for a ray
        that missed the unit sphere, NeoError for the split-fp16 range guard)."""
        for ctx in self._ctx_cache.values():
            flags = ctx.take_flags(wait=True)
            if self._flag_mode() == "never":
                flags |= ctx.poll_flags()
            self._raise_flags(flags)

    def _before_call(self, ctx):
        if self._flag_mode() == "deferred":
            self._raise_flags(ctx.take_flags(wait=False), late=True)      # completed reads of earlier calls; never blocks

    def _after_call(self, ctx):
        mode = self._flag_mode()
        if mode == "immediate":
            self._raise_flags(ctx.poll_flags())
        elif mode == "deferred":
            ctx.post_flags()

    def _context(self, device):
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        ctx = self._ctx_cache.get(key)
        if ctx is None:
            ctx = self._ctx_cache[key] = new_context(device)     # freed by Context's finalizer with the module
        want = self.precision or os.environ.get("NEO360_PRECISION", self.default_precision)
        if getattr(ctx, "_precision", None) != want:
            ctx.set_precision(want)
            ctx._precision = want
        return ctx

    @staticmethod
    def _set_mode(ctx, attr, setter, mode):
        """An integer mode of the library context, set only when it differs from the one cached on `ctx` as `attr`."""
        if getattr(ctx, attr, None) != mode:
            _lib.check(getattr(ctx.lib, setter)(ctx.handle, int(mode)))
            setattr(ctx, attr, mode)

    # the renderer's upload: (key in ctx.uploaded, library function), its MLPs in slot order, and per MLP what the call takes
    # besides the two tables - (arguments in front of them, tensors behind them: uploaded too, so part of the fingerprint)
    _upload = None

    def _mlps(self):
        raise NotImplementedError

    @staticmethod
    def _upload_extra(mlp):
        return (), []

    def _sync_weights(self, ctx):
        """Re-packs on the device every MLP whose parameters moved or changed in place since its last upload."""
        kind, upload = self._upload
        for slot, mlp in enumerate(self._mlps()):
            layers = mlp.ordered_layers()
            ws = [f32(l.weight.detach(), "weight") for l in layers]
            bs = [f32(l.bias.detach(), "bias") for l in layers]
            lead, tail = self._upload_extra(mlp)
            fp = _fingerprint(ws + bs + tail)
            if ctx.uploaded.get((kind, slot)) == fp:
                continue
            _lib.check(getattr(ctx.lib, upload)(ctx.handle, slot, *lead, ptr_table(ws), ptr_table(bs), *[ptr(t) for t in tail],
                                                ctx.stream()))
            ctx.uploaded[(kind, slot)] = fp

    def close(self):
        """Release the library contexts (packed weights, scene features, workspaces) now.  Deferred reads of the
        assertion word that nobody looked at (`poll_flags='deferred'` and no later call / `check_flags()`) are taken
        here; a tripped assertion or range guard becomes a RuntimeWarning instead of vanishing."""
        for ctx in self._ctx_cache.values():
            if ctx.handle and self._flag_mode() == "deferred":
                try:
                    flags = ctx.take_flags(wait=True)
                except Exception:
                    flags = 0
                if flags:
                    warnings.warn("%s.close(): unread device assertions of earlier calls (flags=%d: %s); results of those "
                                  "calls were invalid - call check_flags() before consuming outputs"
                                  % (type(self).__name__, flags & 3, " + ".join(
                                      n for b, n in ((1, "ray missed the unit sphere"), (2, "split-fp16 range guard")) if flags & b)),
                                  RuntimeWarning, stacklevel=2)
            ctx.close()
        self._ctx_cache.clear()

    @staticmethod
    def _raise_flags(flags, late=False):
        """Device assertion word -> the reference's AssertionError / a NeoError for the split-fp16 range guard.
        late: the word was posted by an EARLIER call on this module (deferred mode)."""
        where = " (raised by an earlier call on this module: poll_flags='deferred')" if late else ""
        if flags & 1:
            raise AssertionError("1.0 - p_norm_sq should be greater than 0" + where)
        if flags & 8:
            raise _lib.NeoError("internal error reported by a kernel (flag bit 3: a bounded in-kernel wait ran out); results of that "
                                "call are invalid" + where)
        if flags & 2:
            what = ("weights / feature maps outside the range the split arithmetic keeps fp32 accuracy in (beyond the fp16 range: "
                    "|x| >= 65504 or non-finite; or small everywhere: a linear layer whose largest |w| is below 2^-13 (vanilla, "
                    "Mip-NeRF 360), 2^-11 (NeO-360), 2^-9 (PixelNeRF) or 2^-6 (pillar stage), or a feature map read without "
                    "pre-projection whose largest |x| is below 2^-8)"
                    if flags & 4 else "an operand outside the range the split arithmetic keeps fp32 accuracy in (beyond the fp16 range: "
                    "|x| >= 65504 or non-finite activations / gathered features; or a pillar-stage latent whose largest |x| is below 2^-6)")
            err = _lib.NeoRangeError("split-fp16 arithmetic (precision 'f16x3') met %s: results of that call are invalid; use "
                                     "precision 'f32'" % what + where)
            err.static_operand = bool(flags & 4)
            raise err

    @staticmethod
    def _check_mode(randomized):
        if randomized:
            raise NotImplementedError(
                "randomized=True (stratified jitter / training) is outside the accelerated inference path")

    # Which path a training-shaped call takes (NeRF.forward, NeRF_TP.forward(out_depth=False)):
    #   None (default)  automatic: the differentiable operator chain of training.py when autograd is on and anything that
    #                   could receive a gradient requires one - a parameter of this module (incl. an attached encoder's) or
    #                   a scene tensor given to set_scene; otherwise the fused no-grad kernels;
    #   True / False    always / never the operator chain, whatever autograd says.
    # The operator chain materialises per-point-view feature rows and an activation tape, re-runs an attached encoder per
    # call and synchronises once per call: a forward-only caller outside torch.no_grad() with default nn.Module parameters
    # (requires_grad=True) takes it unless it says `module.differentiable = False` (or wraps the call in no_grad).
    differentiable = None
    _range_latch = None            # render.render_rays_test: operands_key() of the (weights, scene) whose STATIC operands tripped the range guard
    last_precision_used = None     # arithmetic of the last frame render.render_rays_test produced on this module

    # Consecutive fused evaluation calls of one module overlap on the device (context.CallOverlap: two side streams x two scratch
    # lanes of the library context; the caller's stream semantics are unchanged).  What it is for: the reference's own chunk loops
    # - 300 forward calls of 1024 rays per frame (neo360/model.py:861-907, vanilla_nerf/model.py:336-363, model_pixel.py:356-383,
    # mipnerf360/model.py:471-505) - whose calls would otherwise each end on a partly filled machine.
    # False / $NEO360_OVERLAP=0: every call runs on the caller's stream, as before round 6.
    overlap_calls = os.environ.get("NEO360_OVERLAP", "1") != "0"

    def _overlap(self, dev):
        if not self.overlap_calls:
            return None
        table = self.__dict__.setdefault("_overlap_state", {})
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        ov = table.get(key)
        if ov is None:
            ov = table[key] = CallOverlap(torch.device("cuda", key))
        return ov

    def _launch_overlapped(self, ctx, dev, raw, conv, launch):
        """Run `launch()` - output allocation + ONE fused library call + the flag post - on this call's side stream and scratch
        lane (or on the caller's stream when overlap is off); `launch` returns the list of output tensors.  raw / conv: the ray
        tensors as the caller passed them / as the library reads them (fork-point reuse: CallOverlap.begin)."""
        ov = self._overlap(dev)
        if ov is None:
            return launch()
        side, lane, cur = ov.begin(raw, conv)
        ctx.set_lane(lane)
        outs = []
        try:
            with torch.cuda.stream(side):
                outs = launch()
        finally:
            ctx.set_lane(0)
            ov.end(lane, cur, outs)
        return outs

    def _scene_tensors_for_grad(self):
        return ()

    def operands_key(self):
        """Identity of the STATIC operands of the split arithmetic: every parameter (address + version) and the uploaded
        scene.  render.render_rays_test latches a module whose weights / feature maps tripped the range guard to the exact
        kernels for as long as this key stays the same."""
        return (tuple((p.data_ptr(), p._version) for p in self.parameters()), getattr(self, "_scene_serial", 0))

    def _wants_grad(self, randomized=True):
        """randomized: the call's own flag.  An AUTOMATIC switch to the operator chain on a deterministic call (the shape of a
        forward-only caller that merely forgot torch.no_grad(): nn.Module parameters default to requires_grad=True) is announced
        once per module - such a caller wants `module.differentiable = False` or no_grad; a training loop that
        really differentiates a deterministic call sets `module.differentiable = True` and never sees the message."""
        if self.differentiable is not None:
            return bool(self.differentiable)
        if not torch.is_grad_enabled():
            return False
        auto = (any(p.requires_grad for p in self.parameters())
                or any(t is not None and t.requires_grad for t in self._scene_tensors_for_grad()))
        if auto and not randomized and not getattr(self, "_warned_auto_chain", False):
            self._warned_auto_chain = True
            warnings.warn("%s: autograd is on and a parameter / scene tensor requires grad, so this deterministic forward runs on "
                          "the differentiable operator chain (activation tapes, one synchronisation per call) instead of the fused "
                          "kernels.  Forward-only callers: wrap the call in torch.no_grad() or set module.differentiable = False; "
                          "training code: set module.differentiable = True to silence this." % type(self).__name__,
                          RuntimeWarning, stacklevel=3)
        return auto

    def _auto_chain(self):
        """True when the operator chain would be taken by the automatic rule only (nobody asked for it explicitly)."""
        return self.differentiable is None


class NeRF(_HipModule):
    """Vanilla coarse+fine NeRF renderer (vanilla_nerf/model.py:128-216)."""

    def __init__(self, num_levels=2, min_deg_point=0, max_deg_point=10, deg_view=4, num_coarse_samples=64,
                 num_fine_samples=128, use_viewdirs=True, noise_std=0.0, lindisp=False):
        super().__init__()
        if num_levels != 2 or not use_viewdirs or lindisp:
            raise NotImplementedError("only the reference's default 2-level, view-dependent, linear-depth setup")
        self.num_levels = num_levels
        self.min_deg_point, self.max_deg_point, self.deg_view = min_deg_point, max_deg_point, deg_view
        self.num_coarse_samples, self.num_fine_samples = num_coarse_samples, num_fine_samples
        self.use_viewdirs, self.noise_std, self.lindisp = use_viewdirs, noise_std, lindisp
        self.coarse_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view)
        self.fine_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view)

    _upload = ("vanilla", "neo_vanilla_upload_mlp")

    def _mlps(self):
        return (self.coarse_mlp, self.fine_mlp)

    def forward(self, rays, randomized, white_bkgd, near, far, seed=None):
        """rays["rays_o"] (B,3) defines B; rays["rays_d"], rays["viewdirs"] (B,3): any float dtype, any strides.
        Returns [(rgb (B,3), acc (B,), depth (B,))] * 2, as the reference.  randomized=True (stratified samples, random
        quantiles, `noise_std`) or a call that wants gradients (`_wants_grad`: the reference's training_step,
        vanilla_nerf/model.py:281-283) runs on the differentiable operators of training.py (nerf_render_train: NeRFMLP
        with a native backward, samplers on the counter-based generator, compositing with a native backward);
        the deterministic no-grad call is ONE fused library call."""
        if randomized or self._wants_grad(randomized):
            from . import training
            return training.nerf_render_train(self, rays, randomized, white_bkgd, near, far, seed)
        with torch.no_grad():
            return self._forward_fused(rays, white_bkgd, near, far)

    def _forward_fused(self, rays, white_bkgd, near, far):
        raw = (rays["rays_o"], rays["viewdirs"], rays["rays_d"])
        rays_o, viewdirs, rays_d = _ray_rows(rays, ("rays_o", "viewdirs", "rays_d"))
        dev = rays_o.device
        ctx = self._context(dev)
        self._sync_weights(ctx)
        self._before_call(ctx)
        B = rays_o.shape[0]
        outs = []

        def launch():
            outs.extend((torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)) for _ in range(2))
            _lib.check(ctx.lib.neo_vanilla_render(
                ctx.handle, ptr(rays_o), ptr(viewdirs), ptr(rays_d), B, float(near), float(far),
                self.num_coarse_samples, self.num_fine_samples, int(bool(white_bkgd)),
                ptr(outs[0][0]), ptr(outs[0][1]), ptr(outs[0][2]), ptr(outs[1][0]), ptr(outs[1][1]), ptr(outs[1][2]),
                ctx.stream()))
            self._after_call(ctx)
            return [t for lv in outs for t in lv]
        self._launch_overlapped(ctx, dev, raw, (rays_o, viewdirs, rays_d), launch)
        return outs

    @torch.no_grad()
    def eval_mlp(self, level, rays_o, dirs, t):
        """Stage-level access for parity tests: pos_enc + MLP + activations at
        points o + t*dirs.  rays_o (B,3) defines B, dirs (B,3), t (B,N) defines N -> (B,N,4) = (rgb, sigma)."""
        rays_o = dense(rays_o, "rays_o", (None, 3))
        dirs = dense(dirs, "dirs", (rays_o.shape[0], 3), device=rays_o.device)
        t = _sample_rows(t, "t", rays_o)
        ctx = self._context(rays_o.device)
        self._sync_weights(ctx)
        B, N = t.shape
        out = torch.empty(B, N, 4, device=rays_o.device)
        _lib.check(ctx.lib.neo_vanilla_mlp(ctx.handle, level, ptr(rays_o), ptr(dirs), ptr(t), N, B, N, ptr(out),
                                           ctx.stream()))
        self._raise_flags(ctx.poll_flags())     # stage-level access: always immediate
        return out


class NeRFPPMLP(nn.Module):
    """Parameter container with the layout of neo360/model.py:37-108: pts_linears.0..3
    (128 wide; input = pos_enc + 512 local + 128 world; skip concat feeds index 3),
    views_linear.0/.1 (64), bottleneck_layer, density_layer, rgb_layer."""

    def __init__(self, min_deg_point=0, max_deg_point=10, deg_view=4, netdepth=4, netwidth=128,
                 netdepth_condition=2, netwidth_condition=64, skip_layer=2, input_ch=3, input_ch_view=3,
                 num_rgb_channels=3, num_density_channels=1, local_latent_size=512, world_latent_size=128,
                 combine_layer=3, combine_type="average", out_nocs=False, num_src_views=3):
        super().__init__()
        if (netdepth, netwidth, netdepth_condition, netwidth_condition, skip_layer, input_ch_view, num_rgb_channels,
                num_density_channels, local_latent_size, world_latent_size, combine_layer, combine_type, out_nocs,
                min_deg_point, max_deg_point, deg_view) != (4, 128, 2, 64, 2, 3, 3, 1, 512, 128, 3, "average", False,
                                                            0, 10, 4) or input_ch not in (3, 4):
            raise NotImplementedError("the HIP kernel is specialised for the reference's default NeRFPPMLP shape")
        self.input_ch = input_ch
        self.num_src_views = num_src_views
        pos = ((max_deg_point - min_deg_point) * 2 + 1) * input_ch + local_latent_size + world_latent_size
        view = (deg_view * 2 + 1) * input_ch_view
        layers = [_xavier_linear(pos, netwidth)]
        for idx in range(netdepth - 1):
            layers.append(_xavier_linear(netwidth + pos if (idx % skip_layer == 0 and idx > 0) else netwidth, netwidth))
        self.pts_linears = nn.ModuleList(layers)
        self.views_linear = nn.ModuleList([_xavier_linear(netwidth + view, netwidth_condition, xavier=False),
                                           _xavier_linear(netwidth_condition, netwidth_condition)])
        self.bottleneck_layer = _xavier_linear(netwidth, netwidth)
        self.density_layer = _xavier_linear(netwidth, num_density_channels)
        self.rgb_layer = _xavier_linear(netwidth_condition, num_rgb_channels)

    def ordered_layers(self):
        """Upload order fixed by include/neo360_hip.h (neo_tp_upload_mlp)."""
        return list(self.pts_linears) + [self.views_linear[0], self.views_linear[1], self.bottleneck_layer,
                                         self.density_layer, self.rgb_layer]


class NeRF_TP(_HipModule):
    """NeO-360 decoder renderer (neo360/model.py:162-581).

    `forward(rays, randomized, white_bkgd, near, far, out_depth=False)` keeps the
    reference's signature and return tuples.  The scene features the reference's
    GridEncoder produces (three tri-planes + the pixel-aligned latent) are outside the
    accelerated path: provide them once per scene with `set_scene(...)`, or attach any
    `encoder` module with the reference's interface (callable -> three planes, and
    `.spatial_encoder.latent`); an attached encoder is run once per distinct `src_imgs`
    tensor instead of once per chunk (results are identical in eval mode).
    """

    def __init__(self, num_levels=2, min_deg_point=0, max_deg_point=10, deg_view=4, num_coarse_samples=128,
                 num_fine_samples=256, use_viewdirs=True, num_src_views=3, density_noise=0.0, lindisp=False,
                 xyz_min=None, xyz_max=None, is_optimize=False, encoder_type="resnet", feats_c_size=0, attn=False,
                 input_ch_view=3, use_same_stride=False, encoder=None):
        super().__init__()
        if num_levels != 2 or not use_viewdirs or lindisp:
            raise NotImplementedError("only the reference's default 2-level, view-dependent, linear-depth setup")
        self.num_levels, self.num_src_views = num_levels, num_src_views
        self.min_deg_point, self.max_deg_point, self.deg_view = min_deg_point, max_deg_point, deg_view
        self.num_coarse_samples, self.num_fine_samples = num_coarse_samples, num_fine_samples
        self.density_noise, self.lindisp, self.is_optimize = density_noise, lindisp, is_optimize
        if encoder is not None:
            self.encoder = encoder
        self.fg_coarse_mlp = NeRFPPMLP(min_deg_point, max_deg_point, deg_view, num_src_views=num_src_views)
        self.fg_fine_mlp = NeRFPPMLP(min_deg_point, max_deg_point, deg_view, num_src_views=num_src_views)
        self.bg_coarse_mlp = NeRFPPMLP(min_deg_point, max_deg_point, deg_view, num_src_views=num_src_views, input_ch=4)
        self.bg_fine_mlp = NeRFPPMLP(min_deg_point, max_deg_point, deg_view, num_src_views=num_src_views, input_ch=4)
        self.chunk = 1024            # rays per reference forward call (opt.py:195-200)
        self._scene_key = None
        self._scene_ctx = None
        # split path: gather the latent pre-projected through each MLP's first-layer weights (256 instead of 512
        # channels per tap, 51 % fewer MACs per point-view; see csrc/mlp_tp_hp.hip).  False: the reference's order.
        # 2: the tri-planes are pre-projected through the world columns as well (csrc/mlp_tp_hpp.hip): no world GEMM stage.
        # 3 (default): planes projected for the two outside-sphere MLPs only (measured best: profiles/r04_tp_hp_experiments.log).
        self.preproject = {"0": False, "1": True, "2": 2, "3": 3}.get(os.environ.get("NEO360_TP_PREPROJECT", "3"), 3)
        # background culling of the deterministic out_depth=True call (neo_tp_render_culled): None = off (the default path,
        # untouched); a float eps in (0, 1): rays whose foreground transmittance bg_lambda is below eps at BOTH levels skip the two
        # background evaluations and return rgb = fg_rgb, bg_rgb = 0, depth = fg_depth (|rgb change| < 1.002 bg_lambda,
        # |depth change| < 1.001 bg_lambda); every other ray is bitwise the un-culled result.  The training calls do not read it.
        self.cull_background = None
        self.last_cull_survivors = None      # int32 device tensor: rays of the last culled call that kept their background
        self.last_object_hits = None         # int32 device tensor: rays of the last render_objects call that had a box interval
        self.last_instance_pairs = None      # int32 device tensor: hit (instance, ray) pairs of the last render_instances call
        self._occupancy = None               # the installed occupancy grid (set_occupancy): bool (G,G,G) on the device, and its context
        self._occ_ctx = None
        self.last_skip_kept = None           # int64[2] device tensor: kept inside-sphere samples per level of the last render_skipping call
        self.last_terminate_kept = None      # int64[2] device tensor: evaluated inside-sphere samples per level of the last render_terminating call
        self.last_terminate_survivors = None # int32 device tensor: rays of that call whose background ran
        self.last_accel_kept = None          # int64[2] device tensor: evaluated inside-sphere samples per level of the last render_accelerated call
        self.last_accel_survivors = None     # int32 device tensor: rays of that call whose background ran
        self.last_march_kept = None          # int64[4] device tensor: evaluated samples inside / outside the sphere per level of the last render_marching call
        self.last_march_survivors = None     # int32 device tensor: rays of that call whose background ran

    @property
    def cull_background(self):
        return self._cull_background

    @cull_background.setter
    def cull_background(self, eps):
        if eps is not None and not (isinstance(eps, float) and 0.0 < eps < 1.0):
            raise ValueError("cull_background must be None or a float in (0, 1), got %r" % (eps,))
        self._cull_background = eps

    def _context(self, device):
        ctx = super()._context(device)
        mode = int(self.preproject) if (self.preproject in (2, 3) and self.preproject is not True) else int(bool(self.preproject))
        self._set_mode(ctx, "_preproject", "neo_tp_set_preproject", mode)
        return ctx

    def _mlps(self):
        return (self.fg_coarse_mlp, self.fg_fine_mlp, self.bg_coarse_mlp, self.bg_fine_mlp)

    _upload = ("tp", "neo_tp_upload_mlp")

    @staticmethod
    def _upload_extra(mlp):
        return (mlp.input_ch,), []

    @torch.no_grad()
    def set_scene(self, plane_xz, plane_xy, plane_yz, latent, image_wh, preproject=None, _source=None):
        """Scene features in the reference's layout: planes (NV,128,Hp,Wp), latent
        (NV,512,Hf,Wf), image_wh = (W,H) of the source images the latent was encoded from
        (neo360/model.py:267-269).  Re-laid out channels-last on the device, once.  plane_xz defines NV, the plane size and the
        device; the other two planes must have its shape and the latent its NV (ValueError); any float dtype, any strides (a
        permuted view is read by value).  The channel counts the evaluators need (128 / 512) are the library's check (NeoError).
        preproject (None = keep `self.preproject`): see that attribute."""
        src = _source if _source is not None else (plane_xz, plane_xy, plane_yz, latent)
        # the device copy is about to change: until the upload below has succeeded NO tensor set matches it
        # (a failing upload must not leave a fingerprint that names the new tensors next to the old copy)
        self._scene_src = None
        self._scene_ctx = None
        self._occupancy = self._occ_ctx = None      # an occupancy grid describes one scene (neo_tp_set_scene drops the device copy)
        self._scene_key = None        # whoever uploads through an attached encoder records its own key AFTER this call (_ensure_scene);
                                      # an upload from anywhere else (a training step's gather_features) must not leave an eval key behind
        if preproject is not None:
            self.preproject = int(preproject) if (preproject in (2, 3) and preproject is not True) else bool(preproject)
        # plane_xz defines (NV, Cw, Hp, Wp) and the device: the other planes must repeat it, the latent must hold the same NV views
        first = dense(plane_xz, "plane_xz", (None, None, None, None))
        planes = [first] + [dense(p, k, tuple(first.shape), device=first.device) for k, p in (("plane_xy", plane_xy), ("plane_yz", plane_yz))]
        latent = dense(latent, "latent", (first.shape[0], None, None, None), device=first.device)
        ctx = self._context(latent.device)
        NV, Cw, Hp, Wp = planes[0].shape
        _, Cl, Hf, Wf = latent.shape
        _lib.check(ctx.lib.neo_tp_set_scene(ctx.handle, ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), NV, Cw, Hp, Wp,
                                            ptr(latent), Cl, Hf, Wf, float(image_wh[0]), float(image_wh[1]),
                                            ctx.stream()))
        torch.cuda.current_stream(latent.device).synchronize()   # inputs may be freed by the caller
        self._scene_ctx = ctx
        self._scene_serial = getattr(self, "_scene_serial", 0) + 1
        self._scene_wh = (float(image_wh[0]), float(image_wh[1]))
        # identity (weak references, compared with `is`) + versions: a (data_ptr, version, shape) fingerprint alone
        # matches a NEW tensor the caching allocator placed at a freed map's address (a training loop's fresh encoder
        # output at version 0 and the same shape) and the previous step's device copy would be gathered silently.
        # Weak, not strong: an inference caller's 0.5 GB of NCHW maps must stay freeable; a dead reference matches nothing.
        self._scene_src = (tuple(weakref.ref(t) for t in src), tuple(t._version for t in src))

    def scene_matches(self, maps):
        """True when the device-side scene is a copy of exactly these four tensor OBJECTS at their current version."""
        held = getattr(self, "_scene_src", None)
        maps = tuple(maps)
        return (self._scene_ctx is not None and held is not None and len(maps) == len(held[0])
                and all(a is r() for a, r in zip(maps, held[0])) and tuple(t._version for t in maps) == held[1])

    def scene_image_wh(self, rays=None):
        """(W,H) of the source images: from the last set_scene, else from rays["src_imgs"]."""
        wh = getattr(self, "_scene_wh", None)
        if wh is None:
            if rays is None or "src_imgs" not in rays:
                raise _lib.NeoError("image size unknown: call set_scene(...) first or pass rays['src_imgs']")
            wh = (float(rays["src_imgs"].shape[-1]), float(rays["src_imgs"].shape[-2]))
        return wh

    def _ensure_scene(self, rays, dev):
        enc = getattr(self, "encoder", None)
        if enc is None:
            if self._scene_ctx is None:
                raise _lib.NeoError("no scene features: call set_scene(...) or attach an encoder module")
            return
        src = rays["src_imgs"]
        inputs = (src, rays["src_poses"], rays["src_focal"], rays["src_c"])
        if self._scene_key is not None and self._scene_ctx is not None and self._scene_key.matches(inputs, enc):
            return
        planes = enc(*inputs)
        self.set_scene(planes[0], planes[1], planes[2], enc.spatial_encoder.latent,
                       (src.shape[-1], src.shape[-2]))
        self._scene_key = _SceneKey(inputs, enc)
        self.encoder_runs = getattr(self, "encoder_runs", 0) + 1

    def _camera_args(self, rays):
        """Host copies of the source cameras (kernel arguments).  Cached on the identity + version of the three
        tensors: the reference's chunk loop passes the same src_* tensors with every chunk, so only the first call of
        a frame reads them back from the device."""
        src = (rays["src_poses"], rays["src_focal"], rays["src_c"])
        cache = getattr(self, "_cam_cache", None)
        if cache is not None and all(a is b for a, b in zip(src, cache[0])) and tuple(t._version for t in src) == cache[1]:
            return cache[2]
        poses = src[0].detach().float().cpu().contiguous()
        NV = poses.shape[0]
        host_poses = (ctypes.c_float * (16 * NV))(*poses.reshape(-1).tolist())
        focal = float(src[1][0])                            # view 0's intrinsics for every view (model.py:242-244)
        cx, cy = (float(x) for x in src[2][0])
        args = (host_poses, NV, focal, cx, cy)
        self._cam_cache = (src, tuple(t._version for t in src), args)
        return args

    @torch.no_grad()
    def eval_mlp(self, slot, rays, tvals, far=None, chunk=None):
        """Stage-level access for parity tests: feature lookups + pos_enc + NeRFPPMLP +
        activations of one region at given sample positions.  slot 0/1 = fg coarse/fine
        (tvals = t), 2/3 = bg coarse/fine (tvals = descending inverse radius, needs far).
        rays["rays_o"] (B,3) defines B, rays["rays_d"] / rays["viewdirs"] (B,3), tvals (B,N) defines N, far (B,) or (B,1).
        Returns (B,N,4) = (rgb, sigma)."""
        rays_o, rays_d, viewdirs = _ray_rows(rays)
        tvals = _sample_rows(tvals, "tvals", rays_o)
        far = dense(far, "far", [(rays_o.shape[0],), (rays_o.shape[0], 1)], device=rays_o.device) if far is not None else None
        ctx = self._context(rays_o.device)
        self._ensure_scene(rays, rays_o.device)
        self._sync_weights(ctx)
        B, N = tvals.shape
        host_poses, NV, focal, cx, cy = self._camera_args(rays)
        out = torch.empty(B, N, 4, device=rays_o.device)
        _lib.check(ctx.lib.neo_tp_mlp(ctx.handle, slot, ptr(rays_o), ptr(rays_d), ptr(viewdirs), ptr(tvals), ptr(far),
                                      B, N, int(chunk or max(B, 1)), host_poses, NV, focal, cx, cy, ptr(out),
                                      ctx.stream()))
        self._raise_flags(ctx.poll_flags())       # also clears the word: a miss here must not fail a later forward()
        return out

    @torch.no_grad()
    def sample_positions(self, rays, chunk=None):
        """The sample positions of the deterministic render of these rays, per level: [(fg_t (B,N), bg_s (B,N))] with N = 129,
        385 at the reference's counts - the rows the fused call's evaluators run at (level 1: sort(level-0 positions + the
        inverse-CDF samples of the level-0 weights), neo360/helper.py:218-249).  The deterministic training-shaped call and the
        evaluation call launch the same kernels in the same order, so these are bitwise the positions behind
        `forward(..., out_depth=True)`.  For parity work: an oracle evaluated AT these positions is comparable ray by ray, with
        no allowance for the ill-conditioning of the resampling itself (tests/test_gpu_fullsize.py)."""
        levels = self._forward_train(rays, False, False, chunk, None, _raw=True)
        return [(t["fg_t"], t["bg_t"]) for t in levels]

    def _forward_train(self, rays, randomized, white_bkgd, chunk=None, seed=None, _raw=False):
        """out_depth=False: per level (comp_rgb, fg_weights, bg_weights, fg_sdist, bg_sdist, bg_acc)
        (neo360/model.py:531-579), forward values only.  randomized=True draws the stratified level-0 jitter and the
        level-1 quantiles from the library's counter-based generator (`seed`, default: one fresh seed per call from
        torch's CPU generator, so torch.manual_seed makes runs repeatable)."""
        if self.density_noise != 0.0 and randomized:
            raise _lib.NeoError("density_noise is applied by the operator chain (training.tp_render_train), not by the fused call")
        rays_o, rays_d, viewdirs = _ray_rows(rays)
        dev = rays_o.device
        ctx = self._context(dev)
        self._ensure_scene(rays, dev)
        if self._scene_ctx is not ctx:
            raise _lib.NeoError("scene features were uploaded on a different device")
        self._sync_weights(ctx)
        self._before_call(ctx)
        B = rays_o.shape[0]
        host_poses, NV, focal, cx, cy = self._camera_args(rays)
        if randomized:
            seed = int(seed) if seed is not None else int(torch.randint(1, 2 ** 62, (1,)).item())
            seed = seed or 1
        else:
            seed = 0
        n0, n1 = self.num_coarse_samples + 1, self.num_coarse_samples + 1 + self.num_fine_samples
        levels, structs = [], []
        for n in (n0, n1):
            t = dict(rgb=torch.empty(B, 3, device=dev), fg_w=torch.empty(B, n, device=dev), bg_w=torch.empty(B, n, device=dev),
                     fg_t=torch.empty(B, n, device=dev), bg_t=torch.empty(B, n, device=dev), bg_acc=torch.empty(B, device=dev))
            levels.append(t)
            structs.append(_lib.TpTrainOut(t["rgb"].data_ptr(), t["fg_w"].data_ptr(), t["bg_w"].data_ptr(), t["fg_t"].data_ptr(),
                                           t["bg_t"].data_ptr(), t["bg_acc"].data_ptr(), None, None))
        _lib.check(ctx.lib.neo_tp_render_train(
            ctx.handle, ptr(rays_o), ptr(rays_d), ptr(viewdirs), B, int(chunk or max(B, 1)), host_poses, NV, focal, cx, cy,
            self.num_coarse_samples, self.num_fine_samples, int(bool(white_bkgd)), seed,
            ctypes.byref(structs[0]), ctypes.byref(structs[1]), ctx.stream()))
        self._after_call(ctx)
        if _raw:
            return levels
        out = []
        for t in levels:
            fg_t, bg_t = t["fg_t"], t["bg_t"]
            fg_sd = 0.5 * (fg_t[..., 1:] + fg_t[..., :-1])                                   # model.py:564-571
            fg_sd = torch.cat([fg_sd, (fg_sd[:, -1] + (fg_sd[:, -1] - fg_sd[:, -2])).unsqueeze(-1)], dim=-1)
            bg_sd = torch.cat([0.5 * (bg_t[..., 1:] + bg_t[..., :-1]), bg_t[..., -1:]], dim=-1)
            out.append((t["rgb"], t["fg_w"], t["bg_w"], fg_sd, bg_sd, t["bg_acc"]))
        return out

    def _maps_for_grad(self, rays):
        """The four scene tensors a differentiable call gathers from (and sends gradients to): an attached encoder is run
        WITH autograd on this batch, as the reference's forward does (neo360/model.py:281-300); otherwise the very tensors
        given to `set_scene`, if the caller still holds them."""
        enc = getattr(self, "encoder", None)
        if enc is not None:
            src = rays["src_imgs"]
            planes = enc(src, rays["src_poses"], rays["src_focal"], rays["src_c"])
            self._scene_wh = (float(src.shape[-1]), float(src.shape[-2]))
            return planes[0], planes[1], planes[2], enc.spatial_encoder.latent
        held = getattr(self, "_scene_src", None)
        maps = tuple(r() for r in held[0]) if held is not None else ()
        if len(maps) != 4 or any(m is None for m in maps):
            raise _lib.NeoError("a differentiable forward needs the scene tensors: attach an encoder module, or keep the four "
                                "tensors passed to set_scene(...) alive (the module holds only weak references to them)")
        return maps

    def _scene_tensors_for_grad(self):
        held = getattr(self, "_scene_src", None)
        return tuple(r() for r in held[0]) if held is not None else ()

    def forward(self, rays, randomized, white_bkgd, near, far, out_depth=False, chunk=None, seed=None, fine_only=False):
        """out_depth=True (evaluation, neo360/model.py:521-527): per level (comp_rgb, fg_rgb, bg_rgb, fg_acc, bg_lambda,
        comp_depth), randomized=False.  With `fine_only=True` that call returns [None, level-1 tuple]: the coarse level then
        only delivers the densities the fine samples are drawn from (no level-0 tensors, density-only coarse launches where the
        evaluator has them); the level-1 tuple is bitwise the default call's.  With `self.compute_extras` every returned level gains
        a seventh element, the dict of opacity / disparity / distance percentiles described at that attribute.  out_depth=False (the training call, :531-579): per level (comp_rgb, fg_weights,
        bg_weights, fg_sdist, bg_sdist, bg_acc), randomized as asked.  `near`/`far` are ignored
        exactly as in the reference (:277-278).  All rays of the call form ONE reference chunk unless `chunk` is given
        (whole-frame rendering, see render.py).
        The training call is DIFFERENTIABLE when `_wants_grad()` says so (`self.differentiable`; default: autograd on and a
        parameter, an attached encoder's parameter or a set_scene tensor requires grad - the reference's training_step,
        model.py:697-820): it then runs on the operators of training.py (lookups, NeRFPPMLP with a native backward,
        compositing) instead of the fused no-grad kernels; same return tuple, same samples for one seed at any `chunk`."""
        if not out_depth:
            # density_noise (model.py:381-384) exists on the operator chain only: a randomized call with it takes that path
            if self._wants_grad(randomized) or (randomized and self.density_noise != 0.0):
                from . import training
                maps = None
                try:
                    maps = self._maps_for_grad(rays)
                except _lib.NeoError:
                    # the scene tensors are gone (weak references): only an EXPLICIT request for gradients makes that an error; a
                    # deterministic call that got here by the automatic rule falls back to the fused kernels
                    if randomized or not self._auto_chain():
                        raise
                if maps is not None:
                    return training.tp_render_train(self, rays, randomized, white_bkgd, maps, chunk, seed)
            with torch.no_grad():
                return self._forward_train(rays, randomized, white_bkgd, chunk, seed)
        with torch.no_grad():
            return self._forward_eval(rays, randomized, white_bkgd, chunk, fine_only)

    # Opt-in extras of the deterministic out_depth=True call (neo_tp_render_extras, csrc/tp_extras.hip).  True: every returned
    # level's tuple gains a SEVENTH element, dict(opacity (B,), disparity (B,), distance_percentiles (B, len(extras_quantiles))) of
    # the ray's whole interval histogram, inside and outside the sphere together, as DISTANCES ALONG THE RAY (the unit of the ray
    # parameter t of o + t d, i.e. of the reference's fg_depth - its comp_depth adds a disparity to a distance, model.py:523):
    # the total opacity (fg_acc + bg_lambda * bg_acc, which the six-tuple does not carry), the expected disparity, and the distance
    # at each quantile of the cumulative mass (+inf where the ray leaves with more transmittance than the quantile allows) - with the
    # default three quantiles also as distance_percentile_5 / distance_median / distance_percentile_95.  Definitions: ops.tp_extras.
    # The first six elements are bitwise those of the call without it; the level-1 composites then also write their weights and one
    # small launch per level follows.  False (default): the six-tuples and the launch list are unchanged.  Not combined with
    # `cull_background` (a culled ray has no outside rows): ValueError.  The training calls do not read it.
    compute_extras = False
    extras_quantiles = (0.05, 0.5, 0.95)      # at most 8, ascending, in [0, 1]
    _DEFAULT_EXTRAS_QUANTILES = (0.05, 0.5, 0.95)

    def _frame_call(self, rays, chunk=None, use_grid=False):
        """The prologue every fused frame call of this module shares (`_TpFrameCall`): the ray tensors are converted here, the
        device context is not touched before `.run(...)`."""
        return _TpFrameCall(self, rays, chunk, use_grid)

    _LEVEL_KEYS = ("rgb", "fg_rgb", "bg_rgb", "fg_acc", "bg_lambda", "depth")

    @classmethod
    def _level_out(cls, B, dev):
        """One level's outputs of an out_depth=True frame: the six tensors by name and the TpLevelOut that points at them."""
        t = dict(rgb=torch.empty(B, 3, device=dev), fg_rgb=torch.empty(B, 3, device=dev),
                 bg_rgb=torch.empty(B, 3, device=dev), fg_acc=torch.empty(B, device=dev),
                 bg_lambda=torch.empty(B, 1, device=dev), depth=torch.empty(B, device=dev))
        return t, _lib.TpLevelOut(*(t[k].data_ptr() for k in cls._LEVEL_KEYS))

    @classmethod
    def _level_tuple(cls, t):
        return tuple(t[k] for k in cls._LEVEL_KEYS)

    @staticmethod
    def _edit_samples(t, B, n, dev, return_samples):
        """Adds the sample rows (fg_t, fg_w, bg_s) to level dict `t` when asked for; returns the TpEditSamples over whichever of
        its optional rows `t` holds (these and `visibility`), or None when it holds none."""
        if return_samples:
            t.update(fg_t=torch.empty(B, n, device=dev), fg_w=torch.empty(B, n, device=dev), bg_s=torch.empty(B, n, device=dev))
        names = [k for k, _ in _lib.TpEditSamples._fields_]
        if not any(k in t for k in names):
            return None
        return _lib.TpEditSamples(*(t[k].data_ptr() if k in t else None for k in names))

    def _forward_eval(self, rays, randomized, white_bkgd, chunk=None, fine_only=False):
        self._check_mode(randomized)
        extras_on = bool(self.compute_extras)
        if extras_on:
            if self.cull_background is not None:
                raise ValueError("compute_extras and cull_background are not combined: a culled ray has no outside rows")
            quant = tuple(float(q) for q in self.extras_quantiles)
            if len(quant) > ops.MAX_EXTRA_QUANTILES:
                raise ValueError("at most %d extras_quantiles, got %d" % (ops.MAX_EXTRA_QUANTILES, len(quant)))
        call = self._frame_call(rays, chunk, use_grid=True)
        B, dev = call.B, call.dev
        levels = []
        extras, extra_structs = [None, None], [None, None]
        eps = self.cull_background

        def launch():
            ctx = call.ctx
            structs = []
            for level in range(2):
                if level == 0 and fine_only:       # NULL level 0: the library runs the coarse launches for their densities alone
                    levels.append(None)
                    structs.append(None)
                    continue
                t, struct = self._level_out(B, dev)
                levels.append(t)
                structs.append(struct)
                if extras_on:
                    e = dict(opacity=torch.empty(B, device=dev), disparity=torch.empty(B, device=dev),
                             distance_percentiles=torch.empty(B, len(quant), device=dev))
                    extras[level] = e
                    extra_structs[level] = _lib.TpExtrasOut(*(e[k].data_ptr() for k in ("opacity", "disparity", "distance_percentiles")))
            args = call.ray_args + call.frame_args + (
                int(bool(white_bkgd)), ctypes.byref(structs[0]) if structs[0] is not None else None, ctypes.byref(structs[1]))
            extra = []
            if extras_on:
                tab = ops._quantile_table(quant, dev) if quant else None
                _lib.check(ctx.lib.neo_tp_render_extras(
                    *args, ptr(tab), len(quant), *(ctypes.byref(x) if x is not None else None for x in extra_structs), ctx.stream()))
                extra += [v for e in extras if e is not None for v in e.values()]
            elif eps is None:
                _lib.check(ctx.lib.neo_tp_render(*args, ctx.stream()))
            else:
                # the survivor count stays on the device: written by the compaction, never read inside the call
                extra.append(torch.empty((), dtype=torch.int32, device=dev))
                _lib.check(ctx.lib.neo_tp_render_culled(*args, eps, extra[0].data_ptr(), ctx.stream()))
            self._after_call(ctx)
            return [v for t in levels if t is not None for v in t.values()] + extra
        made = call.run(launch)
        if eps is not None:
            self.last_cull_survivors = made[-1]
        out = [None if t is None else self._level_tuple(t) for t in levels]
        if extras_on:
            for level, e in enumerate(extras):
                if e is None:
                    continue
                if quant == self._DEFAULT_EXTRAS_QUANTILES:
                    pct = e["distance_percentiles"]
                    e.update(distance_percentile_5=pct[:, 0], distance_median=pct[:, 1], distance_percentile_95=pct[:, 2])
                out[level] = out[level] + (e,)
        return out

    @staticmethod
    def _object_bound(rays, given, key, B):
        t = given if given is not None else (rays.get(key) if hasattr(rays, "get") else None)
        if t is None:
            raise ValueError("render_objects needs %s: pass it or put it into the batch as rays[%r]" % (key, key))
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError("%s must be a floating-point tensor, got %r" % (key, type(t).__name__ if not isinstance(t, torch.Tensor) else t.dtype))
        if tuple(t.shape) not in ((B,), (B, 1)):
            raise ValueError("%s must have shape (%d,) or (%d, 1) like the rays, got %s" % (key, B, B, tuple(t.shape)))
        return t

    @torch.no_grad()
    def render_objects(self, rays, near_obj=None, far_obj=None, white_bkgd=True, chunk=None, return_samples=False):
        """Object-level evaluation render (neo_tp_render_objects): the two foreground MLPs marched between a per-ray interval
        [near_obj, far_obj] - what `ops.sample_rays_in_bbox` returns for all boxes of a scene, or for one of them - only for the
        rays that have one.  Deterministic (randomized=False), no background, no unit-sphere intersection or assertion.

        Bounds default to rays["near_obj"] / rays["far_obj"] (the reference's batch keys, datasets/nerds360_ae.py:869-872); shape
        (B,) or (B, 1), any float dtype, on the rays' device.  Hit rule: lo = max(near_obj, 1e-4), hi = far_obj; a ray is a hit
        iff both are finite and hi > lo (a NaN bound is a miss, and so is the reference's 0 = "no hit" sentinel).
        Returns [(rgb (B,3), acc (B,), depth (B,))] for the two levels; with return_samples also (t0 (B, n_coarse+1),
        t1 (B, n_coarse+1+n_fine)), the sample rows of the hit rays.  Missed rays: rgb = 1 if white_bkgd else 0, acc = depth = 0,
        zero sample rows.  `chunk` as in forward (quirk Q1: a ray's direction index comes from its own index, B and chunk, never
        from which other rays hit).  `last_object_hits` receives the number of hit rays as a device int32 scalar that this call
        never reads.  Reads neither `cull_background` nor `ray_grid`."""
        B = rays["rays_o"].shape[0]
        raw_near = self._object_bound(rays, near_obj, "near_obj", B)
        raw_far = self._object_bound(rays, far_obj, "far_obj", B)
        call = self._frame_call(rays, chunk)
        dev = call.dev
        near_c = f32(raw_near, "near_obj").reshape(B)
        far_c = f32(raw_far, "far_obj").reshape(B)
        if near_c.device != dev or far_c.device != dev:
            raise ValueError("near_obj / far_obj must be on the rays' device (%s)" % (dev,))
        levels = []

        def launch():
            ctx = call.ctx
            structs = []
            for n in call.n:
                t = dict(rgb=torch.empty(B, 3, device=dev), acc=torch.empty(B, device=dev), depth=torch.empty(B, device=dev))
                if return_samples:
                    t["tvals"] = torch.empty(B, n, device=dev)
                levels.append(t)
                structs.append(_lib.TpObjectOut(t["rgb"].data_ptr(), t["acc"].data_ptr(), t["depth"].data_ptr(),
                                                t["tvals"].data_ptr() if return_samples else None))
            hits = torch.empty((), dtype=torch.int32, device=dev)     # written by the compaction, never read inside the call
            _lib.check(ctx.lib.neo_tp_render_objects(
                *call.ray_args, ptr(near_c), ptr(far_c), *call.frame_args, int(bool(white_bkgd)),
                ctypes.byref(structs[0]), ctypes.byref(structs[1]), hits.data_ptr(), ctx.stream()))
            self._after_call(ctx)
            return [v for t in levels for v in t.values()] + [hits]
        made = call.run(launch, (raw_near, raw_far), (near_c, far_c))
        self.last_object_hits = made[-1]
        out = [(t["rgb"], t["acc"], t["depth"]) for t in levels]
        if return_samples:
            out.append((levels[0]["tvals"], levels[1]["tvals"]))
        return out

    MAX_INSTANCES = 32

    @torch.no_grad()
    def render_instances(self, rays, near_inst, far_inst, white_bkgd=True, chunk=None, per_instance=True):
        """Every instance of a scene in ONE call (neo_tp_render_instances), with the depth-ordered composite of the instances and
        the visible-instance id of every ray.  near_inst / far_inst: (K,B) or (K,B,1), any float dtype, on the rays' device,
        0 <= K <= 32 - what `ops.sample_rays_in_bbox_list` returns.  Deterministic (randomized=False), no background, no
        unit-sphere intersection or assertion, exactly as `render_objects`; reads neither `cull_background` nor `ray_grid`;
        `chunk` as in forward.

        Pair (i, ray) is a hit by the rule of `render_objects` on near_inst[i, ray], far_inst[i, ray]: lo = max(near, 1e-4),
        hi = far, hit iff both are finite and hi > lo (a NaN bound is a miss).  The hit pairs are compacted on the device and
        evaluated in K windows of at most B rows on the kernels of `render_objects`.

        Returns dict(instances=..., composite=...), two levels each:
          instances  [(rgb (K,B,3), acc (K,B), depth (K,B))] - row i is BITWISE `render_objects(rays, near_inst[i], far_inst[i],
                     white_bkgd, chunk)`, missed rays included (rgb = 1 or 0, acc = depth = 0); None when per_instance=False;
          composite  [(rgb (B,3), acc (B,), depth (B,), instance_id (B,) int32)] - the ray's hit instances in ascending lo (ties
                     to the lower index), each with its premultiplied colour p_i (its white_bkgd=False rgb), a_i = acc, d_i =
                     depth; from T = 1, rgb = depth = acc = 0, best = 0, id = -1: v = T a_i; rgb += T p_i; depth += T d_i;
                     acc += v; if v > best: best = v, id = i; T = T (1 - a_i); then rgb += 1 - acc if white_bkgd.  Plain fp32
                     in that order.  A ray without hits: rgb = 1 or 0, acc = depth = 0, id = -1.
        Intervals of overlapping boxes are marched independently, so density inside an overlap counts twice.
        `last_instance_pairs` receives the number of hit pairs as a device int32 scalar that this call never reads."""
        B = rays["rays_o"].shape[0]
        K = ops._edit_bounds(near_inst, far_inst, B, rays["rays_o"].device, None)
        call = self._frame_call(rays, chunk)
        dev = call.dev
        near_c, far_c = ops._edit_rows(near_inst, far_inst, K, B)
        levels = []

        def launch():
            ctx = call.ctx
            structs = []
            for _ in range(2):
                t = dict(comp_rgb=torch.empty(B, 3, device=dev), comp_acc=torch.empty(B, device=dev),
                         comp_depth=torch.empty(B, device=dev), instance_id=torch.empty(B, dtype=torch.int32, device=dev))
                if per_instance:
                    t.update(rgb=torch.empty(K, B, 3, device=dev), acc=torch.empty(K, B, device=dev), depth=torch.empty(K, B, device=dev))
                levels.append(t)
                structs.append(_lib.TpInstanceOut(*(t[k].data_ptr() if k in t else None for k, _ in _lib.TpInstanceOut._fields_)))
            pairs = torch.empty((), dtype=torch.int32, device=dev)    # written by the compaction, never read inside the call
            _lib.check(ctx.lib.neo_tp_render_instances(
                *call.ray_args, ptr(near_c), ptr(far_c), K, *call.frame_args, int(bool(white_bkgd)),
                ctypes.byref(structs[0]), ctypes.byref(structs[1]), pairs.data_ptr(), ctx.stream()))
            self._after_call(ctx)
            return [v for t in levels for v in t.values()] + [pairs]
        made = call.run(launch, (near_inst, far_inst), (near_c, far_c))
        self.last_instance_pairs = made[-1]
        return dict(instances=[(t["rgb"], t["acc"], t["depth"]) for t in levels] if per_instance else None,
                    composite=[(t["comp_rgb"], t["comp_acc"], t["comp_depth"], t["instance_id"]) for t in levels])

    @torch.no_grad()
    def render_edited(self, rays, near_inst, far_inst, density_scale=None, tint=None, layers=None, chunk=None, return_samples=False):
        """The whole scene - both regions, both levels - with instances removed, faded, tinted or re-inserted somewhere else
        (neo_tp_render_edited).  Deterministic (randomized=False); the unit-sphere assertion is that of `forward`; `chunk` as in
        `forward`.  Reads neither `cull_background` nor `compute_extras` (nor `ray_grid`).

        near_inst / far_inst: (K,B) or (K,B,1), any float dtype, on the rays' device, 0 <= K <= 32 - the intervals
        `render_instances` takes, values of the ray parameter t of o + t rays_d.  Pair (i, ray) is a hit by the rule of
        `render_objects` (lo = max(near, 1e-4), hi = far, both finite, hi > lo; a NaN bound is a miss); an inside-sphere sample is
        inside the pair iff lo <= t <= hi.  At both levels, after the evaluator and before the composite, for i ascending and every
        sample inside: sigma *= density_scale[i], rgb *= tint[i] (fp32; overlapping intervals multiply; scale 0 removes the instance
        and what lies behind it is re-weighted by the composite).  density_scale (K values) and tint (K x 3) are HOST sequences or CPU
        tensors, validated on the host - right length, finite, >= 0, else ValueError - and passed as kernel arguments: the call
        synchronises nothing.  None = ones; with K = 0, or every value 1, and no layers the result is bitwise
        `forward(rays, False, False, near, far, out_depth=True, chunk=chunk)`.

        layers: None or dict(key (L,B), rgb (L,B,3), acc (L,B), depth (L,B)) on the rays' device, L <= 32 - e.g.
        `render.instance_layers`: slabs of opacity acc, premultiplied colour rgb and premultiplied depth at the ray parameter key,
        spliced into the inside-sphere composite of BOTH levels in ascending key (`ops.composite_layers`; a layer with a non-finite
        key or acc <= 0 is ignored).  The fine level's sample positions do not depend on them.

        Returns the two level tuples of `forward(..., out_depth=True)`: [(comp_rgb, fg_rgb, bg_rgb, fg_acc, bg_lambda, comp_depth)];
        with layers each tuple gains `visibility` (L,B), the weight each layer's opacity enters the ray with; with return_samples a
        third element holds per level (fg_t, fg_w, bg_s), fg_w being the SCENE weight (exactly 0 inside a removed interval)."""
        B = rays["rays_o"].shape[0]
        K = ops._edit_bounds(near_inst, far_inst, B, rays["rays_o"].device, "render_edited")
        scale, tints = ops.edit_table(K, density_scale, tint)
        L = ops._layer_rows(layers, B, rays["rays_o"].device, "render_edited")
        call = self._frame_call(rays, chunk)
        dev = call.dev
        near_c, far_c = ops._edit_rows(near_inst, far_inst, K, B)
        layer_rows, layer_struct = ops._layer_struct(layers, L)
        levels = []

        def launch():
            ctx = call.ctx
            structs, sample_structs = [], []
            for n in call.n:
                t, struct = self._level_out(B, dev)
                structs.append(struct)
                if L:
                    t["visibility"] = torch.empty(L, B, device=dev)
                sample_structs.append(self._edit_samples(t, B, n, dev, return_samples))
                levels.append(t)
            _lib.check(ctx.lib.neo_tp_render_edited(
                *call.ray_args, ptr(near_c), ptr(far_c), K, scale, tints,
                ctypes.byref(layer_struct) if layer_struct is not None else None, L, *call.frame_args,
                ctypes.byref(structs[0]), ctypes.byref(structs[1]),
                *(ctypes.byref(x) if x is not None else None for x in sample_structs), ctx.stream()))
            self._after_call(ctx)
            return [v for t in levels for v in t.values()]
        raw_layers = tuple(layers[k] for k in ("key", "rgb", "acc", "depth")) if L else ()
        call.run(launch, (near_inst, far_inst) + raw_layers, (near_c, far_c) + tuple(layer_rows))
        out = [self._level_tuple(t) + ((t["visibility"],) if L else ()) for t in levels]
        if return_samples:
            out.append([(t["fg_t"], t["fg_w"], t["bg_s"]) for t in levels])
        return out

    @torch.no_grad()
    def render_decomposed(self, rays, near_inst, far_inst, chunk=None, levels=(1,), return_samples=False):
        """The frame of `forward(rays, False, False, near, far, out_depth=True, chunk=chunk)` - bitwise - together with its split into
        per-instance layers, a "rest" layer and an occlusion-aware id map (neo_tp_render_decomposed).  Deterministic
        (randomized=False); the unit-sphere assertion, `chunk` and `ray_grid` are those of `forward`.  Reads neither
        `cull_background` nor `compute_extras`.

        near_inst / far_inst: (K,B) or (K,B,1), any float dtype, on the rays' device, 0 <= K <= 32 - the intervals
        `render_instances` takes.  Pair (i, ray) is a hit by the rule of `render_objects` (lo = max(near, 1e-4), hi = far, both
        finite, hi > lo; a NaN bound is a miss); an inside-sphere sample is inside the pair iff lo <= t <= hi and belongs to the
        lowest-indexed hit pair it is inside of, else to slot K, the rest.  After the inside-sphere composite of each level in
        `levels` (a subset of (0, 1)), on the rows, positions and scene weights that composite worked on: per slot s = 0 .. K the
        sums of w c (rgb), w (acc) and w t (depth) over the slot's samples, in the composite's own fp32 order - so the slots add up
        to fg_rgb / fg_acc / the foreground depth up to the rounding of the partial sums, a slot that owns nothing is exactly 0,
        and with K = 0 the rest IS them, bitwise.  id = the instance with the largest acc (ties: lower index) iff that is > 0 and
        >= acc[K] + bg_lambda, else -1: the outside-sphere half counts for the rest.  `depth` is the premultiplied sum, like
        `forward`'s; what lies outside the sphere (bg_lambda * bg_rgb) belongs to no slot - `render.render_decomposed_rays` adds it
        to the rest.

        Returns the two level tuples of `forward(..., out_depth=True)`: [(comp_rgb, fg_rgb, bg_rgb, fg_acc, bg_lambda, comp_depth)];
        each level in `levels` gains a seventh element dict(rgb (K+1,B,3), acc (K+1,B), depth (K+1,B), id (B,) int32); with
        return_samples a third element holds per level (fg_t, fg_w, bg_s).  ValueError - before any device access - for intervals
        whose shape, dtype, device or count does not fit, and for levels other than 0 and 1."""
        B = rays["rays_o"].shape[0]
        K = ops._edit_bounds(near_inst, far_inst, B, rays["rays_o"].device, "render_decomposed")
        want = tuple(levels)
        if any(isinstance(lv, bool) or lv not in (0, 1) for lv in want):
            raise ValueError("render_decomposed: levels must be a subset of (0, 1), got %r" % (levels,))
        call = self._frame_call(rays, chunk, use_grid=True)      # the pixel-grid hint of forward: bitwise-neutral
        dev = call.dev
        near_c, far_c = ops._edit_rows(near_inst, far_inst, K, B)
        made = []

        def launch():
            ctx = call.ctx
            structs, dec_structs, sample_structs = [], [], []
            for lv, n in enumerate(call.n):
                t, struct = self._level_out(B, dev)
                structs.append(struct)
                dec = None
                if lv in want:
                    t["decomposed"], dec = ops._decomposed_out(K, B, dev)
                dec_structs.append(dec)
                sample_structs.append(self._edit_samples(t, B, n, dev, return_samples))
                made.append(t)
            _lib.check(ctx.lib.neo_tp_render_decomposed(
                *call.ray_args, ptr(near_c), ptr(far_c), K, *call.frame_args, ctypes.byref(structs[0]), ctypes.byref(structs[1]),
                *(ctypes.byref(x) if x is not None else None for x in dec_structs + sample_structs), ctx.stream()))
            self._after_call(ctx)
            return [v for t in made for x in t.values() for v in (x.values() if isinstance(x, dict) else (x,))]
        call.run(launch, (near_inst, far_inst), (near_c, far_c))
        out = [self._level_tuple(t) + ((t["decomposed"],) if "decomposed" in t else ()) for t in made]
        if return_samples:
            out.append([(t["fg_t"], t["fg_w"], t["bg_s"]) for t in made])
        return out


    # ---- empty-space skipping ------------------------------------------------------------------------------------------------

    # rays per window of render_skipping (None: the library's default, 4096): a window bounds the extra workspace at about 190 bytes
    # per (ray, sample) of ONE window; results do not depend on it
    skip_window = None

    @property
    def occupancy(self):
        """The installed occupancy grid as a bool (G,G,G) device tensor (a copy), or None."""
        return None if self._occupancy is None else self._occupancy.clone()

    @torch.no_grad()
    def set_occupancy(self, grid):
        """Installs (or, with None, removes) the occupancy grid `render_skipping` reads: a bool (G,G,G) tensor on any device over
        the world cube [-1, 1]^3, indexed [ix, iy, iz]; G is 8, 16 or a multiple of 32 in [32, 256].  ValueError - before any device
        access - for another shape, dtype or G.  The grid is copied to the module's device (its parameters') and, as bits, into the
        library context.  `set_scene` removes it, because a grid describes ONE scene; it equally belongs to the source poses the
        scene is looked up with and to the weights of the two inside-sphere MLPs, which the module cannot check: install a new grid
        (`build_occupancy`) whenever either changes.  `forward` and every other call ignore it."""
        if grid is None:
            if self._occ_ctx is not None:
                _lib.check(self._occ_ctx.lib.neo_tp_set_occupancy(self._occ_ctx.handle, None, 0, self._occ_ctx.stream()))
            self._occupancy = self._occ_ctx = None
            return
        G = ops._check_occupancy(grid, "set_occupancy")
        dev = next(self.parameters()).device
        ctx = self._context(dev)
        occ = grid.detach().to(dev).contiguous().clone()
        bits = ops.pack_occupancy(occ)
        _lib.check(ctx.lib.neo_tp_set_occupancy(ctx.handle, ptr(bits), G, ctx.stream()))
        self._occupancy, self._occ_ctx = occ, ctx

    @torch.no_grad()
    def _occupancy_sigma(self, rays, resolution, probes, points_per_piece=1 << 22):
        """max(sigma of slot 0, sigma of slot 1) on the (resolution * probes)^3 lattice of `ops.occupancy_lattice`, its columns
        evaluated as rays by `eval_mlp` in pieces of at most points_per_piece points.  `rays` supplies the source cameras."""
        dev = rays["rays_o"].device
        M = resolution * probes
        c, o, d = ops.occupancy_lattice(resolution, probes, dev)
        per_ray = ("rays_o", "rays_d", "viewdirs")
        sigma = torch.empty(M * M, M, device=dev)
        step = max(1, points_per_piece // M)
        for i in range(0, M * M, step):
            part = {k: v for k, v in rays.items() if k not in per_ray}
            part.update(rays_o=o[i:i + step], rays_d=d[i:i + step], viewdirs=d[i:i + step])
            t = c[None, :].expand(part["rays_o"].shape[0], M).contiguous()
            s0 = self.eval_mlp(0, part, t)[..., 3]
            s1 = self.eval_mlp(1, part, t)[..., 3]
            sigma[i:i + step] = torch.maximum(s0, s1)
        return sigma.reshape(M, M, M)

    @torch.no_grad()
    def build_occupancy(self, rays, resolution, sigma_threshold, probes=2, dilate=1):
        """Builds, installs and returns the occupancy grid of the current scene: both inside-sphere MLPs (slots 0 and 1) are
        evaluated on the (resolution * probes)^3 lattice of cell sub-centres, a cell is occupied iff the larger of the two
        densities at one of its probes is not <= sigma_threshold, the result is dilated by `dilate` cells over the 26-neighbourhood
        and cells without a point inside the unit sphere are cleared (`ops.occupancy_from_sigma`).  `rays` is a batch of this scene
        (its source cameras are what the lookups use; its own rays are not read).
        sigma_threshold has no default: nobody has measured one on trained weights.  It reads as an opacity - a sample of density
        sigma over a step delta has alpha = 1 - exp(-sigma * delta), and delta is about far / 128 at level 0 of the reference's
        counts - so a threshold of 0.01 / delta skips only samples that would be less than 1 % opaque, provided the probes see
        the density at all: anything thinner than a probe spacing, 2 / (resolution * probes), can be missed, which is what
        `dilate` is for.  ValueError, before any device access, for a bad resolution, probes, dilate or threshold."""
        G, probes, dilate = ops._check_build(resolution, sigma_threshold, probes, dilate, "build_occupancy")
        sigma = self._occupancy_sigma(rays, G, probes)
        grid = ops.occupancy_from_sigma(sigma, G, sigma_threshold, probes, dilate, ctx=self._context(sigma.device))
        self.set_occupancy(grid)
        return grid

    @torch.no_grad()
    def render_skipping(self, rays, chunk=None, return_samples=False):
        """`forward(rays, False, False, near, far, out_depth=True, chunk=chunk)` in which the inside-sphere samples that fall into
        clear cells of the installed occupancy grid are not evaluated (neo_tp_render_skipping).  At both levels a sample at
        x = o + t d is kept iff its cell is set or a coordinate of x is not finite (`ops.occupancy_keep`); a skipped sample's
        (rgb, sigma) row is zero, so its weight is exactly 0, and everything downstream - the composite, the level-1 resampling from
        the resulting weights, the outside-sphere half (never skipped), the merge - is `forward`'s on those rows.  Kept samples are
        bitwise `forward`'s; with an all-ones grid so is the whole result.  Reads neither `cull_background` nor `compute_extras`;
        `ray_grid` as `forward`.  NeoError when no grid is installed.

        Returns the two level tuples of `forward(..., out_depth=True)`; with return_samples a third element holds per level
        (fg_t, fg_w, bg_s, fg_keep (B,N) bool) - and, with return_samples="rows", fg_rows (B,N,4) behind them.
        `self.last_skip_kept` (int64[2], on the device) holds the kept samples per level; nothing is read back."""
        if self._occupancy is None:
            raise _lib.NeoError("no occupancy grid installed: call set_occupancy(...) or build_occupancy(...) first")
        out, (self.last_skip_kept,) = self._render_march(
            "neo_tp_render_skipping", rays, chunk, _lib.TpSkipSamples, ("fg_t", "fg_w", "bg_s", "fg_keep"), ("fg_rows",), (), 2,
            survivors=False, check_grid="required", return_samples=return_samples)
        return out

    _MARCH_PER_RAY = dict(stop=torch.int32, bg_stop=torch.int32, bg_value=torch.float32)

    def _render_march(self, entry, rays, chunk, struct_cls, names, rows_names, extra_args, n_kept, survivors=True, check_grid=False,
                      keep_written=True, fine_only=False, return_samples=False):
        """The marshalling behind `render_skipping`, `render_terminating`, `render_accelerated` and `render_marching`: one call of the
        library's `entry` (ray and frame arguments, the two level structs, `extra_args`, the two `struct_cls` sample structs, the
        counters, the stream).  names / rows_names: the sample rows of return_samples / return_samples="rows", in tuple order -
        (B,) for a `_MARCH_PER_RAY` name, (B,N,4) for a rows name, bool for fg_keep (all ones unless keep_written), else (B,N).
        check_grid: NeoError for a grid installed on another context - "required": also for none at all.  Returns the public
        method's result and the device counters: int64[n_kept], and with `survivors` the int32 survivor count."""
        call = self._frame_call(rays, chunk, use_grid=True)
        B, dev = call.B, call.dev
        levels = []
        counts = []
        if return_samples == "rows":
            names = names + rows_names

        def rows(k, n):
            if k in self._MARCH_PER_RAY:
                return torch.empty(B, dtype=self._MARCH_PER_RAY[k], device=dev)
            if k == "fg_keep":      # a call that reads no grid skips nothing and the library writes no mask
                return (torch.empty if keep_written else torch.ones)(B, n, dtype=torch.bool, device=dev)
            return torch.empty((B, n, 4) if k in rows_names else (B, n), device=dev)

        def byref(structs):
            return (ctypes.byref(x) if x is not None else None for x in structs)

        def launch():
            ctx = call.ctx
            foreign = self._occupancy is not None and self._occ_ctx is not ctx
            if check_grid and (foreign or (check_grid == "required" and self._occupancy is None)):
                raise _lib.NeoError("the occupancy grid does not belong to this scene and device: install it again")
            self._set_mode(ctx, "_skip_window", "neo_tp_set_skip_window", int(self.skip_window or 0))
            structs, sample_structs = [], []
            for level, n in enumerate(call.n):
                if level == 0 and fine_only:
                    t, struct = {}, None
                else:
                    t, struct = self._level_out(B, dev)
                structs.append(struct)
                if return_samples:
                    t.update((k, rows(k, n)) for k in names)
                    sample_structs.append(struct_cls(*(t[k].data_ptr() if k in t else None for k, _ in struct_cls._fields_)))
                else:
                    sample_structs.append(None)
                levels.append(t)
            counts.append(torch.empty(n_kept, dtype=torch.int64, device=dev))
            if survivors:
                counts.append(torch.empty((), dtype=torch.int32, device=dev))
            _lib.check(getattr(ctx.lib, entry)(
                *call.ray_args, *call.frame_args, *byref(structs), *extra_args, *byref(sample_structs),
                *(c.data_ptr() for c in counts), ctx.stream()))
            self._after_call(ctx)
            return [v for t in levels for v in t.values()] + counts
        call.run(launch)
        out = [None if (level == 0 and fine_only) else self._level_tuple(t) for level, t in enumerate(levels)]
        if return_samples:
            out.append([tuple(t[k] for k in names) for t in levels])
        return out, counts

    # ---- early ray termination -----------------------------------------------------------------------------------------------

    @torch.no_grad()
    def render_terminating(self, rays, eps, chunk=None, segment=64, coarse=False, return_samples=False, fine_only=False):
        """`forward(rays, False, False, near, far, out_depth=True, chunk=chunk)` in which a ray's inside-sphere march stops once its
        transmittance has fallen below `eps`, and the outside-sphere half is not evaluated for rays that are opaque at both levels
        (neo_tp_render_terminating; include/neo360_hip.h: STOP RULE).  The samples of a level are cut into segments of `segment`
        (a positive multiple of 64); segment 0 is always evaluated, a later one iff the transmittance at every earlier segment
        boundary - the composite's own value there, bit for bit (`ops.termination_stops`) - was not below eps.  A sample behind
        the stop is not evaluated: its (rgb, sigma) row is zero and its weight exactly 0; the evaluated prefix is bitwise `forward`'s,
        and a stopped ray's bg_lambda is the transmittance at its stop.  A ray's background runs iff one of its two bg_lambda is
        not below eps; a culled ray gets rgb = fg_rgb, bg_rgb = 0, depth = fg_depth.

        Level 1 follows the rule; level 0 is evaluated in full unless coarse=True.  With coarse=False a stopped ray's level-1 rgb
        differs from `forward`'s by at most 1.003 * bg_lambda per channel and its depth by at most (t_far + 1.001) * bg_lambda, with
        the returned bg_lambda < eps; a ray that never stops and is not culled is bitwise `forward`'s, and so is everything at
        eps = 0.  coarse=True also zeroes the level-0 weights behind the stop, which moves the level-1 sample positions: NO error
        bound is claimed for that mode.  Needs no per-scene artefact.  Reads none of `cull_background`, `compute_extras` or an
        installed occupancy grid; `ray_grid` as `forward`; `skip_window` bounds the workspace as in `render_skipping`.
        ValueError, before any device access, for eps outside [0, 1) or NaN, or a segment that is not a positive multiple of 64.

        Returns the two level tuples of `forward(..., out_depth=True)` (fine_only=True: None for level 0, whose colours are then not
        computed); with return_samples a third element holds per level (fg_t, fg_w, bg_s, stop (B,) int32) - and, with
        return_samples="rows", fg_rows (B,N,4) behind them; the level-1 bg_s row of a culled ray is zero.
        `self.last_terminate_kept` (int64[2]: evaluated inside-sphere samples per level) and `self.last_terminate_survivors`
        (int32: rays whose background ran) stay on the device; nothing is read back."""
        eps, segment = ops._check_termination(eps, segment, "render_terminating")
        out, (self.last_terminate_kept, self.last_terminate_survivors) = self._render_march(
            "neo_tp_render_terminating", rays, chunk, _lib.TpTermSamples, ("fg_t", "fg_w", "bg_s", "stop"), ("fg_rows",),
            (eps, segment, int(bool(coarse))), 2, fine_only=fine_only, return_samples=return_samples)
        return out

    # ---- occupancy skipping and early termination together ---------------------------------------------------------------------

    @torch.no_grad()
    def render_accelerated(self, rays, eps, chunk=None, segment=64, coarse=False, return_samples=False, fine_only=False):
        """`render_terminating(rays, eps, ...)` that also obeys the installed occupancy grid (neo_tp_render_accelerated;
        include/neo360_hip.h: ACCELERATED FRAME).  At level 1 - and at level 0 with coarse=True - sample j of a ray is evaluated iff
        the grid keeps it (`ops.occupancy_keep`) and j < stop, where stop is `ops.termination_stops` on the level's rows with the
        samples that are not kept zeroed; level 0 with coarse=False obeys the grid only, as in `render_skipping`.  A sample that is
        not evaluated has a zero row and weight exactly 0.  The background and the launch order are `render_terminating`'s.

        With no grid installed the result is bitwise `render_terminating`'s (no error is raised: that is the terminating frame);
        with eps = 0 it is bitwise `render_skipping`'s with the same grid; with neither, `forward`'s.  With coarse=False a stopped
        ray's level-1 rgb differs from `render_skipping`'s by at most 1.003 * bg_lambda per channel and its depth by at most
        (t_far + 1.001) * bg_lambda, with the returned bg_lambda < eps; nothing is claimed for coarse=True.  Reads neither
        `cull_background` nor `compute_extras`; `ray_grid` as `forward`; `skip_window` bounds the workspace as in `render_skipping`.
        ValueError, before any device access, for eps outside [0, 1) or NaN, or a segment that is not a positive multiple of 64;
        NeoError when the installed grid belongs to another context.

        Returns the two level tuples of `forward(..., out_depth=True)` (fine_only=True: None for level 0); with return_samples a
        third element holds per level (fg_t, fg_w, bg_s, stop (B,) int32, fg_keep (B,N) bool - the grid's verdict on the whole row,
        behind the stop as well: the evaluated set is fg_keep & (j < stop)) - and, with return_samples="rows", fg_rows (B,N,4)
        behind them.  `self.last_accel_kept` (int64[2]: evaluated inside-sphere samples per level) and `self.last_accel_survivors`
        (int32: rays whose background ran) stay on the device; nothing is read back."""
        eps, segment = ops._check_termination(eps, segment, "render_accelerated")
        out, (self.last_accel_kept, self.last_accel_survivors) = self._render_march(
            "neo_tp_render_accelerated", rays, chunk, _lib.TpAccelSamples, ("fg_t", "fg_w", "bg_s", "stop", "fg_keep"), ("fg_rows",),
            (eps, segment, int(bool(coarse))), 2, check_grid=True, fine_only=fine_only, return_samples=return_samples)
        return out

    # ---- early termination carried through the outside-sphere march ------------------------------------------------------------

    @torch.no_grad()
    def render_marching(self, rays, eps, chunk=None, segment=64, coarse=False, outside=True, grid=True, return_samples=False,
                        fine_only=False):
        """The driver behind `render_terminating` (grid=False) and `render_accelerated` (grid=True) with the early termination
        carried through the OUTSIDE-sphere march (neo_tp_render_marching; include/neo360_hip.h: OUTSIDE STOP RULE).  With
        outside=True a ray whose background runs - the cull of those two calls, unchanged - marches its level-1 outside samples in
        segments of `segment`: segment 0 always, segment k >= 1 iff at every earlier boundary b the running value bg_lambda *
        (float)carry_b (`ops.termination_stops_outside`: one fp32 multiply of the level's returned lambda with the outside
        composite's own transmittance in front of sample b) was not below eps.  A sample behind bg_stop is not evaluated: its row is
        zero and its weight exactly 0.  Level 0 follows the rule only with coarse=True, which moves the level-1 outside positions: no
        bound is claimed for that mode.

        outside=False is bitwise `render_accelerated` (grid=True) or `render_terminating` (grid=False); eps = 0 is bitwise
        `forward(..., out_depth=True)` (with no grid read).  With coarse=False, against the same call with outside=False: the
        foreground outputs, the inside stops and the cull set are bitwise equal, a ray whose outside march never stops is bitwise
        equal, and a stopped ray's level-1 rgb and depth differ by less than 1.003 * eps.  ValueError, before any device access, for
        eps outside [0, 1) or NaN, or a segment that is not a positive multiple of 64; NeoError when grid=True and the installed
        grid belongs to another context.

        Returns the two level tuples of `forward(..., out_depth=True)` (fine_only=True: None for level 0); with return_samples a
        third element holds per level `render_accelerated`'s tuple (fg_t, fg_w, bg_s, stop, fg_keep) followed by bg_stop (B,) int32
        (0 for a culled ray) and bg_value (B,), the running value at the stop (0 for a culled ray) - and, with
        return_samples="rows", fg_rows (B,N,4) and bg_rows (B,N,4) behind them (zero rows for culled rays).
        `self.last_march_kept` (int64[4]: evaluated samples inside the sphere per level, then outside the sphere per level) and
        `self.last_march_survivors` (int32: rays whose background ran) stay on the device; nothing is read back."""
        eps, segment = ops._check_termination(eps, segment, "render_marching")
        out, (self.last_march_kept, self.last_march_survivors) = self._render_march(
            "neo_tp_render_marching", rays, chunk, _lib.TpMarchSamples,
            ("fg_t", "fg_w", "bg_s", "stop", "fg_keep", "bg_stop", "bg_value"), ("fg_rows", "bg_rows"),
            (eps, segment, int(bool(coarse)), int(bool(grid)), int(bool(outside))), 4, check_grid=bool(grid), keep_written=bool(grid),
            fine_only=fine_only, return_samples=return_samples)
        return out


class _TpFrameCall:
    """One fused frame call of a NeRF_TP module (forward(out_depth=True), render_objects, render_instances, render_edited,
    render_decomposed): the prologue they share and the launch around their one library call.

    Construction converts the three ray tensors and touches no device context, so that a caller's own conversions and
    ValueErrors still come first.  `run(launch, extra_raw, extra_conv)` then does the rest, in this order:
    context, scene check, weight sync, the deferred flags of earlier calls, the host copies of the source cameras, for a
    `use_grid` call the module's `ray_grid` hint (reset when the call is over, however it ends), and `launch()` on the call's side
    stream and scratch lane (`_launch_overlapped`; extra_raw / extra_conv: the call's further input tensors as passed / as the
    library reads them).  `launch` finds the context as `.ctx` and the library arguments all frame entry points start with as
    `.ray_args` = (handle, rays_o, rays_d, viewdirs) and `.frame_args` = (B, chunk, src poses, NV, focal, cx, cy, n_coarse, n_fine)."""

    def __init__(self, net, rays, chunk, use_grid):
        self.net, self.batch, self.use_grid = net, rays, use_grid
        self.raw = (rays["rays_o"], rays["rays_d"], rays["viewdirs"])
        self.rays = _ray_rows(rays)        # rays_o defines B; rays_d / viewdirs of another batch are refused here
        self.dev = self.rays[0].device
        self.B = self.rays[0].shape[0]
        self.chunk = int(chunk or max(self.B, 1))
        self.n = (net.num_coarse_samples + 1, net.num_coarse_samples + 1 + net.num_fine_samples)      # samples per ray, per level
        self.ctx = self.ray_args = self.frame_args = None

    def run(self, launch, extra_raw=(), extra_conv=()):
        net, dev, B = self.net, self.dev, self.B
        ctx = self.ctx = net._context(dev)
        net._ensure_scene(self.batch, dev)
        if net._scene_ctx is not ctx:
            raise _lib.NeoError("scene features were uploaded on a different device")
        net._sync_weights(ctx)
        net._before_call(ctx)
        self.ray_args = (ctx.handle,) + tuple(ptr(t) for t in self.rays)
        self.frame_args = (B, self.chunk) + tuple(net._camera_args(self.batch)) + (net.num_coarse_samples, net.num_fine_samples)
        if self.use_grid:
            # pixel-grid hint (render.render_rays_test / render_frame_sharded set `ray_grid` around a frame): a scheduling hint for
            # the evaluators' tile order, bitwise-neutral; only meaningful for a call that spans whole bands of 8 image rows
            grid = getattr(net, "ray_grid", None)
            ctx.set_ray_grid(*(grid if grid and grid[0] % 8 == 0 and B >= 8 * grid[0] else (0, 0)))
        try:
            return net._launch_overlapped(ctx, dev, self.raw + tuple(extra_raw), self.rays + tuple(extra_conv), launch)
        finally:
            if self.use_grid:
                ctx.set_ray_grid(0)


class PixelNeRFMLP(nn.Module):
    """Parameter container with the layout of vanilla_nerf/model_pixel.py:35-94: pts_linears.0..3 (128 wide;
    input = 63-d pos_enc + 512 pixel-aligned latent; the skip never fires at depth 4), views_linear.0/.1 (128),
    bottleneck_layer, density_layer, rgb_layer."""

    def __init__(self, min_deg_point=0, max_deg_point=10, deg_view=4, netdepth=4, netwidth=128,
                 netdepth_condition=2, netwidth_condition=128, skip_layer=4, input_ch=3, input_ch_view=3,
                 num_rgb_channels=3, num_density_channels=1, latent_size=512, combine_layer=3, combine_type="average"):
        super().__init__()
        if (min_deg_point, max_deg_point, deg_view, netdepth, netwidth, netdepth_condition, netwidth_condition,
                skip_layer, input_ch, input_ch_view, num_rgb_channels, num_density_channels, latent_size,
                combine_layer, combine_type) != (0, 10, 4, 4, 128, 2, 128, 4, 3, 3, 3, 1, 512, 3, "average"):
            raise NotImplementedError("the HIP kernel is specialised for the reference's default PixelNeRF MLP shape")
        pos = ((max_deg_point - min_deg_point) * 2 + 1) * input_ch + latent_size
        view = (deg_view * 2 + 1) * input_ch_view
        self.pts_linears = nn.ModuleList([_xavier_linear(pos, netwidth)] +
                                         [_xavier_linear(netwidth, netwidth) for _ in range(netdepth - 1)])
        self.views_linear = nn.ModuleList([_xavier_linear(netwidth + view, netwidth_condition, xavier=False),
                                           _xavier_linear(netwidth_condition, netwidth_condition)])
        self.bottleneck_layer = _xavier_linear(netwidth, netwidth)
        self.density_layer = _xavier_linear(netwidth, num_density_channels)
        self.rgb_layer = _xavier_linear(netwidth_condition, num_rgb_channels)

    def ordered_layers(self):
        """Upload order fixed by include/neo360_hip.h (neo_pix_upload_mlp)."""
        return list(self.pts_linears) + [self.views_linear[0], self.views_linear[1], self.bottleneck_layer,
                                         self.density_layer, self.rgb_layer]


class PixelNeRF(_HipModule):
    """PixelNeRF baseline decoder renderer (vanilla_nerf/model_pixel.py:133-258).

    `forward(rays, randomized, white_bkgd, near, far)` keeps the reference's signature and returns
    `[(comp_rgb, acc, depth)] x 2`.  The image encoder (ResNet-34 SpatialEncoder) is outside the accelerated
    path: provide its latent once per scene with `set_scene(latent, image_wh)`, or attach an `encoder` module with
    the reference's interface (callable on `src_imgs`, then `.latent`); an attached encoder runs once per
    distinct `src_imgs` tensor instead of once per chunk.  All rays of a call form ONE reference chunk unless
    `chunk` is given (the view-direction tiling of model_pixel.py:219-222 depends on chunk membership)."""

    def __init__(self, num_levels=2, min_deg_point=0, max_deg_point=10, deg_view=4, num_coarse_samples=64,
                 num_fine_samples=64, use_viewdirs=True, noise_std=0.0, lindisp=False, num_src_views=3, encoder=None):
        super().__init__()
        if num_levels != 2 or not use_viewdirs or lindisp:
            raise NotImplementedError("only the reference's default 2-level, view-dependent, linear-depth setup")
        self.num_levels, self.num_src_views = num_levels, num_src_views
        self.num_coarse_samples, self.num_fine_samples = num_coarse_samples, num_fine_samples
        self.noise_std, self.lindisp = noise_std, lindisp
        if encoder is not None:
            self.encoder = encoder
        self.coarse_mlp = PixelNeRFMLP(min_deg_point, max_deg_point, deg_view)
        self.fine_mlp = PixelNeRFMLP(min_deg_point, max_deg_point, deg_view)
        self._scene_key = None
        self._scene_ctx = None
        # gather the latent pre-projected through each MLP's first layer (128 instead of 512 channels per tap, 41 % fewer
        # MACs per point-view; csrc/mlp_pix_h.hip).  False: the reference's operation order.
        self.preproject = os.environ.get("NEO360_PIX_PREPROJECT", "1") != "0"

    def _context(self, device):
        ctx = super()._context(device)
        self._set_mode(ctx, "_pix_preproject", "neo_pix_set_preproject", bool(self.preproject))
        return ctx

    _upload = ("pix", "neo_pix_upload_mlp")

    def _mlps(self):
        return (self.coarse_mlp, self.fine_mlp)

    @torch.no_grad()
    def set_scene(self, latent, image_wh):
        """latent (NV,512,Hf,Wf) as the reference's SpatialEncoder leaves it in `.latent`; image_wh = (W,H) of
        the source images (model_pixel.py:176-177).  Re-laid out channels-last on the device, once.  The module keeps a weak
        reference to the tensor: a differentiable forward sends the latent's gradient there."""
        src = latent
        latent = dense(latent, "latent", (None, None, None, None))
        self._latent_src = weakref.ref(src)
        ctx = self._context(latent.device)
        NV, Cl, Hf, Wf = latent.shape
        _lib.check(ctx.lib.neo_pix_set_scene(ctx.handle, ptr(latent), NV, Cl, Hf, Wf, float(image_wh[0]),
                                             float(image_wh[1]), ctx.stream()))
        torch.cuda.current_stream(latent.device).synchronize()   # the caller may free its tensor
        self._scene_ctx = ctx
        self._scene_serial = getattr(self, "_scene_serial", 0) + 1

    def _ensure_scene(self, rays):
        enc = getattr(self, "encoder", None)
        if enc is None:
            if self._scene_ctx is None:
                raise _lib.NeoError("no scene latent: call set_scene(...) or attach an encoder module")
            return
        src = rays["src_imgs"]
        if self._scene_key is not None and self._scene_ctx is not None and self._scene_key.matches((src,), enc):
            return
        enc(src)
        self.set_scene(enc.latent, (src.shape[-1], src.shape[-2]))
        self._scene_key = _SceneKey((src,), enc)
        self.encoder_runs = getattr(self, "encoder_runs", 0) + 1

    _camera_args = NeRF_TP._camera_args

    @torch.no_grad()
    def eval_mlp(self, slot, rays, tvals, chunk=None):
        """Stage-level access for parity tests: latent lookups + pos_enc + MLP + activations at sample
        positions tvals (B,N) along rays_d.  rays["rays_o"] (B,3) defines B, rays["rays_d"] / rays["viewdirs"] (B,3), tvals
        defines N.  Returns (B,N,4) = (sigmoid rgb, relu sigma)."""
        rays_o, rays_d, viewdirs = _ray_rows(rays)
        tvals = _sample_rows(tvals, "tvals", rays_o)
        ctx = self._context(rays_o.device)
        self._ensure_scene(rays)
        self._sync_weights(ctx)
        B, N = tvals.shape
        host_poses, NV, focal, cx, cy = self._camera_args(rays)
        out = torch.empty(B, N, 4, device=rays_o.device)
        _lib.check(ctx.lib.neo_pix_mlp(ctx.handle, slot, ptr(rays_o), ptr(rays_d), ptr(viewdirs), ptr(tvals), B, N,
                                       int(chunk or max(B, 1)), host_poses, NV, focal, cx, cy, ptr(out), ctx.stream()))
        self._raise_flags(ctx.poll_flags())     # stage-level access: always immediate
        return out

    def _scene_tensors_for_grad(self):
        ref = getattr(self, "_latent_src", None)
        return (ref(),) if ref is not None else ()

    def _latent_for_grad(self, rays):
        """The latent a differentiable call gathers from: an attached encoder is run WITH autograd on this batch, as the
        reference's forward does (model_pixel.py:176); otherwise the tensor given to set_scene, if the caller still holds it."""
        enc = getattr(self, "encoder", None)
        if enc is not None:
            src = rays["src_imgs"]
            enc(src)
            latent = enc.latent
            with torch.no_grad():
                self.set_scene(latent.detach(), (src.shape[-1], src.shape[-2]))
            self._scene_key = None
            return latent
        if self._scene_ctx is None:
            raise _lib.NeoError("no scene latent: call set_scene(...) or attach an encoder module")
        ref = getattr(self, "_latent_src", None)
        latent = ref() if ref is not None else None
        if latent is None:
            raise _lib.NeoError("a differentiable / randomized forward needs the latent tensor: attach an encoder module, or keep "
                                "the tensor passed to set_scene(...) alive (the module holds only a weak reference to it)")
        return latent

    def forward(self, rays, randomized, white_bkgd, near, far, chunk=None, seed=None):
        """randomized=True (stratified sampling, `noise_std`) or a call that wants gradients (`_wants_grad()`: the reference's
        training_step) runs on the operator chain of training.pix_render_train - every matrix product on the library's GEMMs,
        gradients to all 18 parameter tensors of each MLP and to the latent; otherwise the fused no-grad kernels."""
        if randomized or self._wants_grad(randomized):
            from . import training
            # A deterministic call that reached the chain by the AUTOMATIC rule alone keeps working where only the fused path can
            # serve it (a chunked frame; a set_scene latent the caller no longer holds): these calls worked before round 5 made
            # the chain the automatic choice - they fall back to the fused kernels instead of raising.
            fallback = not randomized and self._auto_chain()
            chunked = chunk is not None and chunk < rays["rays_o"].shape[0]
            if chunked and not fallback:
                raise NotImplementedError("the training call renders its rays as ONE reference chunk")
            latent = None
            if not chunked:
                try:
                    latent = self._latent_for_grad(rays)
                except _lib.NeoError:
                    if not fallback:
                        raise
            if latent is not None:
                return training.pix_render_train(self, rays, randomized, white_bkgd, near, far, latent, seed)
        with torch.no_grad():
            return self._forward_fused(rays, white_bkgd, near, far, chunk)

    def _forward_fused(self, rays, white_bkgd, near, far, chunk=None):
        raw = (rays["rays_o"], rays["rays_d"], rays["viewdirs"])
        rays_o, rays_d, viewdirs = _ray_rows(rays)
        dev = rays_o.device
        ctx = self._context(dev)
        self._ensure_scene(rays)
        if self._scene_ctx is not ctx:
            raise _lib.NeoError("the scene latent was uploaded on a different device")
        self._sync_weights(ctx)
        self._before_call(ctx)
        B = rays_o.shape[0]
        host_poses, NV, focal, cx, cy = self._camera_args(rays)
        lv = []

        def launch():
            lv.extend((torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)) for _ in range(2))
            _lib.check(ctx.lib.neo_pix_render(
                ctx.handle, ptr(rays_o), ptr(rays_d), ptr(viewdirs), B, int(chunk or max(B, 1)), host_poses, NV, focal, cx, cy,
                float(near), float(far), self.num_coarse_samples, self.num_fine_samples, int(bool(white_bkgd)),
                ptr(lv[0][0]), ptr(lv[0][1]), ptr(lv[0][2]), ptr(lv[1][0]), ptr(lv[1][1]), ptr(lv[1][2]), ctx.stream()))
            self._after_call(ctx)
            return [t for l in lv for t in l]
        self._launch_overlapped(ctx, dev, raw, (rays_o, rays_d, viewdirs), launch)
        return lv


class MipNeRF360MLP(nn.Module):
    """Parameter container with the layout of mipnerf360/model.py:30-107: pts_linear.0..depth-1
    (input = 504-d integrated positional encoding over the 21-direction geodesic basis, skip concat
    feeds index 5), density_layer and — unless disable_rgb — bottleneck_layer (256),
    views_linear.0 (128), rgb_layer; buffer pos_basis_t (3,21).  kaiming_uniform_ initialisers."""

    def __init__(self, netdepth=8, netwidth=256, disable_rgb=False):
        super().__init__()
        from .geopoly import icosahedron_basis
        self.netdepth, self.netwidth, self.disable_rgb = netdepth, netwidth, disable_rgb
        self.register_buffer("pos_basis_t", icosahedron_basis())
        pos = 12 * 2 * self.pos_basis_t.shape[-1]

        def lin(n_in, n_out):
            layer = nn.Linear(n_in, n_out)
            nn.init.kaiming_uniform_(layer.weight)
            return layer

        layers = [lin(pos, netwidth)]
        for idx in range(netdepth - 1):
            layers.append(lin(netwidth + pos if (idx % 4 == 0 and idx > 0) else netwidth, netwidth))
        self.pts_linear = nn.ModuleList(layers)
        self.density_layer = lin(netwidth, 1)
        if not disable_rgb:
            self.bottleneck_layer = lin(netwidth, 256)
            self.views_linear = nn.ModuleList([lin(256 + 27, 128)])
            self.rgb_layer = lin(128, 3)

    def ordered_layers(self):
        """Upload order fixed by include/neo360_hip.h (neo_mip_upload_mlp)."""
        out = list(self.pts_linear) + [self.density_layer]
        if not self.disable_rgb:
            out += [self.bottleneck_layer, self.views_linear[0], self.rgb_layer]
        return out


class MipNeRF360(_HipModule):
    """Mip-NeRF 360 renderer (mipnerf360/model.py:199-365): two proposal MLPs (4x256) + one NeRF MLP
    (8x1024).  `forward(batch, train_frac, randomized, is_train, near, far)` returns
    (renderings, ray_history) exactly as the reference: renderings[l] = {"rgb": (B,3)},
    ray_history[l] = dict(density (B,n), rgb (B,n,3), sdist (B,n+1), weights (B,n))."""

    def __init__(self, num_prop_samples=64, num_nerf_samples=32, num_levels=3, bg_intensity_range=(1.0, 1.0),
                 anneal_slope=10, stop_level_grad=True, use_viewdirs=True, ray_shape="cone",
                 disable_integration=False, single_jitter=True, dilation_multiplier=0.5, dilation_bias=0.0025,
                 num_glo_features=0, num_glo_embeddings=1000, learned_exposure_scaling=False, near_anneal_rate=None,
                 near_anneal_init=0.95, single_mlp=False, resample_padding=0.0, use_gpu_resampling=False,
                 opaque_background=True):
        super().__init__()
        if (num_levels, tuple(bg_intensity_range), anneal_slope, ray_shape, disable_integration, dilation_multiplier,
                dilation_bias, near_anneal_rate, resample_padding, opaque_background, use_viewdirs) != (
                3, (1.0, 1.0), 10, "cone", False, 0.5, 0.0025, None, 0.0, True, True):
            raise NotImplementedError("the HIP path implements the reference's default MipNeRF360 configuration")
        self.num_prop_samples, self.num_nerf_samples, self.num_levels = num_prop_samples, num_nerf_samples, num_levels
        self.mlps = nn.ModuleList([MipNeRF360MLP(4, 256, disable_rgb=True), MipNeRF360MLP(4, 256, disable_rgb=True),
                                   MipNeRF360MLP(8, 1024)])
        # NeRF MLP schedule (neo_mip_set_layered): None = the library's choice (layer-by-layer GEMMs from 8192 intervals per
        # call), True / False = always / never; $NEO360_MIP_LAYERED = 0 / 1 presets it (A/B runs of bench.py)
        self.layered = {"0": False, "1": True}.get(os.environ.get("NEO360_MIP_LAYERED", ""), None)

    def _context(self, device):
        ctx = super()._context(device)
        mode = -1 if self.layered is None else int(bool(self.layered))
        self._set_mode(ctx, "_mip_layered", "neo_mip_set_layered", mode)
        return ctx

    _upload = ("mip", "neo_mip_upload_mlp")

    # The slot the reference's volumetric_rendering leaves open (helper.py:264-274 takes `compute_extras` and ignores it).  True: every
    # level's rendering dict gains acc, distance_mean, distance_median, distance_percentile_5 and distance_percentile_95
    # (ops.mip_extras on the level's own sdist / weights: one more launch per level); on the operator chain acc and distance_mean
    # carry gradients to the weights (training.mip_expected_distance), the percentiles come detached.  False (default): no launch is
    # added and forward returns what it always returned.
    compute_extras = False
    EXTRA_QUANTILES = (0.05, 0.5, 0.95)

    @staticmethod
    def _extras_dict(acc, mean, pct):
        return dict(acc=acc, distance_mean=mean, distance_median=pct[..., 1], distance_percentile_5=pct[..., 0],
                    distance_percentile_95=pct[..., 2])

    def _mlps(self):
        return self.mlps

    @staticmethod
    def _upload_extra(mlp):
        return (mlp.netwidth, mlp.netdepth, 0 if mlp.disable_rgb else 1), [f32(mlp.pos_basis_t, "pos_basis_t")]

    def forward(self, batch, train_frac, randomized, is_train, near, far, seed=None):
        """randomized=True (one sampling jitter per ray and level) or a call that wants gradients (`_wants_grad()`: the
        reference's training_step, model.py:436-470) runs on the operator chain of training.mip_render_train - resampling,
        encodings and compositing native, every matrix product on the library's GEMMs, gradients to all parameters through the
        colours and the interval weights; otherwise the fused no-grad kernels.  `is_train` only selects how the reference
        evaluates the contraction's Jacobian (helper.py:45-66); both of its forms are the closed form used here."""
        if randomized or self._wants_grad(randomized):
            from . import training
            return training.mip_render_train(self, batch, train_frac, randomized, near, far, seed)
        with torch.no_grad():
            return self._forward_fused(batch, train_frac, near, far)

    def _forward_fused(self, batch, train_frac, near, far):
        raw = (batch["rays_o"], batch["rays_d"], batch["viewdirs"], batch["radii"])
        rays_o, rays_d, viewdirs = _ray_rows(batch)
        radii = dense(raw[3], "radii", _radii_shapes(rays_o.shape[0]), device=rays_o.device)
        dev = rays_o.device
        ctx = self._context(dev)
        self._sync_weights(ctx)
        self._before_call(ctx)
        B = rays_o.shape[0]
        counts = (self.num_prop_samples, self.num_prop_samples, self.num_nerf_samples)
        bufs, extras = [], []

        def launch():
            bufs.extend(dict(rgb=torch.empty(B, 3, device=dev), sdist=torch.empty(B, n + 1, device=dev),
                             weights=torch.empty(B, n, device=dev), rgbdens=torch.empty(B, n, 4, device=dev)) for n in counts)
            arr = (_lib.MipLevelOut * 3)(*[_lib.MipLevelOut(*(b[k].data_ptr() for k in ("rgb", "sdist", "weights", "rgbdens")))
                                           for b in bufs])
            _lib.check(ctx.lib.neo_mip_render(ctx.handle, ptr(rays_o), ptr(rays_d), ptr(viewdirs), ptr(radii), B,
                                              float(train_frac), float(near), float(far), self.num_prop_samples,
                                              self.num_nerf_samples, arr, ctx.stream()))
            self._after_call(ctx)
            if self.compute_extras:            # on this call's stream, behind the render; the outputs join the tracked ones
                from . import ops
                for b in bufs:
                    extras.append(ops.mip_extras(b["sdist"], b["weights"], self.EXTRA_QUANTILES, near, far, ctx=ctx))
            return [t for b in bufs for t in b.values()] + [t for e in extras for t in e]
        self._launch_overlapped(ctx, dev, raw, (rays_o, rays_d, viewdirs, radii), launch)
        renderings = [{"rgb": b["rgb"]} for b in bufs]
        for r, e in zip(renderings, extras):
            r.update(self._extras_dict(*e))
        history = [dict(density=b["rgbdens"][..., 3], rgb=b["rgbdens"][..., :3], sdist=b["sdist"], weights=b["weights"])
                   for b in bufs]
        return renderings, history

    @torch.no_grad()
    def eval_mlp(self, slot, batch, tdist):
        """Stage-level access: cast_rays + MLP for the intervals of tdist (B,n+1) -> (B,n,4) = (rgb, density).
        batch["rays_o"] (B,3) defines B; rays_d, viewdirs (B,3), radii (B,1), (B,) or (1,B); tdist defines n."""
        rays_o, rays_d, viewdirs = _ray_rows(batch)
        radii = dense(batch["radii"], "radii", _radii_shapes(rays_o.shape[0]), device=rays_o.device)
        tdist = _sample_rows(tdist, "tdist", rays_o)
        if tdist.shape[1] < 2:
            raise ValueError("tdist must have shape (%d, n + 1) with n >= 1, got %s" % (rays_o.shape[0], tuple(tdist.shape)))
        ctx = self._context(rays_o.device)
        self._sync_weights(ctx)
        B, n1 = tdist.shape
        out = torch.empty(B, n1 - 1, 4, device=rays_o.device)
        _lib.check(ctx.lib.neo_mip_mlp(ctx.handle, slot, ptr(rays_o), ptr(rays_d), ptr(viewdirs), ptr(radii), ptr(tdist),
                                       B, n1 - 1, ptr(out), ctx.stream()))
        self._raise_flags(ctx.poll_flags())     # stage-level access: always immediate
        return out
