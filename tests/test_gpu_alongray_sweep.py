"""GPU: the wave-per-ray kernels - compositing and its backward, distortion loss, the two inverse-CDF resamplers, the Mip-NeRF 360
resampler and compositing pair - against the fp64 oracle under autograd, case by case of tests/alongray_cases.py: sample counts
on the edges of a 64-lane round and of the entry points, nine rays per case with degenerate rows, ray counts that leave one, two
and three waves of a block idle, bounds per entry (the table's conditions are checked on the CPU by test_alongray_cases_cpu.py).
Also: upstream gradients that are absent, the limits the entry points enforce (refused on the host, nothing launched), and
results that do not depend on how many rays the call holds."""
import pytest
import torch

import alongray_cases as A
from conftest import record_parity
from neo360_amd import _lib, ops, training
from neo360_amd.context import get_context, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _record(kernel, case, checks):
    record_parity("alongray_sweep/%s/%s" % (kernel, case), **A.summarize(checks))
    A.assert_inside(checks, (kernel, case))


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- compositing -----------------------------------------------------------------------------------------------------------------
def _composite(inp, mode, white, which=None, rows=None):
    """Forward through ops.composite and training.composite (the same kernel: bit-identical), backward through training.composite."""
    cut = (lambda x: x[:rows].contiguous()) if rows is not None else (lambda x: x)
    g = lambda k: cut(inp[k]).to(DEV)
    d = g("dirs") if mode != 2 else None
    far = g("far") if mode == 1 else None
    fwd = ops.composite(mode, torch.cat([g("rgb"), g("sigma")], dim=-1), g("t"), d, far, white)
    with torch.enable_grad():
        rg, sg = g("rgb").requires_grad_(True), g("sigma").requires_grad_(True)
        o_rgb, o_acc, o_w, o_lam, o_depth = training.composite(mode, rg, sg, g("t"), d, far, white)
        outs = dict(rgb=o_rgb, acc=o_acc, weights=o_w, depth=o_depth)
        if mode == 1:
            outs["lam"] = o_lam
        names = [k for k in A.COMPOSITE_OUTPUTS if k in outs and (which is None or k in which)]
        loss = sum((outs[k] * cut(inp["up"][k]).to(DEV)).sum() for k in names)
        g_rgb, g_sigma = torch.autograd.grad(loss, [rg, sg])
    for k, key in (("rgb", "rgb"), ("acc", "acc"), ("weights", "weights"), ("depth", "depth"), ("lam", "bg_lambda")):
        if k in outs:
            assert torch.equal(outs[k].detach(), fwd[key]), ("ops.composite and training.composite disagree", k)
    got = {k: v.detach().cpu() for k, v in outs.items()}
    got.update(g_rgb=g_rgb.cpu(), g_sigma=g_sigma[..., 0].cpu())
    return got


@pytest.mark.parametrize("N", A.COMPOSITE_N)
@pytest.mark.parametrize("mode", A.COMPOSITE_MODES)
def test_composite_forward_and_backward(mode, N):
    """Every output and both gradients, entry by entry.  What this found: with alpha = 1 - expf(-sigma delta) the thin row (density
    1e-6) lost all of its weight - next to 1 an ulp of expf's result is 6e-8 of alpha, every expf returned exactly 1 - and in mode 0
    at N = 127 .. 129 the last sample's weight was off by 2.6e-6 against the bound 2e-6 where the fp32 oracle is off by 6.5e-7.  The
    kernels take alpha from the series x - x^2 / 2 below x = 2^-17 since (common.h:alpha_of)."""
    for white in (False, True):
        inp, ref64, ref32 = A.composite_case(mode, N, white)
        got = _composite(inp, mode, white)
        _record("composite", "mode%d_N%d_white%d" % (mode, N, white), A.composite_checks(got, mode, ref64, ref32))


@pytest.mark.parametrize("mode", A.COMPOSITE_MODES)
def test_composite_ray_counts(mode):
    for R in A.RAY_COUNTS:
        inp, ref64, ref32 = A.composite_case(mode, A.COMPOSITE_MID_N, False, R, False)
        _record("composite", "mode%d_N%d_R%d" % (mode, A.COMPOSITE_MID_N, R), A.composite_checks(_composite(inp, mode, False), mode, ref64, ref32))


@pytest.mark.parametrize("which", [("rgb",), ("weights",), ("lam",)])
def test_composite_backward_with_absent_upstream_gradients(which):
    """A loss on one output only: the other upstream gradients never reach the backward as values of the loss."""
    for mode in A.COMPOSITE_MODES:
        if which == ("lam",) and mode != 1:
            continue
        inp, ref64, ref32 = A.composite_case(mode, 65, True, A.R_DEG, True, which)
        got = _composite(inp, mode, True, which)
        checks = A.composite_checks(dict(g_rgb=got["g_rgb"], g_sigma=got["g_sigma"]), mode, ref64, ref32)
        _record("composite", "mode%d_N65_loss_on_%s" % (mode, which[0]), checks)


def test_composite_backward_null_upstream_pointers():
    """The C entry point takes NULL for an upstream gradient that does not exist (autograd hands the wrapper zeros instead): NULL
    everywhere but g_rgb equals the gradient of the rgb-only loss, bit for bit the same as zeros in their place."""
    mode, N = 1, 65
    inp, ref64, ref32 = A.composite_case(mode, N, True, A.R_DEG, True, ("rgb",))
    c = get_context(torch.device(DEV))
    R = A.R_DEG
    rs = torch.cat([inp["rgb"], inp["sigma"]], dim=-1).to(DEV).contiguous()
    t, d, far, up = inp["t"].to(DEV), inp["dirs"].to(DEV), inp["far"].reshape(-1).to(DEV).contiguous(), inp["up"]["rgb"].to(DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    outs = []
    for nulls in (True, False):
        g = torch.full((R, N, 4), -7.0, device=DEV)
        rest = [None] * 4 if nulls else [ptr(z(R)), ptr(z(R)), ptr(z(R, N)), ptr(z(R, 1))]
        _lib.check(c.lib.neo_composite_backward(c.handle, mode, ptr(rs), ptr(t), ptr(d), ptr(far), R, N, 1, ptr(up), rest[0], rest[1],
                                                rest[2], rest[3], ptr(g), c.stream()))
        outs.append(g.cpu())
    assert torch.equal(outs[0], outs[1])
    checks = A.composite_checks(dict(g_rgb=outs[0][..., :3], g_sigma=outs[0][..., 3]), mode, ref64, ref32)
    _record("composite", "mode1_N65_null_upstream", checks)


def test_composite_backward_sample_limit():
    """1024 samples run (the sweep); 1025 are refused by neo_composite_backward on the host and nothing is written."""
    c = get_context(torch.device(DEV))
    R, N = 5, 1025
    rs, t, d = torch.rand(R, N, 4, device=DEV), torch.sort(torch.rand(R, N, device=DEV), dim=-1).values, torch.randn(R, 3, device=DEV)
    g = torch.full((R, N, 4), -7.0, device=DEV)
    rc = c.lib.neo_composite_backward(c.handle, 0, ptr(rs), ptr(t), ptr(d), None, R, N, 0, ptr(torch.ones(R, 3, device=DEV)), None, None,
                                      None, None, ptr(g), c.stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((g == -7.0).all())
    with torch.enable_grad():
        a, b = rs[..., :3].clone().requires_grad_(True), rs[..., 3:].clone().requires_grad_(True)
        out = training.composite(0, a, b, t, d)                    # the forward has no such limit
        assert bool(torch.isfinite(out[0]).all())
        with pytest.raises(_lib.NeoError, match="N <= 1024"):
            out[0].sum().backward()


@pytest.mark.parametrize("mode", A.COMPOSITE_MODES)
def test_composite_rows_do_not_depend_on_the_ray_count(mode):
    """Rows [0, r) of the nine-ray call equal the r-ray call bit for bit: idle waves of a block must not disturb live ones."""
    for N in (65, 1024):
        inp, _, _ = A.composite_case(mode, N, False)
        full = _composite(inp, mode, False)
        for r in (1, 3, 5):
            part = _composite(inp, mode, False, rows=r)
            for k, v in part.items():
                assert torch.equal(v, full[k][:r]), (mode, N, r, k)


# ---- distortion loss -------------------------------------------------------------------------------------------------------------
def _distloss(inp, rows=None):
    cut = (lambda x: x[:rows].contiguous()) if rows is not None else (lambda x: x)
    with torch.enable_grad():
        w = cut(inp["w"]).to(DEV).requires_grad_(True)
        loss = training.eff_distloss(w, cut(inp["m"]).to(DEV), inp["interval"])
        (g,) = torch.autograd.grad(loss * 3.0, w)
    return dict(loss=loss.detach().cpu().reshape(1), g_w=g.cpu())


@pytest.mark.parametrize("N", A.DISTLOSS_N)
def test_distloss_forward_and_backward(N):
    inp, ref64, ref32 = A.distloss_case(N)
    _record("distloss", "N%d" % N, A.distloss_checks(_distloss(inp), ref64, ref32))


def test_distloss_ray_counts_and_row_independence():
    for R in A.RAY_COUNTS:
        inp, ref64, ref32 = A.distloss_case(A.DISTLOSS_MID_N, R, False)
        _record("distloss", "N%d_R%d" % (A.DISTLOSS_MID_N, R), A.distloss_checks(_distloss(inp), ref64, ref32))
    # per-ray losses and gradients straight from the entry point (the wrapper scales by the ray count): bit for bit
    c = get_context(torch.device(DEV))

    def raw(inp, rows):
        w, m = inp["w"][:rows].contiguous().to(DEV), inp["m"][:rows].contiguous().to(DEV)
        loss, grad = torch.empty(rows, device=DEV), torch.empty(rows, w.shape[1], device=DEV)
        _lib.check(c.lib.neo_distloss(c.handle, ptr(w), ptr(m), rows, w.shape[1], inp["interval"], ptr(loss), ptr(grad), c.stream()))
        return loss.cpu(), grad.cpu()

    for N in (65, 1024):
        inp, _, _ = A.distloss_case(N)
        full = raw(inp, A.R_DEG)
        for r in (1, 3, 5):
            assert _same(raw(inp, r), [x[:r] for x in full]), (N, r)


# ---- inverse-CDF resampling ------------------------------------------------------------------------------------------------------
def _resample(inp, n_new, descending, randomized, rows=None):
    cut = (lambda x: x[:rows].contiguous()) if rows is not None else (lambda x: x)
    t_prev, w = cut(inp["t_prev"]).to(DEV), cut(inp["w"]).to(DEV)
    if not randomized:
        return ops.resample(t_prev, w, n_new, descending=descending).cpu(), inp["u_det"]
    R = inp["t_prev"].shape[0]
    u = training.rand_uniform(inp["seed"], inp["stream"], R, n_new)
    assert torch.equal(u.cpu(), A.resample_draws(inp, R, n_new))
    return training.resample_u(t_prev, w, cut(u), descending=descending).cpu(), u.cpu()


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n_prev,n_new", A.RESAMPLE_SHAPES)
def test_resample_deterministic_and_randomized(n_prev, n_new, descending):
    for randomized in (False, True):
        inp, ref64, ref32 = A.resample_case(n_prev, n_new, descending)
        got, u = _resample(inp, n_new, descending, randomized)
        if randomized:
            ref64 = A.resample_oracle(inp["t_prev"], inp["w"], u, torch.float64)
            ref32 = A.resample_oracle(inp["t_prev"], inp["w"], u, torch.float32)
        A.resample_invariants(got, inp["t_prev"], n_new, descending)
        checks = A.resample_checks(got, inp, u, descending, ref64, ref32)
        if descending:
            # the strict 1e-4 on the rows the reference determines (the bound above is exactly that there), counted for the record
            checks["pos_desc"]["fp32"] = float((ref32.double() - ref64).abs().max())
        _record("resample_u" if randomized else "resample", "%s_%d_%d" % ("desc" if descending else "asc", n_prev, n_new), checks)
        if descending:
            record_parity("alongray_sweep/%s/desc_%d_%d" % ("resample_u" if randomized else "resample", n_prev, n_new),
                          rows_determined_to_1e_5=int(A.descending_well_determined(ref64, ref32).sum()), rows=A.R_DEG)


def test_resample_ray_counts_and_row_independence():
    n_prev, n_new = A.RESAMPLE_MID
    for descending in (False, True):
        for R in A.RAY_COUNTS:
            inp, ref64, ref32 = A.resample_case(n_prev, n_new, descending, R, False)
            got, u = _resample(inp, n_new, descending, False)
            A.resample_invariants(got, inp["t_prev"], n_new, descending)
            _record("resample", "%s_%d_%d_R%d" % ("desc" if descending else "asc", n_prev, n_new, R),
                    A.resample_checks(got, inp, u, descending, ref64, ref32, well_from=0))
        # surplus waves of the last block redo the last ray: they must not disturb the live ones
        for shape in (A.RESAMPLE_MID, (129, 895)):
            inp, _, _ = A.resample_case(shape[0], shape[1], descending)
            for randomized in (False, True):
                full, _ = _resample(inp, shape[1], descending, randomized)
                for r in (1, 3, 5):
                    part, _ = _resample(inp, shape[1], descending, randomized, rows=r)
                    assert torch.equal(part, full[:r]), (shape, descending, randomized, r)


def test_resample_limits():
    """n_prev = 3 and 258 and n_prev + n_new = 1025 are refused on the host by both entry points; the output buffer stays untouched."""
    c = get_context(torch.device(DEV))
    R = 5
    for n_prev, n_new in ((3, 16), (258, 16), (129, 896), (257, 768)):
        t_prev = torch.sort(torch.rand(R, n_prev, device=DEV), dim=-1).values
        w, u = torch.rand(R, n_prev, device=DEV), torch.rand(R, n_new, device=DEV)
        out = torch.full((R, n_prev + n_new), -7.0, device=DEV)
        rc0 = c.lib.neo_resample(c.handle, ptr(t_prev), ptr(w), R, n_prev, n_new, 0, ptr(out), c.stream())
        rc1 = c.lib.neo_resample_u(c.handle, ptr(t_prev), ptr(w), ptr(u), R, n_prev, n_new, 0, ptr(out), c.stream())
        torch.cuda.synchronize()
        assert rc0 != 0 and rc1 != 0 and bool((out == -7.0).all()), (n_prev, n_new)
        with pytest.raises(_lib.NeoError, match="unsupported sample counts"):
            ops.resample(t_prev, w, n_new)
        with pytest.raises(_lib.NeoError, match="unsupported sample counts"):
            training.resample_u(t_prev, w, u)


# ---- Mip-NeRF 360 proposal resampling --------------------------------------------------------------------------------------------
def _mip_resample(inp, n, dilate, randomized, rows=None):
    cut = (lambda x: x[:rows].contiguous()) if rows is not None else (lambda x: x)
    s_prev, w_prev = cut(inp["s_prev"]).to(DEV), cut(inp["w_prev"]).to(DEV)
    if randomized:
        sd, td = training.mip_resample_u(s_prev, w_prev, n, A.MIP_NEAR, A.MIP_FAR, dilate, A.MIP_DILATION, A.MIP_ANNEAL,
                                         inp["u_rand"].to(DEV), cut(inp["jitter"]).to(DEV))
    else:
        sd, td = ops.mip_resample(s_prev, w_prev, n, A.MIP_NEAR, A.MIP_FAR, dilate, A.MIP_DILATION, A.MIP_ANNEAL)
        # the caller's table through the randomized entry point without a jitter is the same call
        sd2, td2 = training.mip_resample_u(s_prev, w_prev, n, A.MIP_NEAR, A.MIP_FAR, dilate, A.MIP_DILATION, A.MIP_ANNEAL, inp["u_det"].to(DEV))
        assert torch.equal(sd, sd2) and torch.equal(td, td2)
    return sd.cpu(), td.cpu()


@pytest.mark.parametrize("dilate,n_prev", [(d, p) for d in (True, False) for p in A.MIP_RESAMPLE_NPREV[d]])
def test_mip_resample_deterministic_and_randomized(dilate, n_prev):
    for n in A.MIP_RESAMPLE_N:
        for randomized in (False, True):
            inp, ref64, ref32 = A.mip_resample_case(n_prev, n, dilate, randomized)
            sd, td = _mip_resample(inp, n, dilate, randomized)
            _record("mip_resample_u" if randomized else "mip_resample", "%s_%d_%d" % ("dilated" if dilate else "plain", n_prev, n),
                    A.mip_resample_checks(sd, td, ref64, ref32))


def test_mip_resample_ray_counts_and_row_independence():
    n_prev, n, dilate = A.MIP_RESAMPLE_MID
    for R in A.RAY_COUNTS:
        inp, ref64, ref32 = A.mip_resample_case(n_prev, n, dilate, True, R, False)
        sd, td = _mip_resample(inp, n, dilate, True)
        _record("mip_resample_u", "dilated_%d_%d_R%d" % (n_prev, n, R), A.mip_resample_checks(sd, td, ref64, ref32))
    for p, m, d in ((n_prev, n, dilate), (85, 256, True), (255, 65, False)):
        for randomized in (False, True):
            inp, _, _ = A.mip_resample_case(p, m, d, randomized)
            full = _mip_resample(inp, m, d, randomized)
            for r in (1, 3, 5):
                assert _same(_mip_resample(inp, m, d, randomized, rows=r), [x[:r] for x in full]), (p, m, d, randomized, r)


def test_mip_resample_limits():
    """n = 1 and 257, dilated n_prev = 1 and 86, undilated n_prev = 256: refused on the host, outputs untouched."""
    c = get_context(torch.device(DEV))
    R = 5
    for n_prev, n, dilate in ((24, 1, True), (24, 257, True), (1, 32, True), (86, 32, True), (256, 32, False), (24, 257, False)):
        s_prev = torch.sort(torch.rand(R, n_prev + 1, device=DEV), dim=-1).values
        w_prev, u = torch.rand(R, n_prev, device=DEV), torch.rand(max(n, 1), device=DEV)
        sd, td = torch.full((R, n + 1), -7.0, device=DEV), torch.full((R, n + 1), -7.0, device=DEV)
        rc0 = c.lib.neo_mip_resample(c.handle, ptr(s_prev), ptr(w_prev), R, n_prev, int(dilate), 0.01, 0.7, n, 0.2, 3.0, ptr(sd), ptr(td),
                                     c.stream())
        rc1 = c.lib.neo_mip_resample_u(c.handle, ptr(s_prev), ptr(w_prev), R, n_prev, int(dilate), 0.01, 0.7, n, ptr(u), None, 0.2, 3.0,
                                       ptr(sd), ptr(td), c.stream())
        torch.cuda.synchronize()
        assert rc0 != 0 and rc1 != 0 and bool((sd == -7.0).all()) and bool((td == -7.0).all()), (n_prev, n, dilate)
        with pytest.raises(_lib.NeoError):
            ops.mip_resample(s_prev, w_prev, n, 0.2, 3.0, dilate, 0.01, 0.7)


# ---- Mip-NeRF 360 compositing ----------------------------------------------------------------------------------------------------
def _mip_composite(inp, bg, which=("weights", "rgb"), rows=None):
    cut = (lambda x: x[:rows].contiguous()) if rows is not None else (lambda x: x)
    g = lambda k: cut(inp[k]).to(DEV)
    w0, c0 = ops.mip_composite(torch.cat([g("rgb"), g("density")[..., None]], dim=-1), g("tdist"), g("dirs"), bg)
    with torch.enable_grad():
        a, b = g("rgb").requires_grad_(True), g("density").requires_grad_(True)
        w, c = training.mip_composite(a, b, g("tdist"), g("dirs"), bg)
        loss = ((w * g("up_w")).sum() if "weights" in which else 0.0) + ((c * g("up_c")).sum() if "rgb" in which else 0.0)
        g_rgb, g_dens = torch.autograd.grad(loss, [a, b])
    assert torch.equal(w.detach(), w0) and torch.equal(c.detach(), c0)
    return dict(weights=w.detach().cpu(), rgb=c.detach().cpu(), g_rgb=g_rgb.cpu(), g_density=g_dens.cpu())


@pytest.mark.parametrize("n", A.MIP_COMPOSITE_N)
def test_mip_composite_forward_and_backward(n):
    for bg in (0.0, 1.0):
        inp, ref64, ref32 = A.mip_composite_case(n, bg)
        _record("mip_composite", "n%d_bg%d" % (n, bg), A.mip_composite_checks(_mip_composite(inp, bg), ref64, ref32))


def test_mip_composite_ray_counts_partial_losses_and_row_independence():
    n = A.MIP_COMPOSITE_MID_N
    for R in A.RAY_COUNTS:
        inp, ref64, ref32 = A.mip_composite_case(n, 1.0, R, False)
        _record("mip_composite", "n%d_bg1_R%d" % (n, R), A.mip_composite_checks(_mip_composite(inp, 1.0), ref64, ref32))
    for which in (("weights",), ("rgb",)):
        inp, ref64, ref32 = A.mip_composite_case(65, 1.0, A.R_DEG, True, which)
        got = _mip_composite(inp, 1.0, which)
        _record("mip_composite", "n65_bg1_loss_on_%s" % which[0],
                A.mip_composite_checks(dict(g_rgb=got["g_rgb"], g_density=got["g_density"]), ref64, ref32))
    for m in (65, 256):
        inp, _, _ = A.mip_composite_case(m, 1.0)
        full = _mip_composite(inp, 1.0)
        for r in (1, 3, 5):
            part = _mip_composite(inp, 1.0, rows=r)
            for k, v in part.items():
                assert torch.equal(v, full[k][:r]), (m, r, k)
