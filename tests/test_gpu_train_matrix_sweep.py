"""GPU: the matrix side of training - neo_linear_forward / _input_grad (k_sgemm), neo_linear_weight_grad (k_dw + k_dw_reduce) and the
four training chains (NeRFPPMLP per row and on the projected latent in both chain modes, PixelNeRF on the projected latent, the
vanilla NeRFMLP, the Mip-NeRF 360 MLP) - against fp64, case by case of tests/train_matrix_cases.py: reduction lengths on every arm
of the pipelined K loop, widths and row counts on the tile edges and on the XCD groups of the tile map, row pitches wider than the
row, accumulate = 1, K slices beyond one reduce group, point / view counts on the edges of a 64-row workgroup; bounds per entry
(the table's conditions are checked on the CPU by test_train_matrix_cases_cpu.py).  Also: results that do not depend on how many
points a call holds, chains that repeat bit for bit, the limits the entry points enforce (refused on the host, nothing launched) and
one case with the heads of the fused chain as separate launches (NEO360_TRAIN_HEADS=0, a fresh child process).

The primitives are called through the C entry points so that pitches and `accumulate` reach the kernels; the chains go through
neo360_amd.training."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import record_parity          # first: it puts the repository root on the path (also for the child process below)
import train_matrix_cases as M
from neo360_amd import _lib, training
from neo360_amd.context import get_context, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _record(kernel, case, checks, **extra):
    record_parity("train_matrix_sweep/%s/%s" % (kernel, case), **M.summarize(checks), **extra)
    M.assert_inside(checks, (kernel, case))


def _padded(t, pitch, fill, col0=0):
    """t (r, c) inside a (r, pitch) buffer filled with `fill`, starting at column col0 -> (buffer on the device, view of t's place)."""
    buf = torch.full((t.shape[0], pitch), fill, dtype=torch.float32)
    buf[:, col0:col0 + t.shape[1]] = t
    buf = buf.to(DEV)
    return buf, buf[:, col0:col0 + t.shape[1]]


# ---- forward and input gradient ----------------------------------------------------------------------------------------------------
def _run_linear(kind, case):
    rows, width, red, _ = case
    c = M.linear_case(kind, *case)
    pad = c["pad"]
    ctx = get_context(torch.device(DEV))
    a_buf, _ = _padded(c["a"], pad["lda"], M.PAD_NAN)
    w_buf, w_view = _padded(c["w"], c["w"].shape[1] + pad["w_extra"], M.PAD_NAN, pad["w_col0"])
    start = c["c0"] if c["acc"] else torch.full((rows, width), M.PAD_OUT)
    out_buf, out_view = _padded(start, pad["ldc"], M.PAD_OUT)
    bias = c["bias"].to(DEV) if c["bias"] is not None else None
    if kind == "fwd":
        _lib.check(ctx.lib.neo_linear_forward(ctx.handle, rows, width, red, ptr(a_buf), pad["lda"], ptr(w_view), w_buf.shape[1], ptr(bias),
                                              int(c["relu"]), int(c["acc"]), ptr(out_buf), pad["ldc"], ctx.stream()))
    else:
        _lib.check(ctx.lib.neo_linear_input_grad(ctx.handle, rows, width, red, ptr(a_buf), pad["lda"], ptr(w_view), w_buf.shape[1],
                                                 int(c["acc"]), ptr(out_buf), pad["ldc"], ctx.stream()))
    out = out_buf.cpu()
    assert bool((out[:, width:] == M.PAD_OUT).all()), "padding columns of the result were written"
    return c, out[:, :width].contiguous()


@pytest.mark.parametrize("case", M.linear_table("fwd"), ids=M.linear_id)
def test_linear_forward(case):
    """r1024_n256_k4096: 4096 terms added one after the other by the MFMA chain, 262,144 sums with entries up to 29.7 - the worst of them
    is 7.2e-5 from fp64 against the constant bound 5.9e-5.  That case alone carries 3 x the error of the CPU emulation of the same
    sequential order (train_matrix_cases.SEQ_LIFT); the emulation's error, the lift and the kernel's error are in the parity report."""
    c, got = _run_linear("fwd", case)
    lift = M.linear_lift("fwd", case)
    extra = dict(sequential_fp32_emulation_err=lift / 3.0, lift=lift, constant_bound=M.linear_bound("fwd", c["ref64"])) if lift else {}
    _record("linear_forward", M.linear_id(case), M.linear_checks(c, got, lift), **extra)


@pytest.mark.parametrize("case", M.linear_table("dx"), ids=M.linear_id)
def test_linear_input_grad(case):
    c, got = _run_linear("dx", case)
    _record("linear_input_grad", M.linear_id(case), M.linear_checks(c, got))


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.dw_table(), ids=M.dw_id)
def test_linear_weight_grad(case):
    Mm, N, K, _ = case
    c = M.dw_case(*case)
    pad = c["pad"]
    ctx = get_context(torch.device(DEV))
    gy_buf, _ = _padded(c["gy"], pad["ldy"], M.PAD_NAN)
    x_buf, _ = _padded(c["x"], pad["ldx"], M.PAD_NAN)
    w_buf, _ = _padded(c["w0"] if c["w0"] is not None else torch.zeros(Mm, N), pad["ldw"], M.PAD_OUT)
    db = (c["b0"].clone() if c["b0"] is not None else torch.zeros(Mm)).to(DEV) if c["db"] else None
    _lib.check(ctx.lib.neo_linear_weight_grad(ctx.handle, Mm, N, K, ptr(gy_buf), pad["ldy"], ptr(x_buf), pad["ldx"], ptr(w_buf), pad["ldw"],
                                              ptr(db), ctx.stream()))
    out = w_buf.cpu()
    assert bool((out[:, N:] == M.PAD_OUT).all()), "padding columns of dW were written"
    checks = M.dw_checks(c, out[:, :N].contiguous(), db.cpu() if db is not None else None)
    _record("linear_weight_grad", M.dw_id(case), checks, k_slices=M.dw_slices(Mm, N, K)[3])


# ---- the chains ----------------------------------------------------------------------------------------------------------------------
VARIANTS = {"nerfpp": ("rows",), "nerfpp_proj": ("fused", "layered"), "pix_proj": ("fused", "layered", "operators"), "vanilla": ("rows",),
            "mip": ("fused",)}


def _module(c):
    mlp = c["make"]()
    missing, unexpected = mlp.load_state_dict(c["state"], strict=False)
    assert not unexpected and all("." not in k for k in missing), (missing, unexpected)      # only buffers may be missing
    return mlp.to(DEV)


def _run_chain(case, variant, inp=None, mlp=None):
    """One forward and backward of a chain: {name: cpu tensor} under the names of train_matrix_cases.chain_oracle."""
    kind = case[0]
    c = M.chain_case(case)
    inp = c["inputs"] if inp is None else inp
    mlp = _module(c) if mlp is None else mlp
    g = lambda k: inp[k].to(DEV)
    lib = get_context(torch.device(DEV)).lib
    names = [n for n, _ in mlp.named_parameters()]
    params = [p for _, p in mlp.named_parameters()]
    old_mode = lib.neo_train_chain_mode(-1)
    try:
        if variant in ("fused", "layered"):
            lib.neo_train_chain_mode(1 if variant == "fused" else 0)
        with torch.enable_grad():
            for p in params:
                p.requires_grad_(True)
            ins = {}
            if kind in ("nerfpp", "nerfpp_proj", "pix_proj"):
                nv = case[2]
                ins["g_x_enc"] = g("x_enc").requires_grad_(True)
                if kind == "nerfpp":
                    ins["g_world"], ins["g_local"] = g("world").requires_grad_(True), g("local").requires_grad_(True)
                    rgb, sigma = training.nerfpp_mlp(mlp, ins["g_x_enc"], g("cond"), ins["g_world"], ins["g_local"], nv)
                elif kind == "nerfpp_proj":
                    ins["g_world"], ins["g_pre"] = g("world").requires_grad_(True), g("pre").requires_grad_(True)
                    rgb, sigma = training.nerfpp_mlp_projected(mlp, ins["g_x_enc"], g("cond"), ins["g_world"], ins["g_pre"], nv)
                else:
                    ins["g_pre"] = g("pre").requires_grad_(True)
                    fn = training.pixel_mlp_projected if variant == "operators" else training.pixel_mlp_fused
                    rgb, sigma = fn(mlp, ins["g_x_enc"], g("cond"), ins["g_pre"], nv)
                outs = dict(rgb=rgb, sigma=sigma)
                loss = (rgb * g("up_rgb")).sum() + (sigma * g("up_sigma")).sum()
            elif kind == "vanilla":
                ins["g_x_enc"], ins["g_d_enc"] = g("x_enc").requires_grad_(True), g("d_enc").requires_grad_(True)
                rgb, sigma = training.nerf_mlp(mlp, ins["g_x_enc"], ins["g_d_enc"])
                outs = dict(rgb=rgb, sigma=sigma)
                loss = (rgb * g("up_rgb")).sum() + (sigma * g("up_sigma")).sum()
            else:
                n = case[5]
                dens, rgb = training.mip_mlp_fused(mlp, g("x0").reshape(-1, 504), g("d_enc"), n)
                outs = dict(density=dens)
                loss = (dens * g("up_density")).sum()
                if case[3]:
                    outs["rgb"] = rgb
                    loss = loss + (rgb * g("up_rgb")).sum()
            grads = torch.autograd.grad(loss, params + list(ins.values()))
    finally:
        lib.neo_train_chain_mode(old_mode)
    got = {k: v.detach().cpu() for k, v in outs.items()}
    for k, gr in zip(["gw/" + n for n in names] + list(ins), grads):
        got[k] = gr.detach().cpu()
    return got


def _chain_test(case):
    c = M.chain_case(case)
    for variant in VARIANTS[case[0]]:
        got = _run_chain(case, variant)
        assert set(got) == set(c["ref64"]), (sorted(set(got) ^ set(c["ref64"])))
        label = M.chain_id(case) + ("" if variant == "rows" else "_" + variant)
        _record(case[0], label, M.chain_checks(got, c["ref64"], c["ref32"]), rows=M.chain_rows(case)[1])
        if case[0] in ("nerfpp_proj", "pix_proj"):
            pe = 21 * case[3] if case[0] == "nerfpp_proj" else 63
            for layer, col in M.local_blocks(case[0], pe):     # trained through the texel-space GEMM, not here
                assert float(got["gw/" + layer + ".weight"][:, col:col + 512].abs().max()) == 0.0, (variant, layer)


@pytest.mark.parametrize("case", M.chain_table("nerfpp"), ids=M.chain_id)
def test_nerfpp_mlp_per_row(case):
    _chain_test(case)


@pytest.mark.parametrize("case", M.chain_table("nerfpp_proj"), ids=M.chain_id)
def test_nerfpp_mlp_projected_both_chain_modes(case):
    _chain_test(case)


@pytest.mark.parametrize("case", M.chain_table("pix_proj"), ids=M.chain_id)
def test_pixel_mlp_projected_both_chain_modes_and_operators(case):
    _chain_test(case)


@pytest.mark.parametrize("case", M.chain_table("vanilla"), ids=M.chain_id)
def test_vanilla_mlp(case):
    _chain_test(case)


@pytest.mark.parametrize("case", M.chain_table("mip"), ids=M.chain_id)
def test_mip_mlp(case):
    _chain_test(case)


# ---- results that do not depend on the size of the call, and that repeat ---------------------------------------------------------------
INDEPENDENCE = {"nerfpp": (("nerfpp", 129, 3, 3), (1, 33, 64)), "nerfpp_proj": (("nerfpp_proj", 129, 3, 3), (1, 33, 64)),
                "pix_proj": (("pix_proj", 129, 3), (1, 33, 64)), "vanilla": (("vanilla", 129), (1, 63, 65)),
                "mip": (("mip", 256, 8, 1, 147, 7), (1, 9, 19))}


@pytest.mark.parametrize("kind", sorted(INDEPENDENCE))
def test_chain_results_do_not_depend_on_the_batch_and_repeat(kind):
    """The first P' points (rays) of a larger call equal the P'-point call bit for bit in every output and every input gradient (rows
    are independent but for the view mean / the ray's shared direction term, which stay inside a point); the parameter gradients of
    the smaller call - sums over its own rows, split over K slices - stay inside their bounds against fp64.  A call repeated gives
    the same outputs bit for bit."""
    case, subs = INDEPENDENCE[kind]
    assert case in M.chain_table(kind)
    c = M.chain_case(case)
    mlp = _module(c)
    view_major = kind in ("nerfpp", "nerfpp_proj", "pix_proj")
    for variant in VARIANTS[kind]:
        full = _run_chain(case, variant, mlp=mlp)
        again = _run_chain(case, variant, mlp=mlp)
        for k in full:
            if k in M.OUTPUT_NAMES:
                assert torch.equal(full[k], again[k]), (variant, k, "a repeated call differs")
        for keep in subs:
            inp = M._select(case, c["inputs"], torch.arange(keep))
            part = _run_chain(case, variant, inp=inp, mlp=mlp)
            for k, v in part.items():
                if k.startswith("gw/"):
                    continue
                w = full[k]
                if view_major and k == "g_x_enc":                                   # (NV, P, width)
                    w = w[:, :keep]
                elif view_major and k in ("g_world", "g_local", "g_pre"):           # view-major rows v P + p
                    w = w.reshape(case[2], -1, w.shape[-1])[:, :keep].reshape(-1, w.shape[-1])
                else:
                    w = w[:keep]
                assert torch.equal(v, w), (variant, keep, k, float((v - w).abs().max()))
            ref64 = M.chain_oracle(case, inp, c["state"], torch.float64)
            checks = M.chain_checks(part, ref64, None, [k for k in part if k.startswith("gw/")])
            _record(kind, "%s_first%d_%s" % (M.chain_id(case), keep, variant), checks)


# ---- the heads of the fused chain as separate launches ---------------------------------------------------------------------------------
def test_projected_chain_with_unfused_heads_in_a_fresh_process():
    """NEO360_TRAIN_HEADS=0 (the P-sized forward tail of the fused chain as separate launches) is read when the library loads: the case
    runs in a child process of its own, which compares against the same fp64 reference; its exit status is the verdict."""
    env = dict(os.environ, NEO360_TRAIN_HEADS="0")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--heads-unfused"], env=env,
                       capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if lines:
        record_parity("train_matrix_sweep/nerfpp_proj/%s_heads_unfused" % M.chain_id(M.HEADS_UNFUSED_CASE), **json.loads(lines[-1]))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def _heads_unfused_child():
    assert os.environ.get("NEO360_TRAIN_HEADS") == "0"
    case = M.HEADS_UNFUSED_CASE
    assert case in M.chain_table(case[0])
    c = M.chain_case(case)
    checks = M.chain_checks(_run_chain(case, "fused"), c["ref64"], c["ref32"])
    print(json.dumps(M.summarize(checks)))
    M.assert_inside(checks, case)


# ---- limits: refused on the host, nothing launched ---------------------------------------------------------------------------------------
def test_linear_entry_points_refuse_what_their_grids_cannot_hold():
    """rows > 65535 x 128, features > 4096, M > 1024 and a pitch smaller than the row: an error code from the host and the result
    buffer untouched (the row cap of the chains is asserted by test_gpu_api_rejects.py)."""
    ctx = get_context(torch.device(DEV))
    lib, h, s = ctx.lib, ctx.handle, ctx.stream()
    a, w = torch.randn(64, 64, device=DEV), torch.randn(64, 64, device=DEV)
    out = torch.full((64, 64), M.PAD_OUT, device=DEV)
    big = 65535 * 128 + 1
    rcs = [lib.neo_linear_forward(h, big, 8, 8, ptr(a), 8, ptr(w), 8, None, 0, 0, ptr(out), 8, s),
           lib.neo_linear_input_grad(h, big, 8, 8, ptr(a), 8, ptr(w), 8, 0, ptr(out), 8, s),
           lib.neo_linear_forward(h, 1, M.MAX_F + 1, 8, ptr(a), 8, ptr(w), 8, None, 0, 0, ptr(out), M.MAX_F + 1, s),
           lib.neo_linear_forward(h, 1, 8, M.MAX_F + 1, ptr(a), M.MAX_F + 1, ptr(w), M.MAX_F + 1, None, 0, 0, ptr(out), 8, s),
           lib.neo_linear_input_grad(h, 1, M.MAX_F + 1, 8, ptr(a), 8, ptr(w), M.MAX_F + 1, 0, ptr(out), M.MAX_F + 1, s),
           lib.neo_linear_input_grad(h, 1, 8, M.MAX_F + 1, ptr(a), M.MAX_F + 1, ptr(w), 8, 0, ptr(out), 8, s),
           lib.neo_linear_weight_grad(h, M.MAX_M + 1, 8, 8, ptr(a), M.MAX_M + 1, ptr(w), 8, ptr(out), 8, None, s),
           lib.neo_linear_weight_grad(h, 8, M.MAX_N + 1, 8, ptr(a), 8, ptr(w), M.MAX_N + 1, ptr(out), M.MAX_N + 1, None, s)]
    for ldx, ldw, ldy in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        rcs.append(lib.neo_linear_forward(h, 4, 8, 8, ptr(a), ldx, ptr(w), ldw, None, 0, 0, ptr(out), ldy, s))
        rcs.append(lib.neo_linear_input_grad(h, 4, 8, 8, ptr(a), ldy, ptr(w), ldw, 0, ptr(out), ldx, s))
        rcs.append(lib.neo_linear_weight_grad(h, 8, 8, 4, ptr(a), ldx, ptr(w), ldw, ptr(out), ldy, None, s))
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs), rcs
    assert bool((out == M.PAD_OUT).all())
    with pytest.raises(_lib.NeoError, match="row pitch smaller than the row"):
        _lib.check(lib.neo_linear_forward(h, 4, 8, 8, ptr(a), 7, ptr(w), 8, None, 0, 0, ptr(out), 8, s))
    with pytest.raises(_lib.NeoError, match="M <= 1024"):
        _lib.check(lib.neo_linear_weight_grad(h, M.MAX_M + 1, 8, 8, ptr(a), M.MAX_M + 1, ptr(w), 8, ptr(out), 8, None, s))


def test_mip_chain_refuses_a_width_that_is_not_a_multiple_of_64():
    ctx = get_context(torch.device(DEV))
    x0 = torch.randn(4, 504, device=DEV)
    out = torch.full((4, 4), M.PAD_OUT, device=DEV)
    for width, depth in ((100, 2), (32, 2), (1088, 2), (128, 0), (128, 9)):
        rc = ctx.lib.neo_mip_mlp_train_forward(ctx.handle, width, depth, 0, None, None, ptr(x0), None, 4, 1, ptr(out), ptr(out), ctx.stream())
        torch.cuda.synchronize()
        assert rc != 0 and bool((out == M.PAD_OUT).all()), (width, depth)
    with pytest.raises(_lib.NeoError, match="multiple of 64"):
        _lib.check(ctx.lib.neo_mip_mlp_train_forward(ctx.handle, 100, 2, 0, None, None, ptr(x0), None, 4, 1, ptr(out), ptr(out), ctx.stream()))


if __name__ == "__main__":
    if "--heads-unfused" in sys.argv:
        _heads_unfused_child()
