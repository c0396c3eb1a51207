"""Case table, builders, fp64 / fp32 references and per-entry bounds for the matrix side of training: the three exact-fp32 GEMM entry
points (neo_linear_forward, neo_linear_input_grad, neo_linear_weight_grad = k_sgemm, k_dw + k_dw_reduce of csrc/train_mlp.hip) and
the four training chains built from them (NeRFPPMLP per row and on the projected latent, PixelNeRF on the projected latent, the
vanilla NeRFMLP, the Mip-NeRF 360 MLP; csrc/train_chain.h).  Plain CPU torch: tests/test_train_matrix_cases_cpu.py checks the
conditions of every case on the very inputs tests/test_gpu_train_matrix_sweep.py hands to the kernels.

Every table is derived from the launch geometry, the constant an edge comes from named beside it.  The constants below mirror
csrc/train_mlp.hip / train_chain.h / kernels.h (the CPU test reads them back out of the sources).
Upstream gradients are N(0.5, 1) x 1e-3 (x 1 for the Mip MLP), not zero-mean: a bias gradient is the plain sum of them over the rows,
and a bound relative to a sum that cancels would measure the cancellation, not the kernel.

Bounds (no new constants): primitives 2e-6 x max(1, largest |fp64 entry|) forward, 3e-6 x max(largest |fp64 entry|, 1e-6) input
gradient (test_gpu_pix_training.py::test_linear_matches_fp64_autograd), 2e-6 x largest |fp64 entry| weight gradient and its db rule
(test_gpu_host_r5.py::test_linear_weight_grad_matches_fp64); chains 2e-5 absolute on outputs, 2e-5 x the tensor's largest |fp64
entry| on every gradient (test_gpu_training.py).  Every comparison is per entry (alongray_cases.worst_entry / summarize).

ReLU kinks: a unit whose pre-activation is ~0 has derivative 0 or 1 depending on the last bit in any arithmetic.  The chain builders
draw more candidate points (rays, for the Mip MLP whose intervals share a ray) than a case needs, run the fp64 oracle once with
every argument of torch.relu recorded, reject a candidate with a pre-activation within KINK_MARGIN of zero in any of its views /
intervals and keep the first survivors: every case has exactly the row count its table names.  KINK_CAP bounds the rejected share."""
import contextlib
import functools
import math

import torch

import oracle
from alongray_cases import _gen, worst_entry, summarize, assert_inside      # noqa: F401  (re-exported for the two test files)
from neo360_amd import models, synth
from oracle import mip360

# ---- launch geometry (mirrors of the sources) ------------------------------------------------------------------------------------
GTM, GTN, GK = 128, 64, 32          # k_sgemm: C tile rows, C tile columns as neo_linear_* launch it, K step
DW_NT = (64, 128)                   # k_dw<NT>: tile columns (128 when N > 64); its tile rows are 128
DW_ZG = 16                          # k_dw_reduce: K slices summed per workgroup row
DW_PART_TILES = 520                 # scratch of one weight-gradient call, in partial tiles
DW_MIN_SLICE = 1024                 # dw_gemm: a K slice keeps >= 1024 rows
XCD = 8                             # xcd_pair: row blocks are dealt in groups of 8; blocks past the last full group keep the plain map
CH_ROWS = 64                        # train_chain.h: rows per workgroup of the fused chains (two 32-row halves)
TP_MAX_VIEWS = 8
MAX_M, MAX_N, MAX_F = 1024, 4096, 4096      # neo_linear_weight_grad: M, N; neo_linear_forward / _input_grad: features

FWD, DX, DW_W, DW_B = 2e-6, 3e-6, 2e-6, 2e-6
CHAIN_OUT, CHAIN_GRAD = 2e-5, 2e-5
KINK_MARGIN = 1e-5
KINK_CAP = {"nerfpp": 0.10, "nerfpp_proj": 0.10, "pix_proj": 0.10, "vanilla": 0.10, "mip": 0.25}
MIN_CANDIDATES = 96                 # candidates drawn for the smallest cases: one rejection is ~1 % of them
VIEWS8_GAIN = 3.0
LIFT_MIN_K = 513                    # a sequential-order lift is never applied to a reduction of <= 512 terms
# (family, case id): cases whose bound carries 3 x the error of a CPU fp32 emulation of the kernel's sequential summation order (see
# sequential_fp32_forward).  One case: 262,144 sums of 4096 terms each, largest |entry| 29.7 - the MFMA chain adds the terms one after
# the other, every addition rounds at the size of the running sum, and the largest of that many random walks ends 7.2e-5 from fp64
# (bound 5.9e-5; a blocked CPU matmul, which adds short partial sums, is off by 9.9e-6).  The emulation is the yardstick, never the kernel.
SEQ_LIFT = {("fwd", "r1024_n256_k4096_plain")}


def dw_slices(M, N, K):
    """(NT, tiles_x, tiles_y, K slices) of dw_gemm for one call: the host arithmetic of csrc/train_mlp.hip, restated."""
    NT = 128 if N > 64 else 64
    tx, ty = (N + NT - 1) // NT, (M + 127) // 128
    tiles = tx * ty
    nz = (512 + tiles - 1) // tiles
    nz = min(nz, max(K // DW_MIN_SLICE, 1))
    if nz * tiles > DW_PART_TILES:
        nz = DW_PART_TILES // tiles
    kps = (K + nz - 1) // nz
    kps = (kps + GK - 1) // GK * GK
    return NT, tx, ty, (K + kps - 1) // kps


def full_k_steps(rows, width, K):
    """Full K steps the pipelined interior path of k_sgemm takes in a launch of this shape (None: no interior tile) and whether a
    partial last step follows."""
    interior = rows >= GTM and width >= GTN
    return (K // GK if interior and K >= GK else None), K % GK != 0


# ---- forward and input gradient ------------------------------------------------------------------------------------------------------
# reduction lengths: 0 (remainder only), 1, 2, 3, 4 full steps of GK = 32 (the < 5 prologue and its four drains), 5, 6, 7 (the
# two-ahead prologue, odd and even, drains of 1 .. 4 after the unrolled-by-two loop), each with and without a partial last step
LIN_K = (1, 3, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, 160, 161, 191, 192, 193, 224, 255, 703, 1024, 4096)      # 129, 193: 4 and 6 full steps + a partial one
LIN_N = (1, 3, 63, 64, 65, 127, 128, 130, 256, 4096)                    # GTN = 64: below, on and above one and two column tiles; MAX_F
# GTM = 128: below / on / above one row block; 8 blocks + 1 and 2 x 8 + plain-mapped remainder (XCD groups), exactly 8 blocks
LIN_ROWS = (1, 2, 63, 64, 65, 127, 128, 129, 1024 + 5, 128 * 19 + 5, 128 * 8)
LIN_MID = (GTM + 5, GTN + 3, 3 * GK + 4)                                 # rows, width, reduction: one interior tile and every kind of edge tile
LIN_OPTION_SHAPES = ((133, 67, 100), (129, 65, 33), (64, 63, 31), (300, 130, 224))     # the third is edge tiles only
LIN_CORNERS = ((1, 1, 1), (1, 65, 4096), (1, 4096, 1), (129, 65, 33), (65, 130, 161), (128, 64, 32), (128 * 19 + 5, 4096, 32),
               (1024, 256, 4096), (2, 3, 703))
LIN_OPTIONS = {"fwd": ("plain", "nobias", "relu", "acc", "acc_relu", "pad"), "dx": ("plain", "acc", "pad")}


def linear_table(kind):
    """(rows, width, reduction, option): width = out_f and reduction = in_f for the forward, width = in_f and reduction = out_f for
    the input gradient.  One axis at its edges with the others mid-sized, the all-edge corners, every option at LIN_OPTION_SHAPES."""
    r0, n0, k0 = LIN_MID
    t = [(r0, n0, k, "plain") for k in LIN_K] + [(r0, n, k0, "plain") for n in LIN_N] + [(r, n0, k0, "plain") for r in LIN_ROWS]
    t += [c + ("plain",) for c in LIN_CORNERS]
    t += [s + (o,) for o in LIN_OPTIONS[kind] if o != "plain" for s in LIN_OPTION_SHAPES]
    return list(dict.fromkeys(t))


def linear_id(case):
    return "r%d_n%d_k%d_%s" % case


PAD_NAN = float("nan")       # padding of an operand: a kernel that reads it into a sum shows up as a non-finite result
PAD_OUT = -7.0               # padding of a result: must come back bit-unchanged


@functools.lru_cache(maxsize=None)
def linear_case(kind, rows, width, red, option):
    """Inputs and references of one forward ('fwd') / input-gradient ('dx') case.
    a (rows, red) ~ N(0, 1): x or gy; w ~ 0.1 N(0, 1): (width, red) for the forward, (red, width) for the input gradient (the
    weight of the layer, (out, in)); bias (width,) or None; c0 (rows, width) the non-zero result buffer of accumulate = 1, or None.
    Pitches (option 'pad'): lda = red + 3, ldc = width + 5, W a column block starting at column 1 of a matrix 7 columns wider, so
    that its rows are 4-byte aligned only."""
    gen = _gen(31 if kind == "fwd" else 37, rows, width, red, sum(map(ord, option)))
    a = torch.randn(rows, red, generator=gen)
    w = torch.randn((width, red) if kind == "fwd" else (red, width), generator=gen) * 0.1
    bias = torch.randn(width, generator=gen) * 0.1 if kind == "fwd" and option != "nobias" else None
    acc = option in ("acc", "acc_relu")
    relu = option in ("relu", "acc_relu")
    c0 = torch.randn(rows, width, generator=gen) if acc else None
    pad = dict(lda=red + 3, ldc=width + 5, w_col0=1, w_extra=7) if option == "pad" else dict(lda=red, ldc=width, w_col0=0, w_extra=0)

    def ref(dtype, drop_last_k=False):
        ad, wd = a.to(dtype), w.to(dtype)
        if drop_last_k:
            ad = ad[:, :-1]
            wd = wd[:, :-1] if kind == "fwd" else wd[:-1]
        y = ad @ (wd.t() if kind == "fwd" else wd)
        if bias is not None:
            y = y + bias.to(dtype)
        if acc:
            y = c0.to(dtype) + y                     # documented order: accumulate, then ReLU
        return torch.relu(y) if relu else y

    return dict(kind=kind, a=a, w=w, bias=bias, c0=c0, relu=relu, acc=acc, pad=pad, ref64=ref(torch.float64), ref32=ref(torch.float32),
                ref64_k_dropped=ref(torch.float64, True) if red > 1 else None)


def linear_bound(kind, ref64):
    m = float(ref64.abs().max())
    return FWD * max(1.0, m) if kind == "fwd" else DX * max(m, 1e-6)


def sgemm_k_order(K):
    """The order in which k_sgemm adds the terms of a sum, as its comments document it: K steps of GK = 32; inside a step four groups
    of 8 (c), in a group four MFMAs (e) that each add the pair k = 8 c + e (lane half 0) and k = 8 c + 4 + e (lane half 1)."""
    for k0 in range(0, K, GK):
        for c in range(GK // 8):
            for e in range(4):
                for k in (k0 + 8 * c + e, k0 + 8 * c + 4 + e):
                    if k < K:
                        yield k


@functools.lru_cache(maxsize=None)
def sequential_fp32_forward(kind, rows, width, red, option):
    """A plain fp32 running sum over k in sgemm_k_order (product rounded, then added), then the epilogue: what a faithful sequential
    evaluation of the case gives on the CPU.  -> (result fp32, its largest |error| against fp64)."""
    c = linear_case(kind, rows, width, red, option)
    assert kind == "fwd"
    a, wt = c["a"], c["w"].t().contiguous()
    acc = torch.zeros(rows, width)
    for k in sgemm_k_order(red):
        acc += a[:, k:k + 1] * wt[k]
    y = acc if c["bias"] is None else acc + c["bias"]
    if c["acc"]:
        y = c["c0"] + y
    y = torch.relu(y) if c["relu"] else y
    return y, float((y.double() - c["ref64"]).abs().max())


def linear_lift(kind, case_key):
    """0, or for a case of SEQ_LIFT 3 x the sequential emulation's worst error (never for a reduction of <= 512 terms)."""
    if (kind, linear_id(case_key)) not in SEQ_LIFT:
        return 0.0
    assert case_key[2] >= LIFT_MIN_K
    return 3.0 * sequential_fp32_forward(kind, *case_key)[1]


def linear_checks(case, got, lift=0.0):
    bound = linear_bound(case["kind"], case["ref64"]) + lift
    return {"y" if case["kind"] == "fwd" else "gx": worst_entry(got, case["ref64"], bound, case["ref32"])}


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
DW_M = (1, 3, 64, 127, 128, 129, 300, 1024)                              # 128-row tiles: below / on / above one; MAX_M
DW_N = (1, 27, 63, 64, 65, 128, 130, 504, 4096)                          # NT = 64 up to N = 64, 128 above; MAX_N
# GK = 32 and the 1024-row slices: 1, 2 and 17 (> DW_ZG) slices, a partial last step, one of the length the training step produces
DW_K = (1, 31, 32, 33, 1023, 1024, 1025, 2048 + 7, 17 * 1024 + 3, 70001)
DW_MID = (129, 65, 1100)                                                 # M, N, K: interior + edge tiles, one slice with a partial step
DW_OPTION_SHAPES = ((129, 65, 1100), (128, 128, 2048 + 7), (3, 27, 33), (300, 130, 17 * 1024 + 3))
DW_OPTIONS = ("plain", "nodb", "pad", "unscaled", "onto")


def dw_table():
    m0, n0, k0 = DW_MID
    t = [(m, n0, k0, "plain") for m in DW_M] + [(m0, n, k0, "plain") for n in DW_N]
    t += [(128, 128, k, "plain") for k in DW_K if k != 70001] + [(128, 63, 70001, "plain")]
    t += [(1024, 4096, 33, "plain"), (1, 1, 1, "plain"), (1024, 1, 1025, "plain"), (1, 4096, 31, "plain")]      # 1024 x 4096: the largest grid, 256 tiles
    t += [s + (o,) for o in DW_OPTIONS if o != "plain" for s in DW_OPTION_SHAPES]
    return list(dict.fromkeys(t))


def dw_id(case):
    return "m%d_n%d_k%d_%s" % case


@functools.lru_cache(maxsize=None)
def dw_case(M, N, K, option):
    """gy (K, M) ~ N(0, 1) with rows scaled by 10^U(-4, 0) (not 'unscaled'), x (K, N) ~ N(0, 1); dW (M, N) = gy^T x, db (M) = column
    sums of gy (not 'nodb'); 'onto': added into the caller's non-zero dW0 / db0; 'pad': ldy = M + 3, ldx = N + 5, ldw = N + 9 (dW
    as the column block of a wider gradient)."""
    gen = _gen(41, M, N, K, sum(map(ord, option)))
    gy = torch.randn(K, M, generator=gen)
    if option != "unscaled":
        gy = gy * 10.0 ** (-4.0 * torch.rand(K, 1, generator=gen))
    x = torch.randn(K, N, generator=gen)
    onto = option == "onto"
    w0 = torch.randn(M, N, generator=gen) * math.sqrt(K) * 0.3 if onto else None
    b0 = torch.randn(M, generator=gen) * math.sqrt(K) * 0.3 if onto else None
    pad = dict(ldy=M + 3, ldx=N + 5, ldw=N + 9) if option == "pad" else dict(ldy=M, ldx=N, ldw=N)

    def ref(dtype, drop_last_row=False):
        g, xx = gy.to(dtype), x.to(dtype)
        if drop_last_row:
            g, xx = g[:-1], xx[:-1]
        if dtype == torch.float32 and g.shape[0] > MAX_F:
            # the fp32 oracle of a long reduction adds the products of DW_MIN_SLICE-row slices: on some CPUs torch's one-pass fp32 matmul
            # over 17,000+ rows is a sequential sum whose own error passes the bound (measured: 1.97 of it on one x86 host, 0.2 on
            # another) - the yardstick of fp32 rounding must not depend on the BLAS of the machine that computes it
            dw = sum(g[i:i + DW_MIN_SLICE].t() @ xx[i:i + DW_MIN_SLICE] for i in range(0, g.shape[0], DW_MIN_SLICE))
            db = g.sum(0)
        else:
            dw, db = g.t() @ xx, g.sum(0)
        return (dw + w0.to(dtype), db + b0.to(dtype)) if onto else (dw, db)

    w64, b64 = ref(torch.float64)
    w32, b32 = ref(torch.float32)
    dropped = ref(torch.float64, True)[0] if K > 1 else None
    return dict(gy=gy, x=x, w0=w0, b0=b0, db=option != "nodb", pad=pad, ref64=dict(dw=w64, db=b64), ref32=dict(dw=w32, db=b32),
                dw64_row_dropped=dropped)


def dw_bounds(case):
    w64, b64 = case["ref64"]["dw"], case["ref64"]["db"]
    return dict(dw=DW_W * float(w64.abs().max()),
                db=DW_B * max(float(b64.abs().max()), float(case["gy"].double().abs().sum(0).max()) * 1e-3))


def dw_checks(case, got_w, got_b=None):
    b = dw_bounds(case)
    checks = dict(dw=worst_entry(got_w, case["ref64"]["dw"], b["dw"], case["ref32"]["dw"]))
    if got_b is not None:
        checks["db"] = worst_entry(got_b, case["ref64"]["db"], b["db"], case["ref32"]["db"])
    return checks


# ---- the chains ----------------------------------------------------------------------------------------------------------------------
# (P, NV): P on the edges of CH_ROWS = 64 and of its 32-row halves; NV 1, 2, 3 and TP_MAX_VIEWS = 8; NV P covers 1, < 64 (every staged
# row clamped), multiples of 64, 64 k + 1 (65, 129), 64 k + 32 (a last workgroup whose second half is empty), 64 k + 33 (33, 3 x 715) and
# tiles that straddle two or more views (any P that is not a multiple of 64 with NV > 1; (21, 8): four views in one tile)
POINT_VIEWS = ((1, 1), (1, 2), (2, 3), (21, 1), (21, 3), (21, 8), (31, 2), (32, 1), (32, 2), (32, 3), (33, 1), (33, 3), (63, 1), (63, 2),
               (64, 1), (64, 3), (64, 8), (65, 1), (65, 2), (129, 1), (129, 3), (715, 3))
VANILLA_ROWS = (1, 2, 63, 64, 65, 127, 128, 129, 1024 + 5, 128 * 8)          # one sample per ray: rows are independent
# (width, depth, rgb): the skip concatenation feeds layer 5, so it fires from depth 6 on (a depth-5 network would widen the heads'
# input: neither the module nor the oracle builds one); width 1024 at depths 2 and 8, depth 8 at widths 256 and 1024
MIP_SHAPES = ((64, 1, False), (128, 2, False), (192, 6, True), (256, 4, False), (256, 8, True), (1024, 2, False), (1024, 8, True))
# (rays, intervals per ray): R n = 1, 2, 63, 64, 65, 127, 128, 129, 1029
MIP_RAYS = ((1, 1), (1, 2), (9, 7), (32, 2), (65, 1), (127, 1), (64, 2), (129, 1), (147, 7))
MIP_WIDE_RAYS = ((1, 1), (32, 2), (65, 1), (129, 1))                           # width 1024: few intervals per ray (the kink cap)
HEADS_UNFUSED_CASE = ("nerfpp_proj", 129, 3, 3)
OUTPUT_NAMES = ("rgb", "sigma", "density")


def chain_table(kind):
    if kind in ("nerfpp", "nerfpp_proj"):
        return [(kind, P, NV, 3 if i % 2 == 0 else 4) for i, (P, NV) in enumerate(POINT_VIEWS)] + [(kind, 65, 2, 4), (kind, 64, 3, 3)]
    if kind == "pix_proj":
        return [(kind, P, NV) for P, NV in POINT_VIEWS]
    if kind == "vanilla":
        return [(kind, r) for r in VANILLA_ROWS]
    t = []
    for i, (w, d, rgb) in enumerate(MIP_SHAPES):
        rays = MIP_WIDE_RAYS if w == 1024 else MIP_RAYS
        pick = rays if (w, d) == (256, 4) or w == 1024 else [rays[(i + j) % len(rays)] for j in (0, 2, 4, 7)] + [rays[-1]]
        t += [("mip", w, d, int(rgb), R, n) for R, n in dict.fromkeys(pick)]
    return t


def chain_id(case):
    return "_".join(str(c) for c in case[1:])


def chain_rows(case):
    """Rows the table names for a case: (points or rays kept, rows the kernels see)."""
    kind = case[0]
    if kind in ("nerfpp", "nerfpp_proj", "pix_proj"):
        return case[1], case[1] * case[2]
    if kind == "vanilla":
        return case[1], case[1]
    return case[4], case[4] * case[5]


@contextlib.contextmanager
def _recorded_relu(store):
    """Every argument of torch.relu while the oracle runs: the pre-activations of its ReLU units, whatever its layers are."""
    orig = torch.relu

    def rec(x):
        store.append(x.detach())
        return orig(x)

    torch.relu = rec
    try:
        yield
    finally:
        torch.relu = orig


@contextlib.contextmanager
def _patched(module, name, value):
    orig = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, orig)


def chain_state(case):
    """{parameter name: fp32 tensor} under the module's own names (no prefix), and a constructor of the parameter container."""
    kind = case[0]
    if kind in ("nerfpp", "nerfpp_proj"):
        ch, nv = case[3], case[2]
        prefix = "fg_fine_mlp." if ch == 3 else "bg_fine_mlp."
        sd = synth.nerf_tp_state(0)
        make = lambda: models.NeRFPPMLP(0, 10, 4, input_ch=ch, num_src_views=nv)
    elif kind == "pix_proj":
        prefix, sd = "fine_mlp.", synth.pixelnerf_state(0)
        make = lambda: models.PixelNeRFMLP()
    elif kind == "vanilla":
        prefix, sd = "fine_mlp.", synth.vanilla_state(0)
        make = lambda: models.NeRFMLP()
    else:
        _, w, d, rgb = case[:4]
        with torch.random.fork_rng():
            torch.manual_seed(1000 * d + w + rgb)
            m = models.MipNeRF360MLP(netdepth=d, netwidth=w, disable_rgb=not rgb)
        state = {k: v.detach().clone() for k, v in m.named_parameters()}
        return state, lambda: models.MipNeRF360MLP(netdepth=d, netwidth=w, disable_rgb=not rgb)
    return {k[len(prefix):]: v.clone() for k, v in sd.items() if k.startswith(prefix)}, make


def local_blocks(kind, pe):
    """Column ranges of the 512 local features in the layers that read them: [(layer, first column)]; `pre` holds their products side
    by side, 128 columns each."""
    return [("pts_linears.0", pe), ("pts_linears.3", 128 + pe)] if kind == "nerfpp_proj" else [("pts_linears.0", 63)]


def skip_columns(case):
    """(layer, first column of the re-concatenated input) of the skip layer, or None."""
    kind = case[0]
    if kind in ("nerfpp", "nerfpp_proj"):
        return "pts_linears.3", 128
    if kind == "vanilla":
        return "pts_linears.5", 256
    if kind == "mip" and case[2] >= 6:
        return "pts_linear.5", case[1]
    return None


def _raw_inputs(case, C):
    """C candidate points (rays) of a case, fp32."""
    kind = case[0]
    gen = _gen(*([{"nerfpp": 51, "nerfpp_proj": 52, "pix_proj": 53, "vanilla": 54, "mip": 55}[kind]] + list(case[1:])))
    r = lambda *s: torch.randn(*s, generator=gen)
    up = lambda *s: (torch.randn(*s, generator=gen) + 0.5) * 1e-3
    # eight views multiply a point's chance of sitting on a kink by eight: their inputs are three times as large (pre-activations
    # three times as spread out), which keeps the rejected share of those cases under the cap with the margin as it is
    gain = VIEWS8_GAIN if kind != "mip" and kind != "vanilla" and case[2] == TP_MAX_VIEWS else 1.0
    if kind in ("nerfpp", "nerfpp_proj"):
        nv, pe = case[2], 21 * case[3]
        return dict(x_enc=r(nv, C, pe) * gain, cond=r(nv * C, 27) * gain, world=r(nv * C, 128) * 0.3 * gain, local=r(nv * C, 512) * 0.3 * gain,
                    up_rgb=up(C, 3), up_sigma=up(C, 1))
    if kind == "pix_proj":
        nv = case[2]
        return dict(x_enc=r(nv, C, 63) * gain, cond=r(nv * C, 27) * gain, local=r(nv * C, 512) * 0.3 * gain, up_rgb=up(C, 3), up_sigma=up(C, 1))
    if kind == "vanilla":
        return dict(x_enc=r(C, 1, 63), d_enc=r(C, 27), up_rgb=up(C, 1, 3), up_sigma=up(C, 1, 1))
    n = case[5]
    return dict(x0=r(C, n, 504).clamp_(-1, 1), d_enc=r(C, 27), up_density=up(C, n) * 1e3, up_rgb=up(C, n, 3) * 1e3)


def _select(case, inp, idx):
    kind = case[0]
    out = {}
    for k, v in inp.items():
        if kind in ("nerfpp", "nerfpp_proj", "pix_proj") and k in ("cond", "world", "local", "pre"):
            nv = case[2]
            out[k] = v.reshape(nv, -1, v.shape[-1])[:, idx].reshape(-1, v.shape[-1]).contiguous()
        elif kind in ("nerfpp", "nerfpp_proj", "pix_proj") and k == "x_enc":
            out[k] = v[:, idx].contiguous()
        else:
            out[k] = v[idx].contiguous()
    return out


def with_pre(case, inp, state):
    """The projected chains' `pre`: the local features' contribution to the layers that read them, formed in fp64 from the local
    features and the weight blocks, handed over in fp32."""
    kind = case[0]
    if kind not in ("nerfpp_proj", "pix_proj"):
        return inp
    pe = 21 * case[3] if kind == "nerfpp_proj" else 63
    blocks = [state[l + ".weight"][:, c:c + 512].double() for l, c in local_blocks(kind, pe)]
    out = dict(inp)
    out["pre"] = (inp["local"].double() @ torch.cat(blocks, 0).t()).float()
    return out


def _selector_state(case, state, dtype):
    """The oracle MLP that takes `pre` as given: the local weight blocks replaced by selectors of columns 128 i .. 128 i + 127 of a
    'local feature' vector that is [pre | 0].  Same network, and autograd's gradient of that vector is the gradient of pre."""
    kind = case[0]
    pe = 21 * case[3] if kind == "nerfpp_proj" else 63
    st = {k: v.to(dtype).clone() for k, v in state.items()}
    for i, (layer, c) in enumerate(local_blocks(kind, pe)):
        st[layer + ".weight"][:, c:c + 512] = 0
        st[layer + ".weight"][:, c + 128 * i:c + 128 * i + 128] = torch.eye(128, dtype=dtype)
    return st


def chain_oracle(case, inp, state, dtype, relu_store=None, variant=None, selectors=True):
    """Outputs and gradients of loss = sum(output x upstream) through the oracle's restatement (oracle/mlp.py, oracle/mip360.py:mlp)
    under autograd in `dtype`: {name: tensor}, outputs under OUTPUT_NAMES, parameter gradients 'gw/<name>', input gradients 'g_*'.
    variant (planted errors for the CPU test): 'view0_weightless' the rows of view 0 count 0 in every view mean; 'no_skip' the skip
    segment of the skip layer removed."""
    kind = case[0]
    c = lambda x: x.to(dtype)
    projected = kind in ("nerfpp_proj", "pix_proj")
    st = _selector_state(case, state, dtype) if projected and selectors else {k: c(v).clone() for k, v in state.items()}
    if variant == "no_skip":
        layer, col = skip_columns(case)
        st[layer + ".weight"][:, col:] = 0
    stack = contextlib.ExitStack()
    with stack, torch.enable_grad():
        if relu_store is not None:
            stack.enter_context(_recorded_relu(relu_store))
        if variant == "view0_weightless":
            def vm(x, nv, npts):
                x = x.reshape(-1, nv, npts, x.shape[-1])
                return (x[:, 1:].sum(dim=1) / nv).reshape(-1, x.shape[-1])
            stack.enter_context(_patched(oracle.mlp, "_view_mean", vm))
        p = {k: v.requires_grad_(True) for k, v in st.items()}
        if kind in ("nerfpp", "nerfpp_proj", "pix_proj"):
            nv = case[2]
            rows = inp["cond"].shape[0]
            xe = c(inp["x_enc"]).clone().requires_grad_(True)
            if projected and selectors:
                loc = torch.cat([c(inp["pre"]), torch.zeros(rows, 512 - inp["pre"].shape[1], dtype=dtype)], -1).requires_grad_(True)
            else:
                loc = c(inp["local"]).clone().requires_grad_(True)
            ins = dict(g_x_enc=xe)
            if kind == "pix_proj":
                rgb, sigma = oracle.mlp.pixelnerf_mlp(p, "", xe, c(inp["cond"]), loc, nv)
            else:
                wf = c(inp["world"]).clone().requires_grad_(True)
                ins["g_world"] = wf
                rgb, sigma = oracle.mlp.nerfpp_mlp(p, "", xe, c(inp["cond"]), wf, loc, nv)
            ins["g_pre" if projected and selectors else "g_local"] = loc
            outs = dict(rgb=rgb, sigma=sigma)
            loss = (rgb * c(inp["up_rgb"])).sum() + (sigma * c(inp["up_sigma"])).sum()
        elif kind == "vanilla":
            xe, de = c(inp["x_enc"]).clone().requires_grad_(True), c(inp["d_enc"]).clone().requires_grad_(True)
            ins = dict(g_x_enc=xe, g_d_enc=de)
            rgb, sigma = oracle.mlp.vanilla_mlp(p, "", xe, de)
            outs = dict(rgb=rgb, sigma=sigma)
            loss = (rgb * c(inp["up_rgb"])).sum() + (sigma * c(inp["up_sigma"])).sum()
        else:
            _, w, d, has_rgb = case[:4]
            ins = {}
            x0 = c(inp["x0"])
            # the direction encodings are data of the case: the oracle takes them as they are
            stack.enter_context(_patched(mip360, "dir_enc", lambda v: v))
            dens, rgb = mip360.mlp(p, "", None, x0[..., :3], None, c(inp["d_enc"]), d, bool(has_rgb), x0=x0)
            outs = dict(density=dens)
            loss = (dens * c(inp["up_density"])).sum()
            if has_rgb:
                outs["rgb"] = rgb
                loss = loss + (rgb * c(inp["up_rgb"])).sum()
        names = sorted(p)
        grads = torch.autograd.grad(loss, [p[k] for k in names] + list(ins.values()), allow_unused=True)
    res = {k: v.detach() for k, v in outs.items()}
    for k, g in zip(names + list(ins), grads):
        like = p[k] if k in p else ins[k]
        g = torch.zeros_like(like) if g is None else g
        res[("gw/" + k) if k in p else k] = g
    if projected and selectors:
        res["g_pre"] = res["g_pre"][:, :inp["pre"].shape[1]].contiguous()
        pe = 21 * case[3] if kind == "nerfpp_proj" else 63
        for layer, col in local_blocks(kind, pe):               # these columns are trained through the texel-space GEMM: the chain leaves them 0
            res["gw/" + layer + ".weight"][:, col:col + 512] = 0
    return res


def _near_kink(case, store, C):
    """(C,) smallest |pre-activation| of a candidate over all units, views and intervals."""
    kind = case[0]
    near = torch.full((C,), float("inf"), dtype=torch.float64)
    for t in store:
        m = t.abs().amin(-1).reshape(-1).double()
        if kind in ("nerfpp", "nerfpp_proj", "pix_proj"):
            m = m.reshape(-1, C).amin(0)                     # view-major rows (v C + p), or C rows after a view mean
        else:
            m = m.reshape(C, -1).amin(1)                     # a ray's intervals / samples are consecutive rows
        near = torch.minimum(near, m)
    return near


@functools.lru_cache(maxsize=None)
def chain_case(case):
    """dict(inputs, state, make, ref64, ref32, candidates, rejected): inputs hold exactly the rows the table names."""
    kind = case[0]
    keep_n, _ = chain_rows(case)
    C = max(MIN_CANDIDATES, int(math.ceil(keep_n * (1.5 if kind == "mip" else 1.25))) + 16)
    state, make = chain_state(case)
    cand = with_pre(case, _raw_inputs(case, C), state)
    store = []
    chain_oracle(case, cand, state, torch.float64, relu_store=store)
    ok = _near_kink(case, store, C) > KINK_MARGIN
    idx = ok.nonzero().flatten()[:keep_n]
    assert idx.numel() == keep_n, (case, "too few candidates survive the kink filter", int(ok.sum()), keep_n)
    inp = _select(case, cand, idx)
    return dict(inputs=inp, state=state, make=make, candidates=C, rejected=int((~ok).sum()),
                ref64=chain_oracle(case, inp, state, torch.float64), ref32=chain_oracle(case, inp, state, torch.float32))


def chain_bound(name, ref64):
    return CHAIN_OUT if name in OUTPUT_NAMES else CHAIN_GRAD * max(float(ref64.abs().max()), 1e-30)


def chain_checks(got, ref64, ref32=None, names=None):
    """got {name: tensor} under the names of chain_oracle (a subset is fine) -> {name: worst_entry}."""
    return {k: worst_entry(got[k], ref64[k], chain_bound(k, ref64[k]), None if ref32 is None else ref32[k])
            for k in (names or got) if k in ref64}
