"""Case table of the three fused frame drivers that are not NeO-360's: neo_vanilla_render, neo_pix_render, neo_mip_render.  Plain CPU
torch: tests/test_frame_chain_cases_cpu.py checks the conditions of every case (the host-built level-0 row, finite oracles, the
fp32 oracle inside half of every bound) on the very inputs that tests/test_gpu_frame_chain_sweep.py hands to the drivers.

A case is one frame: sample counts on the edges of the drivers' limits and of the resampler's three sort widths, a ray count, a
(near, far) pair, a background, a parameter state and - PixelNeRF - the caller's chunk.  What the GPU test runs a case under
(arithmetic, pre-projection, NeRF MLP schedule) is the case's `variants`.

Bounds.  Nothing new: per ray and output TOL x max(1, |fp64 value|) on rgb, acc and depth (TOL = 1e-4 of test_gpu_vanilla.py,
test_gpu_pixelnerf.py, test_gpu_mip360.py and README's "parity <= 1e-4"), TOL_HIST x max(1, |fp64 value|) on Mip-NeRF 360's
per-interval weights and densities (2e-4 of test_end_to_end_vs_golden).  The fp64 oracle is evaluated at the sample rows the
implementation under test produced, so the samplers are out of the comparison and no ray is exempt."""
import collections
import functools

import numpy as np
import torch

import cases
import oracle
from alongray_cases import RAY_COUNTS, assert_inside, summarize, worst_entry  # noqa: F401  (re-exported for the two tests)
from neo360_amd import _lib, synth
from oracle import mip360

TOL = 1e-4
TOL_HIST = 2e-4
ORACLE_SHARE = 0.5        # the fp32 oracle, at its own rows against the fp64 oracle at those rows, stays inside this share of every bound

Case = collections.namedtuple("Case", "kind counts R near far white state tf chunk variants")

# ---- sample counts -------------------------------------------------------------------------------------------------------------
# (n_coarse, n_fine); N0 = n_coarse + 1 level-0 samples, N1 = N0 + n_fine merged ones.  The drivers accept 3 <= n_coarse <= 256,
# n_fine >= 1, N1 <= 1024; k_resample sorts N1 entries in 256, 512 or 1024 entries of LDS.
LEVEL_COUNTS = ((3, 1),                     # smallest accepted
                (3, 252), (63, 192),        # N1 = 256: the upper edge of the 256-entry network
                (64, 192),                  # 257
                (64, 447),                  # 512
                (65, 447),                  # 513
                (128, 895), (256, 767),     # 1024, the limit
                (255, 1),                   # many coarse samples, one fine
                (64, 128), (64, 64))        # the two renderers' defaults
LEVEL_MID = (64, 192)
LEVEL_LARGEST = (256, 767)
LEVEL_REFUSED = ((2, 1), (257, 1), (3, 0), (128, 896))
RAGGED_R = 257                              # x 4 level-0 samples of (3, 1) = 1028 points: a ragged evaluator tile
NEAR_FAR = {"vanilla": (0.2, 3.0), "pix": (0.2, 2.5), "mip": (0.2, 3.0)}
NEAR_FAR_MID = ((2.0, 6.0), (0.05, 1.0))
PIX_CHUNKS = (2, 5, 16)                     # does not divide 5 rays; all of them; more than there are

# (n_prop, n_nerf); the driver accepts 2 <= n_prop, 3 n_prop + 1 <= 256, 2 <= n_nerf <= 256
MIP_COUNTS = ((2, 2),                       # smallest
              (21, 63),                     # 3 n_prop + 1 = 64 dilated points: exactly one 64-lane round
              (21, 64), (22, 65),           # one past it
              (64, 32), (64, 128),          # the default and the larger fixture
              (85, 2), (2, 256), (85, 256)) # the largest of each, and of both
MIP_MID = (21, 63)
MIP_DEFAULT = (64, 32)
MIP_LARGEST = (85, 256)
MIP_REFUSED = ((1, 2), (86, 2), (2, 1), (2, 257))
MIP_TRAIN_FRACS = (0.3, 0.0)                # besides 1.0

STATES = ("gain1", "sharp", "empty")
PRECISIONS = ("f16x3", "f32")
RAY_LENGTHS = (1.3, 0.7, 1.0, 1.1, 0.9)     # |rays_d| of ray i is RAY_LENGTHS[i % 5]; viewdirs stay unit


def case_id(c):
    s = "%s_%d+%d_R%d_nf%g-%g_%s" % (c.kind, c.counts[0], c.counts[1], c.R, c.near, c.far, c.state)
    if c.white:
        s += "_white"
    if c.kind == "mip" and c.tf != 1.0:
        s += "_tf%g" % c.tf
    if c.chunk is not None:
        s += "_chunk%d" % c.chunk
    return s


def variant_id(c, v):
    if c.kind == "vanilla":
        return v
    if c.kind == "pix":
        return "preproject%d" % int(v)
    return "%s_layered%s" % (v[0], {None: "Auto", False: "0", True: "1"}[v[1]])


def _level_table(kind):
    """Vanilla and PixelNeRF share one table; the variants are the vanilla arithmetics / PixelNeRF's two operation orders."""
    near, far = NEAR_FAR[kind]
    variants = PRECISIONS if kind == "vanilla" else (True, False)
    mk = lambda counts, R=5, nf=(near, far), white=False, state="gain1", chunk=None: Case(kind, counts, R, nf[0], nf[1], white, state, 1.0,
                                                                                           chunk, variants)
    out = [mk(c) for c in LEVEL_COUNTS]
    out += [mk(LEVEL_MID, R=r) for r in RAY_COUNTS if r != 5]
    out += [mk((3, 1), R=1), mk((3, 1), R=RAGGED_R)]
    out += [mk(LEVEL_MID, nf=nf) for nf in NEAR_FAR_MID]
    out += [mk(c, white=True) for c in (LEVEL_MID, (3, 1))]
    out += [mk(c, state=s) for c in (LEVEL_MID, (3, 1), LEVEL_LARGEST) for s in STATES[1:]]
    out += [mk((3, 1), white=True, state="empty")]           # an empty ray on white: rgb = 1 exactly at both levels
    if kind == "pix":
        out += [mk(LEVEL_MID, chunk=ch) for ch in PIX_CHUNKS]
    return out


def _mip_table():
    near, far = NEAR_FAR["mip"]
    base = (("f16x3", None),)
    mk = lambda counts, R=5, tf=1.0, state="gain1", variants=base: Case("mip", counts, R, near, far, False, state, tf, None, variants)
    every = tuple((p, l) for p in PRECISIONS for l in (None, False, True))
    schedules = tuple(("f16x3", l) for l in (None, False, True))
    out = []
    for c in MIP_COUNTS:
        out.append(mk(c, R=3 if c == MIP_LARGEST else 5, variants=every if c == MIP_DEFAULT else schedules if c == MIP_LARGEST else base))
    out += [mk(MIP_MID, R=r) for r in RAY_COUNTS if r != 5]
    out += [mk(c, tf=tf) for c in (MIP_MID, MIP_DEFAULT) for tf in MIP_TRAIN_FRACS]
    out += [mk(c, state=s) for c in (MIP_MID, MIP_DEFAULT) for s in STATES[1:]]
    return out


@functools.lru_cache(maxsize=None)
def table(kind):
    out = _mip_table() if kind == "mip" else _level_table(kind)
    assert len({case_id(c) for c in out}) == len(out)
    return tuple(out)


def find(kind, counts, R=5, state="gain1", **kw):
    """The one case of the table with these fields (near / far / white / tf / chunk default to the plain case's)."""
    near, far = NEAR_FAR[kind]
    want = dict(near=near, far=far, white=False, tf=1.0, chunk=None)
    want.update(kw)
    hits = [c for c in table(kind) if c.counts == counts and c.R == R and c.state == state and all(getattr(c, k) == v for k, v in want.items())]
    assert len(hits) == 1, (kind, counts, R, state, kw, len(hits))
    return hits[0]


# ---- inputs --------------------------------------------------------------------------------------------------------------------
PER_RAY = ("rays_o", "rays_d", "viewdirs", "radii")


@functools.lru_cache(maxsize=None)
def rays_of(kind, R):
    """The generators' rays (unit rays_d == viewdirs) with rays_d rescaled per ray: the points of vanilla go along viewdirs and its
    intervals scale by |rays_d|, PixelNeRF's points go along rays_d and its direction rows come from viewdirs, Mip-NeRF 360 casts
    along rays_d and encodes viewdirs - a driver that swaps the two is then visible in every case."""
    rays = cases.mip_rays(R) if kind == "mip" else cases.strided_rays(R)
    scale = torch.tensor([RAY_LENGTHS[i % len(RAY_LENGTHS)] for i in range(R)], dtype=torch.float32)[:, None]
    rays["rays_d"] = (rays["viewdirs"] * scale).contiguous()
    return cases.neo_batch(rays) if kind == "pix" else rays


@functools.lru_cache(maxsize=None)
def state_of(kind, state):
    """gain1: the fixtures' state; sharp: density head x 8; empty: the density layer's bias at -100.  PixelNeRF's density is a relu:
    exactly 0.  Vanilla's is softplus(raw - 1), about 1.4e-44: every opacity 1 - exp(-sigma delta) over a finite interval is
    exactly 0, so every weight the resampler reads (weights[1:-1]) is, and k_resample takes its uniform fallback from the driver;
    only the last sample, whose interval is 1e10, keeps a weight of about 1e-34 where the subnormal density is not flushed."""
    gain = 8.0 if state == "sharp" else 1.0
    if kind == "vanilla":
        sd = synth.vanilla_state(0, density_gain=gain)
    elif kind == "pix":
        sd = synth.pixelnerf_state(0, density_gain=gain)
    else:
        sd = synth.mip360_state(0, density_gain=gain, weight_gain=0.5)
    if state == "empty":
        for k in sd:
            if k.endswith("density_layer.bias"):
                sd[k] = torch.full_like(sd[k], -100.0)
    return sd


@functools.lru_cache(maxsize=None)
def scene():
    return cases.small_scene()


def host_edges(n, near, far):
    """The level-0 row as neo_ctx::get_edges builds it on the host: the library's linspace(0, 1, n + 1), then three separate fp32
    operations per entry - near (1 - s) + far s."""
    s = np.asarray(_lib.linspace(0.0, 1.0, n + 1), dtype=np.float32)
    lo = np.float32(near) * (np.float32(1.0) - s)
    hi = np.float32(far) * s
    t = lo + hi
    assert t.dtype == np.float32
    return torch.from_numpy(t)


def seeded_edges(n, near, far):
    """The row of the seeded build (experiments/frame_chain_sweep_seeded.patch): near + (far - near) s."""
    s = np.asarray(_lib.linspace(0.0, 1.0, n + 1), dtype=np.float32)
    return torch.from_numpy(np.float32(near) + (np.float32(far) - np.float32(near)) * s)


def mip_schedule(case):
    """(dilation per level, anneal) as Python doubles, the way the reference's forward forms them (model.py:267-290)."""
    n_prop, n_nerf = case.counts
    dil, prod = [], 1
    for lvl in range(3):
        dil.append(0.0025 + 0.5 * (1.0 - 0.0) / prod)
        prod *= n_prop if lvl < 2 else n_nerf
    return dil, (10 * case.tf) / (9 * case.tf + 1)


# ---- oracles -------------------------------------------------------------------------------------------------------------------
LEVEL_OUTPUTS = ("rgb0", "acc0", "depth0", "rgb1", "acc1", "depth1")
MIP_OUTPUTS = tuple("%s%d" % (k, l) for l in range(3) for k in ("rgb", "w", "dens")) + ("prgb2",)


def _cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


def run_oracle(case, dtype, rows=None, rays=None):
    """Outputs of the pinned oracle in `dtype` (parameters, rays and scene cast to it) under the names of LEVEL_OUTPUTS /
    MIP_OUTPUTS, plus the sample rows it evaluated: t0, t1 and the level-0 weights w0, or sdist0 .. sdist2.  rows: evaluate at GIVEN
    rows - (t0, t1) / (sdist0, sdist1, sdist2) - instead of the oracle's own; they are cast to `dtype` (an fp32 row is exact in
    fp64).  rays: other rays than the case's own (a planted fault of the CPU test)."""
    params = _cast(state_of(case.kind, case.state), dtype)
    rays = _cast(rays_of(case.kind, case.R) if rays is None else rays, dtype)
    rows = None if rows is None else tuple(r.detach().cpu().to(dtype) for r in rows)
    if case.kind == "mip":
        rend, hist = mip360.render(params, rays, case.tf, case.near, case.far, case.counts[0], case.counts[1],
                                   basis=mip360.icosahedron_basis().to(dtype), sdist_given=rows)
        out = {}
        for l in range(3):
            out.update({"rgb%d" % l: rend[l]["rgb"], "w%d" % l: hist[l]["weights"], "dens%d" % l: hist[l]["density"],
                        "sdist%d" % l: hist[l]["sdist"]})
        out["prgb2"] = hist[2]["rgb"]
        return out
    kw = dict(n_coarse=case.counts[0], n_fine=case.counts[1], white_bkgd=case.white, keep=True)
    if case.kind == "vanilla":
        parts = [oracle.vanilla.render(params, rays, case.near, case.far, samples=rows, **kw)]
    else:
        # the caller's chunk loop: the direction rows of a point depend on which rays share its chunk (model_pixel.py:219-222)
        sc = _cast(scene(), dtype)
        chunk = case.chunk or case.R
        parts = []
        for i in range(0, case.R, chunk):
            part = {k: (v[i:i + chunk] if k in PER_RAY else v) for k, v in rays.items()}
            parts.append(oracle.pixelnerf.render(params, part, sc, case.near, case.far,
                                                 samples=None if rows is None else tuple(r[i:i + chunk] for r in rows), **kw))
    out = {}
    for lv in (0, 1):
        for j, k in enumerate(("rgb", "acc", "depth")):
            out["%s%d" % (k, lv)] = torch.cat([p[0][lv][j] for p in parts])
        out["t%d" % lv] = torch.cat([p[1][lv]["t"] for p in parts])
    out["w0"] = torch.cat([p[1][0]["weights"] for p in parts])
    return out


def rows_of(case, out):
    return (out["t0"], out["t1"]) if case.kind != "mip" else tuple(out["sdist%d" % l] for l in range(3))


def bound_of(name, ref64):
    """Per entry: the parity contract relative to max(1, |fp64 value|)."""
    tol = TOL_HIST if name[0] == "w" or name.startswith("dens") else TOL
    return tol * ref64.double().abs().clamp(min=1.0)


def frame_checks(case, got, ref64, ref32):
    """{output: worst_entry} of one frame against the fp64 oracle; ref32: an fp32 evaluation at the same rows (recorded beside it)."""
    names = MIP_OUTPUTS if case.kind == "mip" else LEVEL_OUTPUTS
    return {k: worst_entry(got[k], ref64[k], bound_of(k, ref64[k]), ref32[k]) for k in names}


@functools.lru_cache(maxsize=None)
def oracle_condition(case):
    """The CPU condition of a case: (fp32 oracle at its own rows, fp64 oracle at those rows, checks of the first against the second)."""
    o32 = run_oracle(case, torch.float32)
    o64 = run_oracle(case, torch.float64, rows_of(case, o32))
    return o32, o64, frame_checks(case, o32, o64, o32)
