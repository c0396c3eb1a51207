"""Case table and per-entry bounds for the kernels that MAKE the evaluators' inputs: ray generation, the three slab tests, the
sphere exit, the level-0 samplers, neo_tp_train_points, neo_mip_encode, the activation op with its backward, and the grid-stride
loops of k_pos_enc / k_uniform / k_tp_level0 / k_tp_level0_rand.  Plain CPU torch and numpy: tests/test_frontend_cases_cpu.py
checks the conditions of every case (finite fp64 truth, the fp32 oracle inside the bounds) on the very inputs that
tests/test_gpu_frontend_sweep.py hands to the wrappers in `ops` and `training`.  Companion of tests/alongray_cases.py, whose
worst_entry / summarize / assert_inside do the comparing.

Bounds.  Every constant is one an earlier single-shape test used (named where it is defined); what it is relative to is decided
here, entry by entry.  Where two correct fp32 evaluations of the same formula differ by more than a constant can hold (a
difference of nearly equal directions, sin(2^k x) of an fp32 x, a rotation about a nearly undefined axis) the bound is conftest's
standing rule: tol + 3 x that entry's own |fp32 oracle - fp64 truth| (mip_encode keeps the 2 x of the test it comes from).
No bound comes from a kernel's output."""
import functools
import math
from fractions import Fraction

import numpy as np
import torch

import cases
import oracle
from alongray_cases import assert_inside, summarize, worst_entry      # noqa: F401  (re-exported for the two test files)
from neo360_amd import synth
from oracle import mip360
from oracle import training as T

# ---- the constants of the earlier single-shape tests -------------------------------------------------------------------------------
RAY_DIR = 2e-7        # unit directions (test_gpu_stages.py::test_raygen_vs_golden)
RAY_RADII = 1e-7      # radii, + 3 x noise per entry: differences of nearly equal fp32 directions (the same test)
SPHERE_FAR = 1e-6     # sphere exit depth (test_sphere_mask_and_depth), x max(1, |far|), + 3 x noise per entry
L0_FG, L0_BG = 5e-7, 2e-7                   # level-0 rows: inside x max(1, far); outside
LOOK = (1e-6, 2e-6)                         # train_points lookup points and identity features, per region (test_train_points_match_the_oracle)
OCTAVE9 = (1e-4, 2e-4)                      # its bound on the encodings, which its own comment assigns to octave 9
PE = 5e-7                                   # test_gpu_stages.py::test_pos_enc
MIP_ENC, MIP_LOW = 2e-6, 2e-5               # test_encode_rows_match_the_oracle: per (row, octave) + 2 x noise; the first 63 features
ACT = 2e-6                                  # test_activate_op_matches_autograd, x max(1, |fp64 value|)
NEAR32 = float(np.float32(1e-4))            # the near plane the level-0 kernels are handed (api_train.hip)


def _d(x):
    return x.detach()


def _with_ratio(checks):
    """The same checks with the fp32 oracle standing in for the kernel (what the CPU test asserts)."""
    return {k: dict(v, ratio=v["fp32_ratio"]) for k, v in checks.items()}


def oracle_inside(checks, label):
    assert_inside(_with_ratio(checks), label)


# ---- 1. ray generation -----------------------------------------------------------------------------------------------------------------
RAYGEN_FRAMES = ((3, 1), (3, 5), (4, 64), (5, 51), (17, 15), (3, 257))          # 3, 15, 256, 255, 255, 771 rays; H = 3 is the radii rule's minimum
RAYGEN_FOCALS = (0.8, 40.0)                                                        # x W; 40 W is the long lens
RAYGEN_RANGE_FRAME = (5, 51)
RAYGEN_RANGES = ((0, 1), (254, 255), (0, 255), (100, 101), (204, 255))             # the last one is the last row alone


def raygen_poses():
    """Five c2w (4,4) fp32: three poses on the test orbit (those of test_raygen_vs_golden), the identity rotation, a translation of 1e3."""
    poses = [synth.look_at_origin(az, 0.6 + 0.1 * i, 0.3 - 0.2 * i) for i, az in enumerate((10.0, 130.0, 250.0))]
    ident = torch.eye(4)
    ident[:3, 3] = torch.tensor([0.25, -0.5, 0.125])
    far = synth.look_at_origin(70.0).clone()
    far[:3, 3] = torch.tensor([1e3, -2e3, 5e2])
    return poses + [ident, far]


def raygen_table():
    return [(H, W, fx, pi) for (H, W) in RAYGEN_FRAMES for fx in RAYGEN_FOCALS for pi in range(5)]


def raygen_focal(W, fx):
    """The focal as the kernel receives it: a C float."""
    return float(np.float32(fx * W))


def _raygen64(H, W, focal, pose):
    """oracle.rays.pixel_directions + camera_rays in float64 on the fp32-rounded focal and pose."""
    P = pose.double()
    col = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    row = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    dirs = torch.stack([(col - W / 2) / focal, -(row - H / 2) / focal, -torch.ones(H, W, dtype=torch.float64)], dim=-1)
    world = dirs @ P[:3, :3].T
    origin = P[:3, 3].expand(H, W, 3)
    step = torch.sqrt(((world[:-1] - world[1:]) ** 2).sum(-1))
    step = torch.cat([step, step[-2:-1]], dim=0)
    radii = (step * 2 / math.sqrt(12.0)).reshape(-1)
    unit = world / torch.norm(world, dim=-1, keepdim=True)
    return dict(rays_o=origin.reshape(-1, 3).clone(), viewdirs=unit.reshape(-1, 3), rays_d=unit.reshape(-1, 3).clone(), radii=radii)


@functools.lru_cache(maxsize=None)
def raygen_case(H, W, fx, pi):
    """(focal, pose, fp64 truth, fp32 oracle) of one frame."""
    focal, pose = raygen_focal(W, fx), raygen_poses()[pi]
    o, v, d, r = oracle.rays.camera_rays(oracle.rays.pixel_directions(H, W, focal), pose[:3, :4])
    return focal, pose, _raygen64(H, W, focal, pose), dict(rays_o=o.clone(), viewdirs=v, rays_d=d, radii=r)


def raygen_checks(got, ref64, ref32):
    """got: dict(rays_o, viewdirs, rays_d, radii).  Origins are exact (asserted here), the rest per entry."""
    assert torch.equal(torch.as_tensor(got["rays_o"]).cpu().double(), ref64["rays_o"]), "origins differ from the pose's translation"
    noise = (ref32["radii"].double() - ref64["radii"]).abs()
    return dict(viewdirs=worst_entry(got["viewdirs"], ref64["viewdirs"], RAY_DIR, ref32["viewdirs"]),
                rays_d=worst_entry(got["rays_d"], ref64["rays_d"], RAY_DIR, ref32["rays_d"]),
                radii=worst_entry(got["radii"], ref64["radii"], RAY_RADII + 3.0 * noise, ref32["radii"]))


# ---- 2. slab tests ---------------------------------------------------------------------------------------------------------------------
SLAB_RAYS = 513
SLAB_COUNTS = (1, 2, 255, 256, 257, 513)
SLAB_DESIGNED = 13
# box sets by size: "A" holds the designed rays, "miss" is met by no ray, "Y" encloses "X" (the nearer box is listed second)
SLAB_SETS = {1: ("A",), 2: ("X", "Y"), 3: ("A", "miss", "ob2"), 7: ("X", "A", "miss", "ob1", "ob2", "ob3", "Y")}
_A_T = np.array([-0.5, 0.25, 0.125])


@functools.lru_cache(maxsize=None)
def slab_pool():
    """name -> (R (3,3), T (3,), s (2,3)) in the reference's RTs format: the four boxes of cases.oriented_box_cases() (ob0 = "X",
    three of them rotated), "Y" = X's frame with bounds 1.5 x as large, "A" axis-aligned and symmetric (+-0.25) at a translation
    that is exact in binary, "miss" far from every ray."""
    RTs, _, _ = cases.oriented_box_cases()
    pool = {"X": (RTs["R"][0], RTs["T"][0], RTs["s"][0]), "Y": (RTs["R"][0], RTs["T"][0], RTs["s"][0] * 1.5)}
    for i in (1, 2, 3):
        pool["ob%d" % i] = (RTs["R"][i], RTs["T"][i], RTs["s"][i])
    pool["A"] = (np.eye(3), _A_T.copy(), np.array([[-0.25, -0.25, -0.25], [0.25, 0.25, 0.25]]))
    pool["miss"] = (RTs["R"][2], np.array([40.0, 55.0, -70.0]), np.array([[-0.1, -0.1, -0.1], [0.1, 0.1, 0.1]]))
    return pool


def slab_rts(names):
    pool = slab_pool()
    return dict(R=[pool[n][0] for n in names], T=[pool[n][1] for n in names], s=[pool[n][2] for n in names])


def box_from_world(rot, tran):
    """models/neo360/helper.py:352-356 as ops._box_tables and oracle.rays.sample_rays_in_bbox build it."""
    box = np.eye(4)
    box[:3, :3] = np.reshape(np.array(rot), (3, 3))
    box[:3, -1] = np.array(tran)
    return np.linalg.inv(box)


@functools.lru_cache(maxsize=None)
def slab_rays():
    """(o, d) float32 world-frame rays (513, 3).  Rows 0 .. 12 are designed in the frame of box "A" (axis-aligned, +-0.25; world =
    box frame + A's translation, exact in fp32):
      0, 1   direction x exactly +0.0 / -0.0 (the 1e-14 rule), a hit;   2, 3   the same on y;   4, 5   on z;
      6      origin inside the box (rejected: tmin < 0);
      7      origin exactly on the face x = -0.25: tmin == 0, accepted by the slab test, near rounds to 0.0f = "no hit" in the merge;
      8      the box behind the ray (rejected);
      9      grazes the edge x = y = -0.25: after the x slab lo = 0.75, the y slab's a_hi = 0.75 == lo - not an early-out, tmin == tmax;
      10     parallel to the x slab (direction x = 0.0) and outside it: a miss by the y early-out;
      11     through two opposite corners of the symmetric box (all three slabs give the same interval);
      12     origin 1e6 away.
    The rest are ordinary rays of cases.oriented_box_cases(seed=14) (aimed at the boxes' neighbourhood, a few with zero components
    and origins inside boxes of their own).  No NaN, no inf."""
    _, o, d = cases.oriented_box_cases(seed=14, n=SLAB_RAYS)
    o, d = o.copy(), d.copy()
    rows = [((0.1, -0.75, -1.0), (0.0, 0.6, 0.8)), ((0.1, -0.75, -1.0), (-0.0, 0.6, 0.8)),
            ((-1.0, 0.1, -0.75), (0.8, 0.0, 0.6)), ((-1.0, 0.1, -0.75), (0.8, -0.0, 0.6)),
            ((-0.75, -1.0, 0.1), (0.6, 0.8, 0.0)), ((-0.75, -1.0, 0.1), (0.6, 0.8, -0.0)),
            ((0.0, 0.05, -0.1), (0.6, 0.0, 0.8)),
            ((-0.25, 0.0, 0.0), (0.8, 0.36, 0.48)),
            ((1.0, 0.0, 0.0), (1.0, 0.1, 0.05)),
            ((-1.0, 0.5, 0.0), (1.0, -1.0, 0.0625)),
            ((0.5, -1.0, -1.0), (0.0, 0.6, 0.8)),
            ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),
            ((1e6, 0.125, 0.0625), (-1.0, 1e-8, -2e-8))]
    assert len(rows) == SLAB_DESIGNED
    for i, (ob, db) in enumerate(rows):
        o[i] = (np.array(ob, dtype=np.float64) + _A_T).astype(np.float32)
        d[i] = np.array(db, dtype=np.float32)
    assert np.isfinite(o).all() and np.isfinite(d).all()
    return o, d


def _fma(a, b, c):
    """fma(a, b, c) with ONE rounding: exact rational arithmetic, then Python's correctly rounded Fraction -> float."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def box_frame_exact(rays_o, rays_d, M):
    """o' = R o + t, d' = R d in the kernels' order (rays.hip): fma(R2, x2, fma(R1, x1, R0 * x0)), the translation a separate add.
    rays (n,3) any float dtype (promoted to float64 like the reference's NumPy arrays), M (4,4) float64."""
    o64, d64 = np.asarray(rays_o, dtype=np.float64), np.asarray(rays_d, dtype=np.float64)
    ob, db = np.empty_like(o64), np.empty_like(d64)
    for r in range(o64.shape[0]):
        o, d = [float(v) for v in o64[r]], [float(v) for v in d64[r]]
        for a in range(3):
            m = [float(v) for v in M[a]]
            ob[r, a] = _fma(m[2], o[2], _fma(m[1], o[1], m[0] * o[0])) + m[3]
            db[r, a] = _fma(m[2], d[2], _fma(m[1], d[1], m[0] * d[0]))
    return ob, db


def slab_box_exact(rays_o, rays_d, rot, tran, bounds):
    """One box: the exact-FMA transform, oracle.rays.aabb_slab per ray, then the reference's float32 rounding (torch.Tensor(float64)).
    Returns dict(o, d: box-frame rays float64; hit, tmin, tmax: float64 arrays; hit_mask bool, near, far (n,1) float32)."""
    ob, db = box_frame_exact(rays_o, rays_d, box_from_world(rot, tran))
    hit, tmin, tmax = oracle.rays.aabb_slab_batch(np.array(bounds), ob, db)
    return dict(o=ob, d=db, hit=hit, tmin=tmin, tmax=tmax, hit_mask=torch.Tensor(hit).bool(), near=torch.Tensor(tmin[:, None]),
                far=torch.Tensor(tmax[:, None]))


@functools.lru_cache(maxsize=None)
def slab_box_truth(name):
    """The truth of one pool box on all 513 rays (the kernels are row-independent: a call of R rays is rows [0, R) of this)."""
    o, d = slab_rays()
    return slab_box_exact(o, d, *slab_pool()[name])


def slab_truth(n_boxes, R):
    """dict(per_box: list of per-box truths cut to R rays, near, far (R,1) float32, mask (R,1) bool) of box set n_boxes on rays [0, R)."""
    per = [{k: v[:R] for k, v in slab_box_truth(name).items()} for name in SLAB_SETS[n_boxes]]
    near, far, mask = oracle.rays.merge_boxes([p["near"] for p in per], [p["far"] for p in per])
    return dict(per_box=per, near=near, far=far, mask=mask)


def numpy_product_agrees(R):
    """Whether oracle.rays.rays_to_box_frame (numpy's `@`) equals the exact-FMA restatement bit for bit on a call of rays [0, R),
    for every box of the pool: {box name: bool}."""
    o, d = slab_rays()
    out = {}
    for name, (rot, tran, _) in slab_pool().items():
        no, nd = oracle.rays.rays_to_box_frame(o[:R], d[:R], box_from_world(rot, tran))
        tr = slab_box_truth(name)
        out[name] = bool(np.array_equal(no, tr["o"][:R]) and np.array_equal(nd, tr["d"][:R]))
    return out


# ---- 3. sphere exit --------------------------------------------------------------------------------------------------------------------
SPHERE_COUNTS = (1, 255, 256, 257)
SPHERE_SCALES = (1.0, 1.3, 1e-3, 1e3)
SPHERE_MISS_ROWS = (3, 4)


def sphere_inputs(R, scale, misses=True):
    """rays_o, rays_d (R,3) fp32, |d| = scale.  Rows (as many as R holds): 0 origin at the centre; 1 origin on the sphere pointing
    inward; 2 near-tangent, margin 1 - |closest|^2 = +1e-3 (a hit); 3 near-tangent, margin -1e-3 (a miss); 4 a clear miss; the rest
    ordinary rays from inside the sphere.  misses=False keeps rows 3 and 4 ordinary (the clean call)."""
    rays = cases.strided_rays(max(R, 8))
    o, d = rays["rays_o"][:R].clone(), rays["rays_d"][:R].clone()
    rows = {0: ((0.0, 0.0, 0.0), (0.6, 0.0, 0.8)), 1: ((0.0, 0.0, 1.0), (0.1, 0.2, -1.0)),
            2: ((0.0, math.sqrt(1.0 - 1e-3), -0.5), (0.0, 0.0, 1.0))}
    if misses:
        rows.update({3: ((0.0, math.sqrt(1.0 + 1e-3), -0.5), (0.0, 0.0, 1.0)), 4: ((0.0, 0.0, 3.0), (1.0, 0.0, 0.0))})
    for i, (oo, dd) in rows.items():
        if i < R:
            o[i] = torch.tensor(oo)
            d[i] = torch.nn.functional.normalize(torch.tensor(dd), dim=0)
    return o, (d * scale).contiguous()


def sphere_formula(o, d):
    """The lines of oracle.rays.sphere_exit_depth without its assertion (a call with a miss must return its NaN): far (R,1), ok (R,1)."""
    d1 = -(d * o).sum(-1, keepdim=True) / (d ** 2).sum(-1, keepdim=True)
    closest = o + d1 * d
    inv_len = 1.0 / torch.norm(d, dim=-1, keepdim=True)
    margin = 1.0 - (closest * closest).sum(-1, keepdim=True)
    return d1 + torch.sqrt(margin) * inv_len, margin >= 0


@functools.lru_cache(maxsize=None)
def sphere_case(R, scale, misses=True):
    o, d = sphere_inputs(R, scale, misses)
    return (o, d), sphere_formula(o.double(), d.double()), sphere_formula(o, d)


def sphere_checks(far, ok, ref64, ref32):
    """Mask exact against fp64; NaN exactly where the truth is NaN; far per entry on the hits."""
    far, ok = torch.as_tensor(far).cpu().reshape(-1), torch.as_tensor(ok).cpu().reshape(-1).bool()
    f64, ok64 = ref64[0].reshape(-1), ref64[1].reshape(-1)
    assert torch.equal(ok, ok64), "hit mask differs from the fp64 one"
    assert torch.equal(torch.isnan(far), torch.isnan(f64)), "NaN pattern differs"
    hit = ok64
    f32 = ref32[0].reshape(-1)
    noise = (f32[hit].double() - f64[hit]).abs()
    return dict(far=worst_entry(far[hit], f64[hit], SPHERE_FAR * f64[hit].abs().clamp(min=1.0) + 3.0 * noise, f32[hit]))


# ---- 4. level-0 rows -------------------------------------------------------------------------------------------------------------------
L0_N = (3, 63, 64, 255, 1023)        # the entry's limits and the edges of a 64 / 256-wide round (rows hold n + 1 samples)
L0_R = (1, 5, 257)
L0_SEED, L0_STREAMS = 20240, (3, 4)
L0_BIG = (4100, 1023)                # 4100 x 1024 elements = 16400 blocks of 256: over the cap of 16384
U_TOP = 1.0 - 2.0 ** -24


def level0_far(R, n):
    """far (R,1) fp32 in [0.3, 1.7]; row 0 is 2.0 and row 1 is 1e-4 = near (a constant row); a single-ray case alternates."""
    far = synth.uniform(31, "fe_l0_far_%d_%d" % (R, n), (R, 1), 0.3, 1.7)
    if R == 1:
        far[0] = NEAR32 if n in (3, 64, 1023) else 2.0
    else:
        far[0], far[1] = 2.0, NEAR32
    return far


def _level0_det(far, n, dtype):
    if dtype == torch.float32:
        # the rows do not depend on the rays; the oracles also build the points, so they get one valid ray for every row
        o = torch.tensor([[0.0, 0.0, 0.5]]).expand(far.shape[0], 3)
        d = torch.tensor([[0.6, 0.0, 0.8]]).expand(far.shape[0], 3)
        fg, _ = oracle.sampling.neo_fg_level0(o, d, n, torch.full_like(far, 1e-4), far)
        bg, _, _ = oracle.sampling.neo_bg_level0(o, d, n, far)
        return fg, bg.contiguous()
    e = torch.linspace(0.0, 1.0, n + 1, dtype=torch.float64)
    f = far.double()
    return NEAR32 * (1.0 - e) + f * e, torch.broadcast_to(torch.flip(e, dims=[-1]), (far.shape[0], n + 1)).contiguous()


def level0_draws(R, n):
    """u_fg, u_bg (R, n+1): the device generator's draws (philox_uniform is bit-exact to it); with five rays or more, row 2 is
    u = 0 and row 3 is u = 1 - 2^-24, the two ends of what the generator can return."""
    u_fg, u_bg = (T.philox_uniform(L0_SEED + n, s, R, n + 1) for s in L0_STREAMS)
    return level0_designed_draws(u_fg), level0_designed_draws(u_bg)


def level0_designed_draws(u):
    u = u.clone()
    if u.shape[0] >= 5:
        u[2], u[3] = 0.0, U_TOP
    return u


def _level0_rand(far, n, u_fg, u_bg, dtype):
    if dtype == torch.float32:
        return T.neo_level0_randomized(far, n, u_fg, u_bg)
    e = torch.linspace(0.0, 1.0, n + 1, dtype=torch.float64)
    f = far.double()
    fg = T._stratify(NEAR32 * (1.0 - e) + f * e, u_fg.double())
    bg = T._stratify(torch.broadcast_to(e, (far.shape[0], n + 1)), u_bg.double())
    return fg, torch.flip(bg, dims=[-1])


def level0_case(R, n, randomized):
    """(far, (u_fg, u_bg) or None, fp64 truth (fg, bg), fp32 oracle (fg, bg)); computed once per session, but for the grid-stride
    case (130 MB of rows), which is rebuilt by each of its two users."""
    return (_level0_case if R * n < 1 << 20 else _level0_case.__wrapped__)(R, n, randomized)


@functools.lru_cache(maxsize=None)
def _level0_case(R, n, randomized):
    far = level0_far(R, n)
    if not randomized:
        return far, None, _level0_det(far, n, torch.float64), _level0_det(far, n, torch.float32)
    u = level0_draws(R, n)
    return far, u, _level0_rand(far, n, u[0], u[1], torch.float64), _level0_rand(far, n, u[0], u[1], torch.float32)


def level0_order(fg, bg, far):
    """What the issue asks of the randomized rows, whatever the arithmetic: inside rows ascend in [near, far], outside rows descend
    in [0, 1], the ends exact.  Only a row with far == near is treated apart: it is constant up to the rounding of
    near (1 - e) + far e, in the fp32 oracle too (it leaves the range by 1.2 ulp of near), so it is held to near (1 +- 2^-22) and
    left out of the ascent.  Returns the four booleans."""
    fg, bg, far = torch.as_tensor(fg).cpu().double(), torch.as_tensor(bg).cpu().double(), far.double().reshape(-1, 1)
    rises = (far > NEAR32).reshape(-1)
    up, flat = fg[rises], fg[~rises]
    return dict(fg_ascends=bool((up[:, 1:] >= up[:, :-1]).all()), bg_descends=bool((bg[:, 1:] <= bg[:, :-1]).all()),
                fg_in_range=bool(((up >= NEAR32) & (up <= far[rises])).all())
                and bool(((flat >= NEAR32 * (1 - 2 ** -22)) & (flat <= NEAR32 * (1 + 2 ** -22))).all()),
                bg_in_range=bool(((bg >= 0.0) & (bg <= 1.0)).all()))


def level0_checks(fg, bg, far, ref64, ref32):
    return dict(fg=worst_entry(fg, ref64[0], L0_FG * far.double().clamp(min=1.0), ref32[0]), bg=worst_entry(bg, ref64[1], L0_BG, ref32[1]))


# ---- 5. train_points -------------------------------------------------------------------------------------------------------------------
POINT_SHAPES = ((1, 1), (1, 64), (3, 33), (5, 13), (48, 33))          # P = 1, 64, 99, 65, 1584: one partial 64-point block .. 24 full + 1
POINT_NV = (1, cases.NV)
NEAR_RADIAL_ROW = 2
FULL_SPAN_ROW = 1
RADIAL_N = 13


def point_inputs(region, R, N):
    """rays_o, rays_d (R,3), t (R,N), far (R,1) fp32.  Inside (region 0): level-0 rows near .. far; with three rays or more row 1
    starts at t = 0 and ends at t = far exactly.  Outside (region 1): the inverse radius from 1 to 0, both ends exact; with three
    rays or more row 2 is the near-radial ray o = (0, 0, 0.5), d = normalise(1e-4, 0, 1)."""
    rays = cases.strided_rays(max(R, 8))
    o, d = rays["rays_o"][:R].clone(), rays["rays_d"][:R].clone()
    if region == 1 and R > NEAR_RADIAL_ROW:
        o[NEAR_RADIAL_ROW] = torch.tensor([0.0, 0.0, 0.5])
        d[NEAR_RADIAL_ROW] = torch.nn.functional.normalize(torch.tensor([1e-4, 0.0, 1.0]), dim=0)
    far, ok = sphere_formula(o, d)
    assert bool(ok.all())
    e = torch.linspace(0.0, 1.0, N)
    if region == 0:
        t = (NEAR32 * (1.0 - e) + far * e).contiguous()
        if R > FULL_SPAN_ROW:
            t[FULL_SPAN_ROW] = far[FULL_SPAN_ROW] * e
            t[FULL_SPAN_ROW, 0], t[FULL_SPAN_ROW, -1] = 0.0, far[FULL_SPAN_ROW, 0]
    else:
        t = torch.broadcast_to(torch.flip(e, dims=[-1]), (R, N)).contiguous()
    return o, d, t, far


def radial_inputs():
    """One exactly radial ray in a call of its own (region 1): the reference's rotation axis is 0 / 0 there."""
    o, d = torch.tensor([[0.0, 0.0, 0.5]]), torch.tensor([[0.0, 0.0, 1.0]])
    far, _ = sphere_formula(o, d)
    return o, d, torch.flip(torch.linspace(0.0, 1.0, RADIAL_N), dims=[-1])[None, :].contiguous(), far


def points_oracle(region, o, d, t, far, poses, dtype):
    """look (R N, 3) and x_enc (NV, R N, 63 | 84): the chain of test_train_points_match_the_oracle in `dtype`."""
    c = lambda x: x.to(dtype)
    if region == 0:
        look = oracle.sampling.points_on_rays(c(t), c(o), c(d)).reshape(-1, 3)
        cam = oracle.gather.world_to_camera(look, c(poses))
    else:
        s = c(t)
        look = (c(o)[:, None, :] + (c(far).reshape(-1, 1) * (1.0 - s) + 3.0 * s)[..., None] * c(d)[:, None, :]).reshape(-1, 3)
        p4 = oracle.sampling.inverted_sphere_points(c(o), c(d), s)
        cam = torch.cat((oracle.gather.world_to_camera(p4[..., :3].reshape(-1, 3), c(poses)),
                         p4[..., 3].reshape(1, -1, 1).expand(poses.shape[0], -1, -1)), dim=-1)
    return look, oracle.encoding.pos_enc(cam, 0, 10)


def octave_of_feature(ch):
    """(21 ch,) long: -1 for the identity features, else the octave k of feature f (k-major, channel-minor, sines then shifted sines)."""
    f = torch.arange(21 * ch)
    return torch.where(f < ch, torch.full_like(f, -1), ((f - ch) % (10 * ch)) // ch)


def point_bounds(region, look64, x64, x32):
    """Per-entry bounds of look and x_enc, and the (P,) largest share of an octave's PLAIN bound (the constant without the noise
    term) that the row's fp32-vs-fp64 noise takes, over the views and octaves."""
    ch = 4 if region else 3
    look_b = LOOK[region] * look64.abs().clamp(min=1.0)
    octv = octave_of_feature(ch)
    noise = (x32.double() - x64).abs()
    xb = LOOK[region] * x64.abs().clamp(min=1.0)                      # identity features; the octaves are overwritten below
    share = torch.zeros(x64.shape[1], dtype=torch.float64)
    for k in range(10):
        sel = octv == k
        plain = OCTAVE9[region] * 2.0 ** (k - 9) + PE
        nk = noise[..., sel].amax(dim=-1, keepdim=True)               # (NV, P, 1): the row's noise at this octave
        xb[..., sel] = plain + 3.0 * nk
        share = torch.maximum(share, (nk[..., 0] / plain).amax(dim=0))
    return look_b, xb, share


@functools.lru_cache(maxsize=None)
def point_case(region, R, N, NV):
    """(inputs (o, d, t, far, poses), fp64 truth (look, x_enc), fp32 oracle (look, x_enc))."""
    o, d, t, far = point_inputs(region, R, N)
    poses, _, _ = synth.source_views(NV, cases.IMG_WH[0], cases.IMG_WH[1])
    return ((o, d, t, far, poses), points_oracle(region, o, d, t, far, poses, torch.float64),
            points_oracle(region, o, d, t, far, poses, torch.float32))


def point_checks(region, look, x_enc, ref64, ref32):
    look_b, xb, _ = point_bounds(region, ref64[0], ref64[1], ref32[1])
    return dict(look=worst_entry(look, ref64[0], look_b, ref32[0]), x_enc=worst_entry(x_enc, ref64[1], xb, ref32[1]))


def radial_nan_pattern(x_enc):
    """The NaN pattern of oracle.sampling.inverted_sphere_points on an exactly radial ray, seen through the 84 features: every
    feature of the three spatial coordinates is NaN, every feature of the fourth (the inverse radius) is finite."""
    x_enc = torch.as_tensor(x_enc).cpu()
    spatial = (torch.arange(84) % 4) < 3            # channel-minor in all three blocks (4 | 40 | 40)
    return bool(torch.isnan(x_enc[..., spatial]).all()) and bool(torch.isfinite(x_enc[..., ~spatial]).all())


def radial_checks(look, x_enc, ref64, ref32):
    """The finite part of the exactly radial ray's call: the lookup points and the 21 features of the inverse radius, each under
    its octave's constant + 3 x its own fp32-vs-fp64 noise (the shifted sine's fp32 phase add)."""
    octv = octave_of_feature(4)
    plain = torch.where(octv < 0, torch.tensor(LOOK[1], dtype=torch.float64), OCTAVE9[1] * 2.0 ** (octv.double() - 9) + PE)
    fin = (torch.arange(84) % 4) == 3
    r64, r32 = ref64[1][..., fin], ref32[1][..., fin]
    bound = plain[fin] + 3.0 * (r32.double() - r64).abs()
    return dict(look=worst_entry(look, ref64[0], LOOK[1] * ref64[0].abs().clamp(min=1.0), ref32[0]),
                inverse_radius=worst_entry(torch.as_tensor(x_enc).cpu()[..., fin], r64, bound, r32))


# ---- 6. mip_encode ---------------------------------------------------------------------------------------------------------------------
MIP_SHAPES = ((1, 1), (1, 7), (3, 3), (9, 5), (9, 8), (2, 33))        # P = 1, 7, 9, 45, 72, 66: 8-row blocks: partial; full + partial; 9 full
MIP_WIDE = {5: (0.0, 0.0, 1e-3, 1.0, 1e3, 1e6), 8: (0.0, 0.0, 1e-3, 1e-2, 0.1, 1.0, 1e2, 1e3, 1e6)}
ONE_IN, ONE_OUT = 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23


def _t_mean32(t0, t1):
    t = torch.tensor([[t0, t1]])
    m, _ = mip360.conical_frustum_gaussians(t, torch.zeros(1, 3), torch.tensor([[0.0, 0.0, 1.0]]), torch.ones(1, 1))
    return float(m[0, 0, 2])


def mip_inputs(R, n):
    """rays_o, rays_d (R,3), radii (R,1), tdist (R, n+1) fp32: cases.mip_rays, intervals in [0.2, 5.2].  Designed rays, as many as R holds:
      1 radius 0;   2 radius 1;   (with nine rays:)   3 |d| = 0.5;   4 |d| = 2;   5 a zero-width interval;
      6 the row [0, 0, 1e-3, 1, 1e3, 1e6] (n = 5; its nine-edge analogue at n = 8);
      7 / 8 a ray along z whose first interval's fp32 mean (the oracle's own arithmetic) sits at |x| = 1 - 2^-24 / 1 + 2^-23: one ulp
            inside / outside the contraction's branch (continuous there with its Jacobian: either branch is inside the bound);
    with two rays (the 33-interval case) ray 1 carries the zero-width interval instead."""
    rays = cases.mip_rays(max(R, 9))
    o, d, rad = rays["rays_o"][:R].clone(), rays["rays_d"][:R].clone(), rays["radii"][:R].clone()
    t = torch.sort(torch.rand(R, n + 1, generator=torch.Generator().manual_seed(500 + 37 * R + n)) * 5.0 + 0.2, dim=-1).values
    if R == 2:
        t[1, n // 2 + 1] = t[1, n // 2]
    if R >= 3:
        rad[1], rad[2] = 0.0, 1.0
    if R >= 9:
        d[3], d[4] = d[3] * 0.5, d[4] * 2.0
        t[5, n // 2 + 1] = t[5, n // 2]
        t[6] = torch.tensor(MIP_WIDE[n])
        for ray, target in ((7, ONE_IN), (8, ONE_OUT)):
            d[ray] = torch.tensor([0.0, 0.0, 1.0])
            t[ray] = torch.linspace(0.5, 0.5 + 0.2 * n, n + 1)
            tm = _t_mean32(float(t[ray, 0]), float(t[ray, 1]))
            o[ray] = torch.tensor([0.0, 0.0, float(np.float32(target) - np.float32(tm))])
    return o, d, rad, t.contiguous()


def mip_oracle(o, d, rad, t, dtype):
    """The chain of test_encode_rows_match_the_oracle in `dtype`: (R n, 504)."""
    c = lambda x: x.to(dtype)
    means, covs = mip360.conical_frustum_gaussians(c(t), c(o), c(d), c(rad))
    z, cc = mip360.contract(means, covs)
    lm, lv = mip360.lift_and_diagonalize(z, cc, c(mip360.icosahedron_basis()))
    return mip360.integrated_pos_enc(lm, lv, 0, 12).reshape(-1, 504)


def mip_bounds(ref64, ref32):
    """(P, 504): 2e-6 + 2 x the row's fp32-vs-fp64 noise at the feature's octave, and at most 2e-5 on the first 63 features."""
    noise = (ref32.double() - ref64).abs().reshape(-1, 2, 12, 21)
    per = noise.amax(dim=(1, 3))                                                   # (P, 12)
    b = (MIP_ENC + 2.0 * per)[:, None, :, None].expand(-1, 2, -1, 21).reshape(-1, 504).clone()
    b[:, :63] = b[:, :63].clamp(max=MIP_LOW)
    return b


@functools.lru_cache(maxsize=None)
def mip_case(R, n):
    inp = mip_inputs(R, n)
    return inp, mip_oracle(*inp, torch.float64), mip_oracle(*inp, torch.float32)


def mip_checks(got, ref64, ref32):
    """Every (row, octave) under mip_bounds."""
    return dict(enc=worst_entry(got, ref64, mip_bounds(ref64, ref32), ref32))


def mip_shares(got, ref64, ref32):
    """(P, 12): the largest |got - truth| of each (row, octave) over its own bound, and the same for the fp32 oracle's error in units
    of 2^k x half an ulp of 1 (what rounding a mean of magnitude 1 once costs at octave k), for the record."""
    err = (torch.as_tensor(got).cpu().double() - ref64).abs().reshape(-1, 2, 12, 21).amax(dim=(1, 3))
    noise = (ref32.double() - ref64).abs().reshape(-1, 2, 12, 21).amax(dim=(1, 3))
    unit = 2.0 ** torch.arange(12, dtype=torch.float64) * 2.0 ** -24
    return err / (MIP_ENC + 2.0 * noise), err / unit, noise / unit


# ---- 7. activate -----------------------------------------------------------------------------------------------------------------------
ACT_P = (1, 255, 256, 257, 4097)
ACT_NOISE = ("given", "none", "scale0")
ACT_SCALE, ACT_DESIGNED_NOISE = 0.5, 0.5
_UP, _DOWN = float(np.nextafter(np.float32(20.0), np.float32(30.0))), float(np.nextafter(np.float32(20.0), np.float32(10.0)))
ACT_COLOUR = (100.0, -100.0, 20.0, -20.0, 1e-3, -1e-3, 0.0)
ACT_DENSITY_ARG = (20.0, _UP, _DOWN, -100.0, 100.0, 0.0)       # raw + noise x scale - 1: the softplus threshold, its two neighbours, ...


def activate_inputs(P, noise_kind):
    """raw_rgb (P,3), raw_sigma (P,1), noise (P,) or None, scale, upstream gradient (P,4).  The designed colour values cycle through
    the first entries of raw_rgb; the designed density arguments are met exactly by the first rows (as many as P holds): with the
    noise given their noise is 0.5 and the scale 0.5, so raw = argument + 1 - 0.25, every step exact in fp32."""
    g = torch.Generator().manual_seed(900 + P)
    raw_rgb, raw_sigma = torch.randn(P, 3, generator=g) * 3.0, torch.randn(P, 1, generator=g) * 12.0
    noise, up = torch.rand(P, generator=g), torch.randn(P, 4, generator=g)
    flat = raw_rgb.reshape(-1)
    k = min(flat.numel(), len(ACT_COLOUR))
    flat[:k] = torch.tensor(ACT_COLOUR[:k])
    scale = ACT_SCALE if noise_kind == "given" else 0.0
    m = min(P, len(ACT_DENSITY_ARG))
    noise[:m] = ACT_DESIGNED_NOISE
    raw_sigma[:m, 0] = torch.tensor(ACT_DENSITY_ARG[:m], dtype=torch.float64).add(1.0 - ACT_DESIGNED_NOISE * scale).float()
    return raw_rgb, raw_sigma, (None if noise_kind == "none" else noise), scale, up


def activate_oracle(inp, dtype):
    """Forward (P,4) and the gradients of sum(out x up) for raw_rgb and raw_sigma under autograd in `dtype`."""
    raw_rgb, raw_sigma, noise, scale, up = inp
    with torch.enable_grad():
        a, b = raw_rgb.to(dtype).clone().requires_grad_(True), raw_sigma.to(dtype).clone().requires_grad_(True)
        arg = b + (noise.to(dtype) * scale)[:, None] - 1.0 if noise is not None else b - 1.0
        out = torch.cat([torch.sigmoid(a) * 1.002 - 0.001, torch.nn.functional.softplus(arg)], dim=-1)
        ga, gb = torch.autograd.grad((out * up.to(dtype)).sum(), [a, b])
    return dict(out=_d(out), g_rgb=ga, g_sigma=gb)


@functools.lru_cache(maxsize=None)
def activate_case(P, noise_kind):
    inp = activate_inputs(P, noise_kind)
    return inp, activate_oracle(inp, torch.float64), activate_oracle(inp, torch.float32)


def activate_checks(got, ref64, ref32):
    return {k: worst_entry(got[k], ref64[k], ACT * ref64[k].abs().clamp(min=1.0), ref32[k]) for k in ("out", "g_rgb", "g_sigma")}


# ---- 8. the grid-stride loops ----------------------------------------------------------------------------------------------------------
PE_BIG = (33289, 3)                  # x 63 features = 2,097,207 elements = 8193 blocks of 256: over k_pos_enc's cap of 8192
UNIFORM_BIG = (16385, 257)           # 4,210,945 elements = 16449 blocks: over k_uniform's cap of 16384
UNIFORM_SEED, UNIFORM_STREAM = 777, 9


def pos_enc_truth(x, min_deg, max_deg):
    """fp64 sine of the fp32 arguments the reference forms (2^k x is exact, the phase add rounds in fp32: test_gpu_edges.py): the
    sine of an fp32 argument is what 5e-7 can hold, the argument's own rounding at octave 9 is not."""
    return torch.cat([x.double()] + [torch.sin((x * 2.0 ** k).double()) for k in range(min_deg, max_deg)]
                     + [torch.sin((x * 2.0 ** k + 0.5 * np.pi).double()) for k in range(min_deg, max_deg)], dim=-1)


@functools.lru_cache(maxsize=None)
def pos_enc_big_case():
    x = synth.uniform(11, "fe_pe_big", PE_BIG, -1.7, 1.7)
    return x, pos_enc_truth(x, 0, 10), oracle.encoding.pos_enc(x, 0, 10)


def pos_enc_checks(got, ref64, ref32):
    got = torch.as_tensor(got).cpu()
    assert torch.equal(got[:, :3].double(), ref64[:, :3]), "identity features differ"
    return dict(enc=worst_entry(got, ref64, PE, ref32))
