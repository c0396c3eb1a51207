"""Case table of the compact-launch sweep (tests/test_compact_cases_cpu.py, tests/test_gpu_compact_sweep.py): hit patterns and hit
counts for the three entry points whose evaluators run on compact rows - neo_tp_render_objects, neo_tp_render_instances and
neo_tp_render_culled - in plain CPU torch and numpy.  docs/compact_sweep.md describes the table and what it found.

Scene: cases.small_scene() with object_cases.state() (density bias +6) seen by cases.strided_rays(n).  Sample counts 3 + 4
(N0 = 4, N1 = 8: 16 rows are exactly one 64-point evaluator tile at level 0 and two at level 1) and, on the tile-edge counts only,
3 + 1 (N1 = 5: level 1 ends inside a tile at 16 and 112 rows).

The caller owns the hit pattern: a hit ray gets near = 0.30 + 0.001 (ray % 7), far = 0.90 - 0.002 (ray % 5) (instance i: both
shifted by 0.01 i), a missed ray one of the six miss encodings of the hit rule, cycled over the misses of the row.  A hit ray's
interval therefore depends on its index only, never on the pattern: one all-hit call (and one oracle run) per ray count serves
every pattern of that count.
"""
import numpy as np
import torch

import cases
import object_cases as oc
from alongray_cases import assert_inside, summarize, worst_entry      # noqa: F401  (re-exported for the two test files)

N_COARSE, N_FINE, N_FINE_ODD = 3, 4, 1
N0, N1, N1_ODD = N_COARSE + 1, N_COARSE + 1 + N_FINE, N_COARSE + 1 + N_FINE_ODD
TM = 64               # points of an evaluator tile
BLOCK = 256           # rays (pairs) of a compaction workgroup
TOL = 1e-4            # the project's tolerance against the CPU oracle
L0_BOUND = 5e-7       # frontend_cases: inside level-0 rows, x max(1, far)
MAX_LIFTED_RAYS = 1   # rays of a case whose oracle bound the noise term may lift

R_LIST = (1, 63, 64, 65, 255, 256, 257, 513)
PATTERNS = ("none", "all", "first", "last", "even", "odd", "wave1", "not_wg0", "last_wg", "half", "sparse")
FIXED_R = 257
FIXED_COUNTS = (1, 15, 16, 17, 111, 112, 113, 127, 128, 129, 256)
ALIGNED_COUNTS = (16, 112, 128, 256)     # count * N0 is a whole number of tiles
TILE_EDGE_COUNTS = ALIGNED_COUNTS[:3]     # the counts the 3 + 1 pair runs on (N1 = 5: unaligned at 16 and 112 rows, 10 tiles at 128)
CHUNK_COUNTS = (16, 17, 128)          # at R = 257 with chunk 64: four whole reference chunks and one ray
CHUNK = 64

# the order of the calls on the one module (truth 6): a call with many hits directly before one with few, R = 513 directly before
# R = 1; the fixed counts of R = 257 alternate high / low
R_ORDER = (257, 256, 255, 65, 64, 63, 513, 1)
PATTERN_ORDER = ("all", "first", "not_wg0", "last", "half", "sparse", "wave1", "last_wg", "none", "even", "odd")
FIXED_ORDER = (256, 1, 129, 15, 128, 16, 127, 17, 113, 111, 112)
REPEATED = (("fixed", 257, 16), ("pattern", 1, "all"), ("pattern", 513, "odd"), ("pattern", 257, "last_wg"), ("fixed", 257, 129),
            ("pattern", 64, "none"))


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


# ---- hit patterns ------------------------------------------------------------------------------------------------------------------
def pattern_mask(R, name):
    """The (R,) bool mask of a pattern, or None where the pattern does not exist at this ray count."""
    r = torch.arange(R)
    if name == "none":
        return torch.zeros(R, dtype=torch.bool)
    if name == "all":
        return torch.ones(R, dtype=torch.bool)
    if name == "first":
        return r == 0
    if name == "last":
        return r == R - 1
    if name == "even":
        return r % 2 == 0
    if name == "odd":
        return r % 2 == 1
    if name == "wave1":
        return ((r >= 64) & (r < 128)) if R >= 128 else None
    if name == "not_wg0":
        return (r >= BLOCK) if R > BLOCK else None
    if name == "last_wg":
        return (r >= (R - 1) // BLOCK * BLOCK) if R in (257, 513) else None
    if name in ("half", "sparse"):
        p = 0.5 if name == "half" else 1.0 / 64
        return torch.rand(R, generator=_gen(R, PATTERNS.index(name))) < p
    raise KeyError(name)


def fixed_mask(k, R=FIXED_R):
    """The first k rays of a seeded permutation of R."""
    perm = torch.randperm(R, generator=_gen(R, 99))
    m = torch.zeros(R, dtype=torch.bool)
    m[perm[:k]] = True
    return m


def case_mask(kind, R, what):
    return fixed_mask(what, R) if kind == "fixed" else pattern_mask(R, what)


def table():
    """Every (kind, R, pattern or count) of the objects table, in the stated call order."""
    out = []
    for R in R_ORDER:
        if R == FIXED_R:
            out += [("fixed", R, k) for k in FIXED_ORDER]
        out += [("pattern", R, p) for p in PATTERN_ORDER if pattern_mask(R, p) is not None]
    return out


def case_name(kind, R, what):
    return "R%d_%s" % (R, ("count%d" % what) if kind == "fixed" else what)


MISSES = ("zero", "nan_near", "nan_far", "inf", "far_eq_lo", "far_lt_near")


def intervals(mask, shift=0.0):
    """near, far (R,) float32 of a mask: the interval rule on the hits, the six miss encodings cycled over the misses."""
    R = mask.shape[0]
    r = np.arange(R)
    near = (0.30 + 0.001 * (r % 7) + shift).astype(np.float32)
    far = (0.90 - 0.002 * (r % 5) + shift).astype(np.float32)
    nan, inf = np.float32("nan"), np.float32("inf")
    enc = np.array([(0.0, 0.0), (nan, 0.9), (0.3, nan), (inf, inf), (0.0, np.float32(oc.NEAR)), (0.7, 0.4)], dtype=np.float32)
    miss = np.nonzero(~mask.numpy())[0]                      # far == lo above: the clamped lo itself
    j = np.arange(miss.shape[0]) % len(enc)
    near[miss], far[miss] = enc[j, 0], enc[j, 1]
    return torch.from_numpy(near), torch.from_numpy(far)


def compaction_model(mask):
    """What the two launches of compact.h must produce for a keep mask: map = the kept indices ascending, slot its inverse
    (-1 on the others), and the per-workgroup totals with the prefix every workgroup sums."""
    flat = mask.reshape(-1)
    mp = flat.nonzero().reshape(-1)
    slot = torch.full((flat.shape[0],), -1, dtype=torch.long)
    slot[mp] = torch.arange(mp.shape[0])
    pad = (-flat.shape[0]) % BLOCK
    totals = torch.cat([flat, torch.zeros(pad, dtype=torch.bool)]).reshape(-1, BLOCK).sum(dim=1)
    prefix = torch.cumsum(totals, 0) - totals
    return mp, slot, totals, prefix


def tiles(count, N):
    return (count * N + TM - 1) // TM


# ---- rays, level-0 truth, the oracle pair -------------------------------------------------------------------------------------------
_RAYS = {}


def rays(R):
    """The CPU batch of cases.strided_rays(R) (the strided pattern wraps around the 48 x 64 frame beyond 3072 rays)."""
    if R not in _RAYS:
        _RAYS[R] = cases.neo_batch(cases.strided_rays(R))
    return dict(_RAYS[R])


def level0_truth(near, far, n_coarse=N_COARSE):
    """lo (1 - e) + hi e on an fp64 linspace, from the fp32 bounds: (fp64 rows, the same in plain fp32, the per-entry bound)."""
    lo, hi, _ = oc.hit_rule(near.float(), far.float())
    e = torch.linspace(0.0, 1.0, n_coarse + 1, dtype=torch.float64)
    ref64 = lo.double()[:, None] * (1.0 - e) + hi.double()[:, None] * e
    e32 = torch.linspace(0.0, 1.0, n_coarse + 1)
    ref32 = lo[:, None] * (1.0 - e32) + hi[:, None] * e32
    bound = L0_BOUND * torch.clamp(hi.double(), min=1.0)[:, None].expand_as(ref64)
    return ref64, ref32, bound


def level0_checks(t0, near, far, hit, n_coarse=N_COARSE):
    """Truth 2 on the hit rows of t0 (R, N0): per entry against fp64, ascending, first and last entry exactly lo and hi."""
    t0 = t0.cpu()
    ref64, ref32, bound = level0_truth(near, far, n_coarse)
    lo, hi, _ = oc.hit_rule(near.float(), far.float())
    rows = t0[hit]
    order = dict(ascending=bool((rows[:, 1:] > rows[:, :-1]).all()), first=bool((rows[:, 0] == lo[hit]).all()),
                 last=bool((rows[:, -1] == hi[hit]).all()))
    return dict(t0=worst_entry(rows, ref64[hit], bound[hit], ref32[hit])), order


OUT = ("rgb", "acc", "depth")
_F64 = {}


def _double(d):
    return {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in d.items()}


def oracle_pair(R, near, far, n_fine=N_FINE, t1=None, white=True, chunk=None):
    """object_cases.oracle_render on all R rays as it is (fp32) and with float64 weights, rays and scene, both at the SAME level-1
    positions: t1 if given (the GPU's own), else the fp32 oracle's resampled rows.  The level-0 rows are the fp32 ones in both (they
    are inputs here; truth 2 holds them to fp64 separately)."""
    if "state" not in _F64:
        _F64.update(state=_double(oc.state()), scene=_double(cases.small_scene()))
    b = rays(R)
    o32 = oc.oracle_render(oc.state(), b, near, far, N_COARSE, n_fine, white_bkgd=white, chunk=chunk, t1=t1)
    o64 = oc.oracle_render(_F64["state"], _double(b), near, far, N_COARSE, n_fine, white_bkgd=white, chunk=chunk,
                           t1=(t1 if t1 is not None else o32["t1"]).double(), scene=_F64["scene"])
    assert o64["rgb1"].dtype == torch.float64
    return o32, o64


def _per_ray(x):
    return x.reshape(x.shape[0], -1).amax(dim=1)


def oracle_bounds(o32, o64, hit):
    """Per quantity: (per-ray noise of the fp32 oracle against its fp64 twin, per-ray bound, rays whose bound was lifted).  The
    bound is 1e-4; a ray whose own noise reaches 1e-4 gets 1e-4 + 3 x that noise (conftest's standing rule)."""
    out = {}
    for lv in range(2):
        for k in OUT:
            key = "%s%d" % (k, lv)
            noise = _per_ray((o32[key].double() - o64[key]).abs())
            lifted = hit & (noise >= TOL)
            out[key] = (noise, torch.where(noise >= TOL, TOL + 3.0 * noise, torch.full_like(noise, TOL)), lifted)
    return out


def lifted_rays(bounds):
    return int(torch.stack([v[2] for v in bounds.values()]).any(dim=0).sum())


def oracle_checks(res, o32, o64, hit):
    """Truth 4: every hit ray of both levels of a render_objects result against the fp64 oracle, per ray, no exempt rays."""
    b = oracle_bounds(o32, o64, hit)
    checks = {}
    for lv in range(2):
        for k, got in zip(OUT, res[lv]):
            key = "%s%d" % (k, lv)
            bound = b[key][1][hit].reshape([-1] + [1] * (o64[key].dim() - 1)).expand_as(o64[key][hit])
            checks[key] = worst_entry(got.cpu()[hit], o64[key][hit], bound, o32[key][hit])
    return checks, lifted_rays(b)


# ---- grid-stride and many-workgroup cases -------------------------------------------------------------------------------------------
BIG_WG_R = 65793                      # 257 * 256 + 1: 258 compaction workgroups, the totals sum takes a second trip
BIG_WG_FORCED = (0, 65279, 65280, 65535, 65536, 65792)
SCATTER_R, SCATTER_N_FINE, SCATTER_CHUNK = 4101, 1019, 2048
SCATTER_HITS = (0, 2047, 2048, 4099, 4100)
LEVEL0_R, LEVEL0_N_COARSE, LEVEL0_N_FINE, LEVEL0_CHUNK = 16400, 256, 1, 4096
GRID_CAP = 16384 * 256                # elements one trip of a capped grid covers


def big_wg_mask():
    m = torch.rand(BIG_WG_R, generator=_gen(BIG_WG_R, 1)) < 1.0 / 256
    m[list(BIG_WG_FORCED)] = True
    return m


def scatter_mask():
    m = torch.zeros(SCATTER_R, dtype=torch.bool)
    m[list(SCATTER_HITS)] = True
    return m


# ---- instances ---------------------------------------------------------------------------------------------------------------------
WINDOW_K = (1, 2, 3)
WINDOW_R = (1, 5, 64, 257)
TIE_EVERY = 3                         # instances 0 and 1 share `near` exactly on the rays with ray % 3 == 0
K32 = 32
K32_R = 65
K32_BIG_R = 2057                      # 32 * 2057 = 65824 pairs = 258 workgroups
K32_BIG_ROWS = (0, 15, 31)
ONLY31, NEAREST31, TIE31, ALL32 = 0, 1, 2, 3         # the designed rays of the K = 32, R = 65 case
MARGIN_MAX_FRAC = 0.02


def window_counts(K, R):
    want = [0, 1, R - 1, R, R + 1] + ([2 * R] if K >= 2 else []) + [K * R]
    return sorted({c for c in want if 0 <= c <= K * R})


def windows_model(count, K, R):
    """k_inst_windows: rows of window p of a pair list of `count` entries."""
    return [min(max(count - p * R, 0), R) for p in range(K)]


def window_of_pairs(mask):
    """(K,R) pair mask -> (K,R) long: the window each hit pair lands in (pair = i R + ray, compact index // R), -1 on misses."""
    K, R = mask.shape
    flat = mask.reshape(-1)
    idx = torch.cumsum(flat.long(), 0) - 1
    return torch.where(flat, idx // R, torch.full_like(idx, -1)).reshape(K, R)


def split_rays(mask):
    """Rays with one instance in window 0 and another in window 1."""
    w = window_of_pairs(mask)
    return ((w == 0).any(dim=0) & (w == 1).any(dim=0)).nonzero().reshape(-1)


def window_mask(K, R, count):
    """A (K,R) pair mask with `count` hits: the first `count` pairs of a seeded permutation; where a second window exists, the ray of
    the LAST hit pair is made to hit in instance 0 as well (one other hit pair gives way), so that some ray has its instances split
    over windows 0 and 1."""
    P = K * R
    perm = torch.randperm(P, generator=_gen(K, R, count))
    flat = torch.zeros(P, dtype=torch.bool)
    flat[perm[:count]] = True
    if count > R and split_rays(flat.reshape(K, R)).numel() == 0:
        hits = flat.nonzero().reshape(-1)
        w = (torch.arange(hits.shape[0]) // R)
        first_w1 = int(hits[w == 1][0])               # a hit pair of window 1; its instance is >= 1 because count > R
        ray = first_w1 % R
        if not bool(flat[ray]):
            flat[ray] = True
            drop = next(int(h) for h in hits.tolist() if h != first_w1 and h % R != ray and h > ray)
            flat[drop] = False
    return flat.reshape(K, R)


def instance_intervals(mask, designed=False):
    """near, far (K,R) float32: the interval rule per instance, shifted by 0.01 i; instance 1 takes instance 0's `near` on every third
    ray (a tie, to the lower index).  designed: the four rays of the K = 32, R = 65 case."""
    K, R = mask.shape
    rows = [intervals(mask[i], 0.01 * i) for i in range(K)]
    near, far = torch.stack([n for n, _ in rows]), torch.stack([f for _, f in rows])
    if K >= 2:
        clean = intervals(torch.ones(R, dtype=torch.bool))[0]
        tie = mask[1] & (torch.arange(R) % TIE_EVERY == 0)
        near[1] = torch.where(tie, clean, near[1])
    if designed:
        near[31, NEAREST31] = 0.25                    # in front of every other instance of its ray
        near[31, TIE31] = intervals(torch.ones(R, dtype=torch.bool))[0][TIE31]
    return near, far


def k32_mask(R=K32_R):
    m = torch.rand(K32, R, generator=_gen(K32, R)) < 0.25
    m[:, ONLY31] = False
    m[31, ONLY31] = True
    m[:, NEAREST31] = False
    m[[3, 17, 31], NEAREST31] = True
    m[:, TIE31] = False
    m[[0, 31], TIE31] = True
    m[:, ALL32] = True
    return m


def k32_big_mask():
    return torch.rand(K32, K32_BIG_R, generator=_gen(K32, K32_BIG_R)) < 1.0 / 128


# the two instance kernels with a 16384-block cap (beyond the issue's list; the objects cases above have the other two)
FILL_R = 131073                       # 32 * 131073 = 4,194,336 pairs: k_inst_fill_misses takes a second trip on the last 32
FILL_ROWS = (0, 31)


def fill_mask():
    m = torch.rand(K32, FILL_R, generator=_gen(K32, FILL_R)) < 1.0 / 4096
    m[31, FILL_R - 1] = True          # a hit and, before it, misses among the pairs of the second trip
    m[31, FILL_R - 32:FILL_R - 1] = False
    return m


def composite64(near, far, p, a, d, white):
    """The composite recurrence in fp64 on fp32 per-instance rows (p (K,B,3), a, d (K,B)): rgb, acc, depth, id, and per ray the
    best and second-best visibility with the instance of the second (-1: none).  Order: ascending fp32 lo, ties to the lower index."""
    K, Bn = near.shape
    lo, _, hit = oc.hit_rule(near.float().cpu(), far.float().cpu())
    key = torch.where(hit, lo, torch.full_like(lo, float("inf")))
    order = torch.sort(key, dim=0, stable=True).indices
    p, a, d = p.cpu().double(), a.cpu().double(), d.cpu().double()
    cols = torch.arange(Bn)
    T = torch.ones(Bn, dtype=torch.float64)
    rgb = torch.zeros(Bn, 3, dtype=torch.float64)
    depth, acc = torch.zeros(Bn, dtype=torch.float64), torch.zeros(Bn, dtype=torch.float64)
    best, second = torch.zeros(Bn, dtype=torch.float64), torch.zeros(Bn, dtype=torch.float64)
    ids, second_i = torch.full((Bn,), -1, dtype=torch.int32), torch.full((Bn,), -1, dtype=torch.int32)
    for s in range(K):
        i = order[s]
        ok = hit[i, cols]
        v = T * a[i, cols]
        rgb = torch.where(ok[:, None], rgb + T[:, None] * p[i, cols], rgb)
        depth = torch.where(ok, depth + T * d[i, cols], depth)
        acc = torch.where(ok, acc + v, acc)
        # the winner: the largest visibility, the earliest in the order among equals (`>` only); it must be > 0 to win at all
        win = ok & (v > best)
        runner = ok & ~win & (v > second)
        second = torch.where(win, best, torch.where(runner, v, second))
        second_i = torch.where(win, ids, torch.where(runner, i.to(torch.int32), second_i))
        best = torch.where(win, v, best)
        ids = torch.where(win, i.to(torch.int32), ids)
        T = torch.where(ok, T * (1.0 - a[i, cols]), T)
    if white:
        rgb = rgb + (1.0 - acc)[:, None]
    return dict(rgb=rgb, acc=acc, depth=depth, id=ids, best=best, second=second, second_id=second_i, any_hit=hit.any(dim=0))


def id_checks(got_ids, c64, K):
    """instance_id against the fp64 recurrence: exact where best and second-best visibility differ by more than K 2^-22, either of
    the two elsewhere; -1 exactly on the rays without a hit.  Returns (ok, rays inside the margin)."""
    got = got_ids.cpu().to(torch.int32)
    clear = (c64["best"] - c64["second"]) > K * 2.0 ** -22
    ok = torch.where(clear, got == c64["id"], (got == c64["id"]) | (got == c64["second_id"]))       # no hit: both are -1
    ok = ok & (c64["any_hit"] | (got == -1))
    return bool(ok.all()), int((~clear & c64["any_hit"]).sum())


_INST_ORACLE = {}


def oracle_instance_rows(near, far, tag):
    """The fp32 CPU oracle's per-instance rows (black background) for (K,R) intervals: p (K,R,3), a, d (K,R), zero on misses.
    Level 1, at the oracle's own resampled positions."""
    if tag not in _INST_ORACLE:
        K, R = near.shape
        p, a, d = torch.zeros(K, R, 3), torch.zeros(K, R), torch.zeros(K, R)
        for i in range(K):
            hit = oc.hit_rule(near[i], far[i])[2]
            if bool(hit.any()):
                o = oc.oracle_render(oc.state(), rays(R), near[i], far[i], N_COARSE, N_FINE, white_bkgd=False)
                p[i][hit], a[i][hit], d[i][hit] = o["rgb1"][hit].float(), o["acc1"][hit].float(), o["depth1"][hit].float()
        _INST_ORACLE[tag] = (p, a, d)
    return _INST_ORACLE[tag]


# ---- culling -----------------------------------------------------------------------------------------------------------------------
CULL_R = (63, 64, 65, 257)
CULL_BIAS = 4.0


def cull_targets(R):
    return [0, 1, 15, 16, 17, R - 1, R] + ([112, 128, 129] if R == 257 else [])


def cull_eps(m, k):
    """m (R,) fp32 = max(lambda_0, lambda_1) per ray -> (eps, tie): eps = the k-th largest m (k = 0: nextafter of the largest), so
    that the keep rule !(lambda < eps) keeps exactly k rays; tie: the value at rank k is shared with rank k + 1 (then it keeps more)."""
    s = torch.sort(m.reshape(-1).float().cpu(), descending=True).values
    if k == 0:
        return float(torch.nextafter(s[0], torch.tensor(float("inf")))), False
    eps = float(s[k - 1])
    return eps, bool(k < s.shape[0] and float(s[k]) == eps)
