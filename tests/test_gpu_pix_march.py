"""GPU: empty-space skipping and early ray termination of the PixelNeRF frame (`marching.MarchingPixelNeRF.render_marching`,
neo_pix_render_marching), the compact launch of its evaluators (`marching.eval_points_pix`) and the frame helper
(`marching.render_marching_rays`).

Inputs: tests/pix_march_cases.py - cases.small_scene(), synth.pixelnerf_state(0) with a per-pair density bias,
cases.neo_batch(cases.strided_rays(R)) for R in {1, 63, 64, 65, 257} between 0.2 and 2.5, the count pairs 3 + 4, 7 + 64, 63 + 64 and
64 + 128, the split arithmetic with and without pre-projection and the exact one.  tests/test_pix_march_cpu.py asserts on the oracle
that the inputs mix stopped and never-stopped rays and that the mixed grid keeps and skips; where a test here relies on a mix it
asserts it again on the device's own stops and masks.

Bounds.  The call is a composition of rules that the library states bit for bit: an evaluated sample is the dense launch's row for
the same point and direction, any other sample is a row of zeros, the keep mask is `marching.occupancy_keep_box` (dirs = rays_d)
and the stop is `marching.termination_stops_vanilla` on the masked rows.  So every comparison of the call with `forward`,
`eval_mlp` or the chain of public stage ops is `torch.equal`.  The a-priori bound of the header (1.003 trans per channel, 1.001 far
trans in depth) is asserted against the same call at eps = 0; the parity with the CPU oracle is the project's 1e-4 per ray."""
import pytest
import torch

import cases
import occupancy_cases as oc
import pix_march_cases as pc
import vanilla_march_cases as vc
from neo360_amd import _lib, marching, models, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = pc.PER_RAY
NAMES = ("rgb", "acc", "depth")
ARMS = (("f16x3", True), ("f16x3", False), ("f32", True))          # (arithmetic, preproject): the exact kernel has one operation order
ARM_IDS = ["%s-%s" % (p, "pre" if q else "raw") for p, q in ARMS]
CASES = [(c, a) for c in pc.COUNTS for a in ARMS]
IDS = ["%d+%d-%s" % (c[0], c[1], i) for c in pc.COUNTS for i in ARM_IDS]
STOP_CASES = [(c, a) for c, a in CASES if c in pc.STOPPING]
STOP_IDS = [i for (c, a), i in zip(CASES, IDS) if c in pc.STOPPING]

_NETS = {}
_RAYS = {}


def _net(counts, arm=ARMS[0]):
    key = (counts, arm)
    if key not in _NETS:
        net = marching.MarchingPixelNeRF(num_coarse_samples=counts[0], num_fine_samples=counts[1], num_src_views=cases.NV).to(DEV)
        net.load_state_dict(pc.state(counts))
        net.precision, net.preproject = arm
        sc = pc.scene()
        net.set_scene(sc["latent"].to(DEV), sc["image_wh"])
        _NETS[key] = net
    return _NETS[key]


def _rays(n):
    if n not in _RAYS:
        _RAYS[n] = {k: v.to(DEV) for k, v in pc.rays(n).items()}
    return _RAYS[n]


def _march(net, b, eps, white=False, **kw):
    """[level 0 three, level 1 three, [(t, w, keep, stop, rows) per level], kept int64[2]], cloned."""
    out = net.render_marching(b, eps, white, pc.NEAR, pc.FAR, return_samples=True, **kw)
    net.check_flags()
    return [[t.clone() for t in out[0]], [t.clone() for t in out[1]], [[t.clone() for t in lv] for lv in out[2]],
            net.last_march_kept.clone()]


def _forward(net, b, white=False, chunk=None):
    out = net(b, False, white, pc.NEAR, pc.FAR, chunk=chunk)
    net.check_flags()
    return [[t.clone() for t in lv] for lv in out]


class _installed:
    def __init__(self, net, grid, box=None, clip=False):
        self.args = (net, grid, box, clip)

    def __enter__(self):
        net, grid, box, clip = self.args
        net.set_occupancy(grid, box, clip)

    def __exit__(self, *exc):
        self.args[0].set_occupancy(None)


def _flat(res):
    return [t for lv in res[:2] for t in lv] + [t for lv in res[2] for t in lv] + [res[3]]


def _same(x, y):
    return all(a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(_flat(x), _flat(y)))


def _assert_equals_chain(net, b, got, what, grid, box, clip, eps, white=False, segment=64, coarse=False, chunk=None):
    """The frame from the public stage ops, level by level on the call's own returned positions: the keep mask is
    occupancy_keep_box along rays_d, kept rows are eval_mlp's at the call's chunk and skipped rows zero, the stop is
    termination_stops_vanilla on the masked rows, the composite is ops.composite(0, ...) on the returned rows and the level-1
    positions are ops.resample on the returned level-0 weights.  Everything bitwise.  Returns the stops."""
    o, rd = b["rays_o"], b["rays_d"]
    R = o.shape[0]
    evaluated, stops = [], []
    for lv in range(2):
        t, w, keep, stop, rows = got[2][lv]
        N = t.shape[1]
        assert tuple(w.shape) == tuple(keep.shape) == (R, N) and tuple(rows.shape) == (R, N, 4) and tuple(stop.shape) == (R,)
        assert keep.dtype == torch.bool and stop.dtype == torch.int32
        assert torch.equal(keep, marching.occupancy_keep_box(grid, box, o, rd, t, clip)), (what, lv, "keep mask")
        full = net.eval_mlp(lv, b, t.contiguous(), chunk=chunk)
        masked = torch.where(keep[:, :, None], full, torch.zeros_like(full))
        if eps > 0 and (lv == 1 or coarse):
            own, _ = marching.termination_stops_vanilla(masked, t, rd, eps, segment)
            again, _ = marching.termination_stops_vanilla(rows, t, rd, eps, segment)
            assert torch.equal(stop, own) and torch.equal(stop, again), (what, lv, "stop")
        else:
            assert bool((stop == N).all()), (what, lv)
        mask = keep & pc.front(stop, N)
        assert torch.equal(rows, torch.where(mask[:, :, None], full, torch.zeros_like(full))), (what, lv, "rows")
        assert bool((rows[~mask] == 0).all()) and bool((w[~mask] == 0).all())
        c = ops.composite(0, rows, t, rd, white_bkgd=white)
        for k, x in zip(NAMES, got[lv]):
            assert torch.equal(x, c[k]), (what, lv, k)
        assert torch.equal(w, c["weights"]), (what, lv, "weights")
        if lv == 0:
            assert torch.equal(got[2][1][0], ops.resample(t, w, net.num_fine_samples)), (what, "level-1 positions")
        evaluated.append(int(mask.sum()))
        stops.append(stop)
    assert got[3].tolist() == evaluated, (what, got[3].tolist(), evaluated)
    return stops


# ---- 1. the compact launch -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS + (("f32", False),), ids=ARM_IDS + ["f32-raw"])
def test_eval_points_pix_under_a_device_count(arm):
    net = _net((64, 128), arm)
    cap, N = 257, 5
    b = _rays(cap)
    g = torch.Generator().manual_seed(3)
    t = (pc.NEAR + (pc.FAR - pc.NEAR) * torch.rand(cap, N, generator=g)).to(DEV)
    # cap of the cap x N dense points, spread over rays and samples: point k is sample js[k] of ray bs[k]
    pick = (torch.arange(cap) * 5 + (torch.arange(cap) * 7) % 5) % (cap * N)
    bs, js = (pick // N).to(DEV), (pick % N).to(DEV)
    for chunk in (cap, 64):
        q1 = pc.q1_index(cap, N, chunk).to(DEV)
        assert chunk == cap or not torch.equal(q1[:, 0], torch.arange(cap, device=DEV)), "a short chunk moves the directions"
        rows = dict(b, rays_o=b["rays_o"][bs].contiguous(), rays_d=b["rays_d"][bs].contiguous(),
                    viewdirs=b["viewdirs"][q1[bs, js]].contiguous())
        tt = t[bs, js].contiguous()
        for slot in range(2):
            dense = net.eval_mlp(slot, b, t, chunk=chunk)[bs, js].clone()
            out = torch.empty(cap, 4, device=DEV)
            for n in (cap, 65, 64, 63, 1, 0):      # descending on one buffer set: a stale row that was used would show
                out.fill_(-7.0)
                count = torch.tensor([n], dtype=torch.int32, device=DEV)
                res = marching.eval_points_pix(net, slot, rows, tt, count, out=out)
                assert res is out
                assert torch.equal(out[:n], dense[:n]), (arm, chunk, slot, n)
                assert bool((out[n:] == -7.0).all()), (arm, chunk, slot, n, "rows behind the count are not written")
            big = torch.tensor(cap + 7, dtype=torch.int32, device=DEV)
            assert torch.equal(marching.eval_points_pix(net, slot, rows, tt[:, None], big), dense), "a count beyond the bound is the bound"


# ---- 2. nothing to skip and nothing to stop: forward ------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,arm", CASES, ids=IDS)
def test_no_grid_grid_off_all_ones_grid_and_a_far_box_are_bitwise_forward_at_eps_zero(counts, arm):
    net = _net(counts, arm)
    N = pc.n_level(counts)
    try:
        for n in pc.RAYS:
            b = _rays(n)
            # R = 257: both chunkings (one chunk; 64, a short last chunk) under both windows (48 straddles the chunk boundaries)
            for chunk, window, white in (((None, None, False), (None, 48, True), (64, None, True), (64, 48, False)) if n == 257 else
                                         ((None, None, False), (64, None, True))):
                net.march_window = window
                want = _forward(net, b, white, chunk)
                for grid, box, use in ((None, None, True), (pc.mixed(8), pc.BOX, False), (oc.ones(32), pc.BOX, True), (pc.mixed(8), pc.FAR_AWAY, True)):
                    with _installed(net, grid, box, False):
                        got = _march(net, b, 0.0, white, chunk=chunk, grid=use)
                    what = (counts, arm, n, chunk, window, None if grid is None else (int(grid.shape[0]), box, use))
                    for lv in range(2):
                        for k, x, y in zip(NAMES, got[lv], want[lv]):
                            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, lv, k)
                        t, w, keep, stop, rows = got[2][lv]
                        assert (not use or bool(keep.all())) and bool((stop == N[lv]).all()), (what, lv)
                    assert got[3].tolist() == [n * N[0], n * N[1]], what
    finally:
        net.march_window = None


# ---- 3. a mixed grid: the chain of public stage ops ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,arm", CASES, ids=IDS)
def test_mixed_grid_frame_equals_the_chain_of_stage_ops(counts, arm):
    net = _net(counts, arm)
    for n in pc.RAYS:
        b = _rays(n)
        for G in ((8, 32) if n in (65, 257) else (32,)):
            grid = pc.mixed(G)
            with _installed(net, grid, pc.BOX, True):
                for eps, coarse, chunk in ((0.0, False, None), (pc.EPS, False, 64 if n == 257 else None), (pc.EPS, True, None)):
                    got = _march(net, b, eps, coarse=coarse, chunk=chunk)
                    _assert_equals_chain(net, b, got, (counts, arm, n, G, eps, coarse, chunk), grid, pc.BOX, True, eps, coarse=coarse, chunk=chunk)
                    if n >= 63:
                        for lv in range(2):
                            keep = got[2][lv][2]
                            share = float(keep.float().mean())
                            assert 0.15 <= share <= 0.95, ("the grid keeps some samples and skips some", counts, n, G, lv, share)


# ---- 4. exact kept counts ------------------------------------------------------------------------------------------------------------------

def _grid_for_count(o, d, t1, t0, box, want):
    """A G = 256 grid over `box` that keeps exactly `want` of the level-1 positions t1 and none of the level-0 positions t0: cells
    are added one sample at a time; a cell that holds another sample, would overshoot, or touches the cell of a sample that sits
    near a cell face (whose fp32 cell is not certain) is passed over."""
    G = 256

    def lin(c):
        return (c[..., 0] * G + c[..., 1]) * G + c[..., 2]
    c1 = vc.cell_box(oc.positions(o, d, t1), box, G).long()
    c0 = vc.cell_box(oc.positions(o, d, t0), box, G).long()
    inside = ((c1 >= 0) & (c1 < G)).all(dim=-1)
    face1, face0 = vc.near_face_box(box, o, d, t1, G), vc.near_face_box(box, o, d, t0, G)
    shaky = face1 | ~inside
    taken = set(lin(c0.reshape(-1, 3)).tolist())
    offs = torch.tensor([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)])
    for c in torch.cat([c1[face1], c0[face0]]).reshape(-1, 3):      # the 27 cells around a sample whose own cell is not certain
        taken |= set(lin(c[None, :] + offs).tolist())
    lin1 = torch.where(inside, lin(c1), torch.full_like(lin(c1), -1))
    grid = oc.zeros(G)
    count = 0
    for r in range(t1.shape[0]):
        for j in range(t1.shape[1]):
            if count == want:
                return grid
            cl = int(lin1[r, j])
            if bool(shaky[r, j]) or cl in taken:
                continue
            here = int((lin1 == cl).sum())
            taken.add(cl)
            if count + here > want:
                continue
            grid.view(-1)[cl] = True
            count += here
    assert count == want, (count, want)
    return grid


@pytest.mark.parametrize("want", (0, 1, 63, 64, 65, "all"))
def test_frames_with_exact_kept_counts(want):
    """Grids at G = 256 built from the rays' own returned positions, clip=True: with every level-0 sample skipped the level-0
    weights are zero whatever else the grid holds, so the level-1 positions are those of the all-zeros grid and the counts are
    known exactly."""
    counts = (7, 64)
    net = _net(counts)
    N = pc.n_level(counts)
    b = _rays(3)
    if want == "all":
        grid = oc.ones(256)
        with _installed(net, grid, pc.BOX, False):
            got = _march(net, b, pc.EPS)
        assert int(got[3][0]) == 3 * N[0] and int(got[3][1]) == int(got[2][1][3].sum())
        _assert_equals_chain(net, b, got, "all kept", grid, pc.BOX, False, pc.EPS)
        return
    with _installed(net, oc.zeros(256), pc.BOX, True):
        empty = _march(net, b, pc.EPS)
    assert empty[3].tolist() == [0, 0]
    o, d = b["rays_o"].cpu(), b["rays_d"].cpu()
    t0, t1 = empty[2][0][0].cpu(), empty[2][1][0].cpu()
    grid = _grid_for_count(o, d, t1, t0, pc.BOX, want)
    with _installed(net, grid, pc.BOX, True):
        for eps in (0.0, pc.EPS):
            got = _march(net, b, eps)
            assert torch.equal(got[2][1][0], empty[2][1][0]), "the level-1 positions are those of the empty grid"
            assert int(got[2][1][2].sum()) == want and got[3].tolist() == [0, want], (want, eps, got[3].tolist())
            _assert_equals_chain(net, b, got, ("kept", want, eps), grid, pc.BOX, True, eps)


# ---- 5. the stops and the termination bound -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,arm", STOP_CASES, ids=STOP_IDS)
def test_the_device_stops_mix_and_the_bound_holds_against_the_same_call_at_eps_zero(counts, arm):
    net = _net(counts, arm)
    N1 = pc.n_level(counts)[1]
    n = 257
    b = _rays(n)
    seen = 0
    grids = [None, (32, 0.55)] + ([pc.STOP_GRID[counts]] if pc.STOP_GRID[counts] else [])
    for garm in grids:      # (G, ball radius) or None
        G = garm[0] if garm else None
        grid = pc.mixed(*garm) if garm else None
        with _installed(net, grid, pc.BOX if G else None, True):
            for white in (False, True):
                plain = _march(net, b, 0.0, white)
                for eps in (1e-2, 1e-3):
                    got = _march(net, b, eps, white)
                    for x, y in zip(_flat(got)[:3] + [t for t in got[2][0]] + [got[2][1][0], got[2][1][2]],
                                    _flat(plain)[:3] + [t for t in plain[2][0]] + [plain[2][1][0], plain[2][1][2]]):
                        assert torch.equal(x, y), "level 0, the level-1 positions and the keep masks are identical"
                    stop = got[2][1][3]
                    own, trans = marching.termination_stops_vanilla(got[2][1][4], got[2][1][0], b["rays_d"], eps)
                    assert torch.equal(stop, own)
                    stopped = stop < N1
                    if garm == pc.STOP_GRID[counts] and eps == pc.EPS and not white:      # the frame on which the pair's rays mix
                        print("%s %s grid %s: device level-1 stops %s" % (counts, arm, garm, {int(v): int(c) for v, c in zip(*torch.unique(stop.cpu(), return_counts=True))}))
                        assert 4 * int(stopped.sum()) >= n and 4 * int((~stopped).sum()) >= n, "a quarter stops, a quarter never does"
                        assert G is not None or int(got[3][1]) == int(stop.sum()), "without a grid the evaluated samples are the prefixes"
                    for k, x, y in zip(NAMES, got[1], plain[1]):
                        assert torch.equal(x[~stopped], y[~stopped]), ("a ray that never stops is bitwise unchanged", k)
                    if not bool(stopped.any()):
                        continue
                    seen += int(stopped.sum())
                    assert bool((trans[stopped] < eps).all())
                    d_rgb = (got[1][0] - plain[1][0]).abs().max(dim=-1).values
                    d_depth = (got[1][2] - plain[1][2]).abs()
                    print("%s %s grid %s white %s eps %g: %d of %d stopped; max |rgb change| / trans = %.4f, max |depth change| / (far trans) "
                          "= %.4f, min trans %.3e" % (counts, arm, garm, white, eps, int(stopped.sum()), n, float((d_rgb / trans)[stopped].max()),
                                                      float((d_depth / (pc.FAR * trans))[stopped].max()), float(trans[stopped].min())))
                    assert bool((d_rgb[stopped] <= 1.003 * trans[stopped]).all())
                    assert bool((d_depth[stopped] <= 1.001 * pc.FAR * trans[stopped]).all())
    assert seen > 0, "no ray stopped: the bound was not exercised"


# ---- 6. the CPU oracle ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,arm", CASES, ids=IDS)
def test_parity_with_the_oracle_on_the_devices_own_positions_and_masks(counts, arm):
    net = _net(counts, arm)
    n = 65
    b = _rays(n)
    cpu = pc.rays(n)
    for G, eps, white in ((None, 0.0, False), (32, pc.EPS, False), (32, pc.EPS, True)):
        with _installed(net, pc.mixed(G) if G else None, pc.BOX if G else None, True):
            got = _march(net, b, eps, white)
        samples = tuple(got[2][lv][0].cpu().contiguous() for lv in range(2))
        masks = tuple((got[2][lv][2] & pc.front(got[2][lv][3], got[2][lv][0].shape[1])).cpu() for lv in range(2))
        want, _ = pc.oracle_render_marching(pc.state(counts), cpu, counts, eps, white_bkgd=white, samples=samples, masks=masks)
        for lv in range(2):
            for k, x, y in zip(NAMES, got[lv], want[lv]):
                err = float((x.cpu() - y).abs().max())
                print("%s %s grid %s eps %g white %s level %d %s: max |err| per ray %.3e" % (counts, arm, G, eps, white, lv, k, err))
                assert err < 1e-4, (counts, lv, k, err)


# ---- 7. the empty grid and the clip ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,arm", CASES, ids=IDS)
def test_all_zeros_grid_renders_the_background_and_clip_skips_outside_samples(counts, arm):
    net = _net(counts, arm)
    N = pc.n_level(counts)
    n = 65
    b = _rays(n)
    o, rd = b["rays_o"], b["rays_d"]
    for white in (False, True):
        with _installed(net, oc.zeros(32), pc.BOX, True):
            got = _march(net, b, pc.EPS, white)      # K = 0 launches at both levels; check_flags: no flag is raised
        for lv in range(2):
            rgb, acc, depth = got[lv]
            assert bool((acc == 0).all()) and bool((rgb == (1.0 if white else 0.0)).all()) and bool((depth == 0).all())
            t, w, keep, stop, rows = got[2][lv]
            assert not bool(keep.any()) and bool((rows == 0).all()) and bool((w == 0).all()) and bool((stop == N[lv]).all())
        assert got[3].tolist() == [0, 0]
    # clip=True with a box smaller than the ray span: samples outside have zero rows, samples inside are eval_mlp's
    with _installed(net, oc.ones(8), pc.SMALL, True):
        got = _march(net, b, 0.0)
    for lv in range(2):
        t, w, keep, stop, rows = got[2][lv]
        tc_, oc_, dc_ = t.cpu(), o.cpu(), rd.cpu()
        c = vc.cell_box(oc.positions(oc_, dc_, tc_), pc.SMALL, 8)
        inside = ((c >= 0) & (c < 8)).all(dim=-1)
        sure = ~vc.near_face_box(pc.SMALL, oc_, dc_, tc_, 8)
        assert int((~sure).sum()) <= 0.01 * sure.numel()
        assert torch.equal(keep.cpu()[sure], inside[sure])
        assert 0 < int(keep.sum()) < keep.numel(), "the box is smaller than the ray span"
        assert bool((rows[~keep] == 0).all())
        assert torch.equal(rows[keep], net.eval_mlp(lv, b, t.contiguous())[keep])
    with _installed(net, oc.ones(8), pc.SMALL, False):
        assert _same(_march(net, b, 0.0), _march(net, b, 0.0, grid=False)), "without clip the outside samples are kept"


# ---- 8. building a grid ---------------------------------------------------------------------------------------------------------------------

def test_build_occupancy_is_the_cpu_reduction_of_eval_mlps_own_densities_and_set_scene_removes_the_grid():
    counts = (7, 64)
    net = _net(counts)
    b = _rays(5)
    G, probes = 8, 2
    c, o, d = marching.occupancy_lattice_box(pc.BOX, G, probes, DEV)
    M = G * probes
    t = c[None, :].expand(M * M, M).contiguous()
    lattice = dict(b, rays_o=o, rays_d=d, viewdirs=d)
    sigma = torch.maximum(net.eval_mlp(0, lattice, t)[..., 3], net.eval_mlp(1, lattice, t)[..., 3]).reshape(M, M, M).cpu()
    threshold = float(sigma.median())
    try:
        for dilate in (0, 1):
            grid = net.build_occupancy(b, pc.BOX, G, threshold, probes=probes, dilate=dilate)
            raw = (~(sigma.reshape(G, probes, G, probes, G, probes) <= threshold)).any(dim=5).any(dim=3).any(dim=1)
            assert torch.equal(grid.cpu(), oc.dilate(raw, dilate)), dilate
            assert torch.equal(net.occupancy, grid) and net.occupancy_box == pc.BOX
            if dilate == 0:
                assert 0 < int(grid.sum()) < grid.numel()
        # a grid describes one scene
        sc = pc.scene()
        net.set_scene(sc["latent"].to(DEV), sc["image_wh"])
        assert net.occupancy is None and net.occupancy_box is None
        want = _forward(net, b)
        got = _march(net, b, 0.0)
        assert all(torch.equal(x, y) for lv in range(2) for x, y in zip(got[lv], want[lv])), "no grid after set_scene"
        # a grid of another context is refused
        net.set_occupancy(grid, pc.BOX)
        mine = net._occ_ctx
        net._occ_ctx = object()
        try:
            with pytest.raises(_lib.NeoError, match="does not belong"):
                net.render_marching(b, pc.EPS, False, pc.NEAR, pc.FAR)
        finally:
            net._occ_ctx = mine
    finally:
        net.set_occupancy(None)


# ---- 9. windows, streams, repeatability, the chunk loop -------------------------------------------------------------------------------------

def test_windows_streams_runs_and_the_chunk_loop_give_the_same_bits_and_nothing_blocks():
    counts = (63, 64)
    net = _net(counts)
    n, chunk = 257, 100
    b = _rays(n)
    grid = pc.mixed(32)
    assert net.march_window is None
    with _installed(net, grid, pc.BOX, True):
        try:
            base = _march(net, b, pc.EPS, chunk=chunk)
            coarse = _march(net, b, pc.EPS, chunk=chunk, coarse=True)
            assert _same(_march(net, b, pc.EPS, chunk=chunk), base), "two runs"
            for window in (1, 48, 64):
                net.march_window = window
                assert _same(_march(net, b, pc.EPS, chunk=chunk), base), window
                assert _same(_march(net, b, pc.EPS, chunk=chunk, coarse=True), coarse), window
        finally:
            net.march_window = None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = _march(net, b, pc.EPS, chunk=chunk)
        torch.cuda.current_stream().wait_stream(side)
        assert _same(on_side, base), "a side stream"
        net.overlap_calls = False
        try:
            assert _same(_march(net, b, pc.EPS, chunk=chunk), base), "overlap off"
        finally:
            net.overlap_calls = True
        # the caller's own loop over reference chunks: calls in flight on alternating lanes; no blocking wait
        ctx = net._context(torch.device(DEV))
        before = ctx.sync_count()
        parts, kept = [], []
        for i in range(0, n, chunk):
            parts.append(net.render_marching(pc.part(b, i, i + chunk), pc.EPS, False, pc.NEAR, pc.FAR, return_samples=True))
            kept.append(net.last_march_kept)
        whole = net.render_marching(b, pc.EPS, False, pc.NEAR, pc.FAR, chunk=chunk)
        assert ctx.sync_count() == before, "a marching call blocked on the device"
        net.check_flags()
        for lv in range(2):
            for j in range(3):
                assert torch.equal(torch.cat([p[lv][j] for p in parts]), base[lv][j]), (lv, j)
                assert torch.equal(whole[lv][j], base[lv][j]), (lv, j)
            for j in range(5):
                assert torch.equal(torch.cat([p[2][lv][j] for p in parts]), base[2][lv][j]), (lv, j)
        assert torch.equal(sum(kept), base[3])
        helper = marching.render_marching_rays(net, b, pc.EPS, chunk=chunk, near=pc.NEAR, far=pc.FAR)
        assert torch.equal(helper["rgb"], base[1][0]) and torch.equal(helper["acc"], base[1][1]) and torch.equal(helper["depth"], base[1][2])
        frac = helper["kept_fraction"]
        N = pc.n_level(counts)
        assert frac.is_cuda and frac.dtype == torch.float64 and tuple(frac.shape) == (2,)
        assert all(abs(float(frac[lv]) - int(base[3][lv]) / (n * N[lv])) < 1e-12 for lv in range(2)) and 0.0 < float(frac[1]) < 1.0
        after = _forward(net, b, chunk=chunk)
    plain = _forward(net, b, chunk=chunk)
    assert all(torch.equal(x, y) for lv in range(2) for x, y in zip(after[lv], plain[lv])), "forward does not read the grid"
    none = pc.part(b, 0, 0)
    out = net.render_marching(none, pc.EPS, False, pc.NEAR, pc.FAR, return_samples=True)
    assert tuple(out[1][0].shape) == (0, 3) and tuple(out[2][1][3].shape) == (0,) and net.last_march_kept.tolist() == [0, 0]
    # the vanilla helper path and the TypeError are what they were
    with pytest.raises(TypeError):
        marching.render_marching_rays(models.PixelNeRF(num_src_views=cases.NV), b, pc.EPS)


# ---- 10. the range-guard retry and the module's boundary cases -------------------------------------------------------------------------------

def test_render_marching_rays_retries_a_tripped_frame_on_the_compact_exact_kernels():
    counts = (7, 64)
    sc = pc.scene()
    big = sc["latent"].to(DEV) * 1.0e6
    b = _rays(160)
    nets = []
    for precision in ("f32", None):
        net = marching.MarchingPixelNeRF(num_coarse_samples=counts[0], num_fine_samples=counts[1], num_src_views=cases.NV).to(DEV)
        net.load_state_dict(pc.state(counts))
        net.precision = precision
        net.set_scene(big, sc["image_wh"])
        net.set_occupancy(pc.mixed(32), pc.BOX, True)
        nets.append(net)
    exact, split = nets
    want = marching.render_marching_rays(exact, b, pc.EPS, chunk=64, near=pc.NEAR, far=pc.FAR)
    with pytest.warns(RuntimeWarning, match="re-rendered on the exact fp32 kernels"):
        got = marching.render_marching_rays(split, b, pc.EPS, chunk=64, near=pc.NEAR, far=pc.FAR)
    assert got["precision_used"] == "f32"
    for k in ("rgb", "acc", "depth", "kept_fraction"):
        assert torch.equal(got[k], want[k]), k
    assert bool(torch.isfinite(got["rgb"]).all()) and 0.0 < float(got["kept_fraction"][1]) < 1.0


def test_strided_misaligned_and_other_float_inputs_give_the_dense_calls_bits():
    counts = (7, 64)
    net = _net(counts)
    n = 65
    b = _rays(n)
    grid = pc.mixed(32)
    with _installed(net, grid, pc.BOX, True):
        want = _march(net, b, pc.EPS)
        wide = {k: torch.zeros(n, 7, device=DEV) for k in KEYS}
        odd = {k: torch.zeros(3 * n + 1, device=DEV) for k in KEYS}
        for k in KEYS:
            wide[k][:, 2:5] = b[k]
            odd[k][1:] = b[k].reshape(-1)
        strided = dict(b, **{k: wide[k][:, 2:5] for k in KEYS})
        misaligned = dict(b, **{k: odd[k][1:].reshape(n, 3) for k in KEYS})
        assert not strided["rays_o"].is_contiguous() and misaligned["rays_o"].data_ptr() % 16 != 0
        for what, rays in (("strided", strided), ("misaligned", misaligned), ("fp64", dict(b, **{k: b[k].double() for k in KEYS}))):
            assert _same(_march(net, rays, pc.EPS), want), what
    t = want[2][1][0][:, 0].contiguous()
    count = torch.tensor(n, dtype=torch.int32, device=DEV)
    dense = marching.eval_points_pix(net, 1, b, t, count)
    assert torch.equal(marching.eval_points_pix(net, 1, dict(strided, viewdirs=misaligned["viewdirs"].double()), t[:, None], count), dense)
    # refused by name, before any launch
    bad = dict(b)
    bad["viewdirs"] = b["viewdirs"][:-1]
    with pytest.raises(ValueError, match="viewdirs must have shape"):
        net.render_marching(bad, pc.EPS, False, pc.NEAR, pc.FAR)
    bad["viewdirs"] = b["viewdirs"].long()
    with pytest.raises(ValueError, match="viewdirs must be a floating-point"):
        net.render_marching(bad, pc.EPS, False, pc.NEAR, pc.FAR)
    bad["viewdirs"] = b["viewdirs"].cpu()
    with pytest.raises(ValueError, match="viewdirs is on cpu"):
        net.render_marching(bad, pc.EPS, False, pc.NEAR, pc.FAR)
    with pytest.raises(ValueError, match="count must be an integer"):
        marching.eval_points_pix(net, 1, b, t, count.float())
    with pytest.raises(ValueError, match="out must"):
        marching.eval_points_pix(net, 1, b, t, count, out=torch.empty(n, 6, device=DEV)[:, :4])
    with pytest.raises(ValueError, match="out must have shape"):
        marching.eval_points_pix(net, 1, b, t, count, out=torch.empty(n - 1, 4, device=DEV))
    assert isinstance(net, models.PixelNeRF)
