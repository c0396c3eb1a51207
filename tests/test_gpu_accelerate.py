"""GPU: occupancy skipping and early ray termination together (`NeRF_TP.render_accelerated`, neo_tp_render_accelerated) and the
frame helper (`render.render_accelerated_rays`).

Scene, state, grids, eps and sample counts: tests/accelerate_cases.py (cases.small_scene(), density bias +6, 64 + 70 samples = 65
and 135 per ray, segment 64; point A = oc.box_cells(32) at eps 0.33, point B = oc.mixed(32) at eps 1e-2).  The mixes that
tests/test_accelerate_cpu.py asserts on the oracle are asserted again on the device's own stops where a test relies on them.

Bounds.  The call is a composition of two rules that the library states bit for bit: an evaluated sample is computed by the same
machine code as in the dense frame, any other sample is a row of zeros, the keep mask is `ops.occupancy_keep` and the stop is
`ops.termination_stops` on the masked rows.  So every comparison here is `torch.equal` - against `render_terminating` without a
grid, against `render_skipping` at eps = 0, against the chain of public stage ops otherwise (by the rule of tests/test_gpu_edit.py:
bitwise when that chain is bitwise `forward`, else within 4 x its deviation from it; the stops and the cull set always equal).  The
a-priori bounds of the header (1.003 bg_lambda per channel, (t_far + 1.001) bg_lambda in depth) are asserted against
`render_skipping` with the same grid.

Non-finite inputs.  The two rules are tested on caller rows, as in the parents' tests: a non-finite position is kept under an empty
grid, a NaN density marches on when the rows in front of it are masked.  No test feeds a non-finite position to an evaluator."""
import ctypes

import pytest
import torch

import accelerate_cases as ac
import cases
import occupancy_cases as oc
import terminate_cases as tc
from neo360_amd import _lib, models, ops, render
from test_gpu_objects import EVALUATORS
from test_gpu_terminate import _boundary_transmittance

pytestmark = pytest.mark.gpu
DEV = "cuda"
PER_RAY = ("rays_o", "rays_d", "viewdirs")
NAMES = ("rgb", "fg_rgb", "bg_rgb", "fg_acc", "bg_lambda", "depth")
SHAPES = ((96, None), (300, 128))
N_LEVEL = (ac.N_COARSE + 1, ac.N_COARSE + 1 + ac.N_FINE)


def _net(precision=None, preproject=3):
    net = models.NeRF_TP(num_coarse_samples=ac.N_COARSE, num_fine_samples=ac.N_FINE, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(ac.state())
    sc = tc.scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV),
                  sc["image_wh"], preproject=preproject)
    if precision is not None:
        net.precision = precision
    return net


def _rays(n):
    return {k: v.to(DEV) for k, v in tc.rays(n).items()}


def _first(gb, n):
    return {k: (v[:n].contiguous() if k in PER_RAY else v) for k, v in gb.items()}


def _forward(net, gb, chunk):
    out = net(gb, False, False, 0.0, 0.0, out_depth=True, chunk=chunk)
    net.check_flags()
    return [[t.clone() for t in lv] for lv in out]


def _accelerated(net, gb, eps, chunk=None, segment=64, coarse=False):
    """[level 0 six, level 1 six, [(fg_t, fg_w, bg_s, stop, fg_keep, fg_rows) per level], kept int64[2], survivors int32], cloned."""
    out = net.render_accelerated(gb, eps, chunk=chunk, segment=segment, coarse=coarse, return_samples="rows")
    net.check_flags()
    return [[t.clone() for t in out[0]], [t.clone() for t in out[1]], [[t.clone() for t in lv] for lv in out[2]],
            net.last_accel_kept.clone(), net.last_accel_survivors.clone()]


def _terminating(net, gb, eps, chunk=None, segment=64, coarse=False):
    """As `_accelerated` from render_terminating: samples (fg_t, fg_w, bg_s, stop, fg_rows)."""
    out = net.render_terminating(gb, eps, chunk=chunk, segment=segment, coarse=coarse, return_samples="rows")
    net.check_flags()
    return [[t.clone() for t in out[0]], [t.clone() for t in out[1]], [[t.clone() for t in lv] for lv in out[2]],
            net.last_terminate_kept.clone(), net.last_terminate_survivors.clone()]


def _skipping(net, gb, chunk=None):
    """[level 0 six, level 1 six, [(fg_t, fg_w, bg_s, fg_keep, fg_rows) per level], kept int64[2]], cloned."""
    out = net.render_skipping(gb, chunk=chunk, return_samples="rows")
    net.check_flags()
    return [[t.clone() for t in out[0]], [t.clone() for t in out[1]], [[t.clone() for t in lv] for lv in out[2]], net.last_skip_kept.clone()]


def _flat(res):
    return [t for lv in res[:2] for t in lv] + [t for lv in res[2] for t in lv] + [res[3], res[4]]


def _same_results(x, y):
    return all(torch.equal(a, b) for a, b in zip(_flat(x), _flat(y)))


def _front(stop, N):
    return torch.arange(N, device=stop.device)[None, :] < stop[:, None]


def _stages(net, gb, chunk, positions=None, grid=None, eps=None, segment=64, coarse=False):
    """`_stages` of tests/test_gpu_terminate.py - the frame from public stage ops - with a grid: the rows of the samples that
    `ops.occupancy_keep` clears at positions[level] (the call's returned fg_t) are zero BEFORE `ops.termination_stops` and the
    inside-sphere composite; level 0 follows the stop rule only with coarse.  Returns (levels, stops, keeps, culled)."""
    o, d = gb["rays_o"], gb["rays_d"]
    t_far, _ = ops.intersect_sphere(o, d)
    fg_t, bg_s = net.sample_positions(gb, chunk)[0]
    n_fine = net.num_fine_samples
    parts, stops, keeps = [], [], []
    for level in range(2):
        fg = net.eval_mlp(level, gb, fg_t, chunk=chunk)
        bg = net.eval_mlp(2 + level, gb, bg_s, far=t_far, chunk=chunk)
        N = fg_t.shape[1]
        keep = torch.ones(o.shape[0], N, dtype=torch.bool, device=o.device)
        if grid is not None:
            keep = ops.occupancy_keep(grid, o, d, positions[level])
            fg = torch.where(keep[:, :, None], fg, torch.zeros_like(fg))
        stop = torch.full((o.shape[0],), N, dtype=torch.int32, device=o.device)
        if eps is not None and (level == 1 or coarse):
            stop, _ = ops.termination_stops(fg, fg_t, d, t_far, eps, segment)
            fg = tc.zero_behind(fg, stop)
        stops.append(stop)
        keeps.append(keep)
        f = ops.composite(1, fg, fg_t, d, t_far)
        b = ops.composite(2, bg, bg_s)
        parts.append((f, b))
        if level == 0:
            fg_t = ops.resample(fg_t, f["weights"], n_fine)
            bg_s = ops.resample(bg_s, b["weights"], n_fine, descending=True)
    culled = torch.zeros(o.shape[0], dtype=torch.bool, device=o.device)
    if eps is not None:
        culled = (parts[0][0]["bg_lambda"][:, 0] < eps) & (parts[1][0]["bg_lambda"][:, 0] < eps)
    out = []
    for f, b in parts:
        lam = f["bg_lambda"]
        bg_rgb = torch.where(culled[:, None], torch.zeros_like(b["rgb"]), b["rgb"])
        rgb = torch.where(culled[:, None], f["rgb"], f["rgb"] + lam * b["rgb"])
        depth = torch.where(culled, f["depth"], f["depth"] + lam[:, 0] * b["depth"])
        out.append([rgb, f["rgb"], bg_rgb, f["acc"], lam, depth])
    return out, stops, keeps, culled


def _assert_equals_chain(net, gb, chunk, got, forward, what, grid, eps, segment=64, coarse=False):
    """The rule of tests/test_gpu_edit.py: first the plain chain against plain `forward`; if that deviation is 0 the call equals
    its chain bitwise, otherwise within 4 x it.  The stops, the keep masks and the counts are integers: always equal."""
    parent = _stages(net, gb, chunk)[0]
    net.check_flags()
    worst = max(float((x - y).abs().max()) for lv in range(2) for x, y in zip(parent[lv], forward[lv]))
    want, stops, keeps, culled = _stages(net, gb, chunk, [got[2][0][0], got[2][1][0]], grid, eps, segment, coarse)
    net.check_flags()
    for lv in range(2):
        assert torch.equal(got[2][lv][3], stops[lv]), (what, lv)
        assert torch.equal(got[2][lv][4], keeps[lv]), (what, lv)
        for k, x, y in zip(NAMES, got[lv], want[lv]):
            err = float((x - y).abs().max())
            print("%s level %d %s: call against its stage chain %.3e (plain chain against forward: %.3e)" % (what, lv, k, err, worst))
            if worst == 0.0:
                assert torch.equal(x, y), (what, lv, k)
            else:
                assert err <= 4.0 * worst, (what, lv, k, err, worst)
    assert int(got[4]) == int((~culled).sum()), what
    evaluated = [int((keeps[lv] & _front(stops[lv], N_LEVEL[lv])).sum()) for lv in range(2)]
    assert got[3].tolist() == evaluated, what
    return stops, keeps, culled


_BASE = {}


def _module(n, chunk):
    """One default module per shape, its rays and its plain frame (never modified); no grid installed when handed out."""
    key = (n, chunk)
    if key not in _BASE:
        net = _net()
        gb = _rays(n)
        _BASE[key] = dict(net=net, gb=gb, forward=_forward(net, gb, chunk), frames={})
    return _BASE[key]


def _point(point, n=96, chunk=None, coarse=False):
    """The accelerated frame of an operating point with samples, cached; the module's grid is removed again."""
    base = _module(n, chunk)
    key = (point, coarse)
    if key not in base["frames"]:
        p = ac.POINTS[point]
        grid = p["grid"]()
        base["net"].set_occupancy(grid)
        try:
            base["frames"][key] = dict(grid=grid, eps=p["eps"], got=_accelerated(base["net"], base["gb"], p["eps"], chunk, coarse=coarse),
                                       skip=_skipping(base["net"], base["gb"], chunk))
        finally:
            base["net"].set_occupancy(None)
    return base, base["frames"][key]


# ---- 1. no grid: the terminating frame --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chunk", SHAPES)
def test_without_a_grid_and_with_an_all_ones_grid_it_is_bitwise_the_terminating_frame(n, chunk):
    base = _module(n, chunk)
    net, gb = base["net"], base["gb"]
    for eps in (0.0, 1e-2, 0.33):
        for coarse in (False, True):
            want = _terminating(net, gb, eps, chunk, coarse=coarse)
            for ones in (False, True):
                net.set_occupancy(oc.ones(32) if ones else None)
                try:
                    got = _accelerated(net, gb, eps, chunk, coarse=coarse)
                finally:
                    net.set_occupancy(None)
                what = (n, eps, coarse, ones)
                for lv in range(2):
                    assert len(got[lv]) == len(want[lv]) == 6
                    for k, x, y in zip(NAMES, got[lv], want[lv]):
                        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, lv, k)
                    fg_t, fg_w, bg_s, stop, fg_keep, fg_rows = got[2][lv]
                    for x, y in zip((fg_t, fg_w, bg_s, stop, fg_rows), want[2][lv]):
                        assert x.dtype == y.dtype and torch.equal(x, y), (what, lv)
                    assert fg_keep.dtype == torch.bool and tuple(fg_keep.shape) == (n, N_LEVEL[lv]) and bool(fg_keep.all())
                assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4]), what
            if eps == 0.0:
                for lv in range(2):
                    assert all(torch.equal(x, y) for x, y in zip(want[lv], base["forward"][lv])), "no grid and eps = 0: forward"


# ---- 2. eps = 0: the skipping frame -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,preproject,kernel", EVALUATORS, ids=["%s-pre%d-%s" % (p, int(m), k) for p, m, k in EVALUATORS])
def test_eps_zero_is_bitwise_the_skipping_frame(precision, preproject, kernel):
    net = _net(precision, preproject)
    net.set_occupancy(oc.mixed(32))
    for n, chunk in SHAPES:
        gb = _rays(n)
        want = _skipping(net, gb, chunk)
        for coarse in (False, True):
            got = _accelerated(net, gb, 0.0, chunk, coarse=coarse)
            for lv in range(2):
                for k, x, y in zip(NAMES, got[lv], want[lv]):
                    assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (n, lv, k, coarse)
                fg_t, fg_w, bg_s, stop, fg_keep, fg_rows = got[2][lv]
                for x, y in zip((fg_t, fg_w, bg_s, fg_keep, fg_rows), want[2][lv]):
                    assert x.dtype == y.dtype and torch.equal(x, y), (n, lv, coarse)
                assert bool((stop == N_LEVEL[lv]).all())
                assert 0 < int(fg_keep.sum()) < fg_keep.numel()
            assert torch.equal(got[3], want[3]) and int(got[4]) == n, (n, coarse)
    net.close()


# ---- 3. an empty grid -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chunk", SHAPES)
def test_all_zeros_grid_has_no_foreground_and_culls_nobody(n, chunk):
    base = _module(n, chunk)
    net, gb, forward = base["net"], base["gb"], base["forward"]
    net.set_occupancy(oc.zeros(32))
    try:
        for coarse in (False, True):
            got = _accelerated(net, gb, 0.33, chunk, coarse=coarse)
            for lv in range(2):
                rgb, fg_rgb, bg_rgb, fg_acc, lam, depth = got[lv]
                assert bool((fg_rgb == 0).all()) and bool((fg_acc == 0).all()) and bool((lam == 1).all())
                assert torch.equal(rgb, bg_rgb)
                assert torch.equal(bg_rgb, forward[lv][2]), "the outside-sphere half does not depend on the inside"
                fg_t, fg_w, bg_s, stop, fg_keep, fg_rows = got[2][lv]
                assert bool((stop == N_LEVEL[lv]).all()), "a transmittance of 1 never stops"
                assert not bool(fg_keep.any()) and bool((fg_w == 0).all()) and bool((fg_rows == 0).all())
            assert got[3].tolist() == [0, 0], "the zero-row compact launches"
            assert int(got[4]) == n, "nobody is culled"
    finally:
        net.set_occupancy(None)


# ---- 4. the operating points -------------------------------------------------------------------------------------------------------

POINT_CASES = (("A", 96, None, False), ("A", 96, None, True), ("B", 96, None, False), ("B", 300, 128, False))


@pytest.mark.parametrize("point,n,chunk,coarse", POINT_CASES)
def test_operating_point_equals_its_stage_chain(point, n, chunk, coarse):
    base, frame = _point(point, n, chunk, coarse)
    stops, keeps, culled = _assert_equals_chain(base["net"], base["gb"], chunk, frame["got"], base["forward"],
                                                "%s, %d rays, coarse %s" % (point, n, coarse), frame["grid"], frame["eps"], coarse=coarse)
    seen = ac.stop_counts(stops[1])
    skipped = int((~keeps[1] & _front(stops[1], N_LEVEL[1])).sum())
    print("%s, %d rays: level-1 stops %s, level-0 stops %s, %d culled, %d skipped in front of the stops"
          % (point, n, seen, ac.stop_counts(stops[0]), int(culled.sum()), skipped))
    # the mix of tests/test_accelerate_cpu.py, on the device's own stops
    if not coarse:
        assert set(seen) == ({64, 128, 135} if point == "A" else {128, 135})
        assert bool((stops[0] == N_LEVEL[0]).all())
    else:
        assert set(ac.stop_counts(stops[0])) == {64, 65}
    assert 0 < int(culled.sum()) < n and skipped > 0


@pytest.mark.parametrize("point,n,chunk,coarse", POINT_CASES)
def test_operating_point_rows_stops_counts_and_bounds(point, n, chunk, coarse):
    base, frame = _point(point, n, chunk, coarse)
    net, gb, got, skip, grid, eps = base["net"], base["gb"], frame["got"], frame["skip"], frame["grid"], frame["eps"]
    o, d = gb["rays_o"], gb["rays_d"]
    t_far2, _ = ops.intersect_sphere(o, d)
    t_far = t_far2[:, 0]
    lam0, lam1 = got[0][4][:, 0], got[1][4][:, 0]
    culled = (lam0 < eps) & (lam1 < eps)
    evaluated = []
    for lv in range(2):
        fg_t, fg_w, bg_s, stop, fg_keep, fg_rows = got[2][lv]
        N = N_LEVEL[lv]
        assert tuple(fg_t.shape) == tuple(fg_w.shape) == tuple(bg_s.shape) == tuple(fg_keep.shape) == (n, N)
        assert stop.dtype == torch.int32 and tuple(stop.shape) == (n,) and fg_keep.dtype == torch.bool and tuple(fg_rows.shape) == (n, N, 4)
        assert torch.equal(fg_keep, ops.occupancy_keep(grid, o, d, fg_t)), "fg_keep: the KEEP RULE on the whole row"
        if lv == 1 or coarse:
            own, trans = ops.termination_stops(fg_rows, fg_t, d, t_far2, eps, 64)
            assert torch.equal(stop, own), "stop: the STOP RULE on the returned rows"
            halted = stop < N
            assert torch.equal(got[lv][4][:, 0][halted], trans[halted]), "a stopped ray's bg_lambda is the transmittance at its stop"
        else:
            assert bool((stop == N).all())
        mask = fg_keep & _front(stop, N)
        rows = net.eval_mlp(lv, gb, fg_t, chunk=chunk)
        net.check_flags()
        assert torch.equal(fg_rows[mask], rows[mask]), "evaluated rows are eval_mlp's"
        assert bool((fg_rows[~mask] == 0).all()) and bool((fg_w[~mask] == 0).all())
        assert bool((rows[~mask][:, 3] > 0).any()), "the samples that were not evaluated had density"
        if lv == 1:
            assert bool((~fg_keep & _front(stop, N)).any()) and bool((fg_keep & ~_front(stop, N)).any()), "both rules drop samples"
            assert bool((bg_s[culled] == 0).all())
        evaluated.append(int(mask.sum()))
        assert bool((got[lv][2][culled] == 0).all()) and torch.equal(got[lv][0][culled], got[lv][1][culled])
    assert got[3].tolist() == evaluated and int(got[4]) == int((~culled).sum())
    # the grid moves stops: the terminating frame of the same eps stops elsewhere on some ray
    plain = _terminating(net, gb, eps, chunk, coarse=coarse)
    assert bool((plain[2][1][3] != got[2][1][3]).any())
    # fewer samples than the skipping frame, and fewer than the terminating frame would at the SAME stops (with the grid the
    # transmittance falls later, so the stops themselves may lie further back than without it)
    assert got[3][1] < skip[3][1] and got[3][1] < got[2][1][3].sum()
    if coarse:
        return                    # no bound is claimed
    # the header bound against render_skipping with the same grid: level 0, the level-1 positions and the masks are identical
    for x, y in zip(got[0][3:5], skip[0][3:5]):
        assert torch.equal(x, y)
    assert torch.equal(got[2][1][0], skip[2][1][0]) and torch.equal(got[2][1][4], skip[2][1][3]) and torch.equal(got[2][0][4], skip[2][0][3])
    stop1 = got[2][1][3]
    stopped = stop1 < N_LEVEL[1]
    assert int(stopped.sum()) > 0 and bool((lam1[stopped] < eps).all())
    either = stopped | culled
    d_rgb = (got[1][0] - skip[1][0]).abs().max(dim=-1).values
    d_depth = (got[1][5] - skip[1][5]).abs()
    print("%s, %d rays: %d stopped, %d culled; max |rgb change| / lambda = %.4f, max |depth change| / ((t_far + 1.001) lambda) = %.4f"
          % (point, n, int(stopped.sum()), int(culled.sum()), float((d_rgb / lam1)[either].max()),
             float((d_depth / ((t_far + 1.001) * lam1))[either].max())))
    assert bool((d_rgb[either] <= 1.003 * lam1[either]).all())
    assert bool((d_depth[either] <= (t_far[either] + 1.001) * lam1[either]).all())
    whole = ~either
    for lv in range(2):
        for k, x, y in zip(NAMES, got[lv], skip[lv]):
            assert torch.equal(x[whole], y[whole]), (lv, k)


# ---- 5. launch edges ---------------------------------------------------------------------------------------------------------------

def _grid_for_segment_count(o, d, t1, t0, want):
    """A G = 256 grid that keeps exactly `want` of the FIRST-segment level-1 positions t1[:, :64], none of the later ones and none
    of the level-0 positions t0: cells are added one sample at a time, a cell that holds another sample or would overshoot is
    passed over (`_grid_for_count` of tests/test_gpu_occupancy.py on one segment launch's candidates)."""
    G = 256

    def lin(t):
        c = oc.cell(oc.positions(o, d, t), G).reshape(-1, 3)
        return (c[:, 0] * G + c[:, 1]) * G + c[:, 2]
    lin1 = lin(t1[:, :64])
    taken = set(lin(t0).tolist()) | set(lin(t1[:, 64:]).tolist())
    grid = oc.zeros(G)
    count = 0
    for cell_lin in lin1.tolist():
        if count == want:
            break
        if cell_lin in taken:
            continue
        here = int((lin1 == cell_lin).sum())
        taken.add(cell_lin)
        if count + here > want:
            continue
        grid.view(-1)[cell_lin] = True
        count += here
    assert count == want, (count, want)
    return grid


@pytest.mark.parametrize("rays,want", [(1, 0), (1, 1), (3, 63), (3, 64), (3, 65), (1, "all")])
def test_kept_counts_of_one_segment_launch(rays, want):
    """Grids at G = 256 built from the rays' own level-1 positions: the first segment launch of level 1 (rays x 64 candidates) holds
    exactly `want` kept points, every later one none.  With every level-0 sample skipped the level-0 weights are zero whatever
    else the grid holds, so the level-1 positions are those of the all-zeros grid and the counts are known exactly."""
    base = _module(96, None)
    net = base["net"]
    gb = _first(base["gb"], rays)
    forward = _forward(net, gb, None)
    eps = 0.33
    try:
        if want == "all":
            grid = oc.ones(256)
            net.set_occupancy(grid)
            got = _accelerated(net, gb, eps)
            assert int(got[3][0]) == rays * N_LEVEL[0] and int(got[3][1]) == int(got[2][1][3].sum())
        else:
            net.set_occupancy(oc.zeros(256))
            empty = _accelerated(net, gb, eps)
            o, d = gb["rays_o"].cpu(), gb["rays_d"].cpu()
            t0, t1 = empty[2][0][0].cpu(), empty[2][1][0].cpu()
            assert int(oc.near_face(o, d, t1, 256).sum()) == 0, "a position on a face of the finest grid: the count would not be exact"
            grid = _grid_for_segment_count(o, d, t1, t0, want)
            net.set_occupancy(grid)
            got = _accelerated(net, gb, eps)
            assert torch.equal(got[2][1][0], empty[2][1][0]), "the level-1 positions are those of the empty grid"
            keep1 = got[2][1][4]
            assert int(keep1[:, :64].sum()) == want and int(keep1[:, 64:].sum()) == 0
            assert got[3].tolist() == [0, want]
    finally:
        net.set_occupancy(None)
    _assert_equals_chain(net, gb, None, got, forward, "%d rays, %s kept" % (rays, want), grid, eps)


@pytest.mark.parametrize("alive", (0, 1, 2, "all"))
def test_alive_counts_of_the_second_segment_launch(alive):
    """eps between consecutive sorted boundary transmittances of the rays' own MASKED rows: exactly `alive` rays march past sample
    64 of level 1 (level 0 obeys the grid only, so the level-1 positions do not depend on eps).  Point B's grid: its checkerboard
    leaves every ray kept samples in the first segment, so the transmittances are distinct (under point A's grid whole first
    segments are skipped and several rays tie at exactly 1)."""
    base, frame = _point("B")
    net, gb, grid = base["net"], base["gb"], frame["grid"]
    o, d = gb["rays_o"], gb["rays_d"]
    fg_t1 = frame["got"][2][1][0]
    t_far, _ = ops.intersect_sphere(o, d)
    rows = net.eval_mlp(1, gb, fg_t1)
    rows = torch.where(ops.occupancy_keep(grid, o, d, fg_t1)[:, :, None], rows, torch.zeros_like(rows))
    tb = _boundary_transmittance(rows, fg_t1, d, t_far, 64).sort(descending=True).values
    assert bool((tb[:3] > tb[1:4]).all()) and float(tb[0]) < 0.998, "distinct values at the top"
    if alive == "all":
        eps, count = float(tb[-1]), 96                 # !(T < eps) holds for the smallest as well
    elif alive == 0:
        eps, count = float(tb[0]) + 1e-3, 0
    else:
        eps, count = float((tb[alive - 1].double() + tb[alive].double()) / 2), alive
    net.set_occupancy(grid)
    try:
        got = _accelerated(net, gb, eps)
    finally:
        net.set_occupancy(None)
    assert int((got[2][1][3] > 64).sum()) == count
    assert torch.equal(got[2][1][0], fg_t1)
    _assert_equals_chain(net, gb, None, got, base["forward"], "%s alive" % alive, grid, eps)


# ---- 6. windows, chunk, segment ------------------------------------------------------------------------------------------------------

def test_windows_and_segment_do_not_change_the_composition():
    base, frame = _point("B", 300, 128)
    net, gb, grid, eps = base["net"], base["gb"], frame["grid"], frame["eps"]
    assert net.skip_window is None
    net.set_occupancy(grid)
    try:
        wide = _accelerated(net, gb, eps, 128, segment=128)
        coarse = _accelerated(net, gb, 0.33, 128, coarse=True)
        for window in (1, 128, 299):           # two rays a level-1 window; a ragged last window; one ray left over
            net.skip_window = window
            assert _same_results(_accelerated(net, gb, eps, 128), frame["got"]), window
            assert _same_results(_accelerated(net, gb, eps, 128, segment=128), wide), window
            assert _same_results(_accelerated(net, gb, 0.33, 128, coarse=True), coarse), window
            net.skip_window = None
    finally:
        net.skip_window = None
        net.set_occupancy(None)
    stops, _, _ = _assert_equals_chain(net, gb, 128, wide, base["forward"], "segment 128", grid, eps, segment=128)
    assert set(stops[1].tolist()) == {128, 135}


def test_chunk_decides_the_direction_rows_as_in_forward():
    """chunk = 128 on 300 rays equals its stage chain at that chunk (test_operating_point_equals_its_stage_chain[B-300-128]) - and
    is not the one-chunk frame, exactly as `forward`: the point rows carry the quirk-Q1 directions of their reference chunk."""
    base, frame = _point("B", 300, 128)
    net, gb, grid, eps = base["net"], base["gb"], frame["grid"], frame["eps"]
    net.set_occupancy(grid)
    try:
        other = _accelerated(net, gb, eps, None)
    finally:
        net.set_occupancy(None)
    forward = _forward(net, gb, None)
    assert not torch.equal(forward[1][1], base["forward"][1][1]), "forward depends on the chunk through the direction rows"
    assert not torch.equal(other[1][1], frame["got"][1][1])
    _assert_equals_chain(net, gb, None, other, forward, "300 rays, one chunk", grid, eps)


# ---- 7. non-finite inputs, on caller rows ----------------------------------------------------------------------------------------------

def test_a_non_finite_position_is_kept_and_a_nan_density_marches_on():
    occ, o, d, t = oc.classifier_case(16, 200, 32, 11)
    o, d, t = o.to(DEV), d.to(DEV), t.to(DEV)
    wild = ~torch.isfinite(oc.positions(o, d, t)).all(dim=-1)
    assert int(wild.sum()) >= 3
    assert torch.equal(ops.occupancy_keep(oc.zeros(32), o, d, t), wild), "under an empty grid exactly the non-finite positions are kept"
    keep = ops.occupancy_keep(occ, o, d, t)
    assert bool(keep[wild].all()) and 0 < int(keep.sum()) < keep.numel()
    # the stop rule on masked rows: a NaN density that the grid keeps makes the transmittance NaN, which marches on
    g = torch.Generator().manual_seed(5)
    tt = torch.sort(torch.rand(16, 200, generator=g), dim=-1).values.to(DEV)
    rows = torch.rand(16, 200, 4, generator=g).to(DEV)
    rows[..., 3] *= 20.0
    rows[0, 3, 3] = float("nan")
    keep[0, 3] = True
    masked = torch.where(keep[:, :, None], rows, torch.zeros_like(rows))
    far = torch.full((16, 1), 1.5, device=DEV)
    stop, trans = ops.termination_stops(masked, tt, d, far, 0.5)
    assert int(stop[0]) == 200 and bool(torch.isnan(trans[0])), "a NaN keeps marching"
    assert bool((stop[1:] < 200).any()), "ordinary rays stop"
    none = torch.zeros_like(rows)
    stop, trans = ops.termination_stops(none, tt, d, far, 0.5)
    assert bool((stop == 200).all()) and bool((trans == 1).all()), "rows that are all skipped never stop"


# ---- 8. repeatability, ordering, life cycle ---------------------------------------------------------------------------------------------

def test_calls_are_repeatable_overlap_and_loop_neutral_and_synchronise_nothing():
    base, frame = _point("A")
    net, gb, grid, eps = base["net"], base["gb"], frame["grid"], frame["eps"]
    net.set_occupancy(grid)
    try:
        assert _same_results(_accelerated(net, gb, eps), frame["got"])
        assert net.overlap_calls
        net.overlap_calls = False
        try:
            off = _accelerated(net, gb, eps)
        finally:
            net.overlap_calls = True
        assert _same_results(off, frame["got"])
        # the reference-style loop: three calls of 32 rays, each one reference chunk, in flight on alternating lanes; no blocking wait
        whole = _accelerated(net, gb, eps, 32)
        ctx = net._context(torch.device(DEV))
        before = ctx.sync_count()
        parts, kept, survivors = [], [], []
        for i in range(0, 96, 32):
            part = {k: (v[i:i + 32] if k in PER_RAY else v) for k, v in gb.items()}
            parts.append(net.render_accelerated(part, eps, chunk=32, return_samples="rows"))
            kept.append(net.last_accel_kept)
            survivors.append(net.last_accel_survivors)
        assert ctx.sync_count() == before, "an accelerated call blocked on the device"
        net.check_flags()
        for lv in range(2):
            for j in range(6):
                assert torch.equal(torch.cat([p[lv][j] for p in parts]), whole[lv][j]), (lv, j)
                assert torch.equal(torch.cat([p[2][lv][j] for p in parts]), whole[2][lv][j]), (lv, j)
        assert torch.equal(sum(kept), whole[3]) and int(sum(survivors)) == int(whole[4])
        # neither cull_background nor compute_extras is read; forward is unchanged by the call
        net.cull_background = 0.5
        net.compute_extras = True
        try:
            same = _accelerated(net, gb, eps)
        finally:
            net.cull_background = None
            net.compute_extras = False
        assert len(same[0]) == len(same[1]) == 6 and _same_results(same, frame["got"])
        after = _forward(net, gb, None)
        for lv in range(2):
            assert all(torch.equal(x, y) for x, y in zip(after[lv], base["forward"][lv]))
        # the frame helper: the fine level, the kept fractions and the culled fraction
        helper = render.render_accelerated_rays(net, gb, eps, chunk=96)
        got = frame["got"]
        assert torch.equal(helper["rgb"], got[1][0]) and torch.equal(helper["depth"], got[1][5]) and torch.equal(helper["acc"], got[1][3])
        frac, gone = helper["kept_fraction"], helper["culled_fraction"]
        assert frac.is_cuda and frac.dtype == torch.float64 and tuple(frac.shape) == (2,) and gone.is_cuda and gone.dtype == torch.float64
        assert all(abs(float(frac[lv]) - int(got[3][lv]) / (96 * N_LEVEL[lv])) < 1e-12 for lv in range(2)) and 0.0 < float(frac[1]) < 1.0
        assert abs(float(gone) - (96 - int(got[4])) / 96) < 1e-12
        skipping = render.render_skipping_rays(net, gb, chunk=96)
        zero = render.render_accelerated_rays(net, gb, 0.0, chunk=96)
        assert torch.equal(zero["rgb"], skipping["rgb"]) and torch.equal(zero["depth"], skipping["depth"])
        assert torch.equal(zero["kept_fraction"], skipping["kept_fraction"]) and float(zero["culled_fraction"]) == 0.0
    finally:
        net.set_occupancy(None)


def test_set_scene_drops_the_grid_and_a_grid_of_another_context_is_refused():
    net = _net()
    gb = _rays(96)
    eps = ac.POINTS["A"]["eps"]
    want = _terminating(net, gb, eps)
    grid = ac.POINTS["A"]["grid"]()
    net.set_occupancy(grid)
    with_grid = _accelerated(net, gb, eps)
    assert not torch.equal(with_grid[1][0], want[1][0]) and not torch.equal(with_grid[2][1][3], want[2][1][3]), "the grid matters"
    sc = tc.scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV), sc["image_wh"])
    assert net.occupancy is None, "set_scene clears the grid: it describes one scene"
    got = _accelerated(net, gb, eps)               # no error: without a grid it is the terminating frame
    for lv in range(2):
        assert all(torch.equal(x, y) for x, y in zip(got[lv], want[lv])), lv
        assert torch.equal(got[2][lv][3], want[2][lv][3]) and bool(got[2][lv][4].all())
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])
    # a grid that was installed into another context than the one the call runs in (the module's record of it says so): refused
    # with render_skipping's error, before the library is called
    net.set_occupancy(grid)
    mine = net._occ_ctx
    net._occ_ctx = object()
    try:
        with pytest.raises(_lib.NeoError, match="does not belong"):
            net.render_accelerated(gb, eps)
        with pytest.raises(_lib.NeoError, match="does not belong"):
            net.render_skipping(gb)
    finally:
        net._occ_ctx = mine
    assert _same_results(_accelerated(net, gb, eps), with_grid)
    net.close()


# ---- 9. rejects and R == 0 ---------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_on_the_host_and_no_rays_is_a_valid_call():
    """Every refused call here returns an error before anything is launched: no kernel sees one of these pointers or shapes."""
    base = _module(96, None)
    net, gb = base["net"], base["gb"]
    c = net._context(torch.device(DEV))
    lib, h, s = c.lib, c.handle, c.stream()

    def refused(rc, text):
        assert rc != 0
        msg = lib.neo_last_error().decode()
        assert text in msg, msg
    poses, NV, focal, cx, cy = net._camera_args(gb)
    o, d, v = (gb[k].data_ptr() for k in PER_RAY)
    lvl = _lib.TpLevelOut()
    kept = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    survivors = torch.full((), 7, dtype=torch.int32, device=DEV)
    frame = lambda R=96, chunk=96, nc=ac.N_COARSE, nf=ac.N_FINE, o=o, nv=NV, eps=0.1, seg=64, ctx=h: lib.neo_tp_render_accelerated(
        ctx, o, d, v, R, chunk, poses, nv, focal, cx, cy, nc, nf, ctypes.byref(lvl), ctypes.byref(lvl), eps, seg, 0, None, None,
        kept.data_ptr(), survivors.data_ptr(), s)
    refused(frame(ctx=None), "null context")
    refused(frame(R=-1, eps=2.0), "bad ray count / chunk")
    refused(frame(chunk=0), "bad ray count / chunk")
    refused(frame(nc=2, eps=2.0), "unsupported sample counts")
    for eps in (-0.1, 1.0, float("nan")):
        refused(frame(eps=eps, o=None), "eps must lie in [0, 1)")
        refused(frame(eps=eps, R=0), "eps must lie in [0, 1)")
    for seg in (0, 32, 65, -128):
        refused(frame(seg=seg, o=None), "segment must be a positive multiple of 64")
    refused(frame(o=None), "null pointer")
    refused(frame(nv=NV + 1), "NV differs from the uploaded scene")
    assert kept.tolist() == [7, 7] and int(survivors) == 7, "a refused call writes nothing"
    assert frame(R=0) == 0
    torch.cuda.synchronize()
    assert kept.tolist() == [0, 0] and int(survivors) == 0
    assert c.poll_flags() == 0
    # Python: no rays, with and without a grid
    none = _first(gb, 0)
    for grid in (None, oc.mixed(32)):
        net.set_occupancy(grid)
        try:
            out = net.render_accelerated(none, 0.1, return_samples=True)
        finally:
            net.set_occupancy(None)
        assert tuple(out[1][0].shape) == (0, 3) and tuple(out[2][1][3].shape) == (0,) and tuple(out[2][1][4].shape) == (0, N_LEVEL[1])
        assert net.last_accel_kept.tolist() == [0, 0] and int(net.last_accel_survivors) == 0
    with pytest.raises(ValueError):
        net.render_accelerated(gb, 1.0)
    with pytest.raises(ValueError):
        net.render_accelerated(gb, 0.1, segment=96)
