"""GPU: early ray termination carried through the outside-sphere march of the NeO-360 frame (`NeRF_TP.render_marching`,
neo_tp_render_marching), its stop rule on caller rows (`ops.termination_stops_outside`) and the frame helper
(`render.render_marching_rays`).

Scene, state, eps and sample counts: tests/terminate_cases.py's own (cases.small_scene(), foreground density bias +4, EPS = 1e-2,
65 and 135 samples, segment 64, the 96 strided rays), on which tests/test_march_outside_cpu.py asserts the mix on the oracle: 61
rays culled, 35 survivors whose level-1 outside stops are 64, 128 and 135.  The mix is asserted again on the device's own stops
wherever a test relies on it.

Bounds.  An evaluated outside sample is computed by the same machine code as in the dense launch (test 1 asserts that for the
single-point launch), a sample behind bg_stop is a row of zeros, and the stop is a comparison of one fp32 product of two values the
composites define bit for bit: every comparison is `torch.equal` - the stop against the rule rebuilt from neo_composite mode 2, the
kept rows against `eval_mlp`, the whole call against the chain of public stage ops by the rule of tests/test_gpu_edit.py (bitwise
when that chain is bitwise `forward`, else within 4 x its deviation from it).  The a-priori bound of the header (1.003 eps for the
level-1 rgb and depth) is asserted against the same call with outside=False."""
import ctypes

import pytest
import torch

import cases
import march_outside_cases as mc
import occupancy_cases as oc
import terminate_cases as tc
import test_gpu_terminate as tg
from neo360_amd import _lib, models, ops, render
from neo360_amd.ops import ptr
from test_gpu_objects import EVALUATORS

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = tg.NAMES
PER_RAY = tg.PER_RAY
N_LEVEL = tg.N_LEVEL
IDS = ["%s-pre%d-%s" % (p, int(m), k) for p, m, k in EVALUATORS]
FG_T, FG_W, BG_S, STOP, FG_KEEP, BG_STOP, BG_VALUE, FG_ROWS, BG_ROWS = range(9)


def _marching(net, gb, eps, chunk=None, segment=64, coarse=False, outside=True, grid=True):
    """[level 0 six, level 1 six, [(fg_t, fg_w, bg_s, stop, fg_keep, bg_stop, bg_value, fg_rows, bg_rows) per level], kept int64[4],
    survivors int32], cloned."""
    out = net.render_marching(gb, eps, chunk=chunk, segment=segment, coarse=coarse, outside=outside, grid=grid, return_samples="rows")
    net.check_flags()
    return [[t.clone() for t in out[0]], [t.clone() for t in out[1]], [[t.clone() for t in lv] for lv in out[2]],
            net.last_march_kept.clone(), net.last_march_survivors.clone()]


def _flat(res):
    return [t for lv in res[:2] for t in lv] + [t for lv in res[2] for t in lv] + [res[3], res[4]]


def _all_equal(a, b):
    return all(tg._same(x, y) for x, y in zip(_flat(a), _flat(b)))


def _bg_transmittance(rows, s, b=None):
    """(float)carry_b of neo_composite mode 2, through its lambda pointer (ops.composite passes none in mode 2): the composite of
    rows [0, b] with row b zeroed returns the product over rows [0, b) - the zeroed last sample, whose delta is 1e10, contributes
    alpha(0 * 1e10) = 0 and a factor (1 - 0) + 1e-10f == 1.0f.  b None: the product over all rows."""
    if b is not None:
        rows = rows[:, :b + 1].clone()
        rows[:, b] = 0
        s = s[:, :b + 1]
    rows, s = rows.contiguous().float(), s.contiguous().float()
    R, N = s.shape
    ctx = ops._ctx(s, None)
    lam = torch.empty(R, device=s.device)
    _lib.check(ctx.lib.neo_composite(ctx.handle, 2, ptr(rows), ptr(s), None, None, R, N, 0, None, None, None, None, ptr(lam), ctx.stream()))
    return lam


def _rule(rows, s, lam, eps, segment):
    """The OUTSIDE STOP RULE from neo_composite mode 2 and one torch fp32 multiply: (stop (R,) long, value (R,))."""
    R, N = s.shape
    lam = lam.reshape(R)
    stop = torch.full((R,), N, dtype=torch.long, device=s.device)
    value = lam * _bg_transmittance(rows, s)
    alive = torch.ones(R, dtype=torch.bool, device=s.device)
    for b in tc.boundaries(N, segment):
        vb = lam * _bg_transmittance(rows, s, b)
        halt = alive & (vb < eps)
        stop[halt] = b
        value[halt] = vb[halt]
        alive &= ~halt
    return stop, value


def _stages(net, gb, chunk, eps=None, segment=64, coarse=False, outside=True):
    """tests/test_gpu_terminate.py's `_stages`, extended: with eps and `outside` the outside rows at j >= bg_stop are zero before the
    outside-sphere composite (bg_stop: `ops.termination_stops_outside` on the chain's own rows and lambdas; level 0 only with
    coarse), and the cull is taken from the chain's own lambdas.  Returns (levels, stops, bg_stops, culled)."""
    o, d = gb["rays_o"], gb["rays_d"]
    t_far, _ = ops.intersect_sphere(o, d)
    fg_t, bg_s = net.sample_positions(gb, chunk)[0]
    n_fine = net.num_fine_samples
    parts, stops, bg_stops = [], [], []
    for level in range(2):
        fg = net.eval_mlp(level, gb, fg_t, chunk=chunk)
        bg = net.eval_mlp(2 + level, gb, bg_s, far=t_far, chunk=chunk)
        N = fg_t.shape[1]
        stop = torch.full((o.shape[0],), N, dtype=torch.int32, device=o.device)
        if eps is not None and (level == 1 or coarse):
            stop, _ = ops.termination_stops(fg, fg_t, d, t_far, eps, segment)
            fg = tc.zero_behind(fg, stop)
        f = ops.composite(1, fg, fg_t, d, t_far)
        bg_stop = torch.full((o.shape[0],), N, dtype=torch.int32, device=o.device)
        if eps is not None and outside and (level == 1 or coarse):
            bg_stop, _ = ops.termination_stops_outside(bg, bg_s, f["bg_lambda"], eps, segment)
            bg = tc.zero_behind(bg, bg_stop)
        b = ops.composite(2, bg, bg_s)
        stops.append(stop)
        bg_stops.append(bg_stop)
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
    bg_stops = [torch.where(culled, torch.zeros_like(s), s) for s in bg_stops]
    return out, stops, bg_stops, culled


def _assert_equals_chain(net, gb, chunk, got, forward, what, eps, segment=64, coarse=False):
    parent, _, _, _ = _stages(net, gb, chunk)
    net.check_flags()
    worst = max(float((x - y).abs().max()) for lv in range(2) for x, y in zip(parent[lv], forward[lv]))
    want, stops, bg_stops, culled = _stages(net, gb, chunk, eps, segment, coarse)
    net.check_flags()
    for lv in range(2):
        assert torch.equal(got[2][lv][STOP], stops[lv]), (what, lv)
        assert torch.equal(got[2][lv][BG_STOP], bg_stops[lv]), (what, lv)
        for k, x, y in zip(NAMES, got[lv], want[lv]):
            err = float((x - y).abs().max())
            print("%s level %d %s: call against its stage chain %.3e (plain chain against forward: %.3e)" % (what, lv, k, err, worst))
            if worst == 0.0:
                assert torch.equal(x, y), (what, lv, k)
            else:
                assert err <= 4.0 * worst, (what, lv, k, err, worst)
    assert int(got[4]) == int((~culled).sum()), what
    assert got[3].tolist() == [int(stops[0].sum()), int(stops[1].sum()), int(bg_stops[0].sum()), int(bg_stops[1].sum())], what
    return bg_stops, culled


_BASE = {}


def _base(n=96, chunk=None):
    """One default module without a grid, its plain frame, and its marching frames with and without the outside rule (never modified)."""
    key = (n, chunk)
    if key not in _BASE:
        net = tg._net()
        gb = tg._rays(n)
        _BASE[key] = dict(net=net, gb=gb, forward=tg._forward(net, gb, chunk), mixed=_marching(net, gb, mc.EPS, chunk, grid=False),
                          inside=_marching(net, gb, mc.EPS, chunk, outside=False, grid=False))
    return _BASE[key]


# ---- 1. precondition: the outside single-point launch equals the dense launch ---------------------------------------------------

@pytest.mark.parametrize("precision,preproject,kernel", EVALUATORS, ids=IDS)
def test_outside_single_point_launch_is_bitwise_the_dense_launch(precision, preproject, kernel):
    net = tg._net(precision, preproject)
    for n, chunk in ((96, None), (160, 128)):
        gb = tg._rays(n)
        o, d, v = (gb[k] for k in PER_RAY)
        t_far, _ = ops.intersect_sphere(o, d)
        positions = net.sample_positions(gb, chunk)
        for slot, bg_s in ((2, positions[0][1]), (3, positions[1][1])):
            N = bg_s.shape[1]
            dense = net.eval_mlp(slot, gb, bg_s, far=t_far, chunk=chunk)
            net.check_flags()
            rays_of = torch.tensor([0, 5, n - 31, n - 1], device=DEV)
            r = rays_of.repeat_interleave(N)
            j = torch.arange(N, device=DEV).repeat(len(rays_of))
            c = chunk or n
            c0 = (r // c) * c
            bc = torch.clamp(n - c0, max=c)
            dray = c0 + ((r - c0) * N + j) % bc
            for first, P in ((0, len(r)), (N, 1), (N, 63), (N, 64), (N, 65)):          # whole rows of four rays; P points of ray 5's row
                sel = slice(first, first + P)
                pb = dict(gb, rays_o=o[r[sel]].contiguous(), rays_d=d[r[sel]].contiguous(), viewdirs=v[dray[sel]].contiguous())
                got = net.eval_mlp(slot, pb, bg_s[r[sel], j[sel]][:, None].contiguous(), far=t_far[r[sel]].contiguous(), chunk=chunk)
                net.check_flags()
                assert torch.equal(got[:, 0], dense[r[sel], j[sel]]), (kernel, n, chunk, slot, P)
    net.close()


# ---- 2. the stop rule is the composite's own -----------------------------------------------------------------------------------

RULE_CASES = [(n0, n1, R) for n0, n1 in ((4, 5), (65, 135)) for R in (1, 7, 96)] + [(129, 385, 7)]


@pytest.mark.parametrize("n0,n1,R", RULE_CASES)
def test_outside_stop_rule_is_the_composites_own_transmittance(n0, n1, R):
    net = tg._net(n_coarse=n0 - 1, n_fine=n1 - n0)
    gb = tg._first(tg._rays(96), R)
    t_far, _ = ops.intersect_sphere(gb["rays_o"], gb["rays_d"])
    positions = net.sample_positions(gb, None)
    fwd = tg._forward(net, gb, None)
    seen = set()
    for lv in range(2):
        s = positions[lv][1]
        rows = net.eval_mlp(2 + lv, gb, s, far=t_far)
        net.check_flags()
        lam = fwd[lv][4][:, 0].contiguous()
        N = s.shape[1]
        for segment in (64, 128):
            bounds = tc.boundaries(N, segment)
            picks = [0.0, 0.999]
            if bounds:
                vb = lam * _bg_transmittance(rows, s, bounds[0])
                picks += [float(vb.median()), float(vb.min()), float(vb.max())]
            for eps in picks:
                eps = min(max(eps, 0.0), 0.999)
                want_stop, want_value = _rule(rows, s, lam, eps, segment)
                stop, value = ops.termination_stops_outside(rows, s, lam, eps, segment)
                assert stop.dtype == torch.int32 and tuple(stop.shape) == (R,) and tuple(value.shape) == (R,)
                assert torch.equal(stop.long(), want_stop), (lv, segment, eps)
                assert torch.equal(value, want_value), (lv, segment, eps)
                seen |= set(stop.tolist())
                if not bounds:
                    assert bool((stop == N).all())
    if n1 > 64:
        assert len(seen) >= (2 if R > 1 else 1)
    net.close()


def test_outside_rule_with_nan_and_infinite_densities():
    g = torch.Generator().manual_seed(5)
    R, N = 8, 200
    s = torch.sort(torch.rand(R, N, generator=g), dim=-1, descending=True).values.to(DEV)
    rows = torch.rand(R, N, 4, generator=g).to(DEV)
    rows[..., 3] *= 30.0
    lam = torch.full((R,), 0.5, device=DEV)
    rows[0, 3, 3] = float("nan")           # a NaN density: the running value is NaN from there on
    rows[1, 70, 3] = float("nan")          # ... behind the first boundary
    rows[2, 5, 3] = float("inf")           # alpha = 1: the transmittance is 1e-10 times the rest
    rows[3, 5, 3] = float("-inf")          # a transmittance of +inf
    s[4, 6] = s[4, 5]
    rows[4, 5, 3] = float("inf")           # inf * 0: NaN
    lam[5] = float("nan")                  # a NaN lambda
    for segment in (64, 128):
        for eps in (1e-3, 0.3):
            stop, value = ops.termination_stops_outside(rows, s, lam, eps, segment)
            want_stop, want_value = _rule(rows, s, lam, eps, segment)
            assert torch.equal(stop.long(), want_stop) and tg._same(value, want_value), (segment, eps)
            assert int(stop[0]) == N and bool(torch.isnan(value[0])), "a NaN keeps marching"
            assert int(stop[3]) == N and float(value[3]) == float("inf") and int(stop[4]) == N and bool(torch.isnan(value[4]))
            assert int(stop[5]) == N and bool(torch.isnan(value[5]))
            assert int(stop[2]) == segment and float(value[2]) < 1e-9, "+inf over a positive step is opaque: the composite says so"
            assert bool((stop[6:] < N).any()), "ordinary dense rows stop"


# ---- 3. eps = 0: the dense frame ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,preproject,kernel", EVALUATORS, ids=IDS)
def test_eps_zero_is_bitwise_forward(precision, preproject, kernel):
    net = tg._net(precision, preproject)
    for n, chunk in tg.SHAPES:
        gb = tg._rays(n)
        want = tg._forward(net, gb, chunk)
        for coarse in (False, True):
            got = _marching(net, gb, 0.0, chunk, coarse=coarse)
            for lv in range(2):
                assert len(got[lv]) == len(want[lv]) == 6
                for k, x, y in zip(NAMES, got[lv], want[lv]):
                    assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (n, lv, k, coarse)
                assert bool((got[2][lv][STOP] == N_LEVEL[lv]).all()) and bool((got[2][lv][BG_STOP] == N_LEVEL[lv]).all())
            assert got[3].tolist() == [n * N_LEVEL[0], n * N_LEVEL[1]] * 2 and int(got[4]) == n
    net.close()


# ---- 4. outside=False: the two older calls ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_grid", (False, True))
def test_outside_false_is_bitwise_the_older_call(with_grid):
    base = _base(300, 128)
    net, gb = base["net"], base["gb"]
    for coarse in (False, True):
        if with_grid:
            net.set_occupancy(oc.mixed(32))
        try:
            got = _marching(net, gb, mc.EPS, 128, coarse=coarse, outside=False, grid=with_grid)
            if with_grid:
                want = net.render_accelerated(gb, mc.EPS, chunk=128, coarse=coarse, return_samples="rows")
                kept, survivors = net.last_accel_kept.clone(), net.last_accel_survivors.clone()
                names = (FG_T, FG_W, BG_S, STOP, FG_KEEP, FG_ROWS)
            else:
                want = net.render_terminating(gb, mc.EPS, chunk=128, coarse=coarse, return_samples="rows")
                kept, survivors = net.last_terminate_kept.clone(), net.last_terminate_survivors.clone()
                names = (FG_T, FG_W, BG_S, STOP, FG_ROWS)
            net.check_flags()
        finally:
            net.set_occupancy(None)
        culled = (got[0][4][:, 0] < mc.EPS) & (got[1][4][:, 0] < mc.EPS)
        for lv in range(2):
            for k, x, y in zip(NAMES, got[lv], want[lv]):
                assert torch.equal(x, y), (with_grid, coarse, lv, k)
            for i, y in zip(names, want[2][lv]):
                assert torch.equal(got[2][lv][i], y), (with_grid, coarse, lv, i)
            # the outside outputs of a level that does not follow the rule: N for a survivor, 0 for a culled ray
            assert torch.equal(got[2][lv][BG_STOP], torch.where(culled, 0, N_LEVEL[lv]).int())
            assert bool((got[2][lv][BG_ROWS][culled] == 0).all()) and bool((got[2][lv][BG_VALUE][culled] == 0).all())
        assert torch.equal(got[3][:2], kept) and torch.equal(got[4], survivors)
        assert got[3][2:].tolist() == [int(survivors) * N_LEVEL[0], int(survivors) * N_LEVEL[1]]


# ---- 5. the mixed frame ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chunk", tg.SHAPES)
def test_mixed_frame_equals_its_stage_chain(n, chunk):
    base = _base(n, chunk)
    bg_stops, culled = _assert_equals_chain(base["net"], base["gb"], chunk, base["mixed"], base["forward"], "%d rays" % n, mc.EPS)
    seen = set(bg_stops[1][~culled].tolist())
    print("%d rays: level-1 outside stops %s, %d culled" % (n, {s: int((bg_stops[1][~culled] == s).sum()) for s in sorted(seen)}, int(culled.sum())))
    assert 0 < int(culled.sum()) < n
    if n == 96:
        assert seen == {64, 128, 135}, "the mix of tests/test_march_outside_cpu.py"
    else:
        assert len(seen) >= 2 and min(seen) < 135


@pytest.mark.parametrize("n,chunk", tg.SHAPES)
def test_mixed_frame_rows_weights_bounds_and_counts(n, chunk):
    base = _base(n, chunk)
    net, gb, got, inside = base["net"], base["gb"], base["mixed"], base["inside"]
    t_far, _ = ops.intersect_sphere(gb["rays_o"], gb["rays_d"])
    lam0, lam1 = got[0][4][:, 0], got[1][4][:, 0]
    culled = (lam0 < mc.EPS) & (lam1 < mc.EPS)
    assert int(got[4]) == int((~culled).sum())
    for lv in range(2):
        smp = got[2][lv]
        N = N_LEVEL[lv]
        bg_s, bg_stop, bg_value, bg_rows = smp[BG_S], smp[BG_STOP], smp[BG_VALUE], smp[BG_ROWS]
        assert bg_stop.dtype == torch.int32 and tuple(bg_stop.shape) == tuple(bg_value.shape) == (n,) and tuple(bg_rows.shape) == (n, N, 4)
        assert bool((bg_stop[culled] == 0).all()) and bool((bg_value[culled] == 0).all()) and bool((bg_rows[culled] == 0).all())
        live = ~culled
        assert bool(((bg_stop[live] == N) | ((bg_stop[live] % 64 == 0) & (bg_stop[live] > 0))).all())
        if lv == 0:
            assert bool((bg_stop[live] == N).all()), "coarse=False: level 0 is marched in full"
        # the level-1 bg_s row of a culled ray is zero; a survivor's is forward's (level 0 is marched in full): evaluate at those
        idx = live.nonzero()[:, 0]
        positions = net.sample_positions(gb, chunk)[lv][1]
        assert torch.equal(bg_s[idx], positions[idx])
        rows = net.eval_mlp(2 + lv, gb, positions, far=t_far, chunk=chunk)
        net.check_flags()
        front = (torch.arange(N, device=DEV)[None, :] < bg_stop[:, None]) & live[:, None]
        assert torch.equal(bg_rows[front], rows[front]), "kept rows are eval_mlp's"
        behind = ~front & live[:, None]
        assert bool((bg_rows[behind] == 0).all())
        w = ops.composite(2, bg_rows[idx].contiguous(), bg_s[idx].contiguous())["weights"]
        assert bool((w[behind[idx]] == 0).all()), "weights behind the stop are 0"
        if lv == 1:
            assert bool((rows[behind][:, 3] > 0).any()), "the samples behind the stop had density"
        # bg_stop is the op on the call's own rows
        own_stop, own_value = ops.termination_stops_outside(bg_rows[idx].contiguous(), bg_s[idx].contiguous(), got[lv][4][idx, 0].contiguous(),
                                                            mc.EPS if lv == 1 else 0.0)
        assert torch.equal(bg_stop[idx], own_stop) and torch.equal(bg_value[idx], own_value), lv
        assert int(got[3][2 + lv]) == int(bg_stop.sum()) and int(got[3][lv]) == int(smp[STOP].sum())
    bg_stop1 = got[2][1][BG_STOP]
    stopped = ~culled & (bg_stop1 < N_LEVEL[1])
    assert int(stopped.sum()) > 0 and bool((got[2][1][BG_VALUE][stopped] < mc.EPS).all())
    # against the same call with outside=False: the foreground, the inside stops and the cull set bitwise; unstopped rays bitwise
    for lv in range(2):
        for k, x, y in zip(NAMES, got[lv], inside[lv]):
            if k in ("fg_rgb", "fg_acc", "bg_lambda") or lv == 0:
                assert torch.equal(x, y), (lv, k)
            assert torch.equal(x[~stopped], y[~stopped]), (lv, k)
        for i in (FG_T, FG_W, BG_S, STOP, FG_KEEP, FG_ROWS):
            assert torch.equal(got[2][lv][i], inside[2][lv][i]), (lv, i)
    assert torch.equal(got[4], inside[4]) and torch.equal(got[3][:3], inside[3][:3])
    d_rgb = (got[1][0] - inside[1][0]).abs().max(dim=-1).values
    d_depth = (got[1][5] - inside[1][5]).abs()
    print("%d rays: %d stopped, %d culled; max |rgb change| %.3e, max |depth change| %.3e, bound %.4e; outside kept %d of %d"
          % (n, int(stopped.sum()), int(culled.sum()), float(d_rgb.max()), float(d_depth.max()), mc.BOUND * mc.EPS, int(got[3][3]),
             int(inside[3][3])))
    assert bool((d_rgb <= mc.BOUND * mc.EPS).all()) and bool((d_depth <= mc.BOUND * mc.EPS).all())
    assert float(d_rgb[stopped].max()) > 0.0


# ---- 6. alive counts of a segment launch ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("alive", (0, 1, 2, "all"))
def test_alive_counts_of_an_outside_segment_launch(alive):
    """eps between consecutive sorted running values of the rays themselves at boundary 64 of level 1.  The foreground does not
    depend on the outside march, and at these eps (all above every ray's value at 64 but the chosen ones) the rows in front of 64
    are always evaluated, so v_64 is the same in every call."""
    base = _base(96, None)
    net, gb = base["net"], base["gb"]
    plain = _marching(net, gb, 0.0, grid=False)
    bg_s1, rows1 = plain[2][1][BG_S], plain[2][1][BG_ROWS]
    v64 = (plain[1][4][:, 0] * _bg_transmittance(rows1, bg_s1, 64)).sort(descending=True).values
    assert bool((v64[:3] > v64[1:4]).all()) and float(v64[0]) < 0.998, "distinct values at the top"
    if alive == "all":
        eps, count = float(v64[-1]), None
    elif alive == 0:
        eps, count = float(torch.nextafter(v64[0], v64[0] + 1)), 0
    else:
        eps, count = float((v64[alive - 1].double() + v64[alive].double()) / 2), alive
    got = _marching(net, gb, eps, grid=False)
    survivors = ~((got[0][4][:, 0] < eps) & (got[1][4][:, 0] < eps))
    marched_on = int((got[2][1][BG_STOP] > 64).sum())
    if count is None:
        assert marched_on == int(survivors.sum()) > 0
    else:
        assert marched_on == count
    _assert_equals_chain(net, gb, None, got, base["forward"], "%s alive" % alive, eps)


# ---- 7. coarse = True -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n0,n1,R,eps", ((65, 135, 96, mc.EPS), (129, 385, 7, None)))
def test_coarse_outside_level_obeys_the_rule_and_feeds_the_resampling(n0, n1, R, eps):
    net = tg._net(n_coarse=n0 - 1, n_fine=n1 - n0)
    gb = tg._first(tg._rays(96), R)
    forward = tg._forward(net, gb, None)
    if eps is None:
        # from the rays themselves: the ray with the largest level-0 lambda survives every eps up to it (its inside march cannot stop:
        # no transmittance of its row is below its last one) and its level-0 outside march stops at 64 for every eps above
        # lambda x (the level-0 outside transmittance in front of sample 64), which does not depend on eps: take the geometric mean
        s0 = net.sample_positions(gb, None)[0][1]
        t_far, _ = ops.intersect_sphere(gb["rays_o"], gb["rays_d"])
        lam0 = forward[0][4][:, 0]
        r = int(lam0.argmax())
        v64 = lam0 * _bg_transmittance(net.eval_mlp(2, gb, s0, far=t_far), s0, 64)
        net.check_flags()
        assert 0.0 < float(v64[r]) < 0.9 * float(lam0[r]) and float(lam0[r]) < 1.0
        eps = float((lam0[r].double() * v64[r].double()).sqrt())
    got = _marching(net, gb, eps, coarse=True, grid=False)
    culled = (got[0][4][:, 0] < eps) & (got[1][4][:, 0] < eps)
    live = (~culled).nonzero()[:, 0]
    assert len(live) > 0
    smp0 = got[2][0]
    own, _ = ops.termination_stops_outside(smp0[BG_ROWS][live].contiguous(), smp0[BG_S][live].contiguous(), got[0][4][live, 0].contiguous(), eps)
    assert torch.equal(smp0[BG_STOP][live], own)
    assert bool((smp0[BG_STOP][live] < n0).any()), "level 0 stops outside"
    w0 = ops.composite(2, smp0[BG_ROWS][live].contiguous(), smp0[BG_S][live].contiguous())["weights"]
    behind = torch.arange(n0, device=DEV)[None, :] >= smp0[BG_STOP][live][:, None]
    assert bool((w0[behind] == 0).all())
    assert torch.equal(got[2][1][BG_S][live], ops.resample(smp0[BG_S][live].contiguous(), w0, n1 - n0, descending=True)), \
        "level-1 outside positions: the level-0 outside weights resampled"
    _assert_equals_chain(net, gb, None, got, forward, "coarse %d + %d" % (n0, n1), eps, coarse=True)
    fine = net.render_marching(gb, eps, coarse=True, grid=False, fine_only=True, return_samples="rows")
    net.check_flags()
    assert fine[0] is None
    for k, x, y in zip(NAMES, fine[1], got[1]):
        assert torch.equal(x, y), k
    for x, y in zip(fine[2][1], got[2][1]):
        assert torch.equal(x, y)
    assert torch.equal(fine[2][0][BG_STOP], smp0[BG_STOP]) and torch.equal(net.last_march_kept, got[3])
    net.close()


# ---- 8. the grid and the outside stop together ----------------------------------------------------------------------------------

def test_grid_and_outside_stop_together():
    base = _base(96, None)
    net, gb = base["net"], base["gb"]
    net.set_occupancy(oc.mixed(32))
    try:
        # eps from the rays themselves (the grid empties much of the foreground, so the lambdas are not the gridless frame's): the ray
        # with the largest level-1 lambda survives and is not stopped inside at any eps up to it, and its outside march stops at 64
        # for every eps above lambda x (the outside transmittance in front of sample 64): take the geometric mean
        plain = _marching(net, gb, 0.0)
        lam1 = plain[1][4][:, 0]
        r = int(lam1.argmax())
        v64 = lam1 * _bg_transmittance(plain[2][1][BG_ROWS], plain[2][1][BG_S], 64)
        assert 0.0 < float(v64[r]) < 0.9 * float(lam1[r])
        EPS = float((lam1[r].double() * v64[r].double()).sqrt())
        assert EPS < 1.0
        got = _marching(net, gb, EPS)
        inside = _marching(net, gb, EPS, outside=False)
        accel = net.render_accelerated(gb, EPS, return_samples="rows")
        kept = net.last_accel_kept.clone()
        net.check_flags()
    finally:
        net.set_occupancy(None)
    for lv in range(2):
        for k, x, y in zip(NAMES, inside[lv], accel[lv]):
            assert torch.equal(x, y), (lv, k)
        for k, i in (("fg_rgb", 1), ("fg_acc", 3), ("bg_lambda", 4)):
            assert torch.equal(got[lv][i], accel[lv][i]), (lv, k)
        for i, y in zip((FG_T, FG_W, BG_S, STOP, FG_KEEP, FG_ROWS), accel[2][lv]):
            assert torch.equal(got[2][lv][i], y), (lv, i)
    assert torch.equal(got[3][:2], kept)
    assert not bool(got[2][1][FG_KEEP].all()), "the grid skipped something"
    culled = (got[0][4][:, 0] < EPS) & (got[1][4][:, 0] < EPS)
    stopped = ~culled & (got[2][1][BG_STOP] < N_LEVEL[1])
    assert int(stopped.sum()) > 0 and int(got[3][3]) < int(inside[3][3])
    for k, x, y in zip(NAMES, got[1], inside[1]):
        assert torch.equal(x[~stopped], y[~stopped]), k
    assert bool(((got[1][0] - inside[1][0]).abs() <= mc.BOUND * EPS).all()) and bool(((got[1][5] - inside[1][5]).abs() <= mc.BOUND * EPS).all())
    own, _ = ops.termination_stops_outside(got[2][1][BG_ROWS], got[2][1][BG_S], got[1][4], EPS)
    assert torch.equal(got[2][1][BG_STOP][~culled], own[~culled])


# ---- 9. neutrality --------------------------------------------------------------------------------------------------------------

def test_windows_do_not_change_the_result():
    base = _base(300, 128)
    net, gb = base["net"], base["gb"]
    assert net.skip_window is None
    whole128 = _marching(net, gb, mc.EPS, 128, segment=128, grid=False)
    coarse = _marching(net, gb, mc.EPS, 128, coarse=True, grid=False)
    try:
        for window in (1, 128, 299):           # two rows a window at level 1 (1 x 135 / 64) ... one ragged window
            net.skip_window = window
            assert _all_equal(_marching(net, gb, mc.EPS, 128, grid=False), base["mixed"]), window
            assert _all_equal(_marching(net, gb, mc.EPS, 128, segment=128, grid=False), whole128), window
        net.skip_window = 1
        assert _all_equal(_marching(net, gb, mc.EPS, 128, coarse=True, grid=False), coarse)
    finally:
        net.skip_window = None


def test_chunk_decides_the_direction_rows_as_in_forward():
    base = _base(300, 128)
    net, gb = base["net"], base["gb"]
    other = _marching(net, gb, mc.EPS, None, grid=False)
    forward = tg._forward(net, gb, None)
    assert not torch.equal(other[1][2], base["mixed"][1][2]), "bg_rgb depends on the chunk through the direction rows"
    _assert_equals_chain(net, gb, None, other, forward, "300 rays, one chunk", mc.EPS)


def test_calls_are_repeatable_overlap_and_loop_neutral_and_synchronise_nothing():
    base = _base(96, None)
    net, gb = base["net"], base["gb"]
    assert _all_equal(_marching(net, gb, mc.EPS, grid=False), base["mixed"])
    assert net.overlap_calls
    net.overlap_calls = False
    try:
        off = _marching(net, gb, mc.EPS, grid=False)
    finally:
        net.overlap_calls = True
    assert _all_equal(off, base["mixed"])
    # the reference-style loop: three calls of 32 rays, each one reference chunk, in flight on alternating lanes; no blocking wait
    whole = _marching(net, gb, mc.EPS, 32, grid=False)
    ctx = net._context(torch.device(DEV))
    before = ctx.sync_count()
    parts, kept, survivors = [], [], []
    for i in range(0, 96, 32):
        part = {k: (v[i:i + 32] if k in PER_RAY else v) for k, v in gb.items()}
        parts.append(net.render_marching(part, mc.EPS, chunk=32, grid=False, return_samples="rows"))
        kept.append(net.last_march_kept)
        survivors.append(net.last_march_survivors)
    assert ctx.sync_count() == before, "a marching call blocked on the device"
    net.check_flags()
    for lv in range(2):
        for j in range(6):
            assert torch.equal(torch.cat([p[lv][j] for p in parts]), whole[lv][j]), (lv, j)
        for j in range(9):
            assert torch.equal(torch.cat([p[2][lv][j] for p in parts]), whole[2][lv][j]), (lv, j)
    assert torch.equal(sum(kept), whole[3]) and int(sum(survivors)) == int(whole[4])
    # forward and the older calls are unchanged by the call
    after = tg._forward(net, gb, None)
    for lv in range(2):
        assert all(torch.equal(x, y) for x, y in zip(after[lv], base["forward"][lv]))
    # the frame helper: the fine level, the kept fractions inside and outside, the culled fraction
    frame = render.render_marching_rays(net, gb, mc.EPS, chunk=96, grid=False)
    got = base["mixed"]
    assert torch.equal(frame["rgb"], got[1][0]) and torch.equal(frame["depth"], got[1][5]) and torch.equal(frame["acc"], got[1][3])
    frac, frac_out, gone = frame["kept_fraction"], frame["kept_fraction_outside"], frame["culled_fraction"]
    for f in (frac, frac_out):
        assert f.is_cuda and f.dtype == torch.float64 and tuple(f.shape) == (2,)
    assert gone.is_cuda and gone.dtype == torch.float64
    assert all(abs(float(frac[lv]) - int(got[3][lv]) / (96 * N_LEVEL[lv])) < 1e-12 for lv in range(2))
    assert all(abs(float(frac_out[lv]) - int(got[3][2 + lv]) / (96 * N_LEVEL[lv])) < 1e-12 for lv in range(2))
    assert abs(float(gone) - (96 - int(got[4])) / 96) < 1e-12
    plain = render.render_rays_test(net, gb, chunk=96)
    zero = render.render_marching_rays(net, gb, 0.0, chunk=96)
    assert torch.equal(zero["rgb"], plain["rgb"]) and torch.equal(zero["depth"], plain["depth"])
    assert zero["kept_fraction"].tolist() == [1.0, 1.0] == zero["kept_fraction_outside"].tolist() and float(zero["culled_fraction"]) == 0.0
    with pytest.raises(TypeError):
        render.render_marching_rays(models.NeRF(), gb, mc.EPS)


def test_bad_arguments_are_refused_on_the_host_and_no_rays_is_a_valid_call():
    """Every refused call here returns an error before anything is launched: no kernel sees one of these pointers or shapes."""
    net = tg._net()
    gb = tg._rays(96)
    c = net._context(torch.device(DEV))
    lib, h, s = c.lib, c.handle, c.stream()
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = buf.data_ptr()

    def refused(rc, text):
        assert rc != 0
        msg = lib.neo_last_error().decode()
        assert text in msg, msg
    stops = lambda R=4, N=4, eps=0.1, seg=64, a=p, b=p, c_=p, e=p, f=p, ctx=h: lib.neo_tp_termination_stops_outside(
        ctx, a, b, c_, R, N, eps, seg, e, f, s)
    refused(stops(ctx=None), "null context")
    refused(stops(R=-1), "bad shape")
    refused(stops(N=0), "bad shape")
    refused(stops(R=1 << 22, N=1 << 10), "too many points")
    for eps in (-0.1, 1.0, 2.0, float("nan")):
        refused(stops(eps=eps), "eps must lie in [0, 1)")
    for seg in (0, -64, 32, 100):
        refused(stops(seg=seg), "segment must be a positive multiple of 64")
    for kw in (dict(a=None), dict(b=None), dict(c_=None), dict(e=None), dict(f=None)):
        refused(stops(**kw), "null pointer")
    assert stops(R=0, a=None, b=None, c_=None, e=None, f=None) == 0          # no rays: nothing to do
    poses, NV, focal, cx, cy = net._camera_args(gb)
    o, d, v = (gb[k].data_ptr() for k in PER_RAY)
    lvl = _lib.TpLevelOut()
    kept = torch.full((4,), 7, dtype=torch.int64, device=DEV)
    survivors = torch.full((), 7, dtype=torch.int32, device=DEV)
    frame = lambda R=96, chunk=96, nc=tc.N_COARSE, nf=tc.N_FINE, o=o, nv=NV, eps=0.1, seg=64: lib.neo_tp_render_marching(
        h, o, d, v, R, chunk, poses, nv, focal, cx, cy, nc, nf, ctypes.byref(lvl), ctypes.byref(lvl), eps, seg, 0, 1, 1, None, None,
        kept.data_ptr(), survivors.data_ptr(), s)
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
    assert kept.tolist() == [7, 7, 7, 7] and int(survivors) == 7, "a refused call writes nothing"
    assert frame(R=0) == 0
    torch.cuda.synchronize()
    assert kept.tolist() == [0, 0, 0, 0] and int(survivors) == 0
    assert c.poll_flags() == 0
    none = tg._first(gb, 0)
    out = net.render_marching(none, 0.1, return_samples=True)
    assert tuple(out[1][0].shape) == (0, 3) and tuple(out[2][1][BG_STOP].shape) == (0,)
    stop, value = ops.termination_stops_outside(torch.zeros(0, 9, 4, device=DEV), torch.zeros(0, 9, device=DEV), torch.zeros(0, device=DEV), 0.1)
    assert tuple(stop.shape) == tuple(value.shape) == (0,)
    with pytest.raises(ValueError):
        net.render_marching(gb, 1.0)
    with pytest.raises(ValueError):
        net.render_marching(gb, 0.1, segment=96)
    net.close()
