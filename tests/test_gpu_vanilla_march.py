"""GPU: empty-space skipping and early ray termination of the vanilla frame (`marching.MarchingNeRF.render_marching`,
neo_vanilla_render_marching), its stage functions and the frame helper (`marching.render_marching_rays`).

Inputs: tests/vanilla_march_cases.py - synth.vanilla_state(0) with a per-pair density bias, cases.strided_rays(R) for
R in {1, 63, 64, 65, 257}, the count pairs 3 + 4, 7 + 64, 63 + 64 and 64 + 128 (the last one only at R <= 65), both arithmetics.
tests/test_vanilla_march_cpu.py asserts on the oracle that the inputs mix stopped and never-stopped rays; where a test here
relies on a mix it asserts it again on the device's own stops.

Bounds.  The call is a composition of rules that the library states bit for bit: an evaluated sample is computed by the same
machine code as in `forward`, any other sample is a row of zeros, the keep mask is `marching.occupancy_keep_box` and the stop is
`marching.termination_stops_vanilla` on the masked rows.  So every comparison of the call with `forward` or with the chain of
public stage ops is `torch.equal`.  The a-priori bound of the header (1.003 trans per channel, 1.001 far trans in depth) is
asserted against the same call at eps = 0; the parity with the CPU oracle is the project's 1e-4 per ray."""
import pytest
import torch

import occupancy_cases as oc
import vanilla_march_cases as vc
from neo360_amd import _lib, marching, models, ops
from vanilla_march_gpu import assert_equals_chain as _assert_equals_chain, installed as _installed, march as _march, rays as _rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("rays_o", "rays_d", "viewdirs")
NAMES = ("rgb", "acc", "depth")
ARITH = (None, "f32")
CASES = [(c, p) for c in vc.COUNTS for p in ARITH]
IDS = ["%d+%d-%s" % (c[0], c[1], p or "f16x3") for c, p in CASES]

_NETS = {}


def _net(counts, precision=None):
    key = (counts, precision)
    if key not in _NETS:
        net = marching.MarchingNeRF(num_coarse_samples=counts[0], num_fine_samples=counts[1]).to(DEV)
        net.load_state_dict(vc.state(counts))
        if precision is not None:
            net.precision = precision
        _NETS[key] = net
    return _NETS[key]


def _ray_counts(counts):
    return tuple(n for n in vc.RAYS if not (counts == (64, 128) and n > 65))


def _forward(net, b, white=False):
    out = net(b, False, white, vc.NEAR, vc.FAR)
    net.check_flags()
    return [[t.clone() for t in lv] for lv in out]


def _flat(res):
    return [t for lv in res[:2] for t in lv] + [t for lv in res[2] for t in lv] + [res[3]]


def _same(x, y):
    return all(a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(_flat(x), _flat(y)))


# ---- 1-3. nothing to skip and nothing to stop: forward ------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,precision", CASES, ids=IDS)
def test_no_grid_all_ones_grid_and_a_far_box_are_bitwise_forward_at_eps_zero(counts, precision):
    net = _net(counts, precision)
    N = vc.n_level(counts)
    for n in _ray_counts(counts):
        b = _rays(n)
        for white in (False, True):
            want = _forward(net, b, white)
            settings = ((None, None, False), (oc.ones(8), vc.BOX, False), (oc.ones(32), vc.BOX, False), (vc.mixed(8), vc.FAR_AWAY, False))
            for grid, box, clip in settings:
                with _installed(net, grid, box, clip):
                    got = _march(net, b, 0.0, white)
                    off = _march(net, b, 0.0, white, grid=False)
                what = (counts, n, white, None if grid is None else (int(grid.shape[0]), box))
                for lv in range(2):
                    for k, x, y in zip(NAMES, got[lv], want[lv]):
                        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, lv, k)
                    t, w, keep, stop, rows = got[2][lv]
                    assert bool(keep.all()) and bool((stop == N[lv]).all()), (what, lv)
                assert got[3].tolist() == [n * N[0], n * N[1]], what
                assert _same(off, got), what
        # a box that holds no sample keeps everything only without clip
        with _installed(net, vc.mixed(8), vc.FAR_AWAY, True):
            none = _march(net, b, 0.0)
        assert none[3].tolist() == [0, 0] and not bool(none[2][1][2].any())


# ---- 4-5. a mixed grid: the chain of public stage ops --------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,precision", CASES, ids=IDS)
def test_mixed_grid_frame_equals_the_chain_of_stage_ops(counts, precision):
    net = _net(counts, precision)
    N = vc.n_level(counts)
    for n in _ray_counts(counts):
        b = _rays(n)
        for G in ((8, 32, 256) if n in (65, 257) else (32,)):
            grid = vc.mixed(G)
            with _installed(net, grid, vc.BOX, False):
                for eps, coarse in ((0.0, False), (vc.EPS, False), (vc.EPS, True)):
                    got = _march(net, b, eps, coarse=coarse)
                    stops = _assert_equals_chain(net, b, got, (counts, n, G, eps, coarse), grid, vc.BOX, False, eps, coarse=coarse)
                    keep1 = got[2][1][2]
                    if n >= 63:
                        assert 0 < int(keep1.sum()) < keep1.numel(), "the grid keeps some samples and skips some"
                    if n >= 63 and eps > 0 and not coarse and N[1] > vc.SEGMENT:
                        print("%s, %d rays, G %d: level-1 stops %s" % (counts, n, G, sorted(set(stops[1].tolist()))))


@pytest.mark.parametrize("counts", [c for c in vc.COUNTS if vc.n_level(c)[1] > vc.SEGMENT], ids=lambda c: "%d+%d" % c)
def test_the_device_stops_mix_stopped_and_never_stopped_rays(counts):
    """The condition tests/test_vanilla_march_cpu.py asserts on the oracle, on the device's own stops (the biases sit on a knife's
    edge by construction, so only the presence of both kinds is asserted here)."""
    net = _net(counts)
    N1 = vc.n_level(counts)[1]
    b = _rays(65)
    got = _march(net, b, vc.EPS)
    stop = got[2][1][3]
    print("%s: device level-1 stops %s" % (counts, {int(v): int(c) for v, c in zip(*torch.unique(stop.cpu(), return_counts=True))}))
    assert 0 < int((stop < N1).sum()) < 65
    _assert_equals_chain(net, b, got, (counts, "no grid"), None, None, False, vc.EPS)
    assert int(got[3][1]) == int(stop.sum()), "without a grid the evaluated samples are the prefixes"


# ---- 6. the compact evaluator launch ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ARITH, ids=("f16x3", "f32"))
def test_eval_points_under_a_device_count(precision):
    net = _net((64, 128), precision)
    cap = 300                                   # more than the largest tile (128 points), no multiple of a tile
    b = _rays(cap)
    g = torch.Generator().manual_seed(3)
    t = (vc.NEAR + (vc.FAR - vc.NEAR) * torch.rand(cap, generator=g)).to(DEV)
    o, d = b["rays_o"], b["viewdirs"]
    for level in range(2):
        dense = net.eval_mlp(level, o, d, t[:, None])[:, 0].clone()
        out = torch.empty(cap, 4, device=DEV)
        for n in (cap, 129, 128, 127, 65, 64, 63, 1, 0):      # descending on one buffer set: a stale row that was used would show
            out.fill_(-7.0)
            count = torch.tensor([n], dtype=torch.int32, device=DEV)
            res = marching.eval_points(net, level, o, d, t, count, out=out)
            assert res is out
            assert torch.equal(out[:n], dense[:n]), (level, n)
            assert bool((out[n:] == -7.0).all()), (level, n, "rows behind the count are not written")
        big = torch.tensor(10 * cap, dtype=torch.int32, device=DEV)
        assert torch.equal(marching.eval_points(net, level, o, d, t, big), dense), "a count beyond the bound is the bound"


# ---- 7. exact kept counts ------------------------------------------------------------------------------------------------------------------

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
    N = vc.n_level(counts)
    b = _rays(3)
    if want == "all":
        grid = oc.ones(256)
        with _installed(net, grid, vc.BOX, False):
            got = _march(net, b, vc.EPS)
        assert int(got[3][0]) == 3 * N[0] and int(got[3][1]) == int(got[2][1][3].sum())
        _assert_equals_chain(net, b, got, "all kept", grid, vc.BOX, False, vc.EPS)
        return
    with _installed(net, oc.zeros(256), vc.BOX, True):
        empty = _march(net, b, vc.EPS)
    assert empty[3].tolist() == [0, 0]
    o, d = b["rays_o"].cpu(), b["viewdirs"].cpu()
    t0, t1 = empty[2][0][0].cpu(), empty[2][1][0].cpu()
    grid = _grid_for_count(o, d, t1, t0, vc.BOX, want)
    with _installed(net, grid, vc.BOX, True):
        for eps in (0.0, vc.EPS):
            got = _march(net, b, eps)
            assert torch.equal(got[2][1][0], empty[2][1][0]), "the level-1 positions are those of the empty grid"
            assert int(got[2][1][2].sum()) == want and got[3].tolist() == [0, want], (want, eps, got[3].tolist())
            _assert_equals_chain(net, b, got, ("kept", want, eps), grid, vc.BOX, True, eps)


# ---- 8-9. the empty grid and the clip ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,precision", CASES, ids=IDS)
def test_all_zeros_grid_renders_the_background_and_clip_skips_outside_samples(counts, precision):
    net = _net(counts, precision)
    N = vc.n_level(counts)
    n = 65
    b = _rays(n)
    o, vd = b["rays_o"], b["viewdirs"]
    for white in (False, True):
        with _installed(net, oc.zeros(32), vc.BOX, True):
            got = _march(net, b, vc.EPS, white)
        for lv in range(2):
            rgb, acc, depth = got[lv]
            assert bool((acc == 0).all()) and bool((rgb == (1.0 if white else 0.0)).all()) and bool((depth == 0).all())
            t, w, keep, stop, rows = got[2][lv]
            assert not bool(keep.any()) and bool((rows == 0).all()) and bool((w == 0).all()) and bool((stop == N[lv]).all())
        assert got[3].tolist() == [0, 0]
    # clip=True with a box smaller than the ray span: samples outside have zero rows, samples inside are eval_mlp's
    with _installed(net, oc.ones(8), vc.SMALL, True):
        got = _march(net, b, 0.0)
    for lv in range(2):
        t, w, keep, stop, rows = got[2][lv]
        tc_, oc_, dc_ = t.cpu(), o.cpu(), vd.cpu()
        c = vc.cell_box(oc.positions(oc_, dc_, tc_), vc.SMALL, 8)
        inside = ((c >= 0) & (c < 8)).all(dim=-1)
        sure = ~vc.near_face_box(vc.SMALL, oc_, dc_, tc_, 8)
        assert int((~sure).sum()) <= 0.01 * sure.numel()
        assert torch.equal(keep.cpu()[sure], inside[sure])
        assert 0 < int(keep.sum()) < keep.numel(), "the box is smaller than the ray span"
        assert bool((rows[~keep] == 0).all())
        assert torch.equal(rows[keep], net.eval_mlp(lv, o, vd, t)[keep])
    with _installed(net, oc.ones(8), vc.SMALL, False):
        assert _same(_march(net, b, 0.0), _march(net, b, 0.0, grid=False)), "without clip the outside samples are kept"


# ---- 10. the termination bound -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,precision", [c for c in CASES if vc.n_level(c[0])[1] > vc.SEGMENT],
                         ids=[i for c, i in zip(CASES, IDS) if vc.n_level(c[0])[1] > vc.SEGMENT])
def test_the_bound_against_the_same_call_at_eps_zero(counts, precision):
    net = _net(counts, precision)
    N1 = vc.n_level(counts)[1]
    n = 65 if counts == (64, 128) else 257
    b = _rays(n)
    seen = 0
    for grid in (None, vc.mixed(32)):
        with _installed(net, grid, vc.BOX if grid is not None else None, False):
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
                    for k, x, y in zip(NAMES, got[1], plain[1]):
                        assert torch.equal(x[~stopped], y[~stopped]), ("a ray that never stops is bitwise unchanged", k)
                    if not bool(stopped.any()):
                        continue
                    seen += int(stopped.sum())
                    assert bool((trans[stopped] < eps).all())
                    d_rgb = (got[1][0] - plain[1][0]).abs().max(dim=-1).values
                    d_depth = (got[1][2] - plain[1][2]).abs()
                    print("%s grid %s white %s eps %g: %d of %d stopped; max |rgb change| / trans = %.4f, max |depth change| / (far trans) "
                          "= %.4f, min trans %.3e" % (counts, grid is not None, white, eps, int(stopped.sum()), n,
                                                      float((d_rgb / trans)[stopped].max()),
                                                      float((d_depth / (vc.FAR * trans))[stopped].max()), float(trans[stopped].min())))
                    assert bool((d_rgb[stopped] <= 1.003 * trans[stopped]).all())
                    assert bool((d_depth[stopped] <= 1.001 * vc.FAR * trans[stopped]).all())
    assert seen > 0, "no ray stopped: the bound was not exercised"


# ---- 11. the CPU oracle ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,precision", CASES, ids=IDS)
def test_parity_with_the_oracle_on_the_devices_own_positions_and_masks(counts, precision):
    net = _net(counts, precision)
    n = 65
    b = _rays(n)
    cpu = vc.rays(n)
    for grid, eps, white in ((None, 0.0, False), (vc.mixed(32), vc.EPS, False), (vc.mixed(32), vc.EPS, True)):
        with _installed(net, grid, vc.BOX if grid is not None else None, False):
            got = _march(net, b, eps, white)
        samples = tuple(got[2][lv][0].cpu() for lv in range(2))
        masks = tuple((got[2][lv][2] & vc.front(got[2][lv][3], got[2][lv][0].shape[1])).cpu() for lv in range(2))
        want, _ = vc.oracle_render_marching(vc.state(counts), cpu, counts, eps, white_bkgd=white, samples=samples, masks=masks)
        for lv in range(2):
            for k, x, y in zip(NAMES, got[lv], want[lv]):
                err = float((x.cpu() - y).abs().max())
                print("%s %s grid %s eps %g white %s level %d %s: max |err| per ray %.3e" % (counts, precision, grid is not None, eps, white, lv, k, err))
                assert err < 1e-4, (counts, lv, k, err)


# ---- 12. building a grid --------------------------------------------------------------------------------------------------------------------

def test_build_occupancy_is_the_cpu_reduction_of_eval_mlps_own_densities():
    counts = (7, 64)
    net = _net(counts)
    G, probes = 8, 2
    c, o, d = marching.occupancy_lattice_box(vc.BOX, G, probes, DEV)
    M = G * probes
    t = c[None, :].expand(M * M, M).contiguous()
    sigma = torch.maximum(net.eval_mlp(0, o, d, t)[..., 3], net.eval_mlp(1, o, d, t)[..., 3]).reshape(M, M, M).cpu()
    threshold = float(sigma.median())
    try:
        for dilate in (0, 1):
            grid = net.build_occupancy(vc.BOX, G, threshold, probes=probes, dilate=dilate)
            raw = (~(sigma.reshape(G, probes, G, probes, G, probes) <= threshold)).any(dim=5).any(dim=3).any(dim=1)
            assert torch.equal(grid.cpu(), oc.dilate(raw, dilate)), dilate
            assert torch.equal(net.occupancy, grid) and net.occupancy_box == vc.BOX
            if dilate == 0:
                assert 0 < int(grid.sum()) < grid.numel()
            assert torch.equal(marching.occupancy_from_sigma_box(sigma.to(DEV), G, threshold, probes, dilate), grid)
        # no unit-sphere clip: the corner cells of an all-dense lattice stay set
        assert bool(marching.occupancy_from_sigma_box(torch.ones(M, M, M, device=DEV), G, 0.5, probes, 0).all())
        assert not bool(ops.occupancy_from_sigma(torch.ones(M, M, M, device=DEV), G, 0.5, probes, 0).all())
    finally:
        net.set_occupancy(None)


# ---- 13. windows, repeatability, the chunk loop ----------------------------------------------------------------------------------------------

def test_windows_runs_and_the_chunk_loop_give_the_same_bits_and_nothing_blocks():
    counts = (63, 64)
    net = _net(counts)
    b = _rays(300)
    grid = vc.mixed(32)
    assert net.march_window is None
    with _installed(net, grid, vc.BOX, False):
        try:
            base = _march(net, b, vc.EPS)
            wide = _march(net, b, vc.EPS, segment=128)
            coarse = _march(net, b, vc.EPS, coarse=True)
            assert _same(_march(net, b, vc.EPS), base), "two runs"
            for window in (1, 128, 299):
                net.march_window = window
                assert _same(_march(net, b, vc.EPS), base), window
                assert _same(_march(net, b, vc.EPS, segment=128), wide), window
                assert _same(_march(net, b, vc.EPS, coarse=True), coarse), window
            net.march_window = None
        finally:
            net.march_window = None
        _assert_equals_chain(net, b, wide, "segment 128", grid, vc.BOX, False, vc.EPS, segment=128)
        assert bool((wide[2][1][3] == 128).all())
        net.overlap_calls = False
        try:
            assert _same(_march(net, b, vc.EPS), base), "overlap off"
        finally:
            net.overlap_calls = True
        # the chunk loop: three calls of 100 rays in flight on alternating lanes; no blocking wait
        ctx = net._context(torch.device(DEV))
        before = ctx.sync_count()
        parts, kept = [], []
        for i in range(0, 300, 100):
            part = {k: v[i:i + 100] for k, v in b.items()}
            parts.append(net.render_marching(part, vc.EPS, False, vc.NEAR, vc.FAR, return_samples=True))
            kept.append(net.last_march_kept)
        assert ctx.sync_count() == before, "a marching call blocked on the device"
        net.check_flags()
        for lv in range(2):
            for j in range(3):
                assert torch.equal(torch.cat([p[lv][j] for p in parts]), base[lv][j]), (lv, j)
            for j in range(5):
                assert torch.equal(torch.cat([p[2][lv][j] for p in parts]), base[2][lv][j]), (lv, j)
        assert torch.equal(sum(kept), base[3])
        helper = marching.render_marching_rays(net, b, vc.EPS, chunk=100)
        assert torch.equal(helper["rgb"], base[1][0]) and torch.equal(helper["acc"], base[1][1]) and torch.equal(helper["depth"], base[1][2])
        frac = helper["kept_fraction"]
        N = vc.n_level(counts)
        assert frac.is_cuda and frac.dtype == torch.float64 and tuple(frac.shape) == (2,)
        assert all(abs(float(frac[lv]) - int(base[3][lv]) / (300 * N[lv])) < 1e-12 for lv in range(2)) and 0.0 < float(frac[1]) < 1.0
        after = _forward(net, b)
    plain = _forward(net, b)
    assert all(torch.equal(x, y) for lv in range(2) for x, y in zip(after[lv], plain[lv])), "forward does not read the grid"
    # a grid of another context is refused; no rays is a valid call
    with _installed(net, grid, vc.BOX, False):
        mine = net._occ_ctx
        net._occ_ctx = object()
        try:
            with pytest.raises(_lib.NeoError, match="does not belong"):
                net.render_marching(b, vc.EPS, False, vc.NEAR, vc.FAR)
        finally:
            net._occ_ctx = mine
        none = {k: v[:0] for k, v in b.items()}
        out = net.render_marching(none, vc.EPS, False, vc.NEAR, vc.FAR, return_samples=True)
        assert tuple(out[1][0].shape) == (0, 3) and tuple(out[2][1][3].shape) == (0,) and net.last_march_kept.tolist() == [0, 0]


# ---- 14. the module's own boundary cases ------------------------------------------------------------------------------------------------------

def test_strided_misaligned_and_other_float_inputs_give_the_dense_calls_bits():
    counts = (7, 64)
    net = _net(counts)
    n = 65
    b = _rays(n)
    grid = vc.mixed(32)
    with _installed(net, grid, vc.BOX, False):
        want = _march(net, b, vc.EPS)
        wide = {k: torch.zeros(n, 7, device=DEV) for k in KEYS}
        odd = {k: torch.zeros(3 * n + 1, device=DEV) for k in KEYS}
        for k in KEYS:
            wide[k][:, 2:5] = b[k]
            odd[k][1:] = b[k].reshape(-1)
        strided = {k: wide[k][:, 2:5] for k in KEYS}
        misaligned = {k: odd[k][1:].reshape(n, 3) for k in KEYS}
        assert not strided["rays_o"].is_contiguous() and misaligned["rays_o"].data_ptr() % 16 != 0
        for what, rays in (("strided", strided), ("misaligned", misaligned), ("fp64", {k: b[k].double() for k in KEYS})):
            assert _same(_march(net, rays, vc.EPS), want), what
        half = {k: b[k].half() for k in KEYS}
        assert _same(_march(net, half, vc.EPS), _march(net, {k: half[k].float() for k in KEYS}, vc.EPS)), "fp16"
    # the stage functions: the same tensor contract
    o, vd, rd = b["rays_o"], b["viewdirs"], b["rays_d"]
    t, w, keep, stop, rows = want[2][1]
    t_wide = torch.zeros(n, t.shape[1] + 3, device=DEV)
    t_wide[:, 1:-2] = t
    assert torch.equal(marching.occupancy_keep_box(grid, vc.BOX, strided["rays_o"], misaligned["viewdirs"].double(), t_wide[:, 1:-2]), keep)
    rows_wide = torch.zeros(n, t.shape[1], 6, device=DEV)
    rows_wide[..., 1:5] = rows
    got = marching.termination_stops_vanilla(rows_wide[..., 1:5], t_wide[:, 1:-2].double(), misaligned["rays_d"], vc.EPS)
    assert torch.equal(got[0], stop)
    tt = t[:, 0].contiguous()
    count = torch.tensor(n, dtype=torch.int32, device=DEV)
    dense = marching.eval_points(net, 1, o, vd, tt, count)
    assert torch.equal(marching.eval_points(net, 1, strided["rays_o"], misaligned["viewdirs"].double(), tt[:, None], count), dense)
    # refused by name, before any launch
    bad = dict(b)
    bad["viewdirs"] = b["viewdirs"][:-1]
    with pytest.raises(ValueError, match="viewdirs must have shape"):
        net.render_marching(bad, vc.EPS, False, vc.NEAR, vc.FAR)
    bad["viewdirs"] = b["viewdirs"].reshape(-1)
    with pytest.raises(ValueError, match="viewdirs must have shape"):
        net.render_marching(bad, vc.EPS, False, vc.NEAR, vc.FAR)
    bad["viewdirs"] = b["viewdirs"].long()
    with pytest.raises(ValueError, match="viewdirs must be a floating-point"):
        net.render_marching(bad, vc.EPS, False, vc.NEAR, vc.FAR)
    bad["viewdirs"] = b["viewdirs"].cpu()
    with pytest.raises(ValueError, match="viewdirs is on cpu"):
        net.render_marching(bad, vc.EPS, False, vc.NEAR, vc.FAR)
    with pytest.raises(ValueError, match="t must have shape"):
        marching.occupancy_keep_box(grid, vc.BOX, o, vd, t[:-1])
    with pytest.raises(ValueError, match="rgbsigma must have shape"):
        marching.termination_stops_vanilla(rows[..., :3], t, rd, vc.EPS)
    with pytest.raises(ValueError, match="rays_d is on cpu"):
        marching.termination_stops_vanilla(rows, t, rd.cpu(), vc.EPS)
    with pytest.raises(ValueError, match="count must be an integer"):
        marching.eval_points(net, 1, o, vd, tt, count.float())
    with pytest.raises(ValueError, match="out must"):
        marching.eval_points(net, 1, o, vd, tt, count, out=torch.empty(n, 6, device=DEV)[:, :4])
    with pytest.raises(ValueError, match="out must have shape"):
        marching.eval_points(net, 1, o, vd, tt, count, out=torch.empty(n - 1, 4, device=DEV))
    assert isinstance(net, models.NeRF)
