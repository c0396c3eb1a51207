"""GPU: empty-space skipping of the NeO-360 frame (`NeRF_TP.render_skipping`, neo_tp_render_skipping), its classifier and grid
builder on caller data (`ops.occupancy_keep`, `ops.occupancy_from_sigma`, `NeRF_TP.build_occupancy`) and the frame helper
(`render.render_skipping_rays`).

Scene, state and rays: tests/edit_cases.py / tests/instance_cases.py at 16 + 32 samples (17 and 49 samples a ray), on 96 rays in
one chunk or 300 rays in chunks of 128.  Grids and restatements: tests/occupancy_cases.py, tests/test_occupancy_cpu.py.

Bounds.  A kept sample is evaluated by the same machine code as in the dense frame, a skipped one is a row of zeros, so every
comparison here is exact: the keep mask against its fp32 restatement (outside the samples within 2^-20 * 2 / G of a cell face,
which test_occupancy_cpu.py caps at 1 %), the kept rows against `eval_mlp`, the whole call against the chain of public stage ops
by the rule of tests/test_gpu_edit.py (bitwise when that chain is bitwise `forward`, else within 4 x its deviation from it)."""
import ctypes

import pytest
import torch

import cases
import edit_cases as ec
import instance_cases as ic
import occupancy_cases as occ_c
from neo360_amd import _lib, models, ops, render
from test_gpu_objects import EVALUATORS

pytestmark = pytest.mark.gpu
DEV = "cuda"
PER_RAY = ("rays_o", "rays_d", "viewdirs")
NAMES = ("rgb", "fg_rgb", "bg_rgb", "fg_acc", "bg_lambda", "depth")
SHAPES = ((96, None), (300, 128))          # those of tests/test_gpu_edit.py
N_LEVEL = (ec.N_COARSE + 1, ec.N_COARSE + 1 + ec.N_FINE)


def _net(precision=None, preproject=3):
    net = models.NeRF_TP(num_coarse_samples=ec.N_COARSE, num_fine_samples=ec.N_FINE, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(ec.state())
    sc = ec.scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV),
                  sc["image_wh"], preproject=preproject)
    if precision is not None:
        net.precision = precision
    return net


def _rays(n):
    return {k: v.to(DEV) for k, v in ic.rays(n).items()}


def _forward(net, gb, chunk):
    out = net(gb, False, False, 0.0, 0.0, out_depth=True, chunk=chunk)
    net.check_flags()
    return [[t.clone() for t in lv] for lv in out]


def _skipping(net, gb, chunk=None):
    """[level 0 six, level 1 six, [(fg_t, fg_w, bg_s, fg_keep, fg_rows) per level], kept int64[2]], cloned."""
    out = net.render_skipping(gb, chunk=chunk, return_samples="rows")
    net.check_flags()
    return [[t.clone() for t in out[0]], [t.clone() for t in out[1]], [[t.clone() for t in lv] for lv in out[2]], net.last_skip_kept.clone()]


def _stages(net, gb, chunk, keeps=None):
    """`_stages` of tests/test_gpu_edit.py - the frame from public stage ops - with the rows of the samples keeps[level] clears set
    to zero before the inside-sphere composite."""
    o, d = gb["rays_o"], gb["rays_d"]
    t_far, _ = ops.intersect_sphere(o, d)
    fg_t, bg_s = net.sample_positions(gb, chunk)[0]
    out = []
    for level in range(2):
        fg = net.eval_mlp(level, gb, fg_t, chunk=chunk)
        bg = net.eval_mlp(2 + level, gb, bg_s, far=t_far, chunk=chunk)
        if keeps is not None:
            fg = torch.where(keeps[level][:, :, None], fg, torch.zeros_like(fg))
        f = ops.composite(1, fg, fg_t, d, t_far)
        b = ops.composite(2, bg, bg_s)
        lam = f["bg_lambda"]
        out.append([f["rgb"] + lam * b["rgb"], f["rgb"], b["rgb"], f["acc"], lam, f["depth"] + lam[:, 0] * b["depth"]])
        if level == 0:
            fg_t = ops.resample(fg_t, f["weights"], ec.N_FINE)
            bg_s = ops.resample(bg_s, b["weights"], ec.N_FINE, descending=True)
    return out


def _assert_equals_chain(net, gb, chunk, got, forward, what):
    """The rule of tests/test_gpu_edit.py: first the plain chain against plain `forward`; if that deviation is 0 the skipping call
    equals its chain bitwise, otherwise within 4 x it."""
    parent = _stages(net, gb, chunk)
    net.check_flags()
    worst = max(float((x - y).abs().max()) for lv in range(2) for x, y in zip(parent[lv], forward[lv]))
    want = _stages(net, gb, chunk, [got[2][0][3], got[2][1][3]])
    net.check_flags()
    for lv in range(2):
        for k, x, y in zip(NAMES, got[lv], want[lv]):
            err = float((x - y).abs().max())
            print("%s level %d %s: call against its stage chain %.3e (plain chain against forward: %.3e)" % (what, lv, k, err, worst))
            if worst == 0.0:
                assert torch.equal(x, y), (what, lv, k)
            else:
                assert err <= 4.0 * worst, (what, lv, k, err, worst)


_BASE = {}


def _base(n=96, chunk=None):
    """One default module with the mixed grid installed, its plain frame and its skipping frame with samples (never modified)."""
    key = (n, chunk)
    if key not in _BASE:
        net = _net()
        gb = _rays(n)
        forward = _forward(net, gb, chunk)
        grid = occ_c.mixed(32)
        net.set_occupancy(grid)
        _BASE[key] = dict(net=net, gb=gb, grid=grid, forward=forward, mixed=_skipping(net, gb, chunk))
    return _BASE[key]


# ---- 1. the classifier ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [8, 32, 256])
def test_classifier_is_its_fp32_restatement(G):
    seen_skip = seen_wild = 0
    for N in (1, 17, 49, 64, 65, 385):
        for R in (1, 7, 300):
            grid, o, d, t = occ_c.classifier_case(R, N, G, 1000 * G + 10 * N + R)        # the inputs test_occupancy_cpu.py caps
            want = occ_c.keep_rule(grid, o, d, t)
            face = occ_c.near_face(o, d, t, G)
            got = ops.occupancy_keep(grid, o.to(DEV), d.to(DEV), t.to(DEV))
            assert got.dtype == torch.bool and tuple(got.shape) == (R, N) and got.is_cuda
            assert torch.equal(got.cpu()[~face], want[~face]), (G, N, R)
            wild = ~torch.isfinite(occ_c.positions(o, d, t)).all(dim=-1)
            assert bool(got.cpu()[wild].all()), "a non-finite position is kept"
            assert bool(ops.occupancy_keep(None, o.to(DEV), d.to(DEV), t.to(DEV)).all()), "no grid: everything is kept"
            seen_skip += int((~want).sum())
            seen_wild += int(wild.sum())
            # inputs of full fp32 precision: the kernel's own arithmetic, restated by eager torch on the device, on every sample
            grid, o, d, t = occ_c.classifier_case(R, N, G, 77 + 1000 * G + 10 * N + R, dyadic=False)
            go, gd, gt = o.to(DEV), d.to(DEV), t.to(DEV)
            assert torch.equal(ops.occupancy_keep(grid.to(DEV), go, gd, gt), occ_c.keep_rule(grid.to(DEV), go, gd, gt)), (G, N, R)
    assert seen_skip > 1000 and seen_wild >= 18


# ---- 2. all ones: the dense frame ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,preproject,kernel", EVALUATORS, ids=["%s-pre%d-%s" % (p, int(m), k) for p, m, k in EVALUATORS])
def test_all_ones_grid_is_bitwise_forward(precision, preproject, kernel):
    net = _net(precision, preproject)
    for n, chunk in SHAPES:
        gb = _rays(n)
        want = _forward(net, gb, chunk)
        net.set_occupancy(occ_c.ones(8 if n == 96 else 32))
        got = _skipping(net, gb, chunk)
        for lv in range(2):
            assert len(got[lv]) == len(want[lv]) == 6
            for k, x, y in zip(NAMES, got[lv], want[lv]):
                assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (n, lv, k)
            assert bool(got[2][lv][3].all())
        assert got[3].tolist() == [n * N_LEVEL[0], n * N_LEVEL[1]]


# ---- 3. all zeros: no foreground -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chunk", SHAPES)
def test_all_zeros_grid_has_no_foreground(n, chunk):
    net = _net()
    gb = _rays(n)
    want = _forward(net, gb, chunk)
    net.set_occupancy(occ_c.zeros(32))
    got = _skipping(net, gb, chunk)
    for lv in range(2):
        rgb, fg_rgb, bg_rgb, fg_acc, lam, depth = got[lv]
        assert bool((fg_rgb == 0).all()) and bool((fg_acc == 0).all()) and bool((lam == 1).all())
        assert torch.equal(rgb, bg_rgb)
        assert torch.equal(bg_rgb, want[lv][2]), "the outside-sphere half is never skipped and does not depend on the inside"
        fg_t, fg_w, bg_s, fg_keep, fg_rows = got[2][lv]
        assert not bool(fg_keep.any()) and bool((fg_w == 0).all()) and bool((fg_rows == 0).all())
    assert got[3].tolist() == [0, 0], "the zero-row compact launches"


# ---- 4. a mixed grid -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chunk", SHAPES)
def test_mixed_grid_equals_its_stage_chain(n, chunk):
    base = _base(n, chunk)
    _assert_equals_chain(base["net"], base["gb"], chunk, base["mixed"], base["forward"], "%d rays" % n)


@pytest.mark.parametrize("n,chunk", SHAPES)
def test_mixed_grid_mask_rows_weights_and_visibility(n, chunk):
    base = _base(n, chunk)
    net, gb, grid, got, forward = base["net"], base["gb"], base["grid"], base["mixed"], base["forward"]
    o, d = gb["rays_o"], gb["rays_d"]
    for lv in range(2):
        fg_t, fg_w, bg_s, fg_keep, fg_rows = got[2][lv]
        N = N_LEVEL[lv]
        assert tuple(fg_t.shape) == tuple(fg_w.shape) == tuple(bg_s.shape) == tuple(fg_keep.shape) == (n, N)
        assert fg_keep.dtype == torch.bool and tuple(fg_rows.shape) == (n, N, 4)
        # the mask: bitwise the stage op at the returned positions, and the fp32 restatement away from the cell faces
        assert torch.equal(fg_keep, ops.occupancy_keep(grid, o, d, fg_t)), lv
        face = occ_c.near_face(o.cpu(), d.cpu(), fg_t.cpu(), 32)
        assert int(face.sum()) <= 0.01 * face.numel(), (lv, int(face.sum()))
        want = occ_c.keep_rule(grid, o.cpu(), d.cpu(), fg_t.cpu())
        assert torch.equal(fg_keep.cpu()[~face], want[~face]), lv
        kept, skipped = int(fg_keep.sum()), int((~fg_keep).sum())
        assert kept > n * N // 4 and skipped > n * N // 8, "both states, alternating along the rays"
        assert int(got[3][lv]) == kept
        # kept rows are the evaluator's own, skipped rows are zero and weigh nothing
        rows = net.eval_mlp(lv, gb, fg_t, chunk=chunk)
        net.check_flags()
        assert torch.equal(fg_rows[fg_keep], rows[fg_keep]), lv
        assert bool((fg_rows[~fg_keep] == 0).all()) and bool((fg_w[~fg_keep] == 0).all())
        assert bool((rows[~fg_keep][:, 3] > 0).any()), "the skipped samples had density: the grid matters"
    # the outside-sphere half at level 0 is forward's; rays without a skipped level-0 sample are forward's at level 0
    assert torch.equal(got[0][2], forward[0][2])
    whole0 = got[2][0][3].all(dim=-1)
    for k, x, y in zip(NAMES, got[0], forward[0]):
        assert torch.equal(x[whole0], y[whole0]), k
    changed = int((got[1][0] != forward[1][0]).any(dim=-1).sum())
    print("%d rays: %d differ from forward at level 1, %d keep every level-0 sample" % (n, changed, int(whole0.sum())))
    assert changed >= 20, "the skipping must be visible"


def test_rays_without_a_skipped_sample_are_forward_at_level_0():
    """A grid that clears only cells which the level-0 samples of the first half of the rays never enter: those rays keep every
    level-0 sample and are bitwise `forward`'s at level 0 (level 1 too where no level-1 sample is skipped); the others change."""
    base = _base()
    net, gb, forward = base["net"], base["gb"], base["forward"]
    o, d, t0 = gb["rays_o"].cpu(), gb["rays_d"].cpu(), base["mixed"][2][0][0].cpu()
    cells = occ_c.cell(occ_c.positions(o, d, t0), 32)
    lin = (cells[..., 0] * 32 + cells[..., 1]) * 32 + cells[..., 2]
    grid = occ_c.ones(32)
    grid.view(-1)[lin[48:].reshape(-1)] = False
    grid.view(-1)[lin[:48].reshape(-1)] = True
    try:
        net.set_occupancy(grid)
        got = _skipping(net, gb)
    finally:
        net.set_occupancy(base["grid"])
    whole0 = got[2][0][3].all(dim=-1)
    assert bool(whole0[:48].all()) and 0 < int((~whole0).sum()) <= 48
    for k, x, y in zip(NAMES, got[0], forward[0]):
        assert torch.equal(x[whole0], y[whole0]), k
    whole = whole0 & got[2][1][3].all(dim=-1)
    assert int(whole.sum()) > 0
    for k, x, y in zip(NAMES, got[1], forward[1]):
        assert torch.equal(x[whole], y[whole]), k
    assert int((got[0][1] != forward[0][1]).any(dim=-1).sum()) >= 20 and not bool((got[0][1] != forward[0][1]).any(dim=-1)[whole0].any())


# ---- 5. tile edges -------------------------------------------------------------------------------------------------------------

def _grid_for_count(o, d, t1, level0, want):
    """A G = 256 grid that keeps exactly `want` of the level-1 positions t1 (R,49) and none of the level-0 positions: cells of
    level-1 samples are added one sample at a time, a cell that holds a level-0 sample or would overshoot is passed over."""
    G = 256
    c1 = occ_c.cell(occ_c.positions(o, d, t1), G).reshape(-1, 3)
    c0 = occ_c.cell(occ_c.positions(o, d, level0), G).reshape(-1, 3)
    lin1 = (c1[:, 0] * G + c1[:, 1]) * G + c1[:, 2]
    taken = set(((c0[:, 0] * G + c0[:, 1]) * G + c0[:, 2]).tolist())
    grid = occ_c.zeros(G)
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
def test_tile_edges_of_the_compact_launch(rays, want):
    """Grids at G = 256 built from the rays' own level-1 positions.  With every level-0 sample skipped the level-0 weights are zero
    whatever else the grid holds, so the level-1 positions are those of the all-zeros grid and the kept count is known exactly."""
    net = _net()
    gb = {k: (v[:rays].contiguous() if k in PER_RAY else v) for k, v in _rays(96).items()}
    forward = _forward(net, gb, None)
    if want == "all":
        net.set_occupancy(occ_c.ones(256))
        got = _skipping(net, gb)
        assert got[3].tolist() == [rays * N_LEVEL[0], rays * N_LEVEL[1]]
    else:
        net.set_occupancy(occ_c.zeros(256))
        empty = _skipping(net, gb)
        o, d = gb["rays_o"].cpu(), gb["rays_d"].cpu()
        t0, t1 = empty[2][0][0].cpu(), empty[2][1][0].cpu()
        face = occ_c.near_face(o, d, t1, 256)
        assert int(face.sum()) == 0, "a position on a face of the finest grid: the count below would not be exact"
        net.set_occupancy(_grid_for_count(o, d, t1, t0, want))
        got = _skipping(net, gb)
        assert torch.equal(got[2][1][0], empty[2][1][0]), "the level-1 positions are those of the empty grid"
        assert got[3].tolist() == [0, want] and int(got[2][1][3].sum()) == want
    _assert_equals_chain(net, gb, None, got, forward, "%d rays, %s kept" % (rays, want))


# ---- 6. windows, 7. chunk ------------------------------------------------------------------------------------------------------

def _flat(res):
    return [t for lv in res[:2] for t in lv] + [t for lv in res[2] for t in lv] + [res[3]]


def test_windows_do_not_change_the_result():
    base = _base(300, 128)
    net, gb = base["net"], base["gb"]
    assert net.skip_window is None
    try:
        for window in (128, 1, 299):          # three windows with a ragged last one; one ray a window; a last window of one ray
            net.skip_window = window
            got = _skipping(net, gb, 128)
            assert all(torch.equal(x, y) for x, y in zip(_flat(got), _flat(base["mixed"]))), window
        one = {k: (v[:1].contiguous() if k in PER_RAY else v) for k, v in gb.items()}
        net.skip_window = 128
        small = _skipping(net, one)
        net.skip_window = None
        assert all(torch.equal(x, y) for x, y in zip(_flat(small), _flat(_skipping(net, one)))), "R = 1"
        with pytest.raises(_lib.NeoError):
            net.skip_window = 1 << 20
            net.render_skipping(gb, chunk=128)
    finally:
        net.skip_window = None


def test_chunk_decides_the_direction_rows_of_the_compact_points():
    """chunk = 128 on 300 rays equals its stage chain at that chunk (test_mixed_grid_equals_its_stage_chain[300-128]) - and is not
    the one-chunk frame: the compact rows carry the quirk-Q1 directions of their reference chunk."""
    base = _base(300, 128)
    net, gb = base["net"], base["gb"]
    other = _skipping(net, gb, None)
    assert torch.equal(other[2][0][0], base["mixed"][2][0][0]) and torch.equal(other[2][0][3], base["mixed"][2][0][3])
    assert not torch.equal(other[0][1], base["mixed"][0][1]), "level-0 colours depend on the chunk through the direction rows"
    forward = _forward(net, gb, None)
    _assert_equals_chain(net, gb, None, other, forward, "300 rays, one chunk")


# ---- 8. building a grid --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probes,dilate", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_build_occupancy_is_the_cpu_reduction_of_eval_mlp(probes, dilate):
    G = 16
    net = _net()
    gb = _rays(96)
    M = G * probes
    c, o, d = ops.occupancy_lattice(G, probes, DEV)
    lattice = dict(gb, rays_o=o, rays_d=d, viewdirs=d)
    t = c[None, :].expand(M * M, M).contiguous()
    sigma = torch.maximum(net.eval_mlp(0, lattice, t)[..., 3], net.eval_mlp(1, lattice, t)[..., 3]).reshape(M, M, M)
    net.check_flags()
    assert torch.equal(net._occupancy_sigma(gb, G, probes, points_per_piece=5000), sigma), "pieces do not change a density"
    thr = float(sigma.median())
    want = occ_c.from_sigma(sigma, G, probes, thr, dilate)
    assert net.occupancy is None
    got = net.build_occupancy(gb, G, thr, probes=probes, dilate=dilate)
    assert got.dtype == torch.bool and tuple(got.shape) == (G, G, G)
    assert torch.equal(got.cpu(), want)
    assert 0 < int(want.sum()) < G ** 3 and not bool((want & ~occ_c.sphere_cells(G)).any())
    if dilate == 0:        # (eight probes and a dilation leave no clear cell inside the sphere at the median)
        assert int((want & occ_c.sphere_cells(G)).sum()) < int(occ_c.sphere_cells(G).sum()), "both states occur inside the sphere"
    assert torch.equal(net.occupancy, got) and net.occupancy.data_ptr() != got.data_ptr()
    assert torch.equal(ops.occupancy_from_sigma(sigma, G, thr, probes=probes, dilate=dilate), got)
    # the installed grid is the one the frame reads
    res = _skipping(net, gb)
    assert torch.equal(res[2][0][3], ops.occupancy_keep(got, gb["rays_o"], gb["rays_d"], res[2][0][0]))
    net.close()


# ---- 9. life cycle -------------------------------------------------------------------------------------------------------------

def test_life_cycle_of_the_grid():
    net = _net()
    gb = _rays(96)
    before = _forward(net, gb, None)
    with pytest.raises(_lib.NeoError):
        net.render_skipping(gb)
    grid = occ_c.mixed(32)
    net.set_occupancy(grid.to(DEV))          # a device tensor is as good as a host one
    assert torch.equal(net.occupancy.cpu(), grid) and net.occupancy.is_cuda
    first = _skipping(net, gb)
    after = _forward(net, gb, None)
    for lv in range(2):
        assert all(torch.equal(x, y) for x, y in zip(before[lv], after[lv])), "forward ignores an installed grid"
    assert not torch.equal(first[1][0], before[1][0])
    net.set_occupancy(occ_c.ones(8))         # replacing a grid: another resolution
    assert all(torch.equal(x, y) for x, y in zip(_skipping(net, gb)[1], before[1]))
    net.set_occupancy(None)
    assert net.occupancy is None
    with pytest.raises(_lib.NeoError):
        net.render_skipping(gb)
    net.set_occupancy(grid)
    sc = ec.scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV), sc["image_wh"])
    assert net.occupancy is None, "set_scene clears the grid: it describes one scene"
    with pytest.raises(_lib.NeoError):
        net.render_skipping(gb)
    # ... in the library as well: the C call without a grid keeps everything
    c = net._context(torch.device(DEV))
    keep = torch.zeros(96, 3, dtype=torch.uint8, device=DEV)
    t3 = torch.rand(96, 3, device=DEV)
    assert c.lib.neo_tp_occupancy_keep(c.handle, None, 0, gb["rays_o"].data_ptr(), gb["rays_d"].data_ptr(), t3.data_ptr(), 96, 3,
                                       keep.data_ptr(), c.stream()) == 0
    assert bool((keep == 1).all())
    net.set_occupancy(grid)
    again = _skipping(net, gb)
    assert all(torch.equal(x, y) for x, y in zip(_flat(again), _flat(first)))
    # the frame helper: the fine level and the kept fractions
    frame = render.render_skipping_rays(net, gb, chunk=96)
    assert torch.equal(frame["rgb"], first[1][0]) and torch.equal(frame["depth"], first[1][5]) and torch.equal(frame["acc"], first[1][3])
    frac = frame["kept_fraction"]
    assert frac.is_cuda and frac.dtype == torch.float64 and tuple(frac.shape) == (2,)
    assert all(abs(float(frac[lv]) - int(first[3][lv]) / (96 * N_LEVEL[lv])) < 1e-12 for lv in range(2))
    with pytest.raises(TypeError):
        render.render_skipping_rays(models.NeRF(), gb)
    net.set_occupancy(occ_c.ones(8))
    plain = render.render_rays_test(net, gb, chunk=96)
    same = render.render_skipping_rays(net, gb, chunk=96)
    assert torch.equal(same["rgb"], plain["rgb"]) and torch.equal(same["depth"], plain["depth"]) and same["kept_fraction"].tolist() == [1.0, 1.0]


# ---- 10. rejects ---------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_on_the_host():
    """Every call here returns an error before anything is launched: no kernel sees one of these pointers or shapes."""
    net = _net()
    gb = _rays(96)
    c = net._context(torch.device(DEV))
    lib, h, s = c.lib, c.handle, c.stream()
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = buf.data_ptr()

    def refused(rc, text):
        assert rc != 0
        msg = lib.neo_last_error().decode()
        assert text in msg, msg
    for G in (0, 4, 24, 31, 48, 288, 512, -32):
        refused(lib.neo_tp_set_occupancy(h, p, G, s), "occupancy resolution")
        refused(lib.neo_tp_occupancy_keep(h, p, G, p, p, p, 4, 4, p, s), "occupancy resolution")
        refused(lib.neo_occupancy_from_sigma(h, p, G, 1, 0.5, 0, p, s), "occupancy resolution")
    refused(lib.neo_tp_set_occupancy(None, p, 8, s), "null context")
    for bad in ((-1, 4), (4, 0)):
        refused(lib.neo_tp_occupancy_keep(h, p, 8, p, p, p, bad[0], bad[1], p, s), "bad shape")
    refused(lib.neo_tp_occupancy_keep(h, p, 8, p, p, p, 1 << 22, 1 << 10, p, s), "too many points")
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        refused(lib.neo_tp_occupancy_keep(h, p, 8, args[0], args[1], args[2], 4, 4, args[3], s), "null pointer")
    assert lib.neo_tp_occupancy_keep(h, p, 8, None, None, None, 0, 4, None, s) == 0          # no rays: nothing to do
    for probes in (0, 5):
        refused(lib.neo_occupancy_from_sigma(h, p, 8, probes, 0.5, 0, p, s), "probes")
    for dil in (-1, 5):
        refused(lib.neo_occupancy_from_sigma(h, p, 8, 1, 0.5, dil, p, s), "dilation")
    refused(lib.neo_occupancy_from_sigma(h, p, 8, 1, float("nan"), 0, p, s), "NaN")
    refused(lib.neo_occupancy_from_sigma(h, None, 8, 1, 0.5, 0, p, s), "null pointer")
    refused(lib.neo_occupancy_from_sigma(h, p, 8, 1, 0.5, 0, None, s), "null pointer")
    for w in (-1, 65537):
        refused(lib.neo_tp_set_skip_window(h, w), "skip window")
    # the frame call: the shared preamble's checks, in its order
    poses, NV, focal, cx, cy = net._camera_args(gb)
    o, d, v = (gb[k].data_ptr() for k in PER_RAY)
    lvl = _lib.TpLevelOut()
    frame = lambda R=96, chunk=96, nc=ec.N_COARSE, nf=ec.N_FINE, o=o, nv=NV: lib.neo_tp_render_skipping(
        h, o, d, v, R, chunk, poses, nv, focal, cx, cy, nc, nf, ctypes.byref(lvl), ctypes.byref(lvl), None, None, None, s)
    refused(frame(R=-1), "bad ray count / chunk")
    refused(frame(chunk=0), "bad ray count / chunk")
    refused(frame(nc=2), "unsupported sample counts")
    refused(frame(o=None), "null pointer")
    refused(frame(nv=NV + 1), "NV differs from the uploaded scene")
    assert frame(R=0) == 0
    torch.cuda.synchronize()
    assert c.poll_flags() == 0
    # Python: a grid on another module's scene is not carried along, a wrong argument is a ValueError before the device is touched
    for bad in (occ_c.ones(8).float(), occ_c.ones(8)[:4], torch.ones(24, 24, 24, dtype=torch.bool)):
        with pytest.raises(ValueError):
            net.set_occupancy(bad)
    with pytest.raises(ValueError):
        net.build_occupancy(gb, 16, 1.0, probes=9)
    net.close()


# ---- 11. run behaviour ---------------------------------------------------------------------------------------------------------

def test_skipping_calls_are_repeatable_chunk_and_overlap_neutral_and_synchronise_nothing():
    base = _base()
    net, gb = base["net"], base["gb"]
    again = _skipping(net, gb)
    assert all(torch.equal(x, y) for x, y in zip(_flat(again), _flat(base["mixed"])))
    assert net.overlap_calls
    net.overlap_calls = False
    try:
        off = _skipping(net, gb)
    finally:
        net.overlap_calls = True
    assert all(torch.equal(x, y) for x, y in zip(_flat(off), _flat(base["mixed"])))
    # the reference-style loop: three calls of 32 rays, each one reference chunk, in flight on alternating lanes; no blocking wait
    whole = _skipping(net, gb, 32)
    ctx = net._context(torch.device(DEV))
    before = ctx.sync_count()
    parts, kept = [], []
    for i in range(0, 96, 32):
        part = {k: (v[i:i + 32] if k in PER_RAY else v) for k, v in gb.items()}
        parts.append(net.render_skipping(part, chunk=32, return_samples="rows"))
        kept.append(net.last_skip_kept)
    assert ctx.sync_count() == before, "a skipping call blocked on the device"
    net.check_flags()
    for lv in range(2):
        for j in range(6):
            assert torch.equal(torch.cat([p[lv][j] for p in parts]), whole[lv][j]), (lv, j)
        for j in range(5):
            assert torch.equal(torch.cat([p[2][lv][j] for p in parts]), whole[2][lv][j]), (lv, j)
    assert torch.equal(sum(kept), whole[3])
    # neither cull_background nor compute_extras is read
    net.cull_background = 1e-2
    net.compute_extras = True
    try:
        same = _skipping(net, gb)
    finally:
        net.cull_background = None
        net.compute_extras = False
    assert len(same[0]) == len(same[1]) == 6 and all(torch.equal(x, y) for x, y in zip(_flat(same), _flat(base["mixed"])))
