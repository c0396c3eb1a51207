"""GPU: training the vanilla NeRF through its occupancy grid (`marching.MarchingNeRF.render_train_marching`, `init_occupancy`,
`update_occupancy`; include/neo360_hip.h: VANILLA MARCHING TRAINING) and the stage functions the call is made of.

Inputs: tests/vanilla_march_cases.py (scene, rays, boxes, grids, the masked oracle) through tests/vanilla_train_march_cases.py -
R in {1, 63, 64, 65, 257}, the count pairs 3 + 4, 16 + 24 and 7 + 64, G in {8, 32} (256 where only points are generated).
tests/test_vanilla_train_march_cpu.py asserts that the mixed grid keeps and skips at both levels and that the counted positions
keep exactly their number, so nothing here passes vacuously.

Bounds.  Everything the library states bit for bit - the keep mask, the compaction, the encodings of the kept samples, the
activations of the scattered rows, the call without savings against `training.nerf_render_train`, the probe points' cells, the
running density - is `torch.equal`.  The call with a mixed grid is compared with the masked CPU oracle at the project's parity
bound 1e-4.  Gradients take the criterion of test_vanilla_training_step_gradients_vs_fp64_autograd: weight gradients are summed
with atomics, so no bitwise equality is asked of them."""
import pytest
import torch

import occupancy_cases as oc
import oracle
import vanilla_march_cases as vc
import vanilla_train_march_cases as tm
from neo360_amd import _lib, marching, ops, synth, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("rgb", "acc", "depth")
SHAPES = [(c, n) for c in tm.COUNTS for n in tm.RAYS]
SHAPE_IDS = ["%d+%d-%d" % (c[0], c[1], n) for c, n in SHAPES]

_NETS = {}


def _net(counts):
    if counts not in _NETS:
        net = marching.MarchingNeRF(num_coarse_samples=counts[0], num_fine_samples=counts[1]).to(DEV)
        net.load_state_dict(tm.state())
        _NETS[counts] = net
    net = _NETS[counts]
    net.noise_std = 0.0
    net.set_occupancy(None)
    return net


def _rays(n):
    return {k: v.to(DEV) for k, v in vc.rays(n).items()}


def _dev(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _dir_enc(vd):
    return ops.pos_enc(vd, 0, 4)


def _points(o, d, t):
    return o[:, None, :] + t[..., None] * d[:, None, :]


def _assert_rows(occ, box, clip, o, d, t, what, kept=None):
    """The row builder against the public ops, bitwise; rows behind the count keep their sentinel.  Returns the count."""
    B, N = t.shape
    enc = _dir_enc(d)
    out = (torch.full((B * N,), -7, dtype=torch.int32, device=DEV), torch.full((B * N, 63), -7.0, device=DEV),
           torch.full((B * N, 27), -7.0, device=DEV))
    keep, count, index, x_enc, cond = marching.train_rows(occ, box, o, d, t, enc, clip, out=out)
    assert index is out[0] and x_enc is out[1] and cond is out[2]
    assert keep.dtype == torch.bool and tuple(keep.shape) == (B, N) and count.dtype == torch.int32 and tuple(count.shape) == (1,)
    assert torch.equal(keep, marching.occupancy_keep_box(occ, box, o, d, t, clip)), (what, "keep")
    K = int(count.item())
    assert K == int(keep.sum()), (what, "count")
    if kept is not None:
        assert K == kept, (what, K, kept)
    flat = torch.nonzero(keep.reshape(-1)).reshape(-1)
    assert torch.equal(index[:K].long(), flat), (what, "index")
    assert torch.equal(x_enc[:K], ops.pos_enc(_points(o, d, t), 0, 10).reshape(B * N, 63)[flat]), (what, "x_enc")
    assert torch.equal(cond[:K], enc[flat // N]), (what, "cond")
    assert bool((index[K:] == -7).all()) and bool((x_enc[K:] == -7.0).all()) and bool((cond[K:] == -7.0).all()), (what, "behind the count")
    # the allocating form returns the same live rows
    again = marching.train_rows(occ, box, o, d, t, enc, clip)
    assert torch.equal(again[0], keep) and int(again[1].item()) == K
    assert torch.equal(again[2][:K], index[:K]) and torch.equal(again[3][:K], x_enc[:K]) and torch.equal(again[4][:K], cond[:K])
    return K


# ---- 1. the row builder ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,n", SHAPES, ids=SHAPE_IDS)
def test_row_builder_equals_the_public_ops(counts, n):
    b = _rays(n)
    o, d = b["rays_o"], b["viewdirs"]
    net = _net(counts)
    with torch.no_grad():
        _, (t0, t1) = training.nerf_render_train(net, b, True, False, vc.NEAR, vc.FAR, seed=11, return_samples=True)
    seen = []
    for t in (tm.level0(counts, n).to(DEV), t0, t1):
        for G in tm.GRIDS:
            for clip in (False, True):
                seen.append(_assert_rows(vc.mixed(G), vc.BOX, clip, o, d, t, ("mixed", G, clip)))
                _assert_rows(oc.ones(G), vc.BOX, clip, o, d, t, ("ones", G, clip), kept=None if clip else t.numel())
            _assert_rows(oc.zeros(G), vc.BOX, True, o, d, t, ("empty", G), kept=0)
            _assert_rows(oc.ones(G), vc.FAR_AWAY, False, o, d, t, ("ones far away", G), kept=t.numel())
            _assert_rows(oc.ones(G), vc.FAR_AWAY, True, o, d, t, ("ones far away, clip", G), kept=0)
        _assert_rows(None, None, False, o, d, t, "no grid", kept=t.numel())
    assert any(0 < k for k in seen)


@pytest.mark.parametrize("want", tm.EXACT, ids=lambda w: "all" if w is None else str(w))
def test_row_builder_at_exact_counts(want):
    b, t, kept = tm.counted_case(want)
    b = _dev(b)
    assert _assert_rows(oc.ones(8), vc.SMALL, True, b["rays_o"], b["viewdirs"], t.to(DEV), ("counted", want), kept=kept) == kept


def test_row_builder_takes_no_rays():
    z = torch.zeros(0, 3, device=DEV)
    keep, count, index, x_enc, cond = marching.train_rows(oc.ones(8), vc.BOX, z, z, torch.zeros(0, 5, device=DEV), torch.zeros(0, 27, device=DEV))
    assert tuple(keep.shape) == (0, 5) and int(count.item()) == 0 and index.numel() == x_enc.numel() == cond.numel() == 0


# ---- 2. scatter_activate -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", (False, True), ids=("quiet", "noise"))
@pytest.mark.parametrize("n", (1, 65, 257))
def test_scatter_activate_equals_activate_under_the_mask(n, noise):
    N, P = 9, n * 9
    keep = synth.uniform(5, "keep", (n, N), 0.0, 1.0).to(DEV) < 0.4
    if n == 1:
        keep[0, 3] = True
    index = torch.nonzero(keep.reshape(-1)).reshape(-1).to(torch.int32)
    K = index.shape[0]
    assert 0 < K < P or n == 1
    dense_rgb = synth.uniform(6, "raw_rgb", (P, 3), -3.0, 3.0).to(DEV)
    dense_sigma = synth.uniform(7, "raw_sigma", (P,), -4.0, 25.0).to(DEV)      # beyond softplus' threshold 20 as well
    u = synth.uniform(8, "noise", (P,), 0.0, 1.0).to(DEV) if noise else None
    scale = 0.75 if noise else 0.0
    g_out = synth.uniform(9, "g", (P, 4), -1.0, 1.0).to(DEV)
    with torch.enable_grad():
        a, s = dense_rgb.clone().requires_grad_(True), dense_sigma.clone().requires_grad_(True)
        want = training.activate(a, s, u, scale)
        g_a, g_s = torch.autograd.grad(want, [a, s], g_out)
        rr, rs = dense_rgb[index.long()].clone().requires_grad_(True), dense_sigma[index.long()].clone().requires_grad_(True)
        got = marching.scatter_activate(rr, rs, index, P, u, scale)
        g_rr, g_rs = torch.autograd.grad(got, [rr, rs], g_out)
    assert torch.equal(got, torch.where(keep.reshape(-1, 1), want, torch.zeros_like(want)))
    assert torch.equal(g_rr, g_a[index.long()]) and torch.equal(g_rs, g_s[index.long()])
    # a (K,1) raw_sigma - what nerf_mlp_rows returns - gives the same rows and a (K,1) gradient
    with torch.enable_grad():
        rs1 = dense_sigma[index.long()].reshape(K, 1).clone().requires_grad_(True)
        got1 = marching.scatter_activate(dense_rgb[index.long()], rs1, index, P, u, scale)
        (g1,) = torch.autograd.grad(got1, [rs1], g_out)
    assert torch.equal(got1, got) and tuple(g1.shape) == (K, 1) and torch.equal(g1.reshape(-1), g_rs)


def test_scatter_activate_of_no_rows_is_all_zeros():
    empty = torch.zeros(0, dtype=torch.int32, device=DEV)
    with torch.enable_grad():
        rr, rs = torch.zeros(0, 3, device=DEV, requires_grad=True), torch.zeros(0, 1, device=DEV, requires_grad=True)
        got = marching.scatter_activate(rr, rs, empty, 70, torch.rand(70, device=DEV), 0.5)
        g_rr, g_rs = torch.autograd.grad(got, [rr, rs], torch.ones(70, 4, device=DEV))
    assert tuple(got.shape) == (70, 4) and bool((got == 0).all())
    assert tuple(g_rr.shape) == (0, 3) and tuple(g_rs.shape) == (0, 1)


# ---- 3. the call without savings ------------------------------------------------------------------------------------------------------

def _train_call(net, b, randomized, white, seed, **kw):
    with torch.no_grad():
        out, used = net.render_train_marching(b, randomized, white, vc.NEAR, vc.FAR, seed=seed, return_samples=True, **kw)
    return out, used


@pytest.mark.parametrize("counts,n", SHAPES, ids=SHAPE_IDS)
def test_call_without_savings_equals_nerf_render_train(counts, n):
    net = _net(counts)
    b = _rays(n)
    total = (n * (counts[0] + 1), n * (counts[0] + 1 + counts[1]))
    for randomized, std in ((False, 0.0), (True, 0.0), (True, 0.75)):
        for white in (False, True):
            net.noise_std = std
            net.set_occupancy(None)
            with torch.no_grad():
                want, ts = training.nerf_render_train(net, b, randomized, white, vc.NEAR, vc.FAR, seed=21, return_samples=True)
            for what in ("no grid", "grid=False", "all ones", "far away"):
                kw = {}
                if what == "grid=False":
                    net.set_occupancy(vc.mixed(8), vc.BOX, True)
                    kw = dict(grid=False)
                elif what == "all ones":
                    net.set_occupancy(oc.ones(32), vc.BOX, False)
                elif what == "far away":
                    net.set_occupancy(oc.zeros(8), vc.FAR_AWAY, False)
                else:
                    net.set_occupancy(None)
                got, used = _train_call(net, b, randomized, white, 21, **kw)
                for lv in range(2):
                    assert torch.equal(used[lv][0], ts[lv]), (what, randomized, std, white, lv, "positions")
                    assert bool(used[lv][1].all())
                    for nm, x, y in zip(NAMES, got[lv], want[lv]):
                        assert torch.equal(x, y), (what, randomized, std, white, lv, nm)
                assert net.last_train_kept == total
    net.noise_std = 0.0
    net.set_occupancy(None)


# ---- 4. the call with the mixed grid ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,n", SHAPES, ids=SHAPE_IDS)
def test_call_with_the_mixed_grid_matches_the_masked_oracle(counts, n):
    net = _net(counts)
    b_c = vc.rays(n)
    b = _dev(b_c)
    for G in tm.GRIDS:
        occ = vc.mixed(G)
        net.set_occupancy(occ, vc.BOX, True)
        for randomized, white in ((False, False), (True, True)):
            got, used = _train_call(net, b, randomized, white, 33)
            (t0, m0), (t1, m1) = used
            for t, m in used:
                assert torch.equal(m, marching.occupancy_keep_box(occ, vc.BOX, b["rays_o"], b["viewdirs"], t, True))
            want, _ = vc.oracle_render_marching(tm.state(), b_c, counts, 0.0, white_bkgd=white, samples=(t0.cpu(), t1.cpu()),
                                                masks=(m0.cpu(), m1.cpu()))
            for lv in range(2):
                for nm, x, y in zip(NAMES, got[lv], want[lv]):
                    err = float((x.cpu() - y).abs().max())
                    print("%s %d rays G %d %s level %d %s: %.3e" % (counts, n, G, "random" if randomized else "fixed", lv, nm, err))
                    assert err < 1e-4, (G, randomized, lv, nm, err)
            sums = (int(m0.sum()), int(m1.sum()))
            assert net.last_train_kept == sums
            assert 0 < sums[0] < m0.numel() and 0 < sums[1] < m1.numel()
    net.set_occupancy(None)


# ---- 5. gradients ----------------------------------------------------------------------------------------------------------------------

def _oracle_step_grads(b_c, counts, used, target, dtype):
    cv = lambda v: v.to(dtype)
    sd = tm.state()
    names = sorted(sd)
    with torch.enable_grad():
        pp = {k: cv(v).clone().requires_grad_(True) for k, v in sd.items()}
        want, _ = vc.oracle_render_marching(pp, {k: cv(v) for k, v in b_c.items()}, counts, 0.0,
                                            samples=tuple(cv(t.cpu()) for t, _ in used), masks=tuple(m.cpu() for _, m in used))
        loss = tm.mse2(want, cv(target))
        return float(loss.detach()), torch.autograd.grad(loss, [pp[k] for k in names])


@pytest.mark.parametrize("grid", ("mixed", "ones"))
def test_training_step_gradients_vs_fp64_autograd_of_the_masked_oracle(grid):
    counts, R = (16, 24), 256
    net = _net(counts)
    net.set_occupancy(vc.mixed(32) if grid == "mixed" else oc.ones(32), vc.BOX, True)
    b_c = vc.rays(R)
    b = _dev(b_c)
    target = synth.uniform(91, "vanilla_target", (R, 3), 0.0, 1.0)
    names = sorted(tm.state())
    try:
        with torch.enable_grad():
            for p in net.parameters():
                p.requires_grad_(True)
                p.grad = None
            out, used = net.render_train_marching(b, True, False, vc.NEAR, vc.FAR, seed=5, return_samples=True)
            assert out[0][0].requires_grad and out[1][0].requires_grad
            loss = tm.mse2(out, target.to(DEV))
            params = dict(net.named_parameters())
            g_lib = torch.autograd.grad(loss, [params[k] for k in names])
    finally:
        for p in net.parameters():
            p.requires_grad_(False)
    kept = net.last_train_kept
    total = (R * 17, R * 41)
    if grid == "mixed":
        assert 0 < kept[0] < total[0] and 0 < kept[1] < total[1]
    else:
        assert all(0 < k <= n for k, n in zip(kept, total))
    loss64, g64 = _oracle_step_grads(b_c, counts, used, target, torch.float64)
    _, g32 = _oracle_step_grads(b_c, counts, used, target, torch.float32)
    assert abs(float(loss.detach()) - loss64) < 1e-5 * max(1.0, abs(loss64))
    tm.grad_criterion(names, g_lib, g64, g32)
    net.set_occupancy(None)


@pytest.mark.parametrize("K", (1, 255, 256, 257))
def test_nerf_mlp_rows_gradients_vs_fp64_autograd(K):
    net = _net((16, 24))
    sd = tm.state()
    names = sorted(k for k in sd if k.startswith("coarse_mlp."))
    pts = synth.uniform(41, "pts", (K, 3), -1.0, 1.0)
    dirs = torch.nn.functional.normalize(synth.uniform(42, "dirs", (K, 3), -1.0, 1.0), dim=-1)
    x_c, c_c = oracle.encoding.pos_enc(pts, 0, 10), oracle.encoding.pos_enc(dirs, 0, 4)
    w_rgb, w_sigma = synth.uniform(43, "w_rgb", (K, 3), -1.0, 1.0), synth.uniform(44, "w_sigma", (K, 1), -1.0, 1.0)
    try:
        with torch.enable_grad():
            for p in net.parameters():
                p.requires_grad_(True)
            x = x_c.to(DEV).requires_grad_(True)
            raw_rgb, raw_sigma = marching.nerf_mlp_rows(net.coarse_mlp, x, c_c.to(DEV))
            assert tuple(raw_rgb.shape) == (K, 3) and tuple(raw_sigma.shape) == (K, 1)
            loss = (raw_rgb * w_rgb.to(DEV)).sum() + (raw_sigma * w_sigma.to(DEV)).sum()
            params = dict(net.named_parameters())
            g_lib = torch.autograd.grad(loss, [params[k] for k in names] + [x])
    finally:
        for p in net.parameters():
            p.requires_grad_(False)

    def oracle_grads(dtype):
        cv = lambda v: v.to(dtype)
        with torch.enable_grad():
            pp = {k: cv(v).clone().requires_grad_(True) for k, v in sd.items()}
            xx = cv(x_c).clone().requires_grad_(True)
            rgb, sigma = oracle.mlp.vanilla_mlp(pp, "coarse_mlp.", xx[:, None, :], cv(c_c))      # K rays of one sample: a cond row each
            loss = (rgb[:, 0] * cv(w_rgb)).sum() + (sigma[:, 0] * cv(w_sigma)).sum()
            return float(loss.detach()), torch.autograd.grad(loss, [pp[k] for k in names] + [xx])

    loss64, g64 = oracle_grads(torch.float64)
    _, g32 = oracle_grads(torch.float32)
    assert abs(float(loss.detach()) - loss64) < 1e-4 * max(1.0, abs(loss64))
    tm.grad_criterion(names + ["x_enc"], g_lib, g64, g32)


# ---- 6. the empty grid -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("white", (False, True), ids=("black", "white"))
def test_empty_grid_with_clip_evaluates_nothing(white):
    counts, R = (16, 24), 65
    net = _net(counts)
    net.set_occupancy(oc.zeros(8), vc.BOX, True)
    b = _rays(R)
    try:
        with torch.enable_grad():
            for p in net.parameters():
                p.requires_grad_(True)
                p.grad = None
            out = net.render_train_marching(b, True, white, vc.NEAR, vc.FAR, seed=3)
            tm.mse2(out, torch.full((R, 3), 0.5, device=DEV)).backward()
        grads = [p.grad for p in net.parameters()]
    finally:
        for p in net.parameters():
            p.requires_grad_(False)
            p.grad = None
    assert net.last_train_kept == (0, 0)
    for lv in range(2):
        assert bool((out[lv][0] == (1.0 if white else 0.0)).all()) and bool((out[lv][1] == 0).all())
    assert len(grads) == 24 * 2 and all(g is not None and bool((g == 0).all()) for g in grads)
    net.check_flags()
    assert net._context(torch.device(DEV, torch.cuda.current_device())).poll_flags() == 0
    net.set_occupancy(None)


# ---- 7. probes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("box", (vc.BOX, vc.SMALL, vc.FAR_AWAY), ids=("box", "small", "far_away"))
@pytest.mark.parametrize("G", (8, 32, 256))
def test_probe_points_lie_in_their_own_cells(G, box):
    pts = marching.occupancy_probes(box, G, 7, 3, DEV)
    assert tuple(pts.shape) == (G ** 3, 3) and pts.dtype == torch.float32
    ax = torch.arange(G, device=DEV, dtype=torch.float32)
    cells = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
    assert torch.equal(vc.cell_box(pts, box, G), cells)
    assert torch.equal(marching.occupancy_probes(box, G, 7, 3, DEV), pts), "the same (seed, step) repeats bitwise"
    assert not torch.equal(marching.occupancy_probes(box, G, 7, 4, DEV), pts), "another step differs"
    assert not torch.equal(marching.occupancy_probes(box, G, 8, 3, DEV), pts), "another seed differs"
    lo = torch.tensor(box[0], dtype=torch.float64, device=DEV)
    w = (torch.tensor(box[1], dtype=torch.float64, device=DEV) - lo) / G
    frac = (pts.double() - lo) / w - cells.double()
    for a in range(3):
        assert float(frac[:, a].min()) < 0.05 and float(frac[:, a].max()) > 0.95, (a, float(frac[:, a].min()), float(frac[:, a].max()))
    # the offsets are the library's uniforms: key seed, counter (cell, step, 8 + axis, 0)
    if G == 8:
        u = torch.stack([training.rand_uniform(7, 8 + a, G ** 3, 4)[:, 3] for a in range(3)], dim=-1)
        want, _ = tm.probe_points(box, G, u.cpu(), torch.float32)
        plain = (vc.cell_box(want, box, G) == cells.cpu()).to(DEV)      # candidates that need no pulling back: the formula, bitwise
        assert int(plain.sum()) >= plain.numel() - 3 and torch.equal(pts[plain], want.to(DEV)[plain])


# ---- 8. update_occupancy ------------------------------------------------------------------------------------------------------------

def _probe_sigma(net, pts):
    n = pts.shape[0]
    dirs = torch.zeros(n, 3, device=DEV)
    dirs[:, 0] = 1.0      # any direction: t = 0, and a vanilla density does not read it
    count = torch.full((1,), n, dtype=torch.int32, device=DEV)
    z = torch.zeros(n, device=DEV)
    return torch.maximum(marching.eval_points(net, 0, pts, dirs, z, count)[:, 3], marching.eval_points(net, 1, pts, dirs, z, count)[:, 3])


@pytest.mark.parametrize("G", tm.GRIDS)
def test_update_occupancy_follows_the_weights(G):
    counts = (16, 24)
    net = marching.MarchingNeRF(num_coarse_samples=counts[0], num_fine_samples=counts[1]).to(DEV)
    net.load_state_dict(tm.state())
    with pytest.raises(_lib.NeoError):
        net.update_occupancy(0.5)
    net.init_occupancy(vc.BOX, G, clip=True)
    assert bool(net.occupancy.all()) and bool((net.occupancy_density == 0).all()) and tuple(net.occupancy_density.shape) == (G, G, G)
    decay, seed, dilate = 0.98, 13, 1
    sig = [_probe_sigma(net, marching.occupancy_probes(vc.BOX, G, seed, step, DEV)).reshape(G, G, G) for step in range(3)]
    thr = float(sig[0].median())          # a threshold that splits the cells of THIS scene
    want = torch.zeros(G, G, G, device=DEV)
    for step in range(3):
        grid = net.update_occupancy(thr, decay=decay, dilate=dilate, seed=seed)
        want = torch.maximum(want * decay, sig[step])
        assert torch.equal(net.occupancy_density, want), (step, "density")
        assert torch.equal(grid, marching.occupancy_from_sigma_box(want, G, thr, 1, dilate)) and torch.equal(net.occupancy, grid)
        if step == 0:
            assert torch.equal(want, sig[0])
    assert 0 < int(grid.sum())
    # a cell cleared by hand comes back: every cell is probed at every update
    cell = tuple(int(v) for v in torch.nonzero(want == want.max())[0])
    assert decay * float(want[cell]) > thr, "the densest cell stays above the threshold for one more update, whatever its next probe"
    cleared = grid.clone()
    cleared[cell] = False
    net.set_occupancy(cleared, vc.BOX, True)
    assert not bool(net.occupancy[cell])
    grid = net.update_occupancy(thr, decay=decay, dilate=dilate, seed=seed)
    assert bool(grid[cell]) and bool(net.occupancy[cell])
    # emptied weights: a cell clears at exactly the update where decay^n density first is <= thr
    low = tm.state()
    for k in ("coarse_mlp.density_layer.bias", "fine_mlp.density_layer.bias"):
        low[k] = low[k] - 60.0
    net.load_state_dict(low)
    density = net.occupancy_density
    step0 = 4
    assert float(_probe_sigma(net, marching.occupancy_probes(vc.BOX, G, seed, step0, DEV)).max()) < 1e-3 * thr
    top = float(density.max())
    assert top > thr
    n_clear, d = 0, density.clone()
    while bool((d > thr).any()):
        d = d * decay
        n_clear += 1
        assert n_clear < 200
    for i in range(1, n_clear + 1):
        grid = net.update_occupancy(thr, decay=decay, dilate=0, seed=seed)
        assert bool(grid.any()) == (i < n_clear), (i, n_clear)
    net.close()


# ---- 9. a short Adam loop ------------------------------------------------------------------------------------------------------------

def test_twenty_adam_steps_with_a_running_grid():
    counts, R = (16, 24), 256
    net = marching.MarchingNeRF(num_coarse_samples=counts[0], num_fine_samples=counts[1], noise_std=0.5).to(DEV)
    net.load_state_dict(tm.state())
    net.init_occupancy(vc.BOX, 32, clip=True)
    b = _rays(R)
    target = synth.uniform(91, "vanilla_target", (R, 3), 0.0, 1.0).to(DEV)
    total = (R * 17, R * 41)
    with torch.no_grad():
        pts = marching.occupancy_probes(vc.BOX, 32, 1, 0, DEV)
        thr = float(_probe_sigma(net, pts).median())
    with torch.enable_grad():
        for p in net.parameters():
            p.requires_grad_(True)
        opt = torch.optim.Adam(net.parameters(), lr=5e-4)
        for step in range(20):
            if step % 5 == 0:
                net.update_occupancy(thr)
            opt.zero_grad()
            out = net.render_train_marching(b, True, False, vc.NEAR, vc.FAR, seed=100 + step)
            loss = tm.mse2(out, target)
            loss.backward()
            opt.step()
            assert bool(torch.isfinite(loss)), step
            assert all(0 < k <= n for k, n in zip(net.last_train_kept, total)), (step, net.last_train_kept)
    net.check_flags()
    net.close()


# ---- 10. layouts ---------------------------------------------------------------------------------------------------------------------

def _strided(x):
    wide = torch.zeros(*x.shape[:-1], 2 * x.shape[-1], dtype=x.dtype, device=x.device)
    wide[..., ::2] = x
    return wide[..., ::2]


def _misaligned(x):
    flat = torch.zeros(x.numel() + 1, dtype=x.dtype, device=x.device)
    flat[1:] = x.reshape(-1)
    return flat[1:].reshape(x.shape)


def test_layouts_and_dtypes_give_the_dense_fp32_result():
    n, counts = 65, (16, 24)
    b = _rays(n)
    o, d = b["rays_o"], b["viewdirs"]
    t = tm.level0(counts, n).to(DEV)
    enc = _dir_enc(d)
    occ = vc.mixed(8)
    base = marching.train_rows(occ, vc.BOX, o, d, t, enc, True)
    K = int(base[1].item())
    h = lambda x: x.half().float()      # values fp16 holds exactly, so that the fp16 and the fp32 call see the same numbers
    for what, f in (("strided", _strided), ("misaligned", _misaligned), ("fp64", lambda x: x.double())):
        got = marching.train_rows(occ, vc.BOX, f(o), f(d), f(t), f(enc), True)
        assert int(got[1].item()) == K and all(torch.equal(x[:K], y[:K]) for x, y in zip(got[2:], base[2:])) and torch.equal(got[0], base[0]), what
    base16 = marching.train_rows(occ, vc.BOX, h(o), h(d), h(t), h(enc), True)
    got16 = marching.train_rows(occ, vc.BOX, o.half(), d.half(), t.half(), enc.half(), True)
    K16 = int(base16[1].item())
    assert int(got16[1].item()) == K16 and all(torch.equal(x[:K16], y[:K16]) for x, y in zip(got16[2:], base16[2:])), "fp16"
    # the MLP rows and the scatter
    net = _net(counts)
    x_enc, cond, index = base[3][:K], base[4][:K], base[2][:K]
    rgb, sigma = marching.nerf_mlp_rows(net.coarse_mlp, x_enc, cond)
    packed = marching.scatter_activate(rgb, sigma, index, t.numel())
    for what, f in (("strided", _strided), ("misaligned", _misaligned), ("fp64", lambda x: x.double())):
        r2, s2 = marching.nerf_mlp_rows(net.coarse_mlp, f(x_enc), f(cond))
        assert torch.equal(r2, rgb) and torch.equal(s2, sigma), what
        assert torch.equal(marching.scatter_activate(f(rgb), f(sigma), _misaligned(index) if what == "misaligned" else index, t.numel()), packed), what
    r16, s16 = marching.nerf_mlp_rows(net.coarse_mlp, x_enc.half(), cond.half())
    rh, sh = marching.nerf_mlp_rows(net.coarse_mlp, h(x_enc), h(cond))
    assert torch.equal(r16, rh) and torch.equal(s16, sh)
    assert torch.equal(marching.scatter_activate(rgb.half(), sigma.half(), index, t.numel()), marching.scatter_activate(h(rgb), h(sigma), index, t.numel()))
    # mismatched shapes are refused by name
    with pytest.raises(ValueError, match="dirs must have shape"):
        marching.train_rows(occ, vc.BOX, o, d[:-1], t, enc, True)
    with pytest.raises(ValueError, match="t must have shape"):
        marching.train_rows(occ, vc.BOX, o, d, t[:-1], enc, True)
    with pytest.raises(ValueError, match="dir_enc must have shape"):
        marching.train_rows(occ, vc.BOX, o, d, t, enc[:, :26], True)
    with pytest.raises(ValueError, match="at least one sample"):
        marching.train_rows(occ, vc.BOX, o, d, t[:, :0], enc, True)
    with pytest.raises(ValueError, match=r"out\[1\] \(x_enc\) must have shape"):
        marching.train_rows(occ, vc.BOX, o, d, t, enc, True, out=(base[2], base[3][:-1], base[4]))
    with pytest.raises(ValueError, match="cond must have shape"):
        marching.nerf_mlp_rows(net.coarse_mlp, x_enc, cond[:-1])
    with pytest.raises(ValueError, match="raw_rgb must have shape"):
        marching.scatter_activate(rgb[:-1], sigma, index, t.numel())
    with pytest.raises(ValueError, match="raw_sigma must have shape"):
        marching.scatter_activate(rgb, sigma[:-1], index, t.numel())
    with pytest.raises(ValueError, match="noise must hold"):
        marching.scatter_activate(rgb, sigma, index, t.numel(), torch.zeros(3, device=DEV), 0.5)
    with pytest.raises(ValueError, match="cannot be scattered"):
        marching.scatter_activate(rgb, sigma, index, K - 1)
    with pytest.raises(ValueError, match="viewdirs must have shape"):
        net.render_train_marching(dict(b, viewdirs=d[:3]), False, False, vc.NEAR, vc.FAR)
    other = marching.MarchingNeRF(num_coarse_samples=16, num_fine_samples=24).to(DEV)
    other.load_state_dict(tm.state())
    other.set_occupancy(occ, vc.BOX, True)
    other._occ_ctx = net._context(torch.device(DEV, torch.cuda.current_device()))      # a grid installed through another context
    with pytest.raises(_lib.NeoError, match="does not belong"):
        other.render_train_marching(b, False, False, vc.NEAR, vc.FAR)
    other.render_train_marching(b, False, False, vc.NEAR, vc.FAR, grid=False)
    other.close()
