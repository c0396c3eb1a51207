"""CPU: training through the vanilla occupancy grid (include/neo360_hip.h: VANILLA MARCHING TRAINING) - the declarations, the
host-side refusals of every new function, the masked oracle's fp64 gradients, and that the inputs of
tests/test_gpu_vanilla_train_march.py cannot pass vacuously.  No test here needs a device."""
import os
import re

import pytest
import torch

from conftest import ROOT
import occupancy_cases as oc
import oracle
import vanilla_march_cases as vc
import vanilla_train_march_cases as tm
from neo360_amd import _lib, marching, models

ENTRIES = ("neo_vanilla_train_rows", "neo_vanilla_train_scatter", "neo_vanilla_train_scatter_backward", "neo_vanilla_grid_probes",
           "neo_vanilla_density_update")


def test_header_declares_and_ctypes_binds_the_entry_points(built_lib):
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
        assert m, "%s is not declared in include/neo360_hip.h" % name
        assert len(_lib.SIGNATURES[name][1]) == len([p for p in m.group(1).split(",") if p.strip()]), name
        assert hasattr(_lib.load(), name)
    assert _lib.load().neo_abi_version() == 1
    for phrase in ("VANILLA MARCHING TRAINING", "ROW BUILDER", "PROBE POINTS", "PULLED BACK", "stream_id = 8 + a", "RUNNING DENSITY"):
        assert phrase in text, phrase
    # the scatter pair takes neo_tp_activate's arguments around the index and the two row counts
    assert _lib.SIGNATURES["neo_vanilla_train_rows"][1][:9] == _lib.SIGNATURES["neo_vanilla_occupancy_keep"][1][:9]


def test_every_new_function_validates_on_the_host():
    net = marching.MarchingNeRF(num_coarse_samples=7, num_fine_samples=64)
    net.load_state_dict(vc.state((7, 64)))
    assert net.last_train_kept is None and net.occupancy_density is None
    good = oc.ones(8)
    b = vc.rays(5)
    o, d, t, enc = b["rays_o"], b["viewdirs"], torch.zeros(5, 4), torch.zeros(5, 27)
    bad_boxes = (None, ((0, 0, 0),), ((0, 0, 0), (1, 1, 0)), ((0, float("nan"), 0), (1, 1, 1)), ((1, 1, 1), (0, 0, 0)), "box")
    # train_rows: grid, box, then the tensors by name; a CPU tensor is refused by name before any device is touched
    for bad in (good.float(), good[0], torch.ones(24, 24, 24, dtype=torch.bool), "grid"):
        with pytest.raises(ValueError):
            marching.train_rows(bad, vc.BOX, o, d, t, enc)
    for bad in bad_boxes:
        with pytest.raises(ValueError):
            marching.train_rows(good, bad, o, d, t, enc)
    with pytest.raises(ValueError, match="rays_o must have shape"):
        marching.train_rows(good, vc.BOX, o[:, :2], d, t, enc)
    with pytest.raises(ValueError, match="rays_o must be a floating-point"):
        marching.train_rows(None, None, o.long(), d, t, enc)
    with pytest.raises(ValueError, match="rays_o is on cpu"):
        marching.train_rows(good, vc.BOX, o, d, t, enc)
    with pytest.raises(TypeError):
        marching.train_rows(None, None, "o", d, t, enc)
    # nerf_mlp_rows
    with pytest.raises(TypeError):
        marching.nerf_mlp_rows("mlp", torch.zeros(3, 63), torch.zeros(3, 27))
    with pytest.raises(ValueError, match="x_enc must have shape"):
        marching.nerf_mlp_rows(net.coarse_mlp, torch.zeros(3, 62), torch.zeros(3, 27))
    with pytest.raises(ValueError, match="x_enc must be a floating-point"):
        marching.nerf_mlp_rows(net.coarse_mlp, torch.zeros(3, 63, dtype=torch.int32), torch.zeros(3, 27))
    with pytest.raises(ValueError, match="x_enc is on cpu"):
        marching.nerf_mlp_rows(net.coarse_mlp, torch.zeros(3, 63), torch.zeros(3, 27))
    # scatter_activate: total, index, then the rows
    idx = torch.zeros(3, dtype=torch.int32)
    for total in (-1, 2.0, True, "n"):
        with pytest.raises(ValueError, match="total"):
            marching.scatter_activate(torch.zeros(3, 3), torch.zeros(3), idx, total)
    with pytest.raises(ValueError, match="index must be an integer"):
        marching.scatter_activate(torch.zeros(3, 3), torch.zeros(3), idx.long(), 8)
    with pytest.raises(ValueError, match="index must have shape"):
        marching.scatter_activate(torch.zeros(3, 3), torch.zeros(3), idx[:, None], 8)
    with pytest.raises(ValueError, match="index is on cpu"):
        marching.scatter_activate(torch.zeros(3, 3), torch.zeros(3), idx, 8)
    # occupancy_probes
    for bad in bad_boxes:
        with pytest.raises(ValueError):
            marching.occupancy_probes(bad, 8, 1, 0)
    for G in (12, 0, 512, "8"):
        with pytest.raises(ValueError, match="resolution"):
            marching.occupancy_probes(vc.BOX, G, 1, 0)
    for seed in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            marching.occupancy_probes(vc.BOX, 8, seed, 0)
    for step in (-1, 2 ** 32, 0.0):
        with pytest.raises(ValueError, match="step"):
            marching.occupancy_probes(vc.BOX, 8, 1, step)
    with pytest.raises(ValueError, match="too thin"):
        marching.occupancy_probes(((1e6, 0.0, 0.0), (1e6 + 1.0, 1.0, 1.0)), 256, 1, 0)
    # the module calls
    for bad in bad_boxes:
        with pytest.raises(ValueError):
            net.init_occupancy(bad, 8)
    with pytest.raises(ValueError, match="resolution"):
        net.init_occupancy(vc.BOX, 12)
    with pytest.raises(_lib.NeoError, match="init_occupancy"):
        net.update_occupancy(0.5)
    with pytest.raises(TypeError):
        net.update_occupancy()                                  # sigma_threshold has no default
    net._run = dict(box=vc.BOX, G=8, clip=False, density=torch.zeros(8, 8, 8), updates=0)      # as after init_occupancy, on no device
    for kw in (dict(sigma_threshold=float("nan")), dict(sigma_threshold="x"), dict(dilate=-1), dict(dilate=5), dict(decay=1.5),
               dict(decay=-0.1), dict(decay=float("nan")), dict(decay="d"), dict(seed=-1), dict(seed=1.0)):
        args = dict(sigma_threshold=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            net.update_occupancy(**args)
    net._run = None
    with pytest.raises(ValueError, match="rays_o is on cpu"):
        net.render_train_marching(b, False, False, vc.NEAR, vc.FAR)


def test_the_masked_oracle_gives_fp64_gradients():
    counts, R = (16, 24), 64
    b = {k: v.double() for k, v in vc.rays(R).items()}
    sd = tm.state()
    t0 = tm.level0(counts, R)
    m0 = vc.keep_rule_box(vc.mixed(8), vc.BOX, vc.rays(R)["rays_o"], vc.rays(R)["viewdirs"], t0, True)
    with torch.enable_grad():
        pp = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
        first, extra = vc.oracle_render_marching(pp, b, counts, 0.0, occ=vc.mixed(8), box=vc.BOX, clip=True)
        t1 = extra[1]["t"].detach()
        m1 = extra[1]["keep"]
        out, _ = vc.oracle_render_marching(pp, b, counts, 0.0, samples=(t0.double(), t1), masks=(m0, m1))
        target = torch.full((R, 3), 0.25, dtype=torch.float64)
        grads = torch.autograd.grad(tm.mse2(out, target), [pp[k] for k in sorted(pp)])
    assert torch.equal(extra[0]["keep"], m0)
    assert all(g.dtype == torch.float64 and bool(torch.isfinite(g).all()) for g in grads)
    assert all(float(g.abs().max()) > 0 for g in grads), "every parameter tensor receives a gradient through torch.where"
    assert 0 < int(m0.sum()) < m0.numel() and 0 < int(m1.sum()) < m1.numel()


@pytest.mark.parametrize("G", tm.GRIDS)
@pytest.mark.parametrize("counts", tm.COUNTS, ids=lambda c: "%d+%d" % c)
def test_the_mixed_grid_keeps_and_skips_at_both_levels(counts, G):
    """With vc.BOX, vc.mixed(G) and clip=True the kept share lies in [0.15, 0.85] at level 0 (deterministic positions) and at level 1
    (the oracle's positions) for every R >= 63; a single ray stays strictly between nothing and everything."""
    occ = vc.mixed(G)
    for n in tm.RAYS:
        b = vc.rays(n)
        _, extra = vc.oracle_render_marching(tm.state(), b, counts, 0.0, occ=occ, box=vc.BOX, clip=True)
        assert torch.equal(extra[0]["t"], tm.level0(counts, n))
        shares = [float(e["keep"].float().mean()) for e in extra]
        print("%s G %d, %d rays: kept %.3f at level 0, %.3f at level 1" % (counts, G, n, shares[0], shares[1]))
        if n >= 63:
            assert all(0.15 <= s <= 0.85 for s in shares), (counts, G, n, shares)
        else:
            assert 0.0 < shares[1] < 1.0, (counts, G, n, shares)


@pytest.mark.parametrize("want", tm.EXACT, ids=lambda w: "all" if w is None else str(w))
def test_counted_positions_keep_exactly_that_many_samples(want):
    b, t, kept = tm.counted_case(want)
    keep = vc.keep_rule_box(oc.ones(8), vc.SMALL, b["rays_o"], b["viewdirs"], t, True)
    print("%d rays cross vc.SMALL, %d samples, %d kept" % (t.shape[0], t.numel(), kept))
    assert int(keep.sum()) == kept == (t.numel() if want is None else want)


@pytest.mark.parametrize("box", (vc.BOX, vc.SMALL, vc.FAR_AWAY), ids=("box", "small", "far_away"))
@pytest.mark.parametrize("G", (8, 32))
def test_the_probe_formula_puts_a_point_in_its_own_cell_away_from_faces(G, box):
    g = torch.Generator().manual_seed(G)
    u = torch.rand(G ** 3, 3, generator=g, dtype=torch.float64) * 0.98 + 0.01
    pts, cells = tm.probe_points(box, G, u)
    assert torch.equal(vc.cell_box(pts, box, G), cells)
    # in fp32 the same holds for the centres, which is what a pulled-back coordinate falls on
    centre, _ = tm.probe_points(box, G, torch.full((G ** 3, 3), 0.5), torch.float32)
    assert torch.equal(vc.cell_box(centre, box, G), cells.float())
