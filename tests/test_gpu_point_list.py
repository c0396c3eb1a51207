"""GPU: the one keep rule and the one point-list builder behind the NeO-360 and the vanilla frames (neo-360_amd/csrc/occ_points.h,
point_list.hip, march.h).

1. One rule behind both entry points.  `ops.occupancy_keep` (the unit cube, outside of which the edge cell decides) and
   `marching.occupancy_keep_box` with the box [-1, 1)^3 run the same device function on the same cell expression
   (tests/test_occ_grid_cpu.py), so on points inside the cube their masks are byte-equal; outside of it the unit cube gives the
   box mask of the point moved into the edge cell, the box without clip keeps and the box with clip skips.
2. The builder at its workgroup edges through the vanilla path.  A workgroup of the builder owns 1024 candidates; 15, 16 and 17
   rays x a 64-sample segment are 960, 1024 and 1088 of them, and a window of 16 rays puts the 17th ray into a second window.
   n_coarse = 63 is one level-0 segment of 64; n_coarse = 64 adds a second segment of length 1, whose candidates are the rays that
   the stop rule left alive.  The frame is compared bitwise with the chain of public stage ops, as
   tests/test_gpu_vanilla_march.py::test_mixed_grid_frame_equals_the_chain_of_stage_ops does.

Bounds: every comparison is `torch.equal` - both sides are the same machine code on the same numbers."""
import pytest
import torch

import occupancy_cases as oc
import vanilla_march_cases as vc
from neo360_amd import marching, ops
from vanilla_march_gpu import assert_equals_chain, installed, march, rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
R, N = 5, 65


def _random_grid(G):
    g = torch.Generator().manual_seed(100 + G)
    return torch.rand(G, G, G, generator=g) < 0.5


def _points(G, spread):
    """o (R,3), d (R,3), t (R,N) and the fp32 positions x = o + t d (one multiply, one add: eager torch, as the library)."""
    g = torch.Generator().manual_seed(7 * G + int(spread * 10))
    o = (torch.rand(R, 3, generator=g) - 0.5) * 0.6 * spread
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=g) - 0.5, dim=-1) * spread
    t = torch.rand(R, N, generator=g) * 0.6
    return o, d, t, oc.positions(o, d, t)


def _raw_cell(x, G):
    return torch.floor((x + 1.0) * torch.tensor(0.5 * G, dtype=torch.float32))


@pytest.mark.parametrize("G", (8, 32))
def test_unit_cube_and_unit_box_masks_are_byte_equal_inside_the_cube(G):
    grid = _random_grid(G)
    o, d, t, x = _points(G, 1.0)
    c = _raw_cell(x, G)
    assert x.dtype == torch.float32 and bool(((c >= 0) & (c < G)).all()), "every point has its cell in [0, G) on every axis"
    o, d, t = o.to(DEV), d.to(DEV), t.to(DEV)
    cube = ops.occupancy_keep(grid, o, d, t)
    box = marching.occupancy_keep_box(grid, UNIT, o, d, t, clip=False)
    clipped = marching.occupancy_keep_box(grid, UNIT, o, d, t, clip=True)
    assert cube.dtype == box.dtype == torch.bool and tuple(cube.shape) == tuple(box.shape) == (R, N)
    assert torch.equal(cube, box) and torch.equal(cube, clipped)
    assert 0 < int(cube.sum()) < cube.numel(), "the random grid keeps some points and skips some"
    ci = c.long()
    assert torch.equal(cube.cpu(), grid[ci[..., 0], ci[..., 1], ci[..., 2]])


@pytest.mark.parametrize("G", (8, 32))
def test_outside_the_cube_the_three_policies(G):
    grid = _random_grid(G)
    o, d, t, x = _points(G, 4.0)
    c = _raw_cell(x, G)
    out_axis = ~((c >= 0) & (c < G))
    outside = out_axis.any(dim=-1)
    assert 0 < int(outside.sum()) < outside.numel() and bool(torch.isfinite(x).all())
    # the point moved into the edge cell: an outside coordinate becomes the centre of cell 0 or G - 1 (dyadic, exact in fp32)
    centre = (c.clamp(0, G - 1) + 0.5) * (2.0 / G) - 1.0
    moved = torch.where(out_axis, centre, x).reshape(-1, 3)
    assert torch.equal(_raw_cell(moved, G).reshape(c.shape), c.clamp(0, G - 1))
    zeros3, zeros1 = torch.zeros_like(moved).to(DEV), torch.zeros(moved.shape[0], 1, device=DEV)
    o, d, t = o.to(DEV), d.to(DEV), t.to(DEV)
    cube = ops.occupancy_keep(grid, o, d, t)
    moved_box = marching.occupancy_keep_box(grid, UNIT, moved.to(DEV), zeros3, zeros1, clip=False).reshape(R, N)
    assert torch.equal(cube, moved_box), "the unit cube clamps into the edge cell"
    assert 0 < int(cube.cpu()[outside].sum()) < int(outside.sum()), "edge cells of both kinds are hit"
    kept = marching.occupancy_keep_box(grid, UNIT, o, d, t, clip=False).cpu()
    skipped = marching.occupancy_keep_box(grid, UNIT, o, d, t, clip=True).cpu()
    assert bool(kept[outside].all()) and not bool(skipped[outside].any())
    assert torch.equal(kept[~outside], cube.cpu()[~outside]) and torch.equal(skipped[~outside], cube.cpu()[~outside])


# (n_coarse, n_fine) -> the density bias that, on the CPU oracle at vc.EPS with vc.mixed(8) over vc.BOX, splits these rays between
# the two possible stops of the level named below (vc.BIAS has 63 + 64; 2.65 was found the same way for 64 + 64: 6 of 15 .. 17 rays
# stop at 64 of the 65 level-0 samples, their boundary transmittances no closer than 2 % to eps)
EDGE_COUNTS = {(63, 64): vc.BIAS[(63, 64)], (64, 64): 2.65}
_EDGE_NETS = {}


def _edge_net(counts):
    if counts not in _EDGE_NETS:
        net = marching.MarchingNeRF(num_coarse_samples=counts[0], num_fine_samples=counts[1]).to(DEV)
        net.load_state_dict(vc.state(EDGE_COUNTS[counts]))
        _EDGE_NETS[counts] = net
    return _EDGE_NETS[counts]


@pytest.mark.parametrize("n", (15, 16, 17))
@pytest.mark.parametrize("counts", sorted(EDGE_COUNTS), ids=lambda c: "%d+%d" % c)
def test_builder_at_its_workgroup_edges_through_the_vanilla_march(counts, n):
    net = _edge_net(counts)
    grid = vc.mixed(8)
    b = rays(n)
    net.march_window = 16
    try:
        with installed(net, grid, vc.BOX, False):
            got = march(net, b, vc.EPS, coarse=True)
            stops = assert_equals_chain(net, b, got, (counts, n), grid, vc.BOX, False, vc.EPS, coarse=True)
    finally:
        net.march_window = None
    N0, N1 = vc.n_level(counts)
    assert tuple(got[2][0][0].shape)[-1] == N0 and tuple(got[2][1][0].shape) == (n, N1)
    keep1 = got[2][1][2]
    assert 0 < int(keep1.sum()) < keep1.numel(), "the grid keeps some samples and skips some"
    # a later segment's candidates are the rays left alive: some, not all
    level, first = (0, 64) if N0 > 64 else (1, 64)
    stopped = int((stops[level] == first).sum())
    print("%s, %d rays: level-%d stops %s" % (counts, n, level, sorted(set(stops[level].tolist()))))
    assert 0 < stopped < n, (counts, n, stops[level].tolist())
