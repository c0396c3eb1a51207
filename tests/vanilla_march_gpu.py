"""GPU helpers shared by the vanilla marching-frame tests (tests/test_gpu_vanilla_march.py, tests/test_gpu_point_list.py): the
rays on the device, the call with its samples, a scope that installs a grid, and the frame restated as the chain of public stage
ops.  Inputs and CPU restatements: tests/vanilla_march_cases.py."""
import torch

import vanilla_march_cases as vc
from neo360_amd import marching, ops

DEV = "cuda"
NAMES = ("rgb", "acc", "depth")


def rays(n):
    return {k: v.to(DEV) for k, v in vc.rays(n).items()}


def march(net, b, eps, white=False, **kw):
    """[level 0 three, level 1 three, [(t, w, keep, stop, rows) per level], kept int64[2]], cloned."""
    out = net.render_marching(b, eps, white, vc.NEAR, vc.FAR, return_samples=True, **kw)
    net.check_flags()
    return [[t.clone() for t in out[0]], [t.clone() for t in out[1]], [[t.clone() for t in lv] for lv in out[2]],
            net.last_march_kept.clone()]


def installed(net, grid, box=None, clip=False):
    class _Scope:
        def __enter__(self):
            net.set_occupancy(grid, box, clip)

        def __exit__(self, *exc):
            net.set_occupancy(None)
    return _Scope()


def assert_equals_chain(net, b, got, what, grid, box, clip, eps, white=False, segment=64, coarse=False):
    """The frame from the public stage ops, level by level on the call's own returned positions: the keep mask is
    occupancy_keep_box, kept rows are eval_mlp's and skipped rows zero, the stop is termination_stops_vanilla on the masked rows,
    the composite is ops.composite(0, ...) on the returned rows and the level-1 positions are ops.resample on the returned level-0
    weights.  Everything bitwise.  Returns the stops."""
    o, vd, rd = b["rays_o"], b["viewdirs"], b["rays_d"]
    R = o.shape[0]
    evaluated, stops = [], []
    for lv in range(2):
        t, w, keep, stop, rows = got[2][lv]
        N = t.shape[1]
        assert tuple(w.shape) == tuple(keep.shape) == (R, N) and tuple(rows.shape) == (R, N, 4) and tuple(stop.shape) == (R,)
        assert keep.dtype == torch.bool and stop.dtype == torch.int32
        assert torch.equal(keep, marching.occupancy_keep_box(grid, box, o, vd, t, clip)), (what, lv, "keep mask")
        full = net.eval_mlp(lv, o, vd, t)
        masked = torch.where(keep[:, :, None], full, torch.zeros_like(full))
        if eps > 0 and (lv == 1 or coarse):
            own, _ = marching.termination_stops_vanilla(masked, t, rd, eps, segment)
            again, _ = marching.termination_stops_vanilla(rows, t, rd, eps, segment)
            assert torch.equal(stop, own) and torch.equal(stop, again), (what, lv, "stop")
        else:
            assert bool((stop == N).all()), (what, lv)
        mask = keep & vc.front(stop, N)
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
