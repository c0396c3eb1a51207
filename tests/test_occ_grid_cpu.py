"""CPU: the one cell expression of the occupancy grids (neo-360_amd/csrc/occ_points.h: OccGrid, occ_keep), restated in numpy fp32.

The unit-cube rule used to be floor((x + 1) (0.5 G)) and is now the box rule's floor((x - lo) scale) with lo = -1 and
scale = G / (hi - lo), hi = 1.  In fp32 the two are the same number: x - (-1) is x + 1 exactly, and G / 2 = 0.5 G exactly (G is
a small integer).  The test restates both and compares the cells over an explicit edge list; it also restates what each of
the three policies (clamp to the edge cell, keep, skip) does with the members of that list that fall outside [0, G)."""
import numpy as np
import pytest

F = np.float32
RESOLUTIONS = (8, 16, 32, 256)
OCC_CLAMP, OCC_KEEP, OCC_SKIP = 0, 1, 2


def _edges(G):
    one, inf = F(1.0), F(np.inf)
    xs = [F(0.0), F(-0.0), one, -one,
          np.nextafter(one, F(0.0)), np.nextafter(-one, F(0.0)), np.nextafter(one, inf), np.nextafter(-one, -inf),
          F(1e30), F(-1e30), F(3.4e38), F(-3.4e38),
          F(1e-45), F(-1e-45), F(1e-40), F(-1e-40), np.finfo(F).tiny, -np.finfo(F).tiny]
    for k in range(G + 1):
        b = F(-1.0 + 2.0 * k / G)          # exact: G is a power of two or 32 k', k / G needs at most 8 bits
        xs += [b, np.nextafter(b, -inf), np.nextafter(b, inf)]
    return np.array(xs, dtype=F)


def _raw_old(x, G):
    with np.errstate(over="ignore"):
        return np.floor((x + F(1.0)) * (F(0.5) * F(G)))


def _raw_new(x, G, lo=F(-1.0), hi=F(1.0)):
    scale = F(G) / (hi - lo)               # occ_grid_box's host fp32 scale; occ_grid_unit's 0.5f * G is the same number
    assert scale == F(0.5) * F(G)
    with np.errstate(over="ignore"):
        return np.floor((x - lo) * scale)


def _clamped(c, G):
    c = np.where(c > F(0.0), c, F(0.0))
    c = np.where(c < F(G - 1), c, F(G - 1))      # before the conversion: +-inf lands in an edge cell
    return c.astype(np.int64)


def _keep(x, occ, policy):
    """occ_keep on one axis of a finite point whose other two cells are given by `occ` (a bool row over this axis's cells)."""
    G = occ.shape[0]
    c = _raw_new(x, G)
    inside = (c >= F(0.0)) & (c < F(G))
    if policy == OCC_CLAMP:
        return occ[_clamped(c, G)]
    return np.where(inside, occ[_clamped(c, G)], policy == OCC_KEEP)


@pytest.mark.parametrize("G", RESOLUTIONS)
def test_unit_cube_cells_are_the_box_cells_of_minus_one_to_one(G):
    x = _edges(G)
    assert x.dtype == F and np.isfinite(x).all()
    old, new = _raw_old(x, G), _raw_new(x, G)
    assert old.dtype == F and new.dtype == F
    assert np.array_equal(old, new), "the floored values themselves agree, overflow to +-inf included"
    assert np.array_equal(_clamped(old, G), _clamped(new, G))
    cells = _clamped(new, G)
    assert cells.min() == 0 and cells.max() == G - 1
    # every cell boundary starts its cell (its lower fp32 neighbour need not end the one before: x + 1 rounds)
    bounds = np.array([-1.0 + 2.0 * k / G for k in range(G)], dtype=F)
    assert _clamped(_raw_new(bounds, G), G).tolist() == list(range(G))


@pytest.mark.parametrize("G", RESOLUTIONS)
def test_the_three_outside_policies(G):
    x = _edges(G)
    raw = _raw_new(x, G)
    outside = ~((raw >= F(0.0)) & (raw < F(G)))
    below, above = outside & (raw < F(0.0)), outside & (raw >= F(G))
    # x = 1 itself is outside (cell G), -1 inside; +-1e30 and +-3.4e38 (an overflow to inf) are outside
    assert above[x == F(1.0)].all() and not outside[x == F(-1.0)].any()
    assert outside[np.abs(x) > F(2.0)].all() and below.any() and above.any()
    rng = np.random.default_rng(G)
    for occ in (rng.random(G) < 0.5, np.zeros(G, bool), np.ones(G, bool)):
        clamp, keep, skip = (_keep(x, occ, p) for p in (OCC_CLAMP, OCC_KEEP, OCC_SKIP))
        assert np.array_equal(clamp[below], np.full(int(below.sum()), occ[0]))
        assert np.array_equal(clamp[above], np.full(int(above.sum()), occ[G - 1]))
        assert keep[outside].all() and not skip[outside].any()
        # inside the grid the policy does not matter
        assert np.array_equal(clamp[~outside], keep[~outside]) and np.array_equal(keep[~outside], skip[~outside])
