"""CPU: the conditions of tests/frame_chain_cases.py, on the very inputs tests/test_gpu_frame_chain_sweep.py hands to the fused frame
drivers of vanilla NeRF, PixelNeRF and Mip-NeRF 360: the table holds what it says, the host-built level-0 row is the oracles' row
bit for bit, every case has a ray whose rays_d is not unit, the empty state gives exactly zero level-0 weights, every oracle is
finite, and the fp32 oracle at its own rows stays inside HALF of every bound against the fp64 oracle at those rows."""
import numpy as np
import pytest
import torch

import frame_chain_cases as F

KINDS = ("vanilla", "pix", "mip")


def test_table_holds_the_edges_it_names():
    for kind in ("vanilla", "pix"):
        tab = F.table(kind)
        assert {c.counts for c in tab} == set(F.LEVEL_COUNTS)
        for c in tab:
            nc, nf = c.counts
            assert 3 <= nc <= 256 and nf >= 1 and nc + 1 + nf <= 1024, c          # what the drivers accept
        sums = {nc + 1 + nf for nc, nf in F.LEVEL_COUNTS}
        assert {256, 257, 512, 513, 1024} <= sums                                 # both edges of the three sort widths
        mid = [c for c in tab if c.counts == F.LEVEL_MID]
        assert {c.R for c in mid} == set(F.RAY_COUNTS)
        assert {(c.near, c.far) for c in mid} == {F.NEAR_FAR[kind]} | set(F.NEAR_FAR_MID)
        assert {c.state for c in mid} == set(F.STATES)
        assert any(c.R == F.RAGGED_R and c.counts == (3, 1) for c in tab) and F.RAGGED_R * 4 % 64 != 0
        for counts in (F.LEVEL_MID, (3, 1)):
            assert {c.white for c in tab if c.counts == counts} == {False, True}
        assert any(c.state == "empty" for c in tab if c.counts == F.LEVEL_LARGEST)
    assert {c.chunk for c in F.table("pix")} == {None} | set(F.PIX_CHUNKS)
    assert all(c.variants == F.PRECISIONS for c in F.table("vanilla")) and all(c.variants == (True, False) for c in F.table("pix"))
    for nc, nf in F.LEVEL_REFUSED:
        assert not (3 <= nc <= 256 and nf >= 1 and nc + 1 + nf <= 1024)
    tab = F.table("mip")
    assert {c.counts for c in tab} == set(F.MIP_COUNTS)
    for c in tab:
        n_prop, n_nerf = c.counts
        assert 2 <= n_prop and 3 * n_prop + 1 <= 256 and 2 <= n_nerf <= 256, c
        assert c.R == (3 if c.counts == F.MIP_LARGEST else c.R)
    assert 3 * F.MIP_MID[0] + 1 == 64
    assert {c.R for c in tab if c.counts == F.MIP_MID} == set(F.RAY_COUNTS)
    for counts in (F.MIP_MID, F.MIP_DEFAULT):
        assert {c.tf for c in tab if c.counts == counts} == {1.0, 0.3, 0.0}
    plain = {c.counts: c for c in tab if c.R in (3, 5) and c.state == "gain1" and c.tf == 1.0}
    assert set(plain[F.MIP_DEFAULT].variants) == {(p, l) for p in F.PRECISIONS for l in (None, False, True)}
    assert {l for _, l in plain[F.MIP_LARGEST].variants} == {None, False, True}
    for n_prop, n_nerf in F.MIP_REFUSED:
        assert not (2 <= n_prop and 3 * n_prop + 1 <= 256 and 2 <= n_nerf <= 256)


@pytest.mark.parametrize("kind", ["vanilla", "pix"])
def test_host_built_level0_row_is_the_oracles_row(built_lib, kind):
    """near (1 - s) + far s on the library's linspace, three separate fp32 operations, against the level-0 row of the oracle's
    render(keep=True) at every (n, near, far) of the table - bit for bit.  The seeded form near + (far - near) s is not that row."""
    seen, seeded_differs = set(), 0
    for c in F.table(kind):
        key = (c.counts[0], c.near, c.far)
        if key in seen:
            continue
        seen.add(key)
        t0 = F.oracle_condition(c)[0]["t0"]
        row = F.host_edges(*key)
        assert row.dtype == torch.float32 and t0.shape == (c.R, c.counts[0] + 1)
        assert torch.equal(t0, row[None].expand_as(t0)), key
        assert row[0] == np.float32(c.near) and row[-1] == np.float32(c.far) and bool((row[1:] > row[:-1]).all())
        seeded_differs += int(not torch.equal(F.seeded_edges(*key), row))
    assert len(seen) >= 8 and seeded_differs >= len(seen) - 2


@pytest.mark.parametrize("kind", KINDS)
def test_every_case_has_a_ray_whose_rays_d_is_not_unit(kind):
    for c in F.table(kind):
        rays = F.rays_of(kind, c.R)
        assert rays["rays_o"].shape == (c.R, 3)
        assert float((rays["viewdirs"].norm(dim=-1) - 1).abs().max()) < 1e-6
        assert float((rays["rays_d"].norm(dim=-1) - 1).abs().max()) > 0.05, F.case_id(c)


@pytest.mark.parametrize("kind", ["vanilla", "pix"])
def test_empty_state_gives_zero_level0_weights_and_the_uniform_fallback(kind):
    n = 0
    for c in F.table(kind):
        if c.state != "empty":
            continue
        n += 1
        o32, o64, _ = F.oracle_condition(c)
        # every weight the sampler reads (weights[1:-1]) is exactly 0 in both arithmetics.  The last sample's interval is 1e10:
        # vanilla's softplus(-101) = 1.4e-44 is a subnormal that an fp32 library may or may not flush (this CPU's does, the
        # kernels and the fp64 oracle do not), so its weight is 0 or about 1e-34 - below 1e-30 either way.
        for o in (o32, o64):
            assert float(o["w0"][:, 1:-1].abs().max()) == 0.0, F.case_id(c)
            assert float(o["w0"].abs().max()) < 1e-30 and float(o["acc1"].abs().max()) < 1e-30 and float(o["depth1"].abs().max()) < 1e-30
            assert float((o["rgb1"] - (1.0 if c.white else 0.0)).abs().max()) < 1e-30
        assert all(bool(torch.isfinite(v).all()) for v in o32.values())
        # all-zero weights: the sampler pads them evenly, so the new samples spread over the inner bins' whole range
        new = o32["t1"].shape[1] - o32["t0"].shape[1]
        assert new == c.counts[1] and bool((o32["t1"][:, 1:] >= o32["t1"][:, :-1]).all())
    assert n >= 3


@pytest.mark.parametrize("kind", KINDS)
def test_fp32_oracle_stays_inside_half_of_every_bound(kind):
    """The fp32 oracle at ITS OWN rows against the fp64 oracle at those same rows, every output of every case: finite, and at most
    half of TOL x max(1, |fp64 value|) (TOL_HIST on Mip-NeRF 360's weights and densities)."""
    worst = ("", 0.0)
    for c in F.table(kind):
        o32, o64, checks = F.oracle_condition(c)
        for k, v in list(o32.items()) + list(o64.items()):
            assert bool(torch.isfinite(v).all()), (F.case_id(c), k)
        for k, v in checks.items():
            assert v["ratio"] <= F.ORACLE_SHARE, (F.case_id(c), k, v)
            if v["ratio"] > worst[1]:
                worst = ("%s/%s" % (F.case_id(c), k), v["ratio"])
        rec = F.summarize(checks)
        assert rec["worst_share_of_bound"] <= F.ORACLE_SHARE
    print("%s: %d cases, the fp32 oracle's largest share of a bound %.4f (%s)" % (kind, len(F.table(kind)), worst[1], worst[0]))


def test_mip_schedule_is_the_references():
    """dilation = 0.0025 + 0.5 / prod with prod the product of the counts of the levels BEFORE this one; the anneal of the table's
    train fractions is the same fp32 number whether train_frac reaches the formula as a double or - the driver's ABI - as fp32."""
    c = F.find("mip", F.MIP_DEFAULT)
    dil, anneal = F.mip_schedule(c)
    assert dil == [0.5025, 0.0025 + 0.5 / 64, 0.0025 + 0.5 / 4096] and anneal == 1.0
    late = [0.0025 + 0.5 / p for p in (64, 4096, 4096 * 32)]                    # prod *= n taken before the dilation
    assert all(np.float32(a) != np.float32(b) for a, b in zip(dil, late))
    for tf in (1.0,) + F.MIP_TRAIN_FRACS:
        t32 = float(np.float32(tf))
        assert np.float32(10 * tf / (9 * tf + 1)) == np.float32(10.0 * t32 / (9.0 * t32 + 1.0)), tf
    assert F.mip_schedule(F.find("mip", F.MIP_DEFAULT, tf=0.0))[1] == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_swapped_directions_leave_the_bounds(kind):
    """What the non-unit rays_d is for: the fp64 oracle with viewdirs and rays_d swapped, at the same rows, is outside the bounds of
    the mid case - a driver that hands a kernel the wrong one of the two cannot pass."""
    c = F.find(kind, F.MIP_MID if kind == "mip" else F.LEVEL_MID)
    o32, o64, _ = F.oracle_condition(c)
    rays = F.rays_of(kind, c.R)
    swapped = dict(rays, rays_d=rays["viewdirs"], viewdirs=rays["rays_d"])
    bad = F.run_oracle(c, torch.float64, F.rows_of(c, o32), rays=swapped)
    checks = F.frame_checks(c, bad, o64, o32)
    assert max(v["ratio"] for v in checks.values()) > 1.0, F.summarize(checks)
