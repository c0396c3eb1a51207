"""CPU: the restatements of the empty-space-skipping tests (tests/occupancy_cases.py), the host-side validation of the occupancy
calls and their ABI declarations.  Nothing here needs a device.

The keep rule is stated twice, in fp32 (what the kernel computes) and in fp64 from the same fp32 inputs.  On the classifier
inputs - dyadic by construction, so that the rule's arithmetic is exact in fp32 - the two agree outside the samples within
2^-20 * 2 / G of a cell face, which every comparison leaves out; those samples are at most 1 % of the samples of every input the
GPU tests classify, so the exclusion cannot hide a failure."""
import os
import re

import pytest
import torch

from conftest import ROOT
import edit_cases as ec
import instance_cases as ic
import occupancy_cases as occ_c
import oracle
from neo360_amd import _lib, models, ops

CLASSIFIER_N = (1, 17, 49, 64, 65, 385)
CLASSIFIER_R = (1, 7, 300)
CLASSIFIER_G = (8, 32, 256)


@pytest.mark.parametrize("G", CLASSIFIER_G)
def test_fp32_and_fp64_keep_rules_agree_away_from_faces(G):
    seen_skip = seen_keep = seen_wild = 0
    for N in CLASSIFIER_N:
        for R in CLASSIFIER_R:
            grid, o, d, t = occ_c.classifier_case(R, N, G, 1000 * G + 10 * N + R)
            k32 = occ_c.keep_rule(grid, o, d, t, torch.float32)
            k64 = occ_c.keep_rule(grid, o, d, t, torch.float64)
            face = occ_c.near_face(o, d, t, G)
            assert tuple(k32.shape) == (R, N) and k32.dtype == torch.bool
            assert torch.equal(k32[~face], k64[~face]), (G, N, R)
            assert int(face.sum()) <= 0.01 * R * N, (G, N, R, int(face.sum()))
            wild = ~torch.isfinite(occ_c.positions(o, d, t)).all(dim=-1)
            assert bool(k32[wild].all())
            assert bool(occ_c.keep_rule(None, o, d, t).all())
            seen_skip += int((~k32).sum())
            seen_keep += int(k32.sum())
            seen_wild += int(wild.sum())
    assert seen_skip > 1000 and seen_keep > 1000 and seen_wild >= 3 * len(CLASSIFIER_N)


def test_cells_clamp_and_index():
    x = torch.tensor([-3.0, -1.0, -0.9999, -0.75, 0.0, 0.7499, 0.75, 1.0, 5.0, float("nan"), float("inf")])
    assert occ_c.cell(x, 8).tolist() == [0, 0, 0, 1, 4, 6, 7, 7, 7, 0, 0]
    grid = occ_c.zeros(8)
    grid[1, 4, 7] = True
    o = torch.tensor([[-0.7, 0.1, 0.9], [-0.7, 0.1, 0.7]])
    keep = occ_c.keep_rule(grid, o, torch.zeros(2, 3), torch.zeros(2, 1))
    assert keep.reshape(-1).tolist() == [True, False]


@pytest.mark.parametrize("n,chunk", ((96, None), (300, 128)))
def test_face_samples_of_the_frame_rays_stay_under_the_cap(n, chunk):
    """The level-0 rows of the frames the GPU tests render (the level-1 rows exist on the device only: the GPU test counts them
    against the same cap before it uses the exclusion)."""
    lv0 = ec.oracle_level0(n)
    b = ic.rays(n)
    for G in (32, 256):
        face = occ_c.near_face(b["rays_o"], b["rays_d"], lv0["fg_t"], G)
        assert int(face.sum()) <= 0.01 * face.numel(), (n, G, int(face.sum()))


@pytest.mark.parametrize("G", (8, 16, 32, 96))
def test_packing_round_trips(G):
    g = torch.Generator().manual_seed(G)
    for grid in (torch.rand(G, G, G, generator=g) < 0.5, occ_c.ones(G), occ_c.zeros(G), occ_c.checkerboard(G)):
        words = ops.pack_occupancy(grid)
        assert words.dtype == torch.int32 and tuple(words.shape) == (G ** 3 // 32,)
        assert torch.equal(ops.unpack_occupancy(words, G), grid)
    one = occ_c.zeros(G)
    one[1, 2, 3] = True                     # lin = (1 G + 2) G + 3: bit lin & 31 of word lin >> 5
    lin = (G + 2) * G + 3
    words = ops.pack_occupancy(one).to(torch.int64) & 0xFFFFFFFF
    assert int(words[lin >> 5]) == 1 << (lin & 31) and int((words != 0).sum()) == 1
    top = occ_c.zeros(G)
    top[0, 0, 31 % G if G >= 32 else 0] = True
    assert torch.equal(ops.unpack_occupancy(ops.pack_occupancy(top), G), top)


@pytest.mark.parametrize("G,d", [(8, 0), (8, 1), (16, 1), (16, 2), (32, 3)])
def test_dilation_is_a_box_maximum(G, d):
    g = torch.Generator().manual_seed(10 * G + d)
    grid = torch.rand(G, G, G, generator=g) < 0.03
    grid[0, 0, 0] = grid[G - 1, G - 1, 0] = True          # corners: the padding
    want = torch.nn.functional.max_pool3d(grid[None, None].float(), 2 * d + 1, 1, d)[0, 0] > 0 if d else grid
    assert torch.equal(occ_c.dilate(grid, d), want)


def test_grid_construction_restated():
    G, probes = 8, 2
    sigma = torch.zeros(16, 16, 16)
    sigma[8, 8, 8] = 2.0                    # cell (4, 4, 4)
    sigma[0, 0, 0] = 9.0                    # a corner cell: outside the unit sphere
    sigma[5, 9, 11] = float("nan")          # cell (2, 4, 5): a NaN density is occupied
    raw = occ_c.from_sigma(sigma, G, probes, 1.0, 0)
    assert sorted(map(tuple, raw.nonzero().tolist())) == [(2, 4, 5), (4, 4, 4)]
    assert int(occ_c.from_sigma(sigma, G, probes, 2.0, 0).sum()) == 1          # > threshold, not >=
    grown = occ_c.from_sigma(sigma, G, probes, 1.0, 1)
    ball = occ_c.sphere_cells(G)
    # dilation first, the clip last: the corner cell is cleared, its neighbour inside the sphere is not
    assert bool(grown[3, 3, 3]) and bool(grown[1, 5, 6]) and bool(grown[1, 1, 1]) and not bool(grown[0, 0, 0]) and not bool(grown[0, 1, 1])
    assert int(grown.sum()) == 27 + 27 - 6 + 1 and not bool((grown & ~ball).any())       # the two cubes share 1 x 3 x 2 cells
    assert not bool(ball[0, 0, 0]) and bool(ball[0, 3, 3]) and bool(ball[4, 4, 4]) and torch.equal(ball, ball.flip(0).flip(1).flip(2))
    # every cell the clip clears is outside: its nearest corner is farther than 1 from the origin
    c = torch.arange(G + 1, dtype=torch.float64) * (2.0 / G) - 1.0
    lo, hi = c[:-1], c[1:]
    nearest = torch.where((lo <= 0) & (hi >= 0), torch.zeros(G, dtype=torch.float64), torch.minimum(lo.abs(), hi.abs()))
    dist2 = nearest[:, None, None] ** 2 + nearest[None, :, None] ** 2 + nearest[None, None, :] ** 2
    assert torch.equal(ball, dist2 <= 1.0)


def test_oracle_render_skipping_all_ones_is_the_oracle_render():
    b = ic.rays(96)
    want = oracle.neo360.render(ec.state(), b, ec.scene(), ec.N_COARSE, ec.N_FINE, out_depth=True)
    for grid in (occ_c.ones(32), None):
        got, extra = occ_c.oracle_render_skipping(ec.state(), b, ec.scene(), grid, keep=True)
        for lv in range(2):
            assert len(got[lv]) == len(want[lv]) == 6
            for i, (x, y) in enumerate(zip(got[lv], want[lv])):
                assert x.dtype == y.dtype and torch.equal(x, y), (lv, i)
            assert bool(extra[lv]["fg_keep"].all())


def test_oracle_render_skipping_all_zeros_has_no_foreground():
    b = ic.rays(96)
    plain = oracle.neo360.render(ec.state(), b, ec.scene(), ec.N_COARSE, ec.N_FINE, out_depth=True)
    got, extra = occ_c.oracle_render_skipping(ec.state(), b, ec.scene(), occ_c.zeros(32), keep=True)
    for lv in range(2):
        rgb, fg_rgb, bg_rgb, fg_acc, lam, depth = got[lv]
        assert bool((fg_rgb == 0).all()) and bool((fg_acc == 0).all()) and bool((lam == 1).all())
        assert torch.equal(rgb, bg_rgb) and not bool(extra[lv]["fg_keep"].any()) and bool((extra[lv]["fg_w"] == 0).all())
    # level 0 of the outside-sphere half does not depend on the inside
    assert torch.equal(got[0][2], plain[0][2])


def test_oracle_render_skipping_mixed_changes_only_rays_with_a_skipped_sample():
    b = ic.rays(96)
    grid = occ_c.mixed(32)
    assert 0.4 < float(grid.float().mean()) < 0.9
    plain = oracle.neo360.render(ec.state(), b, ec.scene(), ec.N_COARSE, ec.N_FINE, out_depth=True)
    got, extra = occ_c.oracle_render_skipping(ec.state(), b, ec.scene(), grid, keep=True)
    whole0 = extra[0]["fg_keep"].all(dim=-1)
    assert 0 < int((~whole0).sum())
    for i in range(6):
        assert torch.equal(got[0][i][whole0], plain[0][i][whole0]), i
    assert bool((extra[0]["fg_w"][~extra[0]["fg_keep"]] == 0).all()) and bool((extra[1]["fg_w"][~extra[1]["fg_keep"]] == 0).all())
    changed = int((got[0][0] != plain[0][0]).any(dim=-1).sum())
    assert changed >= 20 and not bool((got[0][0] != plain[0][0]).any(dim=-1)[whole0].any())


def _header():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(bare, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
    assert m, "%s is not declared in include/neo360_hip.h" % name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_header_declares_and_ctypes_binds_the_occupancy_entry_points():
    text, bare = _header()
    for name in ("neo_tp_set_occupancy", "neo_tp_set_skip_window", "neo_tp_occupancy_keep", "neo_occupancy_from_sigma",
                 "neo_tp_render_skipping"):
        assert len(_lib.SIGNATURES[name][1]) == len(_params(bare, name)), name
        assert hasattr(_lib.load(), name)
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*neo_tp_skip_samples\s*;", bare)
    fields = [f.split("*")[-1].strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in _lib.TpSkipSamples._fields_] == ["fg_t", "fg_w", "bg_s", "fg_keep", "fg_rows"]
    assert "OCCUPANCY GRID" in text and "KEEP RULE" in text


def test_occupancy_calls_validate_on_the_host():
    net = models.NeRF_TP(num_coarse_samples=8, num_fine_samples=8)
    assert net.occupancy is None and net.last_skip_kept is None
    b = ic.rays(96)
    good = occ_c.ones(8)
    for bad in (good.float(), good.to(torch.uint8), good[0], good[:, :, :4], torch.ones(24, 24, 24, dtype=torch.bool),
                torch.ones(288, 288, 288, dtype=torch.bool), torch.ones(4, 4, 4, dtype=torch.bool), [[[True]]], "grid"):
        with pytest.raises(ValueError):
            net.set_occupancy(bad)
        with pytest.raises(ValueError):
            ops.occupancy_keep(bad, b["rays_o"], b["rays_d"], torch.zeros(96, 3))
    assert net.occupancy is None
    net.set_occupancy(None)                  # nothing installed: nothing to do, no device needed
    with pytest.raises(_lib.NeoError):       # no grid: refused before any device access
        net.render_skipping(b)
    for kw in (dict(resolution=24), dict(resolution=512), dict(resolution=32.0), dict(probes=0), dict(probes=5), dict(probes=1.5),
               dict(dilate=-1), dict(dilate=5), dict(sigma_threshold=float("nan")), dict(sigma_threshold=None), dict(sigma_threshold="1")):
        args = dict(resolution=16, sigma_threshold=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            net.build_occupancy(b, **args)
    with pytest.raises(TypeError):           # sigma_threshold has no default
        net.build_occupancy(b, 16)
    for args in ((good, b["rays_o"], b["rays_d"], torch.zeros(96)), (good, b["rays_o"][:5], b["rays_d"], torch.zeros(96, 3)),
                 (good, b["rays_o"], b["rays_d"], torch.zeros(96, 3, dtype=torch.long)), (good, b["rays_o"], b["rays_d"], torch.zeros(96, 0))):
        with pytest.raises(ValueError):
            ops.occupancy_keep(*args)
    with pytest.raises(ValueError):
        ops.unpack_occupancy(torch.zeros(5, dtype=torch.int32), 8)
    with pytest.raises(ValueError):
        ops.occupancy_from_sigma(torch.zeros(16, 16, 15), 8, 1.0, probes=2)
    c, o, d = ops.occupancy_lattice(8, 2)
    assert tuple(c.shape) == (16,) and tuple(o.shape) == tuple(d.shape) == (256, 3)
    assert float(c[0]) == -1.0 + 1.0 / 16 and float(c[-1]) == 1.0 - 1.0 / 16 and torch.equal(o[17], torch.tensor([float(c[1]), float(c[1]), 0.0]))
    # every lattice point lies in its own cell
    x = occ_c.positions(o, d, c[None, :].expand(256, 16))
    want = torch.arange(16) // 2
    got = occ_c.cell(x, 8).reshape(16, 16, 16, 3)
    assert torch.equal(got[..., 0], want[:, None, None].expand(16, 16, 16)) and torch.equal(got[..., 2], want[None, None, :].expand(16, 16, 16))
