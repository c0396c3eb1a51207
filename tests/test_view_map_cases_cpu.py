"""CPU: the case table of tests/view_map_cases.py is what it says it is, on the very inputs tests/test_gpu_view_map_sweep.py hands
to the kernels: the first five source views are synth.source_views(5) bit for bit and all eight cameras lie inside the unit
sphere; every ray hits the sphere; the point counts and texel counts the table is there for really occur; every fp64 reference is
finite and the fp32 oracle - the reference's arithmetic - uses at most half of every bound; and every map an evaluator reads has
a non-zero bilinear weight on at least 10 % of the case's (point, view) pairs and on at least 8 pairs, so that a kernel that read
a wrong texel, view or map could not pass."""
import pytest
import torch

import cases
import view_map_cases as V
from neo360_amd import synth

HALF = 0.5


def _half(checks, label):
    for k, v in checks.items():
        assert v["fp32_ratio"] <= HALF, (label, k, "fp32 oracle error %.3e against a bound of %.3e" % (v["fp32"], v["bound"]))
    return max(v["fp32_ratio"] for v in checks.values())


def test_views_extend_the_five_source_views():
    want = synth.source_views(5, *cases.IMG_WH)
    for nv in range(1, V.MAX_VIEWS + 1):
        poses, focal, centre = V.views(nv)
        assert poses.shape == (nv, 4, 4) and focal.shape == (nv,) and centre.shape == (nv, 2)
        k = min(nv, 5)
        for a, b in zip((poses[:k], focal[:k], centre[:k]), want):
            assert a.dtype == b.dtype and torch.equal(a, b[:k])
    for a, b in zip(V.views(5), want):
        assert torch.equal(a, b)
    for a, b in zip(V.views(3), synth.source_views(3, *cases.IMG_WH)):
        assert torch.equal(a, b)
    poses, focal, centre = V.views(8)
    radius = poses[:, :3, 3].double().norm(dim=-1)
    assert bool((radius < 1.0).all()), radius
    assert bool((focal == focal[0]).all()) and bool((centre == centre[0]).all())
    # eight different cameras
    eyes = poses[:, :3, 3]
    assert float(torch.cdist(eyes, eyes).add(torch.eye(8) * 9).min()) > 0.1


def test_table_shape():
    """The remainders the table is there for: P on 1, 63, 64, 65, 129 and a value near 200 off every multiple of 32; chunks that
    do not divide / exceed R; texel counts below, above and off a 64-texel group; the rotation rules."""
    ps = {p for _, p in V.CASES}
    assert {1, 63, 64, 65, 129} <= ps and any(190 <= p <= 210 and p % 32 for p in ps)
    for p, (R, N, chunk) in V.SHAPES.items():
        assert R * N == p
    assert any(R % c and c < R for R, _, c in V.SHAPES.values()) and any(c > R for R, _, c in V.SHAPES.values())
    assert sorted({nv for nv, _, _ in V.SCENES}) == [1, 2, 3, 4, 6, 7, 8]
    for s in range(len(V.SCENES)):
        mine = [p for t, p in V.CASES if t == s]
        assert any(p % 64 == 1 for p in mine) and any(p % 64 == 0 for p in mine), s
    at8 = {p for s, p in V.CASES if V.SCENES[s][0] == 8}
    assert at8 == set(V.SHAPES), at8
    texels = {(nv * ph * pw, nv * lh * lw) for nv, (ph, pw), (lh, lw) in V.SCENES}
    assert (4, 4) in texels and (30, 70) in texels                      # the API minimum; tails below and above one group
    assert any(a % 64 == 0 and b % 64 == 0 for a, b in texels)
    assert sum(1 for a, b in texels if a % 64 and b % 64) >= 5
    assert min(min(ph, pw, lh, lw) for _, (ph, pw), (lh, lw) in V.SCENES) == 2
    ms = [nv * g[0] * g[1] * g[2] for nv, _, g in V.PILLAR]
    assert ms[:5] == [1, 63, 64, 65, 378] and 378 % 64 == 58 and 840 in ms and max(max(g) for _, _, g in V.PILLAR) == 256
    assert {V.PILLAR[i][0] for i in V.PILLAR_GRAD} >= {1, 8} and ms[V.PILLAR_GRAD[0]] == 1 and len(V.PILLAR_GRAD) == 4
    assert {nv for nv, _, _ in V.LOOKUP_SCENES} == {2, 8} and {lh * lw for _, _, (lh, lw) in V.LOOKUP_SCENES} == {4, 35}
    for s in V.RENDER_SCENES:
        assert V.SCENES[s] in ((1, (2, 2), (2, 2)), (8, (2, 3), (3, 2)), (8,) + V.SMALL)


@pytest.mark.parametrize("s", range(len(V.SCENES)))
def test_every_ray_hits_the_sphere_and_every_map_is_read(s):
    for t, P in V.CASES:
        if t != s:
            continue
        c = V.point_case(s, P)
        assert bool(c["hit"].all()) and bool((c["far"] > 0).all())
        assert c["t_in"].shape == c["s_out"].shape == (c["R"], c["N"])
        assert bool((c["t_in"][:, 1:] > c["t_in"][:, :-1]).all()) and bool((c["s_out"][:, 1:] < c["s_out"][:, :-1]).all())
        assert float(c["s_out"].min()) > 0.0 and float(c["s_out"].max()) < 1.0
        need = V.enough_pairs(s, P)
        for inside in (True, False):
            for name, (frac, count) in V.read_fractions(s, P, inside).items():
                assert count >= need, (s, P, "inside" if inside else "outside", name, frac, count, need)
        frac, count = V.read_fractions(s, P, True, flip_y=False)["latent"]          # the PixelNeRF decoder's taps
        assert count >= need, (s, P, "pixelnerf", frac, count, need)


def test_the_floor_is_the_stated_one():
    assert V.MIN_READ_FRACTION == 0.10 and V.MIN_READ_PAIRS == 8
    for s, P in V.CASES:
        pairs = P * V.SCENES[s][0]
        assert V.enough_pairs(s, P) == (1 if P == 1 else max(8, -(-pairs // 10)))


@pytest.mark.parametrize("s", range(len(V.SCENES)))
def test_evaluator_references_finite_and_fp32_oracle_inside_half(s):
    worst = 0.0
    for t, P in V.CASES:
        if t != s:
            continue
        fg64, bg64 = V.neo_reference(s, P)
        fg32, bg32 = V.neo_reference(s, P, torch.float32)
        p64, p32 = V.pix_reference(s, P), V.pix_reference(s, P, torch.float32)
        c = V.point_case(s, P)
        for name, a, b in (("fg", fg64, fg32), ("bg", bg64, bg32), ("pix", p64, p32)):
            assert a.dtype == torch.float64 and b.dtype == torch.float32 and a.shape == b.shape == (c["R"], c["N"], 4)
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
            worst = max(worst, _half(V.eval_checks(b, a, b), (s, P, name)))
    print("scene %d: largest share of a bound the fp32 oracle uses: %.3f" % (s, worst))


def test_chunk_slices_matter():
    """The oracle per chunk slice differs from the oracle on the whole call in the colours (quirk Q1) and not in the densities:
    the table's chunks really exercise the tiling."""
    import oracle
    s, P = 1, 63
    c, sc = V.point_case(s, P), V.to64(V.scene_of(s))
    rgb, sigma = oracle.neo360.region_eval(V._neo_params(torch.float64), V.FG_PREFIX, V.to64(c["batch"]), sc, c["t_in"].double(), True,
                                           c["far"].double())
    fg64, _ = V.neo_reference(s, P)
    assert float((fg64[..., :3] - rgb).abs().max()) > 1e-4 and float((fg64[..., 3:] - sigma).abs().max()) < 1e-12


@pytest.mark.parametrize("i", range(len(V.PILLAR)))
def test_pillar_references_finite_and_fp32_oracle_inside_half(i):
    ref64, ref32 = V.pillar_reference(i), V.pillar_reference(i, torch.float32)
    nv, _, (G0, G1, G2) = V.PILLAR[i]
    for x, shape in zip(ref64, ((nv, G1, G2, 512), (nv, G0, G2, 512), (nv, G0, G1, 512))):
        assert x.dtype == torch.float64 and x.shape == shape and bool(torch.isfinite(x).all())
    share = _half(V.plan_checks(ref32, ref64, ref32), ("pillar", i))
    print("pillar case %d: largest |value| %.2f, fp32 oracle share %.3f" % (i, max(float(x.abs().max()) for x in ref64), share))


@pytest.mark.parametrize("i", range(len(V.LOOKUP_SCENES)))
def test_lookup_references_finite_and_fp32_oracle_inside_half(i):
    ref64, ref32 = V.lookup_reference(i), V.lookup_reference(i, torch.float32)
    c = V.lookup_case(i)
    assert c["pts"].shape == (V.LOOKUP_RAYS * V.LOOKUP_SAMPLES, 3)
    for k, v in ref64.items():
        assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()), k
    _half(V.lookup_checks(ref32, ref64, ref32), ("lookup", i))
    # all scatter traffic lands on the 4 or 35 texels of a view: every texel of the latent gets some
    g = ref64["g_latent"]
    assert float((g.abs().amax(dim=1) > 0).double().mean()) >= 0.5, i


@pytest.mark.parametrize("s", V.RENDER_SCENES)
def test_render_scenes_make_a_mixed_frame_on_the_oracle(s):
    """The culling rule at CULL_EPS on the CPU oracle's two foreground transmittances: between 30 % and 70 % of the rays, so that
    the GPU's own frame stays inside the 20 % .. 80 % the contract test asks for."""
    import oracle
    out = oracle.neo360.render(V.render_state(s), V.render_batch(s), V.scene_of(s), n_coarse=V.RENDER_SAMPLES[0],
                               n_fine=V.RENDER_SAMPLES[1], out_depth=True)
    l0, l1 = out[0][4].reshape(-1), out[1][4].reshape(-1)
    frac = float(((l0 < V.CULL_EPS) & (l1 < V.CULL_EPS)).float().mean())
    print("scene %d: the oracle culls %.3f of the rays" % (s, frac))
    assert 0.3 <= frac <= 0.7, frac
