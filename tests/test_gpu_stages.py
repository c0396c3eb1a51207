"""GPU: each HIP kernel against the CPU oracle and the reference-generated
fixtures, stage by stage (SURVEY.md §4 level 2).  Calls go through the C ABI."""
import numpy as np
import pytest
import torch

import cases
import oracle
from alongray_cases import cdf_space
from conftest import max_abs, record_parity
from neo360_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_raygen_vs_golden(golden):
    g = golden("g1_raygen")
    for tag, (H, W) in (("s", (32, 32)), ("f", (480, 640))):
        for pi, az in enumerate((10.0, 130.0, 250.0)):
            c2w = synth.look_at_origin(az, 0.6 + 0.1 * pi, 0.3 - 0.2 * pi)
            ro, vd, rd, rad = [x.cpu() for x in ops.get_ray_directions_and_rays(H, W, 0.8 * W, c2w)]
            if tag == "f":
                idx = g["idx_f"]
                ro, vd, rd, rad = ro[idx], vd[idx], rd[idx], rad[idx]
            assert max_abs(ro, g["o_%s%d" % (tag, pi)]) == 0.0
            assert max_abs(vd, g["v_%s%d" % (tag, pi)]) < 2e-7
            assert max_abs(rd, g["d_%s%d" % (tag, pi)]) < 2e-7
            # radii are differences of nearly equal fp32 directions (~1e-3): cancellation noise ~3e-8 abs
            assert max_abs(rad, g["r_%s%d" % (tag, pi)]) < 1e-7


def test_aabb_hit_mask_bit_exact(golden):
    g = golden("g2_aabb")
    boxes, o, d = cases.aabb_cases()
    od, dd = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    for bi, b in enumerate(boxes):
        hit, tmin, tmax = ops.bbox_intersection_batch(b, od, dd)
        assert torch.equal(hit.cpu(), g["hit%d" % bi])                       # integer mask: bit-exact
        assert np.array_equal(tmin.cpu().numpy(), g["tmin%d" % bi].numpy())  # fp64 slab distances: bit-exact too
        assert np.array_equal(tmax.cpu().numpy(), g["tmax%d" % bi].numpy())


def test_oriented_boxes_bit_exact(golden):
    """neo_aabb_multi = sample_rays_in_bbox (box-frame transform in float64, slab test, float32 rounding, 0-sentinel
    merge) against outputs of the reference's own function: integer masks and the merged near / far, bit for bit."""
    g = golden("g2_aabb")
    RTs, o, d = cases.oriented_box_cases()
    near, far, mask, per_box = ops.sample_rays_in_bbox(RTs, torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV),
                                                       return_per_box=True)
    for bi in range(len(RTs["R"])):
        assert torch.equal(per_box[bi].cpu(), g["ob_hit%d" % bi]), bi
    assert torch.equal(mask.cpu().to(torch.uint8), g["ob_mask"])
    assert torch.equal(near.cpu(), g["ob_near"]) and torch.equal(far.cpu(), g["ob_far"])
    # one box == the single-box entry point on pre-transformed rays
    single = {k: v[:1] for k, v in RTs.items()}
    n1, f1, m1 = ops.sample_rays_in_bbox(single, torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV))
    assert torch.equal(m1.cpu().squeeze(-1).to(torch.uint8), g["ob_hit0"])
    # empty ray set
    e = torch.zeros(0, 3, device=DEV)
    n0, f0, m0 = ops.sample_rays_in_bbox(RTs, e, e)
    assert n0.shape == (0, 1) and m0.shape == (0, 1)


def test_raygen_range_equals_full_frame():
    """A rank's shard: rays [lo, hi) generated alone are the rows [lo, hi) of the full frame, bit for bit (radii too)."""
    from neo360_amd import synth
    c2w = synth.look_at_origin(40.0)
    full = ops.get_ray_directions_and_rays(48, 64, 51.2, c2w)
    for lo, hi in ((0, 1024), (1024, 2048), (2048, 3072), (3000, 3072), (64 * 47 - 5, 64 * 48)):
        part = ops.get_ray_directions_and_rays(48, 64, 51.2, c2w, ray_range=(lo, hi))
        for a, b in zip(part, full):
            assert torch.equal(a, b[lo:hi])
    buf = ops.get_ray_directions_and_rays(48, 64, 51.2, c2w, ray_range=(100, 200))
    again = ops.get_ray_directions_and_rays(48, 64, 51.2, c2w, ray_range=(300, 400), out=buf)
    assert again[0].data_ptr() == buf[0].data_ptr() and torch.equal(again[3], full[3][300:400])


def test_aabb_empty_and_single():
    b = [[-1, -1, -1], [1, 1, 1]]
    hit, _, _ = ops.bbox_intersection_batch(b, torch.zeros(0, 3, dtype=torch.float64, device=DEV),
                                            torch.zeros(0, 3, dtype=torch.float64, device=DEV))
    assert hit.numel() == 0
    o = torch.tensor([[0.0, 0.0, -3.0], [0.0, 0.0, 0.0]], dtype=torch.float64, device=DEV)
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device=DEV)
    hit, tmin, tmax = ops.bbox_intersection_batch(b, o, d)
    assert hit.tolist() == [1, 0] and tmin.tolist() == [2.0, 0.0] and tmax.tolist() == [4.0, 0.0]


def test_sphere_mask_and_depth(golden):
    g = golden("g3_stages")
    rays = cases.strided_rays(96)
    far, ok = ops.intersect_sphere(rays["rays_o"].to(DEV), rays["rays_d"].to(DEV))
    assert bool(ok.all())
    assert max_abs(far.cpu(), g["far"]) < 1e-6
    # a ray that misses the unit sphere: mask bit and the reference's AssertionError
    o = torch.tensor([[0.0, 0.0, 3.0], [0.0, 0.0, 0.5]], device=DEV)
    d = torch.tensor([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], device=DEV)
    _, ok = ops.intersect_sphere(o, d, check=False)
    assert ok.tolist() == [0, 1]
    ops.get_context = ops.get_context  # keep linters quiet
    with pytest.raises(AssertionError):
        ops.intersect_sphere(o, d)
    _, ok = ops.intersect_sphere(o[1:], d[1:])  # flag was cleared by the poll
    assert ok.tolist() == [1]


def test_pos_enc(golden):
    g = golden("g3_stages")
    x3 = synth.uniform(11, "pe3", (257, 3), -1.7, 1.7)
    x4 = synth.uniform(11, "pe4", (129, 4), -1.0, 1.0)
    assert max_abs(ops.pos_enc(x3.to(DEV), 0, 10).cpu(), g["pe3"]) < 5e-7
    assert max_abs(ops.pos_enc(x4.to(DEV), 0, 10).cpu(), g["pe4"]) < 5e-7
    assert max_abs(ops.pos_enc(x3.to(DEV), 0, 4).cpu(), g["pe3v"]) < 5e-7


_cdf_space = cdf_space      # the helper lives in the shared case table now (tests/alongray_cases.py)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("n_prev,n_new", [(65, 128), (129, 256), (33, 64)])
def test_resample_matches_oracle(desc, n_prev, n_new):
    """Full resample op = pdf sampling with the callers' slicing + sort (+ flip)."""
    R = 96
    t_prev = torch.cumsum(synth.uniform(5, "rs_t%d" % n_prev, (R, n_prev), 0.01, 1.0), dim=-1)
    t_prev = t_prev / t_prev[:, -1:]
    w = synth.uniform(5, "rs_w%d" % n_prev, (R, n_prev), 0.25, 1.0)     # well-conditioned rows ...
    w[1] = 0.0                                                           # ... all-zero weights (uniform fallback)
    w[2] = 0.0
    w[2, 20] = 3.0                                                       # ... one spike, zero density elsewhere
    w[3] = synth.uniform(5, "rs_w3", (n_prev,), 0.0, 1.0)                # ... and arbitrarily small weights
    if desc:
        t_prev = torch.flip(t_prev, dims=[-1]).contiguous()
    mids = 0.5 * (t_prev[:, 1:] + t_prev[:, :-1])
    want = oracle.sampling.merge_sorted(t_prev, oracle.sampling.piecewise_constant_samples(mids, w[:, 1:-1], n_new))
    got = ops.resample(t_prev.to(DEV), w.to(DEV), n_new, descending=desc).cpu()
    if desc:
        got = torch.flip(got, dims=[-1])
    assert got.shape == want.shape
    assert bool((got[:, 1:] >= got[:, :-1]).all())                       # sorted
    good = torch.ones(R, dtype=torch.bool)
    good[2] = good[3] = False
    if not desc:
        # positions on well-conditioned rows; cdf space (every row): an ulp of the cdf moves a sample by ulp / density
        assert max_abs(got[good], want[good]) < 5e-6
        assert max_abs(_cdf_space(got, mids, w[:, 1:-1]), _cdf_space(want, mids, w[:, 1:-1])) < 2e-6
        record_parity("resample_vs_oracle/asc_%d_%d" % (n_prev, n_new), max_pos_well_conditioned=max_abs(got[good], want[good]))
    else:
        # descending bins (the background branch): every sample interpolates across the WHOLE range (bin0 = first bin,
        # bin1 = last bin: the reference's mask / max / min search is not an inverse cdf there), so an ulp of the fp32 cdf
        # moves it n_bins times further.  Bound = the reference arithmetic's own rounding on these inputs: the pinned
        # oracle (bit-exact to neo360/helper.py:174-215, tests/test_oracle_golden.py) run in fp64 on the same rows
        # (fixture-side evidence for the fixture rows: g3_pdf_noise.npz, test_resample_golden_bins[desc]).
        want64 = oracle.sampling.merge_sorted(t_prev.double(), oracle.sampling.piecewise_constant_samples(
            mids.double(), w[:, 1:-1].double(), n_new))
        noise = (want.double() - want64).abs()
        err = (got.double() - want.double()).abs()
        record_parity("resample_vs_oracle/desc_%d_%d" % (n_prev, n_new), max_pos_err=float(err[good].max()),
                      reference_self_noise_max=float(noise[good].max()))
        row_noise = noise.amax(dim=-1, keepdim=True)            # per row, as the end-to-end rule is per ray
        # same rule as the end-to-end test: 1e-4 on every row the reference arithmetic determines to better than 1e-5,
        # otherwise within 1e-4 + 3 x that row's fp32-vs-fp64 disagreement
        assert float((err - (1e-4 + 3.0 * row_noise))[good].max()) <= 0.0, (float(err[good].max()), float(noise[good].max()))
        well = good & (row_noise.squeeze(-1) < 1e-5)
        assert float(err[well].max()) < 1e-4


@pytest.mark.parametrize("tag", ["asc", "desc"])
def test_resample_golden_bins(golden, tag):
    """The fixture's (bins, weights) pairs - ascending AND descending (the background branch, neo360/helper.py:204-210,
    model.py:319-331) - reproduced by feeding t_prev whose fp32 midpoints are exactly the fixture's bins; expected =
    the reference's own samples (fixture g3: pdf_asc / pdf_desc) merged with t_prev the way the callers do."""
    g = golden("g3_stages")
    noise = golden("g3_pdf_noise")
    bins, w = cases.pdf_cases()[tag]
    desc = tag == "desc"
    t_prev = torch.zeros(bins.shape[0], bins.shape[1] + 1, dtype=torch.float64)
    t_prev[:, 0] = bins[:, 0].double() + (1e-3 if desc else -1e-3)
    for k in range(bins.shape[1]):
        t_prev[:, k + 1] = 2 * bins[:, k].double() - t_prev[:, k]
    t_prev = t_prev.float()
    mids = 0.5 * (t_prev[:, 1:] + t_prev[:, :-1])
    keep = (mids == bins).all(dim=1)            # rows whose fp32 midpoints reproduce the fixture's bins exactly
    assert int(keep.sum()) > 10
    wfull = torch.cat([torch.zeros(w.shape[0], 1), w, torch.zeros(w.shape[0], 1)], dim=1)
    got = ops.resample(t_prev.to(DEV), wfull.to(DEV), 128, descending=desc).cpu()
    want = torch.sort(torch.cat([t_prev, g["pdf_" + tag]], dim=-1), dim=-1).values
    if desc:
        want = torch.flip(want, dims=[-1])
    # the reference's own fp32-vs-fp64 disagreement on each row's samples (fixture g3_pdf_noise)
    self_noise = noise["noise_pdf_" + tag].double()
    err = (got.double() - want.double()).abs()
    record_parity("resample_golden_bins/" + tag, max_pos_err=float(err[keep].max()),
                  reference_self_noise_max=float(self_noise[keep].max()), rows=int(keep.sum()))
    if not desc:
        assert max_abs(_cdf_space(got[keep], bins[keep], w[keep]), _cdf_space(want[keep], bins[keep], w[keep])) < 2e-6
    # positions: 1e-4 on every row the reference determines to better than 1e-5 (all ascending rows are), the other rows
    # within 1e-4 + 3 x the reference's own fp32-vs-fp64 disagreement on that row (fixture g3_pdf_noise)
    row_noise = self_noise.amax(dim=-1, keepdim=True)
    assert float((err - (1e-4 + 3.0 * row_noise))[keep].max()) <= 0.0, (float(err[keep].max()), float(self_noise[keep].max()))
    well = keep & (row_noise.squeeze(-1) < 1e-5)
    if bool(well.any()):
        assert float(err[well].max()) < 1e-4
    if not desc:
        assert bool(well[keep].all()) and float(err[keep].max()) < 1e-5


def test_composite_modes(golden):
    g = golden("g3_stages")
    rgb, sigma, t, dirs, far = cases.composite_case()
    rs = torch.cat([rgb, sigma], dim=-1).to(DEV)
    r = ops.composite(1, rs, t.to(DEV), dirs.to(DEV), far.to(DEV))
    for nm, key in (("rgb", "rgb"), ("acc", "acc"), ("w", "weights"), ("lam", "bg_lambda"), ("depth", "depth")):
        assert max_abs(r[key].cpu(), g["cfg_" + nm]) < 2e-6, nm
    t_desc = torch.flip(t / t.max(), dims=[-1]).contiguous()
    r = ops.composite(2, rs, t_desc.to(DEV))
    for nm, key in (("rgb", "rgb"), ("acc", "acc"), ("w", "weights"), ("depth", "depth")):
        assert max_abs(r[key].cpu(), g["cbg_" + nm]) < 2e-6, nm
    r = ops.composite(0, rs, t.to(DEV), (dirs * 1.3).to(DEV), white_bkgd=True)
    for nm, key in (("rgb", "rgb"), ("acc", "acc"), ("w", "weights"), ("depth", "depth")):
        assert max_abs(r[key].cpu(), g["cv_" + nm]) < 2e-6, nm
