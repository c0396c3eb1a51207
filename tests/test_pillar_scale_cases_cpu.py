"""CPU: the power-of-two rescalings of tests/pillar_scale_cases.py do what the GPU tests rely on.

For case L (latent) and case W (a packed weight): the fp32 oracle - the reference's arithmetic - returns bitwise the same
floor-plans for the scaled and the unscaled operands, the largest scaled operand is beyond the fp16 range (so the split
arithmetic's range guard must trip on it) and no scaled weight has become subnormal (so the scaling lost no bits)."""
import pytest
import torch

import cases
import oracle
import pillar_scale_cases as P
from neo360_amd import synth

GRID = (12, 10, 8)


def _inputs():
    sc = cases.small_scene()
    poses, focal, centre = synth.source_views(cases.NV, *cases.IMG_WH)
    return sc, poses, focal, centre, synth.pillar_state(0)


@pytest.mark.parametrize("case", ["L", "W"])
def test_scaled_case_is_bitwise_invariant_and_out_of_fp16_range(case):
    torch.set_num_threads(8)
    sc, poses, focal, centre, params = _inputs()
    p2, lat2, scaled = P.CASES[case](params, sc["latent"])
    big, small = P.largest(scaled), P.smallest_nonzero(scaled)
    print("case %s: largest scaled operand %.4g, smallest non-zero scaled operand %.4g" % (case, big, small))
    want = oracle.pillar.floorplans(params, sc["latent"], sc["image_wh"], poses, focal, centre, GRID)
    got = oracle.pillar.floorplans(p2, lat2, sc["image_wh"], poses, focal, centre, GRID)
    for name, a, b in zip(("yz", "xz", "xy"), got, want):
        assert a.dtype == torch.float32 and torch.equal(a, b), (case, name, float((a - b).abs().max()))
    assert big >= P.FP16_MAX, (case, big)
    assert small >= P.FP32_MIN_NORMAL, (case, small)
    for t in scaled.values():
        assert bool(torch.isfinite(t).all())


def test_decoder_compensation_touches_the_local_latent_columns_only():
    sd = synth.nerf_tp_state(0)
    out = P.decoder_compensated(sd)
    for prefix, ch in (("fg_coarse_mlp.", 3), ("bg_fine_mlp.", 4)):
        pe = 21 * ch
        w0, v0 = sd[prefix + "pts_linears.0.weight"], out[prefix + "pts_linears.0.weight"]
        w3, v3 = sd[prefix + "pts_linears.3.weight"], out[prefix + "pts_linears.3.weight"]
        assert w0.shape == (128, pe + 640) and w3.shape == (128, 128 + pe + 640)
        assert torch.equal(v0[:, :pe], w0[:, :pe]) and torch.equal(v0[:, pe + 512:], w0[:, pe + 512:])
        assert torch.equal(v0[:, pe:pe + 512], w0[:, pe:pe + 512] * P.DOWN)
        assert torch.equal(v3[:, :128 + pe], w3[:, :128 + pe]) and torch.equal(v3[:, 128 + pe + 512:], w3[:, 128 + pe + 512:])
        assert torch.equal(v3[:, 128 + pe:128 + pe + 512], w3[:, 128 + pe:128 + pe + 512] * P.DOWN)
    for k in sd:
        if "pts_linears.0.weight" not in k and "pts_linears.3.weight" not in k:
            assert torch.equal(sd[k], out[k]), k
