"""CPU: the conditions of tests/dense_mlp_cases.py - finite fp64 references, the fp32 oracle inside a third of every bound on
every case, the fp32 oracle bitwise invariant under every power-of-two rescaling, the UP states out of the fp16 range through
their activations only, and the degenerate rows of the 9 x 7 Mip case really degenerate."""
import pytest
import torch

import dense_mlp_cases as D


def _oracle_share(ref64, ref32, label):
    assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(ref32).all()), label
    checks = D.eval_checks(ref32, ref64, ref32)
    for k, v in checks.items():
        assert v["ratio"] <= D.ORACLE_SHARE, (label, k, "the fp32 oracle uses %.3f of the bound %.3e" % (v["ratio"], v["bound"]))


@pytest.mark.parametrize("shape", D.MIP_SHAPES, ids=D.shape_id)
@pytest.mark.parametrize("slot", [0, 2])
def test_mip_references(shape, slot):
    ref64, ref32 = D.mip_reference(*shape, slot), D.mip_reference(*shape, slot, D.MIP_GAIN, torch.float32)
    assert ref64.dtype == torch.float64 and ref64.shape == shape + (4,)
    _oracle_share(ref64, ref32, ("mip", shape, slot))
    if slot == 0:
        assert float(ref64[..., :3].abs().max()) == 0.0


def test_mip_strong_weights_reference():
    shape, gain, radii = D.MIP_STRONG
    ref64 = D.mip_reference(*shape, 2, gain, torch.float64, radii)
    _oracle_share(ref64, D.mip_reference(*shape, 2, gain, torch.float32, radii), ("mip strong", shape))
    assert float(ref64[..., 3].max()) > 0.75                    # the point of the case: densities several times the default's


@pytest.mark.parametrize("shape", D.VANILLA_SHAPES, ids=D.shape_id)
@pytest.mark.parametrize("prefix", [p for p, _ in D.VANILLA_LEVELS])
def test_vanilla_references(shape, prefix):
    ref64 = D.vanilla_reference(*shape, prefix)
    assert ref64.dtype == torch.float64 and ref64.shape == shape + (4,)
    _oracle_share(ref64, D.vanilla_reference(*shape, prefix, torch.float32), ("vanilla", shape, prefix))


def test_point_counts_sit_on_the_tile_edges():
    assert [r * n for r, n in D.MIP_SHAPES] == [1, 31, 33, 63, 65, 203, 2047, 2048, 2049]
    assert [r * n for r, n in D.MIP_BITWISE_SHAPES] == [8191, 8193, 16385]
    assert [r * n for r, n in D.VANILLA_SHAPES] == [1, 63, 64, 65, 127, 128, 129, 203, 257]


def test_mip_degenerate_rows():
    rays, tdist = D.mip_inputs(*D.MIP_DEG)
    assert float(tdist[0, 4]) == float(tdist[0, 3]) and float(rays["radii"][1]) == 0.0
    assert bool((tdist[:, 1:] >= tdist[:, :-1]).all()) and float(tdist[3, -1]) == 1e6
    norms = D.mip_means(*D.MIP_DEG).norm(dim=-1)
    assert float(norms[2].min()) < 2e-3                           # an interval mean next to the world origin
    assert float(norms[3].max()) > 1e5
    side = norms[D.STRADDLE_ROW] <= 1.0                           # the contraction's branch, as oracle.mip360.contract takes it
    assert int(side.sum()) >= 2 and int((~side).sum()) >= 2, norms[D.STRADDLE_ROW]
    means32 = D.mip_means(*D.MIP_DEG, torch.float32).norm(dim=-1)
    assert torch.equal(means32[D.STRADDLE_ROW] <= 1.0, side)      # and no mean so close to 1 that fp32 and fp64 take different sides


def test_vanilla_degenerate_rows():
    inp = D.vanilla_inputs(*D.VANILLA_DEG)
    assert float(inp["t"][0, 4]) == float(inp["t"][0, 3]) and float(inp["dirs"][1].abs().max()) == 0.0
    assert abs(float(inp["dirs"][2].norm()) - 1.7) < 1e-5
    assert bool((inp["t"][:, 1:] >= inp["t"][:, :-1]).all()) and float(inp["t"].min()) >= D.NEAR and float(inp["t"].max()) <= D.FAR


@pytest.mark.parametrize("net,direction,shift", D.scale_states(), ids=lambda v: str(v))
def test_fp32_oracle_is_bitwise_invariant_under_rescaling(net, direction, shift):
    state, scaled = D.scaled_state(net, shift, up=direction == "up")
    assert torch.equal(D.scale_oracle(net, state, torch.float32), D.scale_reference(net, torch.float32))
    for name, t in scaled.items():
        nz = t[t != 0].abs()
        assert float(nz.min()) >= D.FP32_MIN_NORMAL and bool(torch.isfinite(t).all()), (name, "fp32-subnormal or non-finite weight")


@pytest.mark.parametrize("net", list(D.SCALE_NETS))
def test_up_states_leave_the_fp16_range_through_activations_only(net):
    state, scaled = D.scaled_state(net, D.UP_SHIFT[net], up=True)
    assert max(D.layer_weight_maxima(net, state).values()) < D.FP16_MAX
    assert max(float(t.abs().max()) for t in scaled.values()) < D.FP16_MAX
    assert float(D.layer1_activations(net, state).max()) >= D.FP16_MAX
    assert max(D.layer1_activations(net, state, behind=True)) < D.FP16_MAX / 2       # only layer 1's activations leave the range
    assert not D.below_low(net, state)                                                # and no layer is under the low end
    # one more doubling would take a weight out of the range: the shift is the largest that fits
    assert max(float(t.abs().max()) for t in D.scaled_state(net, D.UP_SHIFT[net] + 1, up=True)[1].values()) >= D.FP16_MAX


def test_low_end_rule_on_the_table():
    """Which DOWN states the static low-end check flags: layer 1's largest |w| below LOW.  No unscaled network is flagged."""
    assert D.LOW == 2.0 ** round(__import__("math").log2(D.LOW))
    for net in D.SCALE_NETS:
        assert not D.below_low(net, D.base_state(net))
        flagged = [s for s in D.DOWN_SHIFTS if D.below_low(net, D.scaled_state(net, s)[0])]
        assert flagged == [s for s in D.DOWN_SHIFTS if s >= min(flagged)], (net, flagged)      # monotone in the shift
    for gain in (D.MIP_GAIN, 1.0):
        for slot in (0, 1, 2):
            ws = [float(v.abs().max()) for k, v in D.mip_state(gain).items() if k.startswith("mlps.%d." % slot) and k.endswith(".weight")]
            assert min(ws) >= D.LOW
