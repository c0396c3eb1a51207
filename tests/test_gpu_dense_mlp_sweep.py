"""GPU: the vanilla NeRF and Mip-NeRF 360 point evaluators - exact fp32 and split-fp16, fused and layer by layer - through
NeRF.eval_mlp and MipNeRF360.eval_mlp on point counts either side of every tile edge, per entry against fp64; the two vanilla
split kernels that only an environment variable selects, each in a child process; power-of-two rescalings of two trunk layers
(exact kernels: bitwise the same output; split kernels: inside the bound or flagged, never silently outside); the range guard of
the Mip-NeRF 360 slots.  Cases, references and bounds: tests/dense_mlp_cases.py (checked on the CPU by
tests/test_dense_mlp_cases_cpu.py); the worst share of a bound per case goes to the parity report under dense_mlp_sweep/."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import alongray_cases as A
import dense_mlp_cases as D
from conftest import record_parity
from neo360_amd import _lib, models, render, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 180          # seconds: a child imports torch, opens the device and evaluates 18 small cases (about 10 s)

# label -> (slot, precision, layered)
MIP_PATHS = {"prop-f32": (0, "f32", False), "prop-f16x3": (0, "f16x3", False), "nerf-f32": (2, "f32", False),
             "nerf-fused": (2, "f16x3", False), "nerf-layered": (2, "f16x3", True)}
EXACT_OF = {"prop-f16x3": "prop-f32", "nerf-fused": "nerf-f32", "nerf-layered": "nerf-f32"}
_NETS, _MIP_OUT, _VAN_OUT = {}, {}, {}


def _dev(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _mip_net(precision, layered, gain=D.MIP_GAIN):
    key = ("mip", precision, layered, gain)
    if key not in _NETS:
        net = models.MipNeRF360().to(DEV)
        net.precision = precision
        net.layered = layered
        net.load_state_dict(D.mip_state(gain))
        _NETS[key] = net
    return _NETS[key]


def _vanilla_net(precision):
    key = ("vanilla", precision)
    if key not in _NETS:
        net = models.NeRF().to(DEV)
        net.precision = precision
        net.load_state_dict(synth.vanilla_state(0))
        _NETS[key] = net
    return _NETS[key]


def _mip_output(path, shape, gain=D.MIP_GAIN, radii_gain=1.0):
    key = (path, shape, gain, radii_gain)
    if key not in _MIP_OUT:
        slot, precision, layered = MIP_PATHS[path]
        rays, tdist = D.mip_inputs(*shape, radii_gain)
        _MIP_OUT[key] = _mip_net(precision, layered, gain).eval_mlp(slot, _dev(rays), tdist.to(DEV)).cpu()
    return _MIP_OUT[key]


def _vanilla_output(precision, level, shape):
    key = (precision, level, shape)
    if key not in _VAN_OUT:
        inp = _dev(D.vanilla_inputs(*shape))
        _VAN_OUT[key] = _vanilla_net(precision).eval_mlp(level, inp["rays_o"], inp["dirs"], inp["t"]).cpu()
    return _VAN_OUT[key]


def _judge(label, checks):
    record_parity("dense_mlp_sweep/" + label, **A.summarize(checks))
    print(label, {k: "%.2e of %.2e (fp32 oracle %.2e)" % (v["err"], v["bound"], v["fp32"]) for k, v in checks.items()})
    A.assert_inside(checks, label)
    return checks


# ---- Mip-NeRF 360 ------------------------------------------------------------------------------------------------------------------
def _mip_checks(path, shape, gain=D.MIP_GAIN, radii_gain=1.0):
    slot = MIP_PATHS[path][0]
    got = _mip_output(path, shape, gain, radii_gain)
    assert got.shape == shape + (4,)
    ref64 = D.mip_reference(*shape, slot, gain, torch.float64, radii_gain)
    checks = D.eval_checks(got, ref64, D.mip_reference(*shape, slot, gain, torch.float32, radii_gain))
    if path in EXACT_OF:
        checks.update(D.split_vs_exact_checks(got, _mip_output(EXACT_OF[path], shape, gain, radii_gain), ref64))
    if slot == 0:
        assert float(got[..., :3].abs().max()) == 0.0              # a proposal MLP has no colour
    return checks


@pytest.mark.parametrize("shape", D.MIP_SHAPES, ids=D.shape_id)
@pytest.mark.parametrize("path", list(MIP_PATHS))
def test_mip_evaluators(path, shape):
    _judge("mip/%s/%s" % (path, D.shape_id(shape)), _mip_checks(path, shape))


@pytest.mark.parametrize("path", list(MIP_PATHS))
def test_mip_evaluators_strong_weights(path):
    shape, gain, radii = D.MIP_STRONG
    _judge("mip/%s/%s-gain1" % (path, D.shape_id(shape)), _mip_checks(path, shape, gain, radii))


@pytest.mark.parametrize("shape", D.MIP_SHAPES + D.MIP_BITWISE_SHAPES, ids=D.shape_id)
def test_mip_layered_equals_fused(shape):
    """The layer-by-layer schedule runs the same products in the same k order as the fused evaluator: bitwise equal outputs, with
    a last tile of 1 .. 31 intervals, a padded batch (2048) one short, full and one over, and one interval into a second batch."""
    fused, layer = _mip_output("nerf-fused", shape), _mip_output("nerf-layered", shape)
    assert bool(torch.isfinite(layer).all())
    assert torch.equal(layer, fused), float((layer - fused).abs().max())
    if shape in D.MIP_AUTO_SHAPES:                                 # one below and one above the automatic switch at 8192 intervals
        rays, tdist = D.mip_inputs(*shape)
        assert torch.equal(_mip_net("f16x3", None).eval_mlp(2, _dev(rays), tdist.to(DEV)).cpu(), fused)


# ---- vanilla NeRF ------------------------------------------------------------------------------------------------------------------
def _vanilla_checks(got, prefix, shape, exact=None):
    assert got.shape == shape + (4,)
    ref64 = D.vanilla_reference(*shape, prefix)
    checks = D.eval_checks(got, ref64, D.vanilla_reference(*shape, prefix, torch.float32))
    if exact is not None:
        checks.update(D.split_vs_exact_checks(got, exact, ref64))
    return checks


@pytest.mark.parametrize("shape", D.VANILLA_SHAPES, ids=D.shape_id)
@pytest.mark.parametrize("prefix,level", D.VANILLA_LEVELS, ids=[p[:-5] for p, _ in D.VANILLA_LEVELS])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_vanilla_evaluators(precision, prefix, level, shape):
    exact = _vanilla_output("f32", level, shape) if precision == "f16x3" else None
    _judge("vanilla/%s/%s%s" % (precision, prefix, D.shape_id(shape)), _vanilla_checks(_vanilla_output(precision, level, shape), prefix, shape, exact))


def test_vanilla_kernel_variants_in_child_processes(tmp_path):
    """k_vanilla_mlp_h<8,2> ($NEO_VANILLA_H_WAVES=8) and k_vanilla_mlp_h<4,4> ($NEO_VANILLA_H_TILE=128): the variable is read once
    per process, so each runs the vanilla table in a fresh child, one after the other; the parent judges the outputs by the same
    references and bounds.  A child that times out or dies ends the test; nothing is retried."""
    judged = []
    for tag, var in (("waves8", "NEO_VANILLA_H_WAVES=8"), ("tile128", "NEO_VANILLA_H_TILE=128")):
        env = {k: v for k, v in os.environ.items() if k not in ("NEO_VANILLA_H_WAVES", "NEO_VANILLA_H_TILE")}
        env.update([var.split("=")])
        out = tmp_path / (tag + ".npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "dense_mlp_child.py"), str(out)], env=env, timeout=CHILD_TIMEOUT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, (tag, r.returncode, r.stdout[-2000:])
        with np.load(out) as z:
            got = {k: torch.from_numpy(z[k]) for k in z.files}
        for shape in D.VANILLA_SHAPES:
            for prefix, level in D.VANILLA_LEVELS:
                label = "vanilla/%s/%s%s" % (tag, prefix, D.shape_id(shape))
                checks = _vanilla_checks(got[prefix + D.shape_id(shape)], prefix, shape, _vanilla_output("f32", level, shape))
                record_parity("dense_mlp_sweep/" + label, **A.summarize(checks))
                judged.append((label, checks))
    for label, checks in judged:
        A.assert_inside(checks, label)


# ---- power-of-two rescalings -------------------------------------------------------------------------------------------------------
# split path -> (net of the scale table, how to evaluate the 9 x 7 case with a state)
SPLIT_PATHS = {"vanilla": "vanilla", "mip-prop-fused": "mip_prop", "mip-nerf-fused": "mip_nerf", "mip-nerf-layered": "mip_nerf"}
_SCALE_NETS = {}


def _scale_net(path, precision):
    """One module per (path, arithmetic), reloaded with every state of the table."""
    key = (path, precision)
    if key not in _SCALE_NETS:
        if path == "vanilla":
            net = models.NeRF().to(DEV)
        else:
            net = models.MipNeRF360().to(DEV)
            net.layered = path.endswith("layered")
        net.precision = precision
        _SCALE_NETS[key] = net
    return _SCALE_NETS[key]


def _scale_eval(path, precision, state):
    net = _scale_net(path, precision)
    net.load_state_dict(state)
    if path == "vanilla":
        inp = _dev(D.vanilla_inputs(*D.VANILLA_DEG))
        return net.eval_mlp(0, inp["rays_o"], inp["dirs"], inp["t"]).cpu()
    rays, tdist = D.mip_inputs(*D.MIP_DEG)
    return net.eval_mlp(int(D.SCALE_NETS[SPLIT_PATHS[path]][0][5]), _dev(rays), tdist.to(DEV)).cpu()


_STATE_IDS = ["%s-%s%d" % s for s in D.scale_states()]


@pytest.mark.parametrize("net,direction,shift", D.scale_states(), ids=_STATE_IDS)
def test_exact_kernels_bitwise_under_rescaling(net, direction, shift):
    """k_vanilla_mlp and k_mip_mlp: a power of two only moves the exponent of every product and partial sum, so the output is the
    same bits for the scaled and the unscaled network - no tolerance."""
    path = {"vanilla": "vanilla", "mip_prop": "mip-prop-fused", "mip_nerf": "mip-nerf-fused"}[net]
    base = _scale_eval(path, "f32", D.base_state(net))
    _judge("scale/f32/%s/base" % net, D.eval_checks(base, D.scale_reference(net), D.scale_reference(net, torch.float32)))
    got = _scale_eval(path, "f32", D.scaled_state(net, shift, up=direction == "up")[0])
    assert torch.equal(got, base), float((got - base).abs().max())


_SPLIT_STATES = [(path,) + s for path, net in SPLIT_PATHS.items() for s in D.scale_states() if s[0] == net]


@pytest.mark.parametrize("path,net,direction,shift", _SPLIT_STATES, ids=["%s-%s%d" % (s[0], s[2], s[3]) for s in _SPLIT_STATES])
def test_split_kernels_inside_the_bound_or_flagged(path, net, direction, shift):
    """Every state of the table either raises NeoRangeError or is inside the per-entry bound against fp64.  Which: an UP state
    raises on its activations (static_operand False); a DOWN state with a layer under the low end of the split arithmetic
    (dense_mlp_cases.LOW) raises as a static operand; every other state is inside the bound, and uses at most half of it.  After
    a raise the same module with healthy weights evaluates cleanly."""
    state = D.scaled_state(net, shift, up=direction == "up")[0]
    label = "scale/%s/%s%d" % (path, direction, shift)
    ref64, ref32 = D.scale_reference(net), D.scale_reference(net, torch.float32)
    expect_raise = direction == "up" or D.below_low(net, state)
    try:
        got = _scale_eval(path, "f16x3", state)
    except _lib.NeoRangeError as err:
        record_parity("dense_mlp_sweep/" + label, flagged=1.0, static_operand=float(err.static_operand))
        assert expect_raise, (label, "flagged, but every operand is inside the range")
        assert err.static_operand is (direction == "down"), (label, err.static_operand)
        assert ("fp32 accuracy" if direction == "down" else "fp16 range") in str(err)
        healthy = _scale_eval(path, "f16x3", D.base_state(net))           # the flag word was cleared by the raise
        _judge(label + "/healthy-after", D.eval_checks(healthy, ref64, ref32))
        return
    checks = _judge(label, D.eval_checks(got, ref64, ref32))               # never silently outside
    assert not expect_raise, (label, "expected the range guard to trip", A.summarize(checks))
    assert max(v["ratio"] for v in checks.values()) <= 0.5, (label, "an unflagged state may use half of its bound", A.summarize(checks))


# ---- the range guard of the Mip-NeRF 360 slots ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot,layered", [(0, False), (2, False), (2, True)])
def test_mip_weight_out_of_range_raises(slot, layered):
    """Mirrors test_gpu_range_guard.py::test_vanilla_weight_out_of_range_raises for the Mip-NeRF 360 slots."""
    rays, tdist = D.mip_inputs(*D.MIP_DEG)
    rays, tdist = _dev(rays), tdist.to(DEV)
    name = "mlps.%d.pts_linear.3.weight" % slot
    state = {k: v.clone() for k, v in D.mip_state().items()}
    state[name][5, 7] = 7.0e4
    net = models.MipNeRF360().to(DEV)
    net.layered = layered
    net.load_state_dict(state)
    with pytest.raises(_lib.NeoRangeError, match="fp16 range") as exc:
        net.eval_mlp(slot, rays, tdist)
    assert exc.value.static_operand is True
    exact = models.MipNeRF360().to(DEV)                          # the exact path has no such limit and no flag leaks into it
    exact.precision = "f32"
    exact.load_state_dict(state)
    assert bool(torch.isfinite(exact.eval_mlp(slot, rays, tdist)).all())
    exact.check_flags()
    state[name][5, 7] = float("nan")
    net.load_state_dict(state)
    with pytest.raises(_lib.NeoError):
        net.eval_mlp(slot, rays, tdist)
    net.load_state_dict(D.mip_state())                           # the word was cleared: healthy weights on the same module work
    got = net.eval_mlp(slot, rays, tdist).cpu()
    A.assert_inside(D.eval_checks(got, D.mip_reference(*D.MIP_DEG, slot)), "healthy after a raise")
    net.close()
    exact.close()


def test_mip_frame_with_small_weights_is_rendered_in_f32():
    """A Mip-NeRF 360 model in a DOWN state the low-end check flags goes through render.render_rays_test: one warning, the frame
    bitwise what precision 'f32' returns, and the module latched for the next frame."""
    shift = max(D.DOWN_SHIFTS)
    state = D.scaled_state("mip_nerf", shift)[0]
    assert D.below_low("mip_nerf", state)
    batch = _dev(D.mip_inputs(24, 1)[0])
    net = models.MipNeRF360(num_prop_samples=16, num_nerf_samples=8).to(DEV)
    net.load_state_dict(state)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        first = render.render_rays_test(net, batch)
        second = render.render_rays_test(net, batch)
    assert len([w for w in seen if "fp16 range" in str(w.message)]) == 1
    assert first["precision_used"] == "f32" and second["precision_used"] == "f32"
    assert net._range_latch == net.operands_key()
    exact = models.MipNeRF360(num_prop_samples=16, num_nerf_samples=8).to(DEV)
    exact.precision = "f32"
    exact.load_state_dict(state)
    want = render.render_rays_test(exact, batch)
    assert torch.equal(first["rgb"], want["rgb"]) and torch.equal(second["rgb"], want["rgb"])
    assert bool(torch.isfinite(first["rgb"]).all())
    net.close()
    exact.close()
