"""CPU: the host side of the opt-in background culling (NeRF_TP.cull_background, neo_tp_render_culled) and the scene the GPU
tests of it (tests/test_gpu_cull_background.py) stand on.

The scene is pinned to the REFERENCE arithmetic, not to the code under test: the CPU oracle renders cases.small_scene() with the
two foreground density biases raised by +3 / +4 / +5 and must show the foreground transmittances (bg_lambda) the GPU tests were
designed around.  The quoted figures were taken at 128 + 256 samples and are given to two significant digits; the transmittance
of a ray is the exponential of an integral of the density and moves by less than one unit of the last quoted digit between
sample counts, which is the tolerance used here at 32 + 32 samples."""
import os
import re

import pytest
import torch

import cases
import oracle
from conftest import ROOT
from neo360_amd import _lib, models, synth


def test_attribute_defaults_to_off_and_validates():
    net = models.NeRF_TP(num_coarse_samples=8, num_fine_samples=8)
    assert net.cull_background is None and net.last_cull_survivors is None
    for ok in (1e-2, 0.5, 1e-6, float(torch.tensor(0.25))):
        net.cull_background = ok
        assert net.cull_background == ok
    net.cull_background = None
    assert net.cull_background is None
    for bad in (0.0, 1.0, -1e-3, 1.5, float("nan"), float("inf"), 1, 0, True, False, "0.01", [0.01], torch.tensor(0.01)):
        with pytest.raises(ValueError):
            net.cull_background = bad
        assert net.cull_background is None, "a rejected value must not stick"


def test_header_declares_and_ctypes_binds_the_culled_render():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
        assert m, "%s is not declared in include/neo360_hip.h" % name
        return [p.strip() for p in m.group(1).split(",")]
    plain, culled = params("neo_tp_render"), params("neo_tp_render_culled")
    # neo_tp_render's arguments, then `float eps` and the `int* survivors_out` device pointer, then the stream
    assert culled[:len(plain) - 1] == plain[:-1]
    assert re.fullmatch(r"float\s+eps", culled[len(plain) - 1])
    assert re.fullmatch(r"int\s*\*\s*survivors_out", culled[len(plain)])
    assert culled[-1] == plain[-1] and len(culled) == len(plain) + 2
    res, args = _lib.SIGNATURES["neo_tp_render_culled"]
    res0, args0 = _lib.SIGNATURES["neo_tp_render"]
    assert res is res0 and len(args) == len(culled)
    assert args[:len(args0) - 1] == args0[:-1] and args[-3] is _lib._f and args[-2] is _lib._vp and args[-1] is args0[-1]
    # the bound is stated where the entry point is declared
    comment = text[:text.index("int neo_tp_render_culled")].rsplit("/*", 1)[1]
    assert "1.002" in comment and "1.001" in comment and "range check" in comment


def _lambdas(bias, n_coarse=32, n_fine=32):
    st = synth.nerf_tp_state(0)
    for k in ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias"):
        st[k] = st[k] + bias
    out = oracle.neo360.render(st, cases.neo_batch(cases.strided_rays(96)), cases.small_scene(), n_coarse=n_coarse, n_fine=n_fine,
                               out_depth=True)
    return out[0][4].reshape(-1), out[1][4].reshape(-1)


@pytest.mark.parametrize("bias,lo,hi,unit", [(3.0, 0.026, 0.055, 1e-3), (4.0, 0.0055, 0.0147, 1e-4), (5.0, 0.0011, 0.0037, 1e-4)])
def test_oracle_puts_the_test_scene_where_the_gpu_tests_expect_it(bias, lo, hi, unit):
    l0, l1 = _lambdas(bias)
    print("bias %+g: level-1 lambda %.5f .. %.5f, median %.5f; level-0 %.5f .. %.5f"
          % (bias, float(l1.min()), float(l1.max()), float(l1.median()), float(l0.min()), float(l0.max())))
    assert abs(float(l1.min()) - lo) <= unit and abs(float(l1.max()) - hi) <= unit
    gone = (l0 < 1e-2) & (l1 < 1e-2)          # the culling rule at the GPU tests' eps
    if bias == 3.0:
        assert not bool(gone.any())
    elif bias == 5.0:
        assert bool(gone.all())
    else:
        assert abs(float(l1.median()) - 0.0089) <= unit
        assert not bool((l1 < 5e-3).any())
        frac = float((l1 < 1e-2).float().mean())
        assert abs(frac - 0.64) <= 0.05, frac      # 64 % at 128 + 256 samples; one ray of 96 is 1 %
        assert 0.2 <= float(gone.float().mean()) <= 0.8, "a mixed frame at eps = 1e-2"


def test_oracle_extremes_cull_nothing_and_everything():
    l0, l1 = _lambdas(0.0)
    assert float(torch.minimum(l0, l1).min()) > 0.5           # about 0.6 on every ray: nothing is culled at 1e-2
    l0, l1 = _lambdas(8.0)
    assert float(torch.maximum(l0, l1).max()) < 6e-5          # everything is
