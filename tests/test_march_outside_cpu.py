"""CPU: the restatements of the outside-sphere termination tests (tests/march_outside_cases.py) on the CPU oracle, the pure rule in
fp32 against fp64, the host-side validation of the marching calls and their ABI declarations.  Nothing here needs a device.

THE MIX.  tests/terminate_cases.py's inputs (foreground density bias +4, the background untouched, EPS = 1e-2, 65 and 135 samples,
segment 64, the 96 strided rays): the oracle culls 61 rays and 35 survive; the survivors' level-1 outside stops are 64 (26 rays),
128 (7 rays) and N = 135 (2 rays) - all three stops at ONE eps, because the running value starts at the ray's own bg_lambda, which
differs from ray to ray by orders of magnitude, not at 1.  The survivor closest to the threshold at a boundary is 1.8e-3 eps away
from it (NEAR_TOL = 1e-5), and the largest level-1 |rgb change| against the same frame with outside=False is 5.3e-3 against the
bound 1.003e-2."""
import os
import re

import pytest
import torch

from conftest import ROOT
import march_outside_cases as mc
import terminate_cases as tc
from neo360_amd import _lib, models, ops

N1 = mc.N_COARSE + 1 + mc.N_FINE


def test_the_mix_of_outside_stops_and_culled_rays():
    inside_only, got, extra = mc.oracle_frames(96)
    culled, bg_stop = extra[1]["culled"], extra[1]["bg_stop"]
    survivors = ~culled
    seen = {s: int((bg_stop[survivors] == s).sum()) for s in sorted(set(bg_stop[survivors].tolist()))}
    dist = mc.threshold_distance(extra[1]["T64_bg"], extra[1]["lam"], mc.EPS, mc.SEGMENT)[survivors]
    print("eps %g: %d culled, %d survive; level-1 outside stops of the survivors %s; closest boundary value %.2e eps from the threshold"
          % (mc.EPS, int(culled.sum()), int(survivors.sum()), seen, float(dist.min())))
    assert len(seen) == 3 and set(seen) == {64, 128, N1}, "three distinct stops among the survivors"
    assert int(culled.sum()) >= 1 and int((survivors & (bg_stop < N1)).sum()) >= 1
    assert bool((bg_stop[culled] == 0).all()) and bool((extra[1]["bg_value"][culled] == 0).all())
    assert bool((extra[0]["bg_stop"][survivors] == mc.N_COARSE + 1).all()), "coarse=False: level 0 is marched in full"
    near = mc.near_threshold_outside(extra[1]["T64_bg"], extra[1]["lam"], mc.EPS, mc.SEGMENT)
    assert not bool(near[survivors].any()), "no survivor within NEAR_TOL eps of the threshold in fp64"
    # the fp64 statement of the rule agrees on every survivor
    s64, _ = mc.stops_outside(extra[1]["T64_bg"], extra[1]["lam"].double(), mc.EPS, mc.SEGMENT)
    assert torch.equal(s64[survivors], bg_stop[survivors])


def test_stopped_rays_obey_the_bounds_and_the_others_are_equal():
    inside_only, got, extra = mc.oracle_frames(96)
    culled, bg_stop = extra[1]["culled"], extra[1]["bg_stop"]
    stopped = ~culled & (bg_stop < N1)
    d_rgb = (got[1][0] - inside_only[1][0]).abs().max(dim=-1).values
    d_depth = (got[1][5] - inside_only[1][5]).abs()
    print("eps %g: max |rgb change| %.3e, max |depth change| %.3e over %d stopped rays; the bound is %.4e"
          % (mc.EPS, float(d_rgb.max()), float(d_depth.max()), int(stopped.sum()), mc.BOUND * mc.EPS))
    assert bool((d_rgb <= mc.BOUND * mc.EPS).all()) and bool((d_depth <= mc.BOUND * mc.EPS).all())
    assert float(d_rgb[stopped].max()) > 0.0, "the stop changed something"
    assert bool((extra[1]["bg_value"][stopped] < mc.EPS).all())
    same = ~stopped
    for lv in range(2):
        for i in range(6):
            x, y = got[lv][i], inside_only[lv][i]
            assert torch.equal(x[same] if lv == 1 else x, y[same] if lv == 1 else y), (lv, i)
    for i in (1, 3, 4):           # fg_rgb, fg_acc, bg_lambda: the foreground reads nothing of the background
        assert torch.equal(got[1][i], inside_only[1][i]), i


def test_weights_behind_the_outside_stop_are_zero():
    _, _, extra = mc.oracle_frames(96)
    for lv in range(2):
        bg_w, bg_stop, culled = extra[lv]["bg_w"], extra[lv]["bg_stop"], extra[lv]["culled"]
        N = bg_w.shape[1]
        behind = (torch.arange(N)[None, :] >= bg_stop[:, None]) & ~culled[:, None]
        assert bool((bg_w[behind] == 0).all()), lv
        assert bool(((bg_stop == N) | (bg_stop % mc.SEGMENT == 0)).all())
    assert bool(behind.any())


def test_eps_zero_stops_nothing():
    b = tc.rays(8)
    plain = tc.oracle_render_terminating(tc.state(), b, tc.scene(), 0.0, n_coarse=8, n_fine=8)
    got, extra = mc.oracle_render_marching(tc.state(), b, tc.scene(), 0.0, n_coarse=8, n_fine=8, keep=True)
    for lv in range(2):
        for i, (x, y) in enumerate(zip(got[lv], plain[lv])):
            assert torch.equal(x, y), (lv, i)
        assert bool((extra[lv]["bg_stop"] == extra[lv]["bg_s"].shape[1]).all())


def _rows(R=12, N=200, seed=3):
    g = torch.Generator().manual_seed(seed)
    s = torch.sort(torch.rand(R, N, generator=g), dim=-1, descending=True).values
    sigma = torch.rand(R, N, generator=g) * 30.0
    lam = 10.0 ** (-3.0 * torch.rand(R, generator=g))
    return sigma, s, lam


@pytest.mark.parametrize("segment", (64, 128))
@pytest.mark.parametrize("eps", (1e-2, 1e-3, 0.3))
def test_the_pure_rule_in_fp32_against_fp64_with_nan_and_infinite_densities(eps, segment):
    sigma, s, lam = _rows()
    sigma[0, 3] = float("nan")            # a NaN density: the running value is NaN from there on and marches on
    sigma[1, 70] = float("nan")           # ... behind the first boundary
    sigma[2, 5] = float("inf")            # alpha = 1: the transmittance is 1e-10 times the rest: a stop at the first boundary
    sigma[3, 5] = float("-inf")           # a transmittance of +inf: marches on
    s[4, 6] = s[4, 5]
    sigma[4, 5] = float("inf")            # inf * 0: NaN
    lam[5] = float("nan")                 # a NaN lambda marches on
    lam[6] = 0.0                          # an opaque foreground that survived through its other level: stops at the first boundary
    T32, T64 = mc.transmittance_outside(sigma, s), mc.transmittance_outside(sigma, s, torch.float64)
    s32, v32 = mc.stops_outside(T32, lam, eps, segment)
    s64, v64 = mc.stops_outside(T64, lam.double(), eps, segment)
    N = s.shape[1]
    for r in (0, 3, 4, 5):
        assert int(s32[r]) == N and int(s64[r]) == N, r
    assert bool(torch.isnan(v32[0])) and bool(torch.isnan(v32[4])) and bool(torch.isnan(v32[5])) and float(v32[3]) == float("inf")
    assert int(s32[2]) == segment and int(s32[6]) == segment and float(v32[6]) == 0.0
    if eps < 0.3:
        assert int(s32[1]) == N or int(s32[1]) == segment      # stopped at the first boundary, or NaN from sample 70 on
    near = mc.near_threshold_outside(T64, lam, eps, segment)
    finite = torch.isfinite(v64) & ~near
    assert int(near.sum()) <= 1
    assert torch.equal(s32[~near], s64[~near])
    assert bool(((v32.double() - v64).abs()[finite] <= 1e-5 * v64[finite].abs() + 1e-37).all())
    assert bool((s32[7:] < N).any()), "ordinary dense rows stop"


def test_the_outside_rule_on_small_rows():
    # boundaries 64 and 128 of 130 samples; lam T falls below eps = 0.05 before 64 / between 64 and 128 / never / NaN marches on
    T = torch.ones(5, 130)
    T[0, 10:] = 0.4
    T[1, 70:] = 0.4
    T[3, 5:] = float("nan")
    lam = torch.tensor([0.1, 0.1, 0.1, 0.1, 0.01])
    stop, value = mc.stops_outside(T, lam, 0.05, 64)
    assert stop.tolist() == [64, 128, 130, 130, 64]          # row 4: the foreground leftover alone is below eps: one segment
    assert value[:3].tolist() == [pytest.approx(0.04), pytest.approx(0.04), pytest.approx(0.1)] and bool(torch.isnan(value[3]))
    assert mc.stops_outside(T, lam, 0.05, 128)[0].tolist() == [128, 128, 130, 130, 128]
    assert mc.stops_outside(T[:, :64], lam, 0.05, 64)[0].tolist() == [64] * 5      # a single segment: nothing to stop
    assert mc.stops_outside(T, lam, 0.0, 64)[0].tolist() == [130] * 5
    assert float(value[4]) == pytest.approx(0.01)


def _header():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(bare, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
    assert m, "%s is not declared in include/neo360_hip.h" % name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_header_declares_and_ctypes_binds_the_marching_entry_points():
    text, bare = _header()
    for name in ("neo_tp_render_marching", "neo_tp_termination_stops_outside"):
        assert len(_lib.SIGNATURES[name][1]) == len(_params(bare, name)), name
        assert hasattr(_lib.load(), name)
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*neo_tp_march_samples\s*;", bare)
    fields = [f.split("*")[-1].strip() for f in m.group(1).split(";") if f.strip()]
    accel = [n for n, _ in _lib.TpAccelSamples._fields_]
    assert fields == [n for n, _ in _lib.TpMarchSamples._fields_] == accel + ["bg_stop", "bg_value", "bg_rows"]
    assert "OUTSIDE STOP RULE" in text
    # the two older entry points keep their signatures
    assert len(_params(bare, "neo_tp_render_terminating")) == len(_params(bare, "neo_tp_render_accelerated")) == 23
    assert len(_params(bare, "neo_tp_render_marching")) == 25


def test_marching_calls_validate_on_the_host():
    net = models.NeRF_TP(num_coarse_samples=8, num_fine_samples=8)
    assert net.last_march_kept is None and net.last_march_survivors is None
    b = tc.rays(96)
    rows, s, lam = torch.zeros(96, 9, 4), torch.zeros(96, 9), torch.ones(96)
    for eps in (-1e-3, 1.0, 1.5, float("nan"), float("inf"), None, "0.1", True):
        with pytest.raises(ValueError):
            net.render_marching(b, eps)
        with pytest.raises(ValueError):
            ops.termination_stops_outside(rows, s, lam, eps)
    for segment in (0, -64, 32, 65, 96, 64.0, None, True):
        with pytest.raises(ValueError):
            net.render_marching(b, 0.01, segment=segment)
        with pytest.raises(ValueError):
            ops.termination_stops_outside(rows, s, lam, 0.01, segment=segment)
    for args in ((rows[:, :8], s, lam), (rows, s[0], lam), (rows, s, lam[:5]), (rows, s.long(), lam), (rows[..., :3], s, lam),
                 (rows[:, :0], s[:, :0], lam), (rows, s, torch.ones(96, 2))):
        with pytest.raises(ValueError):
            ops.termination_stops_outside(*args, 0.01)
    with pytest.raises(TypeError):           # eps has no default
        net.render_marching(b)
