"""CPU: the restatements of the early-ray-termination tests (tests/terminate_cases.py) on the CPU oracle, the host-side validation
of the termination calls and their ABI declarations.  Nothing here needs a device.

THE MIX.  tests/terminate_cases.py fixes BIAS = 4 and EPS = 1e-2 at 64 + 70 samples (65 and 135 per ray, segment 64).  On the 96
rays the oracle then stops 6 rays at 128 and marches 90 to N = 135, culls 61 rays and keeps 35: two different level-1 stops, N
among them, culled and surviving rays.  A THIRD stop (64) cannot appear at the same eps on this scene, whatever the bias: the
synthetic scene is a nearly homogeneous fog and the fine samples are quantiles of the coarse weights, so the transmittance in
front of sample 64 lies in one narrow band for all rays and the one in front of sample 128 in another, far below it (bias 4:
0.300 .. 0.380 against 0.0085 .. 0.021; bias -4: 0.9942 .. 0.9965 against 0.9883 .. 0.9918; bias 12: 0.161 .. 0.181 against
4.5e-8 .. 5.5e-7) - no eps is below some ray's first band and not below another ray's second.  The stop at 64 is therefore
covered by a second operating point, EPS_HIGH = 0.33 inside the first band: stops 64 and 128, every ray culled.  Both mixes are
asserted here, so the GPU tests that render them cannot pass vacuously; together they show all three stops.

Where the fp64 restatement of a boundary transmittance is compared with fp32 values, rays with |T - eps| <= 1e-5 eps at a boundary
are left out; their share is capped at 1 % of every input, asserted."""
import os
import re

import pytest
import torch

from conftest import ROOT
import terminate_cases as tc
from neo360_amd import _lib, models, ops

EPS_HIGH = 0.33


@pytest.mark.parametrize("eps,want_stops,mixed_cull", ((tc.EPS, (128, 135), True), (EPS_HIGH, (64, 128), False)))
def test_the_mix_of_stops_and_culled_rays(eps, want_stops, mixed_cull):
    plain, got, extra = tc.oracle_frames(96, eps)
    stop1 = extra[1]["stop"]
    seen = sorted(set(stop1.tolist()))
    print("eps %g: level-1 stops %s, culled %d of 96" % (eps, {s: int((stop1 == s).sum()) for s in seen}, int(extra[1]["culled"].sum())))
    assert tuple(seen) == want_stops
    assert all(int((stop1 == s).sum()) >= 3 for s in seen)
    assert bool((extra[0]["stop"] == tc.N_COARSE + 1).all())          # coarse=False: level 0 is marched in full
    culled = extra[1]["culled"]
    if mixed_cull:
        assert int(culled.sum()) >= 10 and int((~culled).sum()) >= 10
        assert bool(((stop1 < 135) & culled).any()) and bool(((stop1 == 135) & ~culled).any())
    else:
        assert bool(culled.all())


def test_all_three_stops_appear_over_the_two_operating_points():
    seen = set()
    for eps in (tc.EPS, EPS_HIGH):
        seen |= set(tc.oracle_frames(96, eps)[2][1]["stop"].tolist())
    assert seen == {64, 128, 135}


@pytest.mark.parametrize("eps", (tc.EPS, EPS_HIGH))
def test_stopped_rays_obey_the_bounds_and_the_others_are_equal(eps):
    plain, got, extra = tc.oracle_frames(96, eps)
    N1 = tc.N_COARSE + 1 + tc.N_FINE
    stop, culled, far = extra[1]["stop"], extra[1]["culled"], extra[1]["far"].squeeze(-1)
    lam = got[1][4].squeeze(-1)
    stopped = stop < N1
    assert bool((lam[stopped] < eps).all())
    d_rgb = (got[1][0] - plain[1][0]).abs().max(dim=-1).values
    d_depth = (got[1][5] - plain[1][5]).abs()
    print("eps %g: max |rgb change| / lambda = %.4f, max |depth change| / ((t_far + 1.001) lambda) = %.4f over %d stopped rays"
          % (eps, float((d_rgb / lam)[stopped].max()), float((d_depth / ((far + 1.001) * lam))[stopped].max()), int(stopped.sum())))
    assert bool((d_rgb[stopped] <= 1.003 * lam[stopped]).all())
    assert bool((d_depth[stopped] <= (far[stopped] + 1.001) * lam[stopped]).all())
    # a culled ray that marched to N obeys the bound as well: its lambda is the plain frame's
    assert bool((d_rgb[culled] <= 1.003 * lam[culled]).all())
    same = ~stopped & ~culled
    for i in range(6):
        assert torch.equal(got[1][i][same], plain[1][i][same]), i
        # level 0 is marched in full: only the dropped background differs
        assert torch.equal(got[0][i][~culled], plain[0][i][~culled]), i
    for lv in range(2):
        assert bool((got[lv][2][culled] == 0).all()) and torch.equal(got[lv][0][culled], got[lv][1][culled])
        for i in (1, 3, 4):        # fg_rgb, fg_acc, bg_lambda of a ray that was not stopped do not know about the cull
            keep = culled & ~(stopped if lv == 1 else torch.zeros_like(stopped))
            assert torch.equal(got[lv][i][keep], plain[lv][i][keep]), (lv, i)


def test_eps_zero_is_the_plain_frame():
    plain, got, extra = tc.oracle_frames(96, 0.0)
    for lv in range(2):
        assert len(got[lv]) == len(plain[lv]) == 6
        for i, (x, y) in enumerate(zip(got[lv], plain[lv])):
            assert x.dtype == y.dtype and torch.equal(x, y), (lv, i)
        assert bool((extra[lv]["stop"] == extra[lv]["fg_t"].shape[1]).all()) and not bool(extra[lv]["culled"].any())


@pytest.mark.parametrize("eps,coarse", ((tc.EPS, False), (EPS_HIGH, False), (EPS_HIGH, True)))
def test_the_evaluated_set_is_a_prefix_of_whole_segments(eps, coarse):
    _, got, extra = tc.oracle_frames(96, eps, coarse)
    for lv in range(2):
        stop, w = extra[lv]["stop"], extra[lv]["fg_w"]
        N = w.shape[1]
        assert bool(((stop == N) | ((stop % tc.SEGMENT == 0) & (stop > 0) & (stop < N))).all())
        j = torch.arange(N)
        assert bool((w[j[None, :] >= stop[:, None]] == 0).all())
        # the transmittance the composite returns for a stopped ray is the one at its stop
        halted = stop < N
        want = extra[lv]["T"][torch.arange(96), (stop - 1).clamp(min=0)]
        assert torch.equal(got[lv][4].squeeze(-1)[halted], want[halted])
    if coarse:
        assert set(extra[0]["stop"].tolist()) == {64}          # the level-0 transmittance at 64 of 65 samples is far below 0.33


@pytest.mark.parametrize("eps", (tc.EPS, EPS_HIGH, 1e-3, 0.5))
@pytest.mark.parametrize("segment", (64, 128))
def test_fp32_and_fp64_stops_agree_away_from_the_threshold(eps, segment):
    _, _, extra = tc.oracle_frames(96, 0.0)
    for lv in range(2):
        T, T64 = extra[lv]["T"], extra[lv]["T64"]
        s32, t32 = tc.stops(T, eps, segment)
        s64, t64 = tc.stops(T64, eps, segment)
        near = tc.near_threshold(T64, eps, segment)
        assert int(near.sum()) <= 0.01 * near.numel(), (lv, int(near.sum()))
        assert torch.equal(s32[~near], s64[~near]), lv
        assert bool(((t32.double() - t64).abs()[~near] <= 1e-5 * t64[~near]).all())


def test_the_stop_rule_on_small_rows():
    # 3 rays, 130 samples, segment 64: boundaries 64 and 128.  T drops below eps = 0.5 before 64 / between 64 and 128 / never; a NaN marches on
    T = torch.ones(4, 130)
    T[0, 10:] = 0.4
    T[1, 70:] = 0.4
    T[3, 5:] = float("nan")
    stop, trans = tc.stops(T, 0.5, 64)
    assert stop.tolist() == [64, 128, 130, 130]
    assert trans[:3].tolist() == [pytest.approx(0.4), pytest.approx(0.4), 1.0] and bool(torch.isnan(trans[3]))
    assert tc.stops(T, 0.5, 128)[0].tolist() == [128, 128, 130, 130]
    assert tc.stops(T[:, :64], 0.5, 64)[0].tolist() == [64] * 4               # a single segment: nothing to stop
    assert tc.stops(T, 0.0, 64)[0].tolist() == [130] * 4
    rows = torch.ones(2, 5, 4)
    assert tc.zero_behind(rows, torch.tensor([2, 5]))[..., 0].tolist() == [[1, 1, 0, 0, 0], [1, 1, 1, 1, 1]]


def _header():
    text = open(os.path.join(ROOT, "include", "neo360_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(bare, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S)
    assert m, "%s is not declared in include/neo360_hip.h" % name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_header_declares_and_ctypes_binds_the_termination_entry_points():
    text, bare = _header()
    for name in ("neo_tp_render_terminating", "neo_tp_termination_stops"):
        assert len(_lib.SIGNATURES[name][1]) == len(_params(bare, name)), name
        assert hasattr(_lib.load(), name)
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*neo_tp_term_samples\s*;", bare)
    fields = [f.split("*")[-1].strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in _lib.TpTermSamples._fields_] == ["fg_t", "fg_w", "bg_s", "stop", "fg_rows"]
    assert "STOP RULE" in text and "1.003" in text


def test_termination_calls_validate_on_the_host():
    net = models.NeRF_TP(num_coarse_samples=8, num_fine_samples=8)
    assert net.last_terminate_kept is None and net.last_terminate_survivors is None
    b = tc.rays(96)
    rows, t, d, far = torch.zeros(96, 9, 4), torch.zeros(96, 9), b["rays_d"], torch.ones(96)
    for eps in (-1e-3, 1.0, 1.5, float("nan"), float("inf"), None, "0.1", True):
        with pytest.raises(ValueError):
            net.render_terminating(b, eps)
        with pytest.raises(ValueError):
            ops.termination_stops(rows, t, d, far, eps)
    for segment in (0, -64, 32, 65, 96, 64.0, None, True):
        with pytest.raises(ValueError):
            net.render_terminating(b, 0.01, segment=segment)
        with pytest.raises(ValueError):
            ops.termination_stops(rows, t, d, far, 0.01, segment=segment)
    for args in ((rows[:, :8], t, d, far), (rows, t[0], d, far), (rows, t, d[:5], far), (rows, t, d, far[:5]),
                 (rows, t.long(), d, far), (rows[..., :3], t, d, far), (rows[:, :0], t[:, :0], d, far)):
        with pytest.raises(ValueError):
            ops.termination_stops(*args, 0.01)
    with pytest.raises(TypeError):           # eps has no default
        net.render_terminating(b)
