"""CPU: the conditions of tests/split_scale_cases.py, on the very states tests/test_gpu_split_scale_sweep.py hands to the kernels.
Every state leaves the fp32 oracle bit for bit where it was, holds nothing subnormal and nothing at or beyond 65504 - neither a
weight nor an activation -, so it can only trip the LOW end of the split arithmetic; the base states' fp32 oracle uses at most a
third of every bound; and `below_low` agrees with a restatement of the library's rule from the base maxima."""
import pytest
import torch

import alongray_cases as A
import split_scale_cases as S
import view_map_cases as V

FAMILIES = tuple(S.KINDS)
ALL_STATES = [(f, k, s) for f in FAMILIES for k, s in S.states(f)]
_IDS = ["%s-%s-%d" % t for t in ALL_STATES]


def test_point_cases_are_in_the_view_map_table():
    """Their references are the cached ones of view_map_cases (and have its conditions checked by test_view_map_cases_cpu.py)."""
    for case in S.POINT_CASES:
        assert case in V.CASES
    assert V.SCENES[7] == (3, (3, 5), (5, 7)) and V.SHAPES[63] == (9, 7, 4)          # chunk 4 does not divide 9 rays
    assert V.SCENES[2][0] == 4 and V.SHAPES[203] == (7, 29, 7) and 203 == 6 * 32 + 11
    assert V.PILLAR[1] == (1, (5, 7), (3, 7, 3)) and V.PILLAR[3] == (5, (5, 7), (13, 1, 1))


@pytest.mark.parametrize("family", FAMILIES)
def test_fp32_oracle_of_the_base_state_uses_a_third_of_every_bound(family):
    for case in S.cases(family):
        got32 = S.reference(family, case, torch.float32)
        for chk in S.checks(family, case, got32):
            for name, v in chk.items():
                assert v["ratio"] <= S.ORACLE_SHARE, (family, case, name, v)


@pytest.mark.parametrize("family,kind,shift", ALL_STATES, ids=_IDS)
def test_state_is_the_same_network_and_stays_inside_the_range(family, kind, shift):
    for case in S.cases(family):
        state = S.make_state(family, kind, shift, case)
        touched = state[2]
        with S.linear_maxima() as seen:
            got = S.evaluate(family, case, state, torch.float32)
        base = S.reference(family, case, torch.float32)
        for g, b in zip(got, base):
            assert torch.equal(g, b), (family, kind, shift, case, float((g - b).abs().max()))
        for name, t in touched.items():
            nz = t[t != 0].abs()
            assert float(nz.min()) >= S.FP32_MIN_NORMAL, (name, float(nz.min()))           # nothing subnormal
            assert float(nz.max()) < S.FP16_MAX, (name, float(nz.max()))                   # no weight, bias or map beyond fp16
        assert seen and max(max(x, y) for x, y in seen) < S.FP16_MAX, (family, kind, shift, max(max(x, y) for x, y in seen))
        assert min(float(t.abs().max()) for t in touched.values()) < 4.0 * 2.0 ** -shift  # something really shrank (base maxima are under 4)


@pytest.mark.parametrize("family", FAMILIES)
def test_last_shift_is_the_largest_that_stays_inside_the_range(family):
    """LAST_SHIFT: 18 unless the compensated operand leaves the fp16 range there; then the largest shift below it that does not."""
    for kind in S.KINDS[family]:
        last = S.shifts(family, kind)[-1]
        case = S.cases(family)[0]
        largest = lambda s: max(float(t.abs().max()) for t in S.make_state(family, kind, s, case)[2].values())
        assert largest(last) < S.FP16_MAX
        assert last == 18 or largest(last + 1) >= S.FP16_MAX, (family, kind, last)
        assert S.shifts(family, kind)[:-1] == tuple(s for s in (4, 6, 8, 10, 12, 14) if s < last)


def _maxima(sd, prefix=""):
    return {k[len(prefix):-len(".weight")]: float(v.abs().max()) for k, v in sd.items() if k.startswith(prefix) and k.endswith(".weight")}


DOWN_LAYER = {"T0": "pts_linears.0", "T1": "pts_linears.1", "T2": "pts_linears.2", "V0": "views_linear.0", "B": "bottleneck_layer",
              "P0": "depth_fc.common_branch.0", "P1": "depth_fc.common_branch.2", "A": "pillar_aggregator_xz.0"}


def _restated(family, kind, shift, case, variant=None, slot=None):
    """The rule of csrc/kernels.h and the launch sites, from the BASE maxima and the constants written out: the scaled layer's
    largest |w| x 2^-shift under 2^-11 (NeO-360) / 2^-9 (PixelNeRF) / 2^-6 (pillar stage) - unless the launched fragment set folds
    that layer in fp64 -, or a raw-split map's largest |x| x 2^-shift under 2^-8 (decoders) / 2^-6 (the pillar stage's latent)."""
    f = 2.0 ** -shift
    if family == "pillar":
        c = V.pillar_case(case)
        if kind == "L":
            return float(c["latent"].abs().max()) * f < 2.0 ** -6
        return _maxima(c["params"])[DOWN_LAYER[kind]] * f < 2.0 ** -6
    sc = V.scene_of(case[0])
    planes, latent = max(float(sc[m].abs().max()) for m in S.MAPS[:3]), float(sc["latent"].abs().max())
    if family == "pixelnerf":
        if kind == "F":
            return (not variant) and latent * f < 2.0 ** -8
        return kind != "B" and _maxima(S.pix_base_state(), V.PIX_PREFIX)[DOWN_LAYER[kind]] * f < 2.0 ** -9
    if kind == "F":
        raw_planes = variant in ("f16x3-pp1", "f16x3-noproj") or (variant == "f16x3" and slot == "inside")
        return (raw_planes and planes * f < 2.0 ** -8) or (variant == "f16x3-noproj" and latent * f < 2.0 ** -8)
    if kind == "B" and variant != "f16x3-noproj":
        return False
    return _maxima(S.neo_base_state(), S.NEO_SLOTS[slot][1])[DOWN_LAYER[kind]] * f < 2.0 ** -11


@pytest.mark.parametrize("family,kind,shift", ALL_STATES, ids=_IDS)
def test_below_low_is_the_rule_of_the_library(family, kind, shift):
    for case in S.cases(family):
        state = S.make_state(family, kind, shift, case)
        if family == "pillar":
            combos = [(None, None)]
        elif family == "pixelnerf":
            combos = [(v, None) for v in S.PIX_VARIANTS]
        else:
            combos = [(v, sl) for v in S.NEO_SPLIT_VARIANTS for sl in S.NEO_SLOTS]
        for variant, slot in combos:
            assert S.below_low(family, state, variant, slot) == _restated(family, kind, shift, case, variant, slot), (case, variant, slot)
        assert not S.below_low(family, S.base_state(family, case), *combos[0])              # no unscaled state is flagged


def test_the_table_reaches_both_sides_of_the_rule():
    """Every kind has unflagged and flagged states on at least one variant, so the sweep sees the curve on both sides of LOW
    (PixelNeRF's kind B has none: both of its split kernels fold the bottleneck in fp64, test_below_low_is_the_rule_of_the_library)."""
    for family in FAMILIES:
        for kind in S.KINDS[family]:
            if (family, kind) == ("pixelnerf", "B"):
                continue
            variant, slot = {"neo360": ("f16x3-noproj", "inside"), "pixelnerf": (False, None), "pillar": (None, None)}[family]
            case = S.cases(family)[0]
            flags = [S.below_low(family, S.make_state(family, kind, s, case), variant, slot) for s in S.shifts(family, kind)]
            assert flags[0] is False and flags[-1] is True and flags == sorted(flags), (family, kind, flags)
    assert S.static_trip("pillar", "L") is False and S.static_trip("pillar", "P0") and S.static_trip("neo360", "F")
    assert A.scale_of(torch.zeros(1)) == 1.0
