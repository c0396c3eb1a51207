"""GPU: power-of-two rescalings through the NeO-360 decoder (NeRF_TP.eval_mlp, every pre-projection mode), the PixelNeRF decoder
and the scene encoder's pillar stage - the low end of the split-fp16 arithmetic on the project's main path.  Exact kernels: bitwise
the unscaled output.  Split kernels: inside the per-entry bound against fp64 (and at most half of it) or flagged, never silently
outside; whether a state is flagged is what split_scale_cases.below_low says; a flag on a static operand is raised again by a second
call on the same module; flagged models render whole frames on the exact kernels.  States, references and bounds:
tests/split_scale_cases.py (checked on the CPU by tests/test_split_scale_cases_cpu.py); one record per (family, variant, kind,
shift) goes to the parity report under split_scale_sweep/.  One module per (family, variant), reloaded with every state."""
import warnings

import pytest
import torch

import alongray_cases as A
import split_scale_cases as S
import view_map_cases as V
from conftest import record_parity
from neo360_amd import _lib, encoder, models, render

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NETS, _SCENE_OF, _BATCH, _RECORDED = {}, {}, {}, {}

PIX_IDS = {True: "pre", False: "noproj"}
PIX_EXACT, PIX_SPLIT = [("f32", q) for q in S.PIX_VARIANTS], [("f16x3", q) for q in S.PIX_VARIANTS]
# (family, variant) of every kernel in the sweep
EXACT = ([("neo360", v) for v in S.NEO_EXACT_VARIANTS] + [("pixelnerf", v) for v in PIX_EXACT] + [("pillar", "f32")])
SPLIT = ([("neo360", v) for v in S.NEO_SPLIT_VARIANTS] + [("pixelnerf", v) for v in PIX_SPLIT] + [("pillar", "f16x3")])


def _variant_id(family, variant):
    return variant if family != "pixelnerf" else "%s-%s" % (variant[0], PIX_IDS[variant[1]])


def _label(family, variant, kind, shift):
    return "split_scale_sweep/%s/%s/%s/s%d" % (family, _variant_id(family, variant), kind, shift)


def _dev(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _point_batch(case):
    if case not in _BATCH:
        c = V.point_case(*case)
        _BATCH[case] = (_dev(c["batch"]), c["far"].to(DEV), c["t_in"].to(DEV), c["s_out"].to(DEV), c["chunk"])
    return _BATCH[case]


def _net(family, variant):
    """The one module of (family, variant); a GridEncoder raises its range errors."""
    key = (family, variant)
    if key not in _NETS:
        if family == "neo360":
            net = models.NeRF_TP(num_coarse_samples=16, num_fine_samples=24).to(DEV)
            net.precision = variant.split("-")[0]
        elif family == "pixelnerf":
            net = models.PixelNeRF().to(DEV)
            net.precision, net.preproject = variant
        else:
            net = encoder.GridEncoder(grid_size=(1, 1, 1)).to(DEV)
            net.precision, net.on_range = variant, "raise"
        _NETS[key] = net
    return _NETS[key]


def _load(family, variant, state, scene_key):
    """State (and, for the decoders, scene) into the module; the scene is uploaded again only when it is another one."""
    net = _net(family, variant)
    net.load_state_dict(state[0], strict=family != "pillar")
    if family != "pillar" and _SCENE_OF.get((family, variant)) != scene_key:
        sc = state[1]
        if family == "neo360":
            net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV), sc["image_wh"],
                          preproject={"pp1": True, "pp2": 2, "noproj": False}.get(variant.split("-")[-1], 3))
        else:
            net.set_scene(sc["latent"].to(DEV), sc["image_wh"])
        _SCENE_OF[(family, variant)] = scene_key
    return net


def _run(family, variant, case, state, scene_key):
    """{output name: tensor tuple entry or the NeoRangeError it raised}: neo360 -> inside, outside; pixelnerf -> out; pillar ->
    plans (the three floor-plans as one entry)."""
    net = _load(family, variant, state, scene_key)
    calls = {}
    if family == "pillar":
        c = V.pillar_case(case)
        net.grid_size = [int(g) for g in c["grid"]]
        calls["plans"] = lambda: tuple(t.cpu() for t in net.floorplans(state[1].to(DEV), c["poses"].to(DEV), c["focal"].to(DEV),
                                                                       c["centre"].to(DEV), c["image_wh"]))
    else:
        gb, far, t_in, s_out, chunk = _point_batch(case)
        if family == "neo360":
            calls["inside"] = lambda: net.eval_mlp(V.FG_SLOT, gb, t_in, far=far, chunk=chunk).cpu()
            calls["outside"] = lambda: net.eval_mlp(V.BG_SLOT, gb, s_out, far=far, chunk=chunk).cpu()
        else:
            calls["out"] = lambda: net.eval_mlp(V.PIX_SLOT, gb, t_in, chunk=chunk).cpu()
    out = {}
    for name, call in calls.items():
        try:
            out[name] = call()
        except _lib.NeoRangeError as err:
            out[name] = err
    return out


def _scene_key(case, kind, shift):
    return (case, shift if kind == "F" else 0)


def _checks_of(family, case, name, got):
    """{quantity: worst_entry} of one output of `_run`."""
    if family == "pillar":
        return S.checks(family, case, got)[0]
    ref64, ref32 = S.reference(family, case), S.reference(family, case, torch.float32)
    i = {"inside": 0, "outside": 1, "out": 0}[name]
    return V.eval_checks(got, ref64[i], ref32[i])


def _merge(worst, checks):
    for k, v in checks.items():
        if k not in worst or v["ratio"] > worst[k]["ratio"]:
            worst[k] = v


def _record(label, worst, **extra):
    rec = A.summarize(worst) if worst else {}
    rec.update(extra)
    record_parity(label, **rec)
    _RECORDED[label] = rec


def sweep_state(family, variant, kind, shift):
    """One (family, split variant, kind, shift) on every case: -> [(case, output name, raised error or None, checks or None,
    expected to raise)], and the largest |operand| of the state.  No assertion (also used to measure a library's curve)."""
    rows, operand = [], 0.0
    for case in S.cases(family):
        state = S.make_state(family, kind, shift, case)
        operand = max(operand, S.largest_operand(state[2]))
        for name, got in _run(family, variant, case, state, _scene_key(case, kind, shift)).items():
            slot = name if family == "neo360" else None
            expect = S.below_low(family, state, variant[1] if family == "pixelnerf" else variant, slot)
            if isinstance(got, Exception):
                rows.append((case, name, got, None, expect))
            else:
                rows.append((case, name, None, _checks_of(family, case, name, got), expect))
    return rows, operand


def _healthy(family, variant, label):
    worst = {}
    for case in S.cases(family):
        for name, got in _run(family, variant, case, S.base_state(family, case), _scene_key(case, "", 0)).items():
            assert not isinstance(got, Exception), (label, "the base state raised after a flagged one", str(got))
            _merge(worst, _checks_of(family, case, name, got))
    A.assert_inside(worst, label + "/healthy-after")
    return worst


# ---- exact kernels --------------------------------------------------------------------------------------------------------------------
_EXACT_STATES = [(f, v, k, s) for f, v in EXACT for k in S.KINDS[f] for s in (S.MIDDLE_SHIFT, S.shifts(f, k)[-1])]
_SPLIT_STATES = [(f, v, k, s) for f, v in SPLIT for k, s in S.states(f)]


def _ids(states):
    return ["%s-%s-%s-s%d" % (f, _variant_id(f, v), k, s) for f, v, k, s in states]


@pytest.mark.parametrize("family,variant,kind,shift", _EXACT_STATES, ids=_ids(_EXACT_STATES))
def test_exact_kernels_bitwise_under_rescaling(family, variant, kind, shift):
    """k_tp_mlp (raw, latent pre-projected, no projection), k_pix_mlp and the fp32 pillar stage: a power of two only moves the
    exponent of every product and partial sum, so the output is the same bits for the scaled and the unscaled state - no tolerance."""
    label = _label(family, variant, kind, shift)
    worst, differ = {}, []
    for case in S.cases(family):
        base = _run(family, variant, case, S.base_state(family, case), _scene_key(case, "", 0))
        state = S.make_state(family, kind, shift, case)
        got = _run(family, variant, case, state, _scene_key(case, kind, shift))
        for name in base:
            assert not isinstance(base[name], Exception) and not isinstance(got[name], Exception), (label, case, name)
            _merge(worst, _checks_of(family, case, name, base[name]))
            pairs = zip(got[name], base[name]) if family == "pillar" else [(got[name], base[name])]
            for g, b in pairs:
                if not torch.equal(g, b):
                    differ.append((case, name, float((g - b).abs().max())))
    _record(label, worst, bitwise_equal=float(not differ))
    A.assert_inside(worst, label + "/base")
    assert not differ, (label, differ)


# ---- split kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,variant,kind,shift", _SPLIT_STATES, ids=_ids(_SPLIT_STATES))
def test_split_kernels_inside_the_bound_or_flagged(family, variant, kind, shift):
    """Every evaluation of every state either raises NeoRangeError or is inside its per-entry bound against fp64; an unflagged one
    uses at most half of the bound; which of the two happens is split_scale_cases.below_low; a raise on a weight or an uploaded map
    says static_operand, one on the pillar stage's latent does not; after a raise the same module evaluates the base state inside
    the bound."""
    label = _label(family, variant, kind, shift)
    rows, operand = sweep_state(family, variant, kind, shift)
    worst, flagged, static, problems = {}, 0, [], []
    for case, name, err, checks, expect in rows:
        where = (S.case_id(family, case), name)
        if err is not None:
            flagged += 1
            static.append(bool(err.static_operand))
            if not expect:
                problems.append(where + ("flagged, but the low-end rule does not cover this state",))
            if err.static_operand is not S.static_trip(family, kind):
                problems.append(where + ("static_operand is %r" % err.static_operand,))
            if "fp32 accuracy" not in str(err):
                problems.append(where + ("message: " + str(err),))
            continue
        _merge(worst, checks)
        print(label, where, {k: "%.2e of %.2e (fp32 oracle %.2e)" % (v["err"], v["bound"], v["fp32"]) for k, v in checks.items()})
        share = max(v["ratio"] for v in checks.values())
        if share > 1.0:
            problems.append(where + ("SILENTLY outside the bound: %.3g of it" % share, A.summarize(checks)))
        elif expect:
            problems.append(where + ("expected the range guard to trip",))
        elif share > S.HALF:
            problems.append(where + ("an unflagged state may use half of its bound: %.3g" % share,))
    extra = dict(evaluations=float(len(rows)), flagged=float(flagged), largest_operand=float("%.3g" % operand))
    if static:
        extra["static_operand"] = float(all(static))
    _record(label, worst, **extra)
    if flagged:
        _healthy(family, variant, label)                     # the flag word was cleared by the raise
    assert not problems, (label, problems)


# ---- every uploaded layer is looked at --------------------------------------------------------------------------------------------------
MLP_LAYERS = ("pts_linears.0", "pts_linears.1", "pts_linears.2", "pts_linears.3", "views_linear.0", "views_linear.1", "bottleneck_layer",
              "density_layer", "rgb_layer")
LAYER_PROBES = {"neo360": ("f16x3-noproj", V.BG_PREFIX, MLP_LAYERS, ()),                  # the last slot (3), raw kernel: nothing folded
                "pixelnerf": (("f16x3", False), V.PIX_PREFIX, MLP_LAYERS, S.PIX_FOLDED),
                "pillar": ("f16x3", "", S.PILLAR_LAYERS, ())}


@pytest.mark.parametrize("family", list(LAYER_PROBES))
def test_every_uploaded_layer_is_held_to_the_low_end(family):
    """One of the nine uploaded layers at a time x 2^-16, nothing compensated (only the flag is looked at): every layer raises as
    a static operand - the 128- and 192-element heads included, which are shorter than one block of the reduction - except a
    bottleneck that the fragment set folds away."""
    variant, prefix, layers, folded = LAYER_PROBES[family]
    case = S.cases(family)[0]
    base = S.base_state(family, case)
    wrong = []
    for layer in layers:
        sd = dict(base[0])
        sd[prefix + layer + ".weight"] = sd[prefix + layer + ".weight"] * 2.0 ** -16
        got = _run(family, variant, case, (sd, base[1]), _scene_key(case, "", 0))
        name = "outside" if family == "neo360" else next(iter(got))
        raised = isinstance(got[name], Exception)
        if raised != (layer not in folded) or (raised and got[name].static_operand is not True):
            wrong.append((layer, raised))
    _healthy(family, variant, "layers/" + family)
    assert not wrong, (family, wrong)


# ---- a static trip is raised again ------------------------------------------------------------------------------------------------------
def _frame_batch(s):
    return _dev(V.render_batch(s))


STICKY = [("neo360", "f16x3", "T1"), ("neo360", "f16x3-noproj", "F"), ("pixelnerf", ("f16x3", False), "T1")]


@pytest.mark.parametrize("poll", ["immediate", "deferred"])
@pytest.mark.parametrize("family,variant,kind", STICKY, ids=["%s-%s-%s" % (f, _variant_id(f, v), k) for f, v, k in STICKY])
def test_a_static_trip_is_raised_again(family, variant, kind, poll):
    """A flagged state evaluated twice on the same module, nothing loaded in between: both calls raise (the one-time checks of
    static operands are armed again when the host takes the flag).  'immediate': eval_mlp, which reads the word itself;
    'deferred': the whole forward, whose flag is posted behind the call and taken by check_flags().  Then the base state is
    healthy on the same module."""
    shift = S.shifts(family, kind)[-1]
    case = S.POINT_CASES[0]
    state = S.make_state(family, kind, shift, case)
    slot = "inside" if family == "neo360" else None
    assert S.below_low(family, state, variant[1] if family == "pixelnerf" else variant, slot)
    net = _load(family, variant, state, _scene_key(case, kind, shift))
    gb, far, t_in, s_out, chunk = _point_batch(case)
    prev = net.poll_flags
    net.poll_flags = poll
    try:
        for attempt in (1, 2):
            with pytest.raises(_lib.NeoRangeError, match="fp32 accuracy") as exc:
                if poll == "immediate":
                    if family == "neo360":
                        net.eval_mlp(V.FG_SLOT, gb, t_in, far=far, chunk=chunk)
                    else:
                        net.eval_mlp(V.PIX_SLOT, gb, t_in, chunk=chunk)
                else:
                    if family == "neo360":
                        net(gb, False, False, 0.0, 0.0, out_depth=True)
                    else:
                        net(gb, False, False, 0.2, 3.0)
                    net.check_flags()
            assert exc.value.static_operand is True, attempt
    finally:
        net.poll_flags = prev
    _healthy(family, variant, "sticky/%s/%s/%s/%s" % (family, _variant_id(family, variant), kind, poll))


# ---- the frame path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["T1", "F"])
def test_neo360_frame_in_a_flagged_state_is_rendered_in_f32(kind):
    """Mirrors test_mip_frame_with_small_weights_is_rendered_in_f32: a NeRF_TP in a flagged T1 state / on a flagged F scene goes
    through render.render_rays_test twice (48 rays, 16 + 24 samples): one warning, both frames bitwise what precision 'f32'
    returns, and the module latched."""
    s = S.POINT_CASES[0][0]
    shift = S.shifts("neo360", kind)[-1]
    sd, sc, _ = S.neo_state(kind, shift, s, prefixes=S.NEO_ALL_PREFIXES)
    assert S.below_low("neo360", (sd, sc), "f16x3", "inside")
    batch = _frame_batch(s)

    def build(precision):
        net = models.NeRF_TP(num_coarse_samples=V.RENDER_SAMPLES[0], num_fine_samples=V.RENDER_SAMPLES[1], num_src_views=V.SCENES[s][0]).to(DEV)
        net.precision = precision
        net.load_state_dict(sd)
        net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV), sc["image_wh"])
        return net
    net = build(None)
    assert batch["rays_o"].shape[0] == V.RENDER_RAYS
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        first = render.render_rays_test(net, batch)
        second = render.render_rays_test(net, batch)
    assert len([w for w in seen if "fp16 range" in str(w.message)]) == 1, [str(w.message) for w in seen]
    assert first["precision_used"] == "f32" and second["precision_used"] == "f32"
    assert net._range_latch == net.operands_key()
    exact = build("f32")
    want = render.render_rays_test(exact, batch)
    for k in ("rgb", "depth"):
        assert torch.equal(first[k], want[k]) and torch.equal(second[k], want[k]), k
    assert bool(torch.isfinite(first["rgb"]).all())
    net.close()
    exact.close()


@pytest.mark.parametrize("kind", ["P0", "L"])
def test_grid_encoder_retries_a_flagged_state_in_f32(kind):
    """GridEncoder with the default retry on a flagged state: the floor-plans are bitwise the 'f32' run's; a weight kind latches
    the module, the latent (this call's input) does not."""
    i = S.PILLAR_CASES[0]
    c = V.pillar_case(i)
    params, lat, _ = S.pillar_state(kind, S.shifts("pillar", kind)[-1], i)
    assert S.below_low("pillar", (params, lat))
    args = (c["poses"].to(DEV), c["focal"].to(DEV), c["centre"].to(DEV), c["image_wh"])

    def build(precision):
        enc = encoder.GridEncoder(grid_size=c["grid"]).to(DEV)
        enc.precision = precision
        enc.load_state_dict(params, strict=False)
        return enc
    enc, exact = build(None), build("f32")
    want = exact.floorplans(lat.to(DEV), *args)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        first = enc.floorplans(lat.to(DEV), *args)
        second = enc.floorplans(lat.to(DEV), *args)
    assert len([w for w in seen if issubclass(w.category, RuntimeWarning)]) == 1, [str(w.message) for w in seen]
    assert enc.last_precision_used == "f32"
    for a, b, w in zip(first, second, want):
        assert torch.equal(a, w) and torch.equal(b, w)
    if kind == "L":
        assert enc._range_latch is None
    else:
        assert enc._range_latch == enc.operands_key()
    enc.close()
    exact.close()


# ---- every state was compared -----------------------------------------------------------------------------------------------------------
def test_every_state_was_compared():
    """One record per (family, variant, kind, shift): every split state and the two shifts of every exact kernel."""
    want = {_label(*t) for t in _EXACT_STATES + _SPLIT_STATES}
    assert set(_RECORDED) == want and len(want) == len(_EXACT_STATES) + len(_SPLIT_STATES)
    flagged = [k for k, r in _RECORDED.items() if r.get("flagged")]
    assert flagged and all("static_operand" in _RECORDED[k] for k in flagged)
    for net in _NETS.values():
        net.close()
    _NETS.clear()
    _SCENE_OF.clear()
