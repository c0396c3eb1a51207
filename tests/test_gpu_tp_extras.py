"""GPU: the NeO-360 extras (ops.tp_extras over neo_tp_extras, NeRF_TP.compute_extras over neo_tp_render_extras) against the fp64
restatement of tests/tp_extras_cases.py: every finite entry at DISTLOSS x max(1, largest finite |fp64 value| of the tensor), every
infinite entry exactly, in both families and both forms; the grid family's percentiles at knots exactly; bitwise repeatability; the
NULL outputs, R = 0, n_u = 0 and the limits of the C entry point; and the attribute on the small synthetic module: off - the
six-tuples of before; on - the same six elements bit for bit plus a dict that IS ops.tp_extras on the call's own rows."""
import pytest
import torch

import cases
import object_cases as oc
import tp_extras_cases as T
from conftest import record_parity
from neo360_amd import _lib, models, ops, render
from neo360_amd.context import get_context, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
PER_RAY = ("rays_o", "rays_d", "viewdirs", "near_obj", "far_obj")
NAMED = ("distance_percentile_5", "distance_median", "distance_percentile_95")
TWO_M22 = 2.0 ** -22


def _run(inp, form, u=T.U3):
    out = ops.tp_extras(quantiles=u, **T.kernel_kwargs(inp, form, DEV))
    assert sorted(out) == ["disparity", "distance_percentiles", "opacity"]
    return dict(opacity=out["opacity"].cpu(), disparity=out["disparity"].cpu(), pct=out["distance_percentiles"].cpu())


def _hold(cid, got, ref, family):
    """Print each figure, record it, then assert: finite entries inside the bound, infinite ones exact, knot hits of the grid exact."""
    chk = T.checks(got, ref, cid)
    print(cid, {k: "%.3g of %.3g" % (v["err"], v["bound"]) for k, v in chk.items()})
    record_parity("tp_extras/%s" % cid, **T.summarize(chk))
    T.assert_inside(chk, cid)
    if family == "grid":
        at = ref["at_knot"]
        assert torch.equal(got["pct"][at], ref["pct"][at].float()), (cid, "a percentile at a knot is not its bracket's first edge")
        assert torch.equal(got["opacity"], ref["opacity"].float()), (cid, "exact knots: the opacity is exact")


# ---- 1. the sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", T.FORMS)
@pytest.mark.parametrize("n", T.NS, ids=lambda n: "n%d" % n)
@pytest.mark.parametrize("family", T.FAMILIES)
def test_sweep_against_the_restatement(family, n, form):
    inp, ref = T.case(family, n, form)
    got = _run(inp, form)
    _hold(T.case_id(family, n, form), got, ref, family)
    if family == "random":
        assert float(got["opacity"][0]) == 0.0 and float(got["disparity"][0]) == 0.0 and bool(torch.isinf(got["pct"][0]).all())


@pytest.mark.parametrize("form", T.FORMS)
def test_eight_quantiles_with_both_ends(form):
    family, n = T.U8_CASE
    inp, ref = T.case(family, n, form, T.R_CASE, T.U8)
    got = _run(inp, form, T.U8)
    _hold(T.case_id(family, n, form, T.R_CASE, T.U8), got, ref, family)
    three = _run(inp, form, (T.U8[2], T.U8[3], T.U8[4]))        # a quantile does not depend on which others share the call
    assert torch.equal(got["pct"][:, 2:5], three["pct"])
    as_tensor = ops.tp_extras(quantiles=T.quantiles(T.U8).to(DEV), **T.kernel_kwargs(inp, form, DEV))
    assert torch.equal(as_tensor["distance_percentiles"].cpu(), got["pct"])


@pytest.mark.parametrize("family", T.FAMILIES)
def test_ray_counts_and_row_independence(family):
    for form in T.FORMS:
        for R in T.RAY_COUNTS:
            inp, ref = T.case(family, T.MID_N, form, R)
            _hold(T.case_id(family, T.MID_N, form, R), _run(inp, form), ref, family)
        for n in (65, 1024):
            inp, _ = T.case(family, n, form)
            full = _run(inp, form)
            for a, b in ((0, 1), (2, 5), (4, 9), (8, 9)):
                part = _run({k: v[a:b].contiguous() for k, v in inp.items()}, form)
                for k, v in part.items():
                    assert torch.equal(v, full[k][a:b]), (family, form, n, a, b, k)


def test_two_runs_agree_bit_for_bit():
    for family, n, form in (("random", 129, "two"), ("random", 1024, "two"), ("random", 385, "inside"), ("grid", 1024, "two")):
        inp, _ = T.case(family, n, form)
        first, second = _run(inp, form), _run(inp, form)
        for k in T.OUTPUTS:
            assert torch.equal(first[k], second[k]), (family, n, form, k)


# ---- 2. the C entry point --------------------------------------------------------------------------------------------------------
def _raw(c, kw, u, want=(True, True, True), R=None, N=None, n_u=None):
    fg_t = kw["fg_t"]
    R = fg_t.shape[0] if R is None else R
    N = fg_t.shape[1] if N is None else N
    n_u = (u.numel() if u is not None else 0) if n_u is None else n_u
    outs = [torch.full(s, -7.0, device=DEV) for s in ((max(R, 1),), (max(R, 1),), (max(R, 1), 8))]
    rc = c.lib.neo_tp_extras(c.handle, ptr(fg_t), ptr(kw["fg_w"]), ptr(kw["far"]), ptr(kw.get("bg_s")), ptr(kw.get("bg_w")),
                             ptr(kw.get("bg_lambda")), ptr(kw["rays_o"]), ptr(kw["rays_d"]), R, N, ptr(u), n_u,
                             *(ptr(o) if w else None for o, w in zip(outs, want)), c.stream())
    torch.cuda.synchronize()
    return rc, outs


def test_null_outputs_no_rays_and_no_quantiles():
    c = get_context(torch.device(DEV))
    u = T.quantiles(T.U3).to(DEV)
    for family, n, form in (("random", 65, "two"), ("grid", 129, "inside")):
        inp, ref = T.case(family, n, form)
        kw = T.kernel_kwargs(inp, form, DEV)
        rc, full = _raw(c, kw, u)
        assert rc == 0
        got = dict(opacity=full[0].cpu(), disparity=full[1].cpu(), pct=full[2].reshape(-1)[:T.R_CASE * 3].reshape(T.R_CASE, 3).cpu())
        _hold(T.case_id(family, n, form) + "_entry_point", got, ref, family)
        for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, False, False)):
            rc, part = _raw(c, kw, u, want)
            assert rc == 0
            for o, f, present in zip(part, full, want):
                assert torch.equal(o, f) if present else bool((o == -7.0).all()), (family, want)
        rc, none = _raw(c, kw, u, n_u=0)              # no quantiles: the percentile buffer is not written, the rest is the full call's
        assert rc == 0 and torch.equal(none[0], full[0]) and torch.equal(none[1], full[1]) and bool((none[2] == -7.0).all())
        rc, none = _raw(c, kw, None)                  # ... and a NULL table goes with n_u = 0
        assert rc == 0 and torch.equal(none[0], full[0]) and bool((none[2] == -7.0).all())
        rc, empty = _raw(c, {k: None for k in kw}, None, R=0, N=n)       # no rays: nothing to do, nothing read
        assert rc == 0 and all(bool((o == -7.0).all()) for o in empty)
    out = ops.tp_extras(quantiles=(), **T.kernel_kwargs(inp, form, DEV))
    assert out["distance_percentiles"].shape == (T.R_CASE, 0) and torch.equal(out["opacity"], full[0])
    zero = ops.tp_extras(**{k: v[:0] for k, v in T.kernel_kwargs(inp, form, DEV).items()})
    assert zero["opacity"].shape == (0,) and zero["distance_percentiles"].shape == (0, 3)


def test_argument_rejects():
    c = get_context(torch.device(DEV))
    inp, _ = T.case("random", 64, "two")
    kw = T.kernel_kwargs(inp, "two", DEV)
    u = torch.linspace(0, 1, 9, device=DEV)

    def refused(rc_outs):
        rc, outs = rc_outs
        assert rc < 0 and c.lib.neo_last_error(), rc
        assert all(bool((o == -7.0).all()) for o in outs)

    refused(_raw(c, kw, u[:3], N=0))
    refused(_raw(c, kw, u[:3], N=1025))
    refused(_raw(c, kw, u, n_u=9))
    refused(_raw(c, kw, u, n_u=-1))
    refused(_raw(c, kw, u[:3], R=-1))
    refused(_raw(c, kw, None, n_u=3))
    for missing in ("fg_t", "fg_w", "far", "rays_o", "rays_d"):
        refused(_raw(c, dict(kw, **{missing: None}), u[:3], R=T.R_CASE, N=64))
    for missing in ("bg_s", "bg_w", "bg_lambda"):             # only some of the three outside pointers
        refused(_raw(c, dict(kw, **{missing: None}), u[:3]))
    # the Python operator: ValueError before any launch
    with pytest.raises(ValueError, match="go together"):
        ops.tp_extras(**dict(kw, bg_lambda=None))
    with pytest.raises(ValueError, match="go together"):
        ops.tp_extras(**dict(kw, bg_s=None, bg_w=None))
    with pytest.raises(ValueError, match="at most 8"):
        ops.tp_extras(quantiles=tuple(i / 9 for i in range(9)), **kw)
    with pytest.raises(ValueError, match="at most 8"):
        ops.tp_extras(quantiles=u, **kw)
    with pytest.raises(ValueError, match="shape"):
        ops.tp_extras(**dict(kw, fg_w=kw["fg_w"][:, :63]))
    with pytest.raises(ValueError, match="shape"):
        ops.tp_extras(**dict(kw, far=kw["far"][:5]))
    with pytest.raises(ValueError, match="shape"):
        ops.tp_extras(**dict(kw, rays_d=kw["rays_d"][:, :2]))
    with pytest.raises(ValueError, match="shape"):
        ops.tp_extras(**dict(kw, bg_lambda=kw["bg_lambda"].reshape(3, 3)))
    with pytest.raises(ValueError, match="floating"):
        ops.tp_extras(**dict(kw, fg_w=kw["fg_w"].to(torch.int32)))
    with pytest.raises(ValueError, match="device"):
        ops.tp_extras(**dict(kw, bg_s=kw["bg_s"].cpu()))
    with pytest.raises(ValueError, match="device"):
        ops.tp_extras(**{k: v.cpu() for k, v in kw.items()})
    with pytest.raises(ValueError, match="1024"):
        ops.tp_extras(**{k: (torch.zeros(2, 1025, device=DEV) if v.dim() == 2 and v.shape[1] == 64 else v[:2]) for k, v in kw.items()})
    # far and lambda as (R, 1), as the module holds them
    a = ops.tp_extras(**dict(kw, far=kw["far"][:, None], bg_lambda=kw["bg_lambda"][:, None]))
    b = ops.tp_extras(**kw)
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---- 3. the module ---------------------------------------------------------------------------------------------------------------
def _net(precision=None):
    net = models.NeRF_TP(num_coarse_samples=16, num_fine_samples=32, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(oc.state())
    sc = cases.small_scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV), sc["image_wh"])
    if precision is not None:
        net.precision = precision
    return net


def _batch():
    b, _ = oc.batch(96)
    return {k: v.to(DEV) for k, v in b.items()}


def _forward(net, batch, extras, **kw):
    net.compute_extras = extras
    try:
        out = net(batch, False, False, 0.0, 0.0, out_depth=True, **kw)
        net.check_flags()
    finally:
        net.compute_extras = False
    return out


def _own_rows(net, batch, level, bg_lambda, chunk=None):
    """ops.tp_extras on the rows of the deterministic training-shaped call (the same kernels in the same order as the evaluation
    call), the call's own bg_lambda and the sphere exit."""
    rows = net._forward_train(batch, False, False, chunk, None, _raw=True)[level]
    far, _ = ops.intersect_sphere(batch["rays_o"], batch["rays_d"])
    return rows, far, ops.tp_extras(rows["fg_t"], rows["fg_w"], far, batch["rays_o"], batch["rays_d"], rows["bg_t"], rows["bg_w"], bg_lambda)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_attribute_keeps_the_six_elements_and_adds_the_dict(precision):
    net, batch = _net(precision), _batch()
    assert net.compute_extras is False
    plain = _forward(net, batch, False)
    extra = _forward(net, batch, True)
    again = _forward(net, batch, False)
    assert all(len(lv) == 6 for lv in plain) and all(len(lv) == 7 for lv in extra) and all(len(lv) == 6 for lv in again)
    for lv in range(2):
        for i in range(6):
            assert torch.equal(extra[lv][i], plain[lv][i]) and torch.equal(again[lv][i], plain[lv][i]), (lv, i)
        e = extra[lv][6]
        assert sorted(e) == sorted(("opacity", "disparity", "distance_percentiles") + NAMED)
        assert e["opacity"].shape == (96,) and e["disparity"].shape == (96,) and e["distance_percentiles"].shape == (96, 3)
        for i, k in enumerate(NAMED):
            assert torch.equal(e[k], e["distance_percentiles"][:, i])
    fine = _forward(net, batch, True, fine_only=True)
    assert fine[0] is None and len(fine[1]) == 7
    for i in range(6):
        assert torch.equal(fine[1][i], plain[1][i]), i
    for k, v in extra[1][6].items():
        assert torch.equal(fine[1][6][k], v), k
    assert _forward(net, batch, False, fine_only=True)[0] is None and len(_forward(net, batch, False, fine_only=True)[1]) == 6


def test_extras_are_the_operator_on_the_calls_own_rows():
    """... bit for bit, also with a short last chunk; then what the numbers must satisfy, and the fp64 restatement on CPU copies."""
    net, batch = _net(), _batch()
    for chunk in (None, 40):
        extra = _forward(net, batch, True, chunk=chunk)
        for lv in range(2):
            rows, far, want = _own_rows(net, batch, lv, extra[lv][4], chunk)
            e = extra[lv][6]
            for k, v in want.items():
                assert torch.equal(e[k], v), (chunk, lv, k)
            fg_acc, pct = extra[lv][3], e["distance_percentiles"]
            assert bool((e["opacity"] >= fg_acc - TWO_M22).all()) and bool((e["opacity"] <= 1.0 + 1e-5).all())
            assert bool((pct[:, 1:] >= pct[:, :-1]).all())
            assert bool((e["disparity"] >= 0).all()) and bool(torch.isfinite(e["disparity"]).all())
            # a median inside the sphere: the inside intervals that start at or before it hold at least half of the mass
            med, farv = e["distance_median"], far.reshape(-1)
            ins = med < farv
            started = (rows["fg_w"].double() * (rows["fg_t"] <= med[:, None])).sum(-1)
            assert bool((started[ins] >= 0.5 - 1e-6).all())
            assert bool((rows["fg_w"].double().sum(-1)[(med > farv) & torch.isfinite(med)] <= 0.5 + 1e-6).all())
            inp = dict(rays_o=batch["rays_o"], rays_d=batch["rays_d"], far=farv, fg_t=rows["fg_t"], fg_w=rows["fg_w"], bg_s=rows["bg_t"],
                       bg_w=rows["bg_w"], lam=extra[lv][4].reshape(-1))
            ref = T.evaluate({k: v.cpu() for k, v in inp.items()}, "two", T.U3)
            got = dict(opacity=e["opacity"].cpu(), disparity=e["disparity"].cpu(), pct=pct.cpu())
            chk = T.checks(got, ref, "module")
            print("module chunk=%s level=%d" % (chunk, lv), {k: "%.3g of %.3g" % (v["err"], v["bound"]) for k, v in chk.items()})
            record_parity("tp_extras/module_chunk%s_level%d" % (chunk, lv), **T.summarize(chk))
            T.assert_inside(chk, ("module", chunk, lv))
    # the rays do not all tell the same story (the total opacity does: the last outside step of 1e10 is opaque wherever sigma > 0)
    assert int(ins.sum()) > 0 and float(med.std()) > 0


def test_chunk_loop_with_overlap_on():
    """Three calls of 32 rays in flight on alternating lanes: each returns the dict of the same call made alone, which is the operator
    on that call's own rows."""
    net, batch = _net(), _batch()
    assert net.overlap_calls
    parts = [{k: (v[32 * i:32 * (i + 1)] if k in PER_RAY else v) for k, v in batch.items()} for i in range(3)]
    net.compute_extras = True
    try:
        outs = [net(p, False, False, 0.0, 0.0, out_depth=True) for p in parts]
        net.check_flags()
        net.overlap_calls = False
        for i, p in enumerate(parts):
            alone = net(p, False, False, 0.0, 0.0, out_depth=True)
            net.check_flags()
            for lv in range(2):
                for j in range(6):
                    assert torch.equal(outs[i][lv][j], alone[lv][j]), (i, lv, j)
                _, _, want = _own_rows(net, p, lv, alone[lv][4])
                for k, v in want.items():
                    assert torch.equal(outs[i][lv][6][k], v) and torch.equal(alone[lv][6][k], v), (i, lv, k)
    finally:
        net.compute_extras = False
        net.overlap_calls = True


def test_other_quantiles_culling_and_the_frame():
    net, batch = _net(), _batch()
    plain = _forward(net, batch, False)
    net.extras_quantiles = (0.25, 0.75)
    try:
        two = _forward(net, batch, True)
    finally:
        del net.extras_quantiles
    assert net.extras_quantiles == (0.05, 0.5, 0.95)
    assert sorted(two[1][6]) == ["disparity", "distance_percentiles", "opacity"] and two[1][6]["distance_percentiles"].shape == (96, 2)
    net.extras_quantiles = tuple(i / 9 for i in range(9))
    try:
        with pytest.raises(ValueError, match="at most 8"):
            _forward(net, batch, True)
    finally:
        del net.extras_quantiles
    net.cull_background = 0.5
    try:
        with pytest.raises(ValueError, match="cull_background"):
            _forward(net, batch, True)
        culled = _forward(net, batch, False)             # culling alone is what it was
        assert all(len(lv) == 6 for lv in culled)
    finally:
        net.cull_background = None
    # the frame API: new keys beside unchanged old ones
    frame0 = render.render_rays_test(net, batch, chunk=96)
    net.compute_extras = True
    try:
        frame1 = render.render_rays_test(net, batch, chunk=96)
        tile = render.render_frame_sharded(net, batch, 1, 0, chunk=96)
    finally:
        net.compute_extras = False
    assert sorted(frame0) == ["acc", "bg_rgb", "depth", "fg_rgb", "rgb"]
    assert sorted(frame1) == sorted(list(frame0) + ["opacity", "disparity"] + list(NAMED))
    for k, v in frame0.items():
        assert torch.equal(frame1[k], v), k
    assert torch.equal(frame1["rgb"], plain[1][0]) and torch.equal(frame1["acc"], plain[1][3])
    extra = _forward(net, batch, True)
    for k in ("opacity", "disparity") + NAMED:
        assert torch.equal(frame1[k], extra[1][6][k]), k
    assert tile.shape == (96, 5) and torch.equal(tile[:, 3], frame0["depth"]) and torch.equal(tile[:, 4], frame0["acc"])


def test_inside_only_form_on_object_rows():
    """render_objects(return_samples=True) exposes the level-1 sample rows of the hit rays; their weights are rebuilt with the public
    stage operators (bitwise the compact launches: tests/test_gpu_objects.py).  The inside-only histogram ending at far_obj sums to
    that call's acc, and its percentiles lie inside the object interval or at +inf."""
    net, batch = _net(), _batch()
    res = net.render_objects(batch, return_samples=True)
    net.check_flags()
    _, mask = oc.batch(96)
    hit = mask.to(DEV)
    far = torch.where(hit, batch["far_obj"].reshape(-1), torch.full((96,), 0.5, device=DEV))
    t1 = torch.where(hit[:, None], res[2][1], torch.linspace(0.1, 0.5, 49, device=DEV).expand(96, -1)).contiguous()
    c1 = ops.composite(1, net.eval_mlp(1, batch, t1), t1, batch["rays_d"], t_far=far, white_bkgd=True)
    assert torch.equal(c1["acc"][hit], res[1][1][hit])
    e = ops.tp_extras(t1, c1["weights"], far, batch["rays_o"], batch["rays_d"])
    assert float((e["opacity"][hit] - res[1][1][hit]).abs().max()) <= TWO_M22
    pct = e["distance_percentiles"][hit]
    lo = torch.clamp(batch["near_obj"].reshape(-1)[hit], min=1e-4)[:, None]
    fin = torch.isfinite(pct)
    assert bool(((pct >= lo) & (pct <= far[hit][:, None]))[fin].all()) and bool(torch.isinf(pct[~fin]).all())
    assert torch.equal(fin, torch.tensor(T.U3, device=DEV)[None, :].double() < c1["weights"][hit].double().sum(-1, keepdim=True))
