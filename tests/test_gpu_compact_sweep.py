"""GPU: hit patterns and hit counts swept through the compact evaluator launches - NeRF_TP.render_objects, NeRF_TP.render_instances
and NeRF_TP.forward with cull_background - case by case of tests/compact_cases.py (its conditions are checked on the CPU by
tests/test_compact_cases_cpu.py; docs/compact_sweep.md has the table and the result).  In all three the row count exists only in a
device word: the two-launch compaction of compact.h writes it, and every kernel downstream reads its extent from it while its grid
is sized for all R rays.

Per case: the count and the missed rays exactly; the level-0 rows against fp64; every hit ray bitwise the NON-compact evaluators
(rebuilt on all R rays from the public stage operators - the evaluators the earlier sweeps hold to fp64 per entry); every hit ray
against the CPU oracle in float64 at the GPU's own level-1 positions; a hit ray's result independent of the pattern, of the calls
before it on the same module, and of the caller's chunk loop.  Every case lands in the parity report under compact_sweep/..."""
import time

import pytest
import torch

import cases
import compact_cases as C
import instance_cases as ic
import object_cases as oc
from conftest import record_parity
from neo360_amd import models, ops, synth
from test_gpu_cull_background import EVALUATORS as CULL_EVALUATORS
from test_gpu_cull_background import NAMES as CULL_NAMES
from test_gpu_cull_background import _assert_contract
from test_gpu_objects import EVALUATORS

pytestmark = pytest.mark.gpu
DEV = "cuda"
PER_RAY = ("rays_o", "rays_d", "viewdirs")
OUT = C.OUT
IDS = ["%s-pre%d-%s" % (p, int(m), k) for p, m, k in EVALUATORS]


def _net(precision=None, preproject=3, n_coarse=C.N_COARSE, n_fine=C.N_FINE, state=None):
    net = models.NeRF_TP(num_coarse_samples=n_coarse, num_fine_samples=n_fine, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(state if state is not None else oc.state())
    sc = cases.small_scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV),
                  sc["image_wh"], preproject=preproject)
    if precision is not None:
        net.precision = precision
    return net


_GB = {}


def _gb(R):
    if R not in _GB:
        _GB[R] = {k: v.to(DEV) for k, v in C.rays(R).items()}
    return _GB[R]


def _objects(net, gb, near, far, white=True, chunk=None):
    """render_objects with its sample rows, cloned: [[rgb, acc, depth] x 2, [t0, t1]], and the hit count."""
    out = net.render_objects(gb, near_obj=near, far_obj=far, white_bkgd=white, chunk=chunk, return_samples=True)
    net.check_flags()
    return [[t.clone() for t in lv] for lv in out], int(net.last_object_hits)


def _same(a, b, rows=None):
    """Bitwise equality of two render_objects results (on `rows` only, if given)."""
    for lv in range(3):
        for x, y in zip(a[lv], b[lv]):
            if not torch.equal(x if rows is None else x[rows], y if rows is None else y[rows]):
                return False
    return True


def _assert_misses(res, miss, white):
    for lv in range(2):
        rgb, acc, depth = res[lv]
        assert bool((rgb[miss] == (1.0 if white else 0.0)).all()), lv
        assert bool((acc[miss] == 0.0).all()) and bool((depth[miss] == 0.0).all()), lv
        assert bool((res[2][lv][miss] == 0.0).all()), lv


def _rebuild(net, gb, res, hit, far_obj, n_coarse, n_fine, white=True, chunk=None):
    """Every ray on the NON-compact evaluators, from the public stage operators: the exposed t0 -> eval_mlp (slot 0) ->
    ops.composite (mode 1, t_far = far_obj) -> ops.resample -> eval_mlp (slot 1) -> composite.  Missed rays are marched through a
    dummy interval and are to be ignored.  (test_gpu_objects.test_compact_launches_are_bitwise_the_non_compact_evaluators)"""
    R = hit.shape[0]
    far = torch.where(hit, far_obj, torch.full_like(far_obj, 0.5))
    dummy = torch.linspace(0.1, 0.5, n_coarse + 1, device=DEV).expand(R, -1)
    t0 = torch.where(hit[:, None], res[2][0], dummy).contiguous()
    c0 = ops.composite(1, net.eval_mlp(0, gb, t0, chunk=chunk), t0, gb["rays_d"], t_far=far, white_bkgd=white)
    t1 = ops.resample(t0, c0["weights"], n_fine)
    c1 = ops.composite(1, net.eval_mlp(1, gb, t1, chunk=chunk), t1, gb["rays_d"], t_far=far, white_bkgd=white)
    return t1, c0, c1


def _assert_rebuild(net, gb, res, hit, far_obj, n_coarse, n_fine, label, white=True, chunk=None):
    t1, c0, c1 = _rebuild(net, gb, res, hit, far_obj, n_coarse, n_fine, white, chunk)
    assert torch.equal(t1[hit], res[2][1][hit]), (label, "level-1 rows")
    for lv, c in enumerate((c0, c1)):
        for k, got in zip(OUT, res[lv]):
            assert torch.equal(got[hit], c[k][hit]), (label, lv, k)


def _level0_ok(res, near, far, mask, label, n_coarse=C.N_COARSE):
    """Truth 2; only after it may a row be fed onward."""
    if not bool(mask.any()):
        return {}
    checks, order = C.level0_checks(res[2][0], near, far, mask, n_coarse)
    assert all(order.values()), (label, order)
    C.assert_inside(checks, label)
    return checks


# ---- the objects table, run once on ONE module in the stated order ---------------------------------------------------------------
_T = {}


def _run_case(net, case, white=True, chunk=None):
    kind, R, what = case
    mask = C.case_mask(*case)
    near, far = C.intervals(mask)
    res, hits = _objects(net, _gb(R), near.to(DEV), far.to(DEV), white, chunk)
    return dict(res=res, hits=hits, mask=mask, near=near, far=far)


def _table():
    if not _T:
        net = _net()
        _T.update(net=net, cases={case: _run_case(net, case) for case in C.table()})
    return _T


def _cases_of(R):
    return [(case, got) for case, got in _table()["cases"].items() if case[1] == R]


def _record(case, **kw):
    record_parity("compact_sweep/objects/" + C.case_name(*case), **kw)


@pytest.mark.parametrize("R", C.R_LIST)
def test_counts_and_missed_rays_are_exact(R):
    """Truth 1: last_object_hits is the mask's sum; a missed ray is rgb = 1 (0 on black), acc = depth = 0 and a zero sample row -
    whichever of the six miss encodings it carries."""
    net = _table()["net"]
    for case, got in _cases_of(R):
        mask = got["mask"]
        assert got["hits"] == int(mask.sum()), case
        miss = ~mask.to(DEV)
        _assert_misses(got["res"], miss, True)
        assert bool((got["res"][2][0][~miss] != 0).all()) and bool((got["res"][2][1][~miss] != 0).all()), case
        black, hits = _objects(net, _gb(R), got["near"].to(DEV), got["far"].to(DEV), white=False)
        assert hits == got["hits"], case
        _assert_misses(black, miss, False)
        for lv in range(2):                   # the colour changes nothing but rgb
            assert torch.equal(black[lv][1], got["res"][lv][1]) and torch.equal(black[lv][2], got["res"][lv][2]), case
            assert torch.equal(black[2][lv], got["res"][2][lv]), case
        _record(case, rays=R, hits=got["hits"], tiles_level0=C.tiles(got["hits"], C.N0), tiles_level1=C.tiles(got["hits"], C.N1))


@pytest.mark.parametrize("R", C.R_LIST)
def test_level0_rows_against_fp64(R):
    for case, got in _cases_of(R):
        checks = _level0_ok(got["res"], got["near"], got["far"], got["mask"], case)
        if checks:
            _record(case, **C.summarize(checks))


@pytest.mark.parametrize("R", C.R_LIST)
def test_patterns_are_bitwise_the_non_compact_evaluators(R):
    """Truth 3 on the default configuration, every pattern and every fixed count."""
    net = _table()["net"]
    for case, got in _cases_of(R):
        _level0_ok(got["res"], got["near"], got["far"], got["mask"], case)
        _assert_rebuild(net, _gb(R), got["res"], got["mask"].to(DEV), got["far"].to(DEV), C.N_COARSE, C.N_FINE, case)
        _record(case, bit_for_bit_non_compact=True)


@pytest.mark.parametrize("precision,preproject,kernel", EVALUATORS, ids=IDS)
def test_fixed_counts_are_bitwise_the_non_compact_evaluators(precision, preproject, kernel):
    """Truth 3 on all five evaluator configurations: 1 tile exact +- 1 row, 7 and 8 tiles exact +- 1, 9 tiles, 16 tiles at level 0;
    with 3 + 1 samples on the tile-edge counts, where level 1 ends inside a tile (16, 112 rows) or on one (128 rows)."""
    R = C.FIXED_R
    gb = _gb(R)
    for n_fine, counts in ((C.N_FINE, C.FIXED_ORDER), (C.N_FINE_ODD, C.TILE_EDGE_COUNTS)):
        net = _net(precision, preproject, n_fine=n_fine)
        ctx = net._context(torch.device(DEV))
        for k in counts:
            mask = C.fixed_mask(k)
            near, far = C.intervals(mask)
            ctx.set_timing(True)
            try:
                res, hits = _objects(net, gb, near.to(DEV), far.to(DEV))
                torch.cuda.synchronize()
                launched = [name for _, name, _, _ in ctx.read_spans()]
            finally:
                ctx.set_timing(False)
            assert launched == [kernel, kernel], launched
            assert hits == k
            label = (precision, preproject, n_fine, k)
            _level0_ok(res, near, far, mask, label)
            _assert_misses(res, ~mask.to(DEV), True)
            _assert_rebuild(net, gb, res, mask.to(DEV), far.to(DEV), C.N_COARSE, n_fine, label)
            record_parity("compact_sweep/objects_evaluators/%s_pre%d_fine%d_count%d" % (precision, int(preproject), n_fine, k),
                          bit_for_bit_non_compact=True, kernel=kernel, tiles_level0=C.tiles(k, C.N0),
                          tiles_level1=C.tiles(k, C.N_COARSE + 1 + n_fine))


_ORACLE = {}


def _oracle_at(R, t1, n_fine=C.N_FINE):
    """The oracle pair of the all-hit intervals at level-1 rows t1 (R, N1) - shared by every pattern that has those rows."""
    for key_t1, pair in _ORACLE.get((R, n_fine), []):
        if torch.equal(key_t1, t1):
            return pair
    near, far = C.intervals(torch.ones(R, dtype=torch.bool))
    pair = C.oracle_pair(R, near, far, n_fine, t1=t1)
    _ORACLE.setdefault((R, n_fine), []).append((t1, pair))
    return pair


def _assert_oracle(res, mask, full, R, label, name, n_fine=C.N_FINE):
    """Truth 4.  The oracle runs on all R rays with the all-hit intervals (a hit ray's interval does not depend on the pattern) at the
    case's own level-1 rows; the rows of its missed rays - zero in the result - are taken from the all-hit call and ignored."""
    t1 = torch.where(mask[:, None], res[2][1].cpu(), full[2][1].cpu())
    o32, o64 = _oracle_at(R, t1, n_fine)
    checks, lifted = C.oracle_checks(res, o32, o64, mask)
    assert lifted <= C.MAX_LIFTED_RAYS, (label, lifted)
    record_parity(name, rays=R, hits=int(mask.sum()), lifted_rays=lifted, **C.summarize(checks))
    C.assert_inside(checks, label)


def test_every_hit_ray_matches_the_float64_oracle():
    """Truth 4: the fixed counts at R = 257 and Bernoulli(1/2) at every R, 1e-4 with no exempt rays."""
    tab = _table()["cases"]
    todo = [("fixed", C.FIXED_R, k) for k in C.FIXED_COUNTS] + [("pattern", R, "half") for R in C.R_LIST]
    for case in todo:
        got = tab[case]
        if not bool(got["mask"].any()):
            continue
        _level0_ok(got["res"], got["near"], got["far"], got["mask"], case)
        full = tab[("pattern", case[1], "all")]["res"]
        _assert_oracle(got["res"], got["mask"], full, case[1], case, "compact_sweep/objects_oracle/" + C.case_name(*case))
    # 3 + 1 samples on the tile-edge counts
    net = _net(n_fine=C.N_FINE_ODD)
    R = C.FIXED_R
    ones = torch.ones(R, dtype=torch.bool)
    full, _ = _objects(net, _gb(R), *(x.to(DEV) for x in C.intervals(ones)))
    for k in C.TILE_EDGE_COUNTS:
        mask = C.fixed_mask(k)
        near, far = C.intervals(mask)
        res, hits = _objects(net, _gb(R), near.to(DEV), far.to(DEV))
        assert hits == k
        _level0_ok(res, near, far, mask, k)
        _assert_oracle(res, mask, full, R, ("3+1", k), "compact_sweep/objects_oracle/R257_count%d_fine1" % k, C.N_FINE_ODD)


@pytest.mark.parametrize("R", C.R_LIST)
def test_a_hit_ray_is_bitwise_the_all_hit_call(R):
    """Truth 5: one all-hit call per R serves every pattern."""
    full = _table()["cases"][("pattern", R, "all")]["res"]
    for case, got in _cases_of(R):
        assert _same(got["res"], full, got["mask"].to(DEV)), case
        _record(case, bit_for_bit_all_hit_call=True)


def test_call_history_leaves_no_trace():
    """Truth 6: the whole table ran on one module, many hits directly before few and R = 513 directly before R = 1.  Six of its cases
    on a fresh module, and once more on the first one after everything else, give the same bits: nothing is read beyond `count`."""
    tab = _table()
    fresh = _net()
    for case in C.REPEATED:
        want = tab["cases"][case]
        a = _run_case(fresh, case)
        b = _run_case(tab["net"], case)
        assert a["hits"] == b["hits"] == want["hits"], case
        assert _same(a["res"], want["res"]) and _same(b["res"], want["res"]), case
        _record(case, bit_for_bit_fresh_module=True)


def test_chunked_calls_equal_the_callers_loop():
    """Truth 7: R = 257 at chunk 64 (four whole reference chunks and one ray) against five calls of at most 64 rays."""
    net = _table()["net"]
    R, gb = C.FIXED_R, _gb(C.FIXED_R)
    for k in C.CHUNK_COUNTS:
        mask = C.fixed_mask(k)
        near, far = (x.to(DEV) for x in C.intervals(mask))
        whole, hits = _objects(net, gb, near, far, chunk=C.CHUNK)
        assert hits == k
        parts, total = [], 0
        for i in range(0, R, C.CHUNK):
            part = {key: (v[i:i + C.CHUNK] if key in PER_RAY else v) for key, v in gb.items()}
            res, n = _objects(net, part, near[i:i + C.CHUNK], far[i:i + C.CHUNK])
            parts.append(res)
            total += n
        assert total == k and len(parts) == 5
        joined = [[torch.cat([p[lv][j] for p in parts]) for j in range(len(whole[lv]))] for lv in range(3)]
        assert _same(whole, joined), k
        _assert_rebuild(net, gb, whole, mask.to(DEV), far, C.N_COARSE, C.N_FINE, ("chunk", k), chunk=C.CHUNK)
        record_parity("compact_sweep/objects_chunks/R257_count%d_chunk64" % k, bit_for_bit=True, calls=5)


# ---- grid-stride and many-workgroup cases ----------------------------------------------------------------------------------------
def test_totals_sum_takes_a_second_trip():
    """R = 65793 = 258 compaction workgroups with hits in workgroups 0, 254, 255, 256 and 257: workgroup 257 sums 257 totals, the
    257th on the second trip of emit_body's loop."""
    R = C.BIG_WG_R
    mask = C.big_wg_mask()
    near, far = C.intervals(mask)
    gb = _gb(R)
    net = _table()["net"]
    res, hits = _objects(net, gb, near.to(DEV), far.to(DEV))
    assert hits == int(mask.sum())
    hit = mask.to(DEV)
    # map[slot] through the outputs: every hit ray has its own non-zero rows, every miss zero rows
    _assert_misses(res, ~hit, True)
    assert bool((res[2][0][hit] != 0).all()) and bool((res[2][1][hit] != 0).all())
    checks = _level0_ok(res, near, far, mask, "big_wg")
    _assert_rebuild(net, gb, res, hit, far.to(DEV), C.N_COARSE, C.N_FINE, "big_wg")
    record_parity("compact_sweep/objects_grid/R65793_workgroups258", hits=hits, bit_for_bit_non_compact=True, **C.summarize(checks))


def test_scatter_takes_a_second_trip():
    """R = 4101 rays x 1023 level-1 samples = 4,195,323 elements on a grid capped at 16384 blocks of 256."""
    R, chunk = C.SCATTER_R, C.SCATTER_CHUNK
    mask = C.scatter_mask()
    near, far = (x.to(DEV) for x in C.intervals(mask))
    gb = _gb(R)
    net = _net(n_fine=C.SCATTER_N_FINE)
    whole, hits = _objects(net, gb, near, far, chunk=chunk)
    assert hits == 5
    parts = []
    for i in range(0, R, chunk):
        part = {key: (v[i:i + chunk] if key in PER_RAY else v) for key, v in gb.items()}
        parts.append(_objects(net, part, near[i:i + chunk], far[i:i + chunk])[0])
    assert [p[0][0].shape[0] for p in parts] == [2048, 2048, 5]
    joined = [[torch.cat([p[lv][j] for p in parts]) for j in range(len(whole[lv]))] for lv in range(3)]
    assert _same(whole, joined)
    hit = mask.to(DEV)
    _assert_misses(whole, ~hit, True)
    assert whole[2][1].shape == (R, 1023) and bool((whole[2][1][hit] != 0).all())
    checks = _level0_ok(whole, near.cpu(), far.cpu(), mask, "scatter")
    record_parity("compact_sweep/objects_grid/R4101_N1023_scatter", hits=hits, bit_for_bit=True, calls=3, **C.summarize(checks))


def test_level0_builder_takes_a_second_trip():
    """R = 16400 rays, all hit, 257 level-0 samples = 4,214,800 rows x samples on a grid capped at 16384 blocks of 256: level-0 rows
    on every ray against fp64, results bitwise the caller's loop over 4096-ray pieces."""
    R, chunk = C.LEVEL0_R, C.LEVEL0_CHUNK
    mask = torch.ones(R, dtype=torch.bool)
    near, far = C.intervals(mask)
    gb = _gb(R)
    net = _net(n_coarse=C.LEVEL0_N_COARSE, n_fine=C.LEVEL0_N_FINE)
    t = time.time()
    whole, hits = _objects(net, gb, near.to(DEV), far.to(DEV), chunk=chunk)
    torch.cuda.synchronize()
    print("16400 rays x (257 + 258) samples: %.2f s" % (time.time() - t))
    assert hits == R
    checks = _level0_ok(whole, near, far, mask, "level0_grid", C.LEVEL0_N_COARSE)
    near, far = near.to(DEV), far.to(DEV)
    parts = []
    for i in range(0, R, chunk):
        part = {key: (v[i:i + chunk] if key in PER_RAY else v) for key, v in gb.items()}
        parts.append(_objects(net, part, near[i:i + chunk], far[i:i + chunk])[0])
    joined = [[torch.cat([p[lv][j] for p in parts]) for j in range(len(whole[lv]))] for lv in range(3)]
    assert _same(whole, joined)
    record_parity("compact_sweep/objects_grid/R16400_N257_level0", hits=hits, bit_for_bit=True, calls=5, **C.summarize(checks))


# ---- instances -------------------------------------------------------------------------------------------------------------------
def _instances(net, gb, near, far, **kw):
    out = net.render_instances(gb, near, far, **kw)
    net.check_flags()
    inst = None if out["instances"] is None else [[t.clone() for t in lv] for lv in out["instances"]]
    return dict(instances=inst, composite=[[t.clone() for t in lv] for lv in out["composite"]]), int(net.last_instance_pairs)


def _assert_instance_call(net, gb, mask, near, far, label, name, rows=None, composite=True):
    """One (K,R) pair mask, both background colours: the pair count; per-instance rows bitwise render_objects (tied to the
    non-compact evaluators by the objects tests above); the composite against the fp64 recurrence on the call's own fp32 rows; the
    id map; per_instance=False."""
    K, R = mask.shape
    near_d, far_d = near.to(DEV), far.to(DEV)
    got = {}
    for white in (True, False):
        res, pairs = _instances(net, gb, near_d, far_d, white_bkgd=white)
        assert pairs == int(mask.sum()), (label, white, pairs)
        for i in (range(K) if rows is None else rows):
            want, hits = _objects(net, gb, near_d[i], far_d[i], white)
            assert hits == int(mask[i].sum()), (label, i)
            for lv in range(2):
                for k, x, y in zip(OUT, res["instances"][lv], want[lv]):
                    assert torch.equal(x[i], y), (label, white, i, lv, k)
        miss = ~mask.to(DEV)
        for lv in range(2):
            rgb, acc, depth = res["instances"][lv]
            assert bool((rgb[miss] == (1.0 if white else 0.0)).all()) and bool((acc[miss] == 0).all()) and bool((depth[miss] == 0).all()), label
        lean, _ = _instances(net, gb, near_d, far_d, white_bkgd=white, per_instance=False)
        assert lean["instances"] is None
        for lv in range(2):
            assert all(torch.equal(x, y) for x, y in zip(lean["composite"][lv], res["composite"][lv])), (label, white, lv)
        got[white] = res
    if not composite:
        record_parity(name, pairs=int(mask.sum()), bit_for_bit_render_objects=True, instances_compared=len(rows))
        return got
    black, white = got[False], got[True]
    worst, inside = {}, 0
    for lv in range(2):
        p, a, d = black["instances"][lv]
        c64 = C.composite64(near, far, p, a, d, white=False)
        g_rgb, g_acc, g_depth, g_ids = black["composite"][lv]
        assert g_ids.dtype == torch.int32
        r_rgb, r_acc, r_depth = (x.cpu() for x in ic.composite(near_d, far_d, p, a, d, white=False)[:3])     # the fp32 restatement
        checks = dict(rgb=C.worst_entry(g_rgb, c64["rgb"], K * 2.0 ** -23, r_rgb), acc=C.worst_entry(g_acc, c64["acc"], K * 2.0 ** -23, r_acc),
                      depth=C.worst_entry(g_depth, c64["depth"], K * 2.0 ** -22, r_depth))
        C.assert_inside(checks, (label, lv))
        for k, v in checks.items():
            worst["%s%d" % (k, lv)] = v
        ok, close = C.id_checks(g_ids, c64, K)
        assert ok, (label, lv, "instance_id")
        inside = max(inside, close)
        none = ~mask.any(dim=0).to(DEV)
        assert torch.equal(g_ids < 0, none), (label, lv)                     # -1 exactly on the rays without a hit
        w_rgb, w_acc, w_depth, w_ids = white["composite"][lv]
        assert torch.equal(w_acc, g_acc) and torch.equal(w_depth, g_depth) and torch.equal(w_ids, g_ids), (label, lv)
        assert float((w_rgb - (g_rgb + (1.0 - g_acc)[:, None])).abs().max()) <= 2.0 ** -23, (label, lv)
        assert bool((w_rgb[none] == 1.0).all()) and bool((g_rgb[none] == 0.0).all()) and bool((g_acc[none] == 0).all()) and bool((g_depth[none] == 0).all())
    record_parity(name, pairs=int(mask.sum()), windows=sum(1 for n in C.windows_model(int(mask.sum()), K, R) if n),
                  bit_for_bit_render_objects=True, rays_inside_id_margin=inside, **C.summarize(worst))
    return got


_INST = {}


def _inst_net():
    if "net" not in _INST:
        _INST["net"] = _net()
    return _INST["net"]


@pytest.mark.parametrize("K,R", [(K, R) for K in C.WINDOW_K for R in C.WINDOW_R])
def test_instance_windows(K, R):
    """Pair counts 0, 1, R - 1, R, R + 1, 2 R, K R: empty, exactly full and full +- 1 windows, a ray whose instances are split over
    two windows, ties in `near` between instances 0 and 1, K = 1 with R = 1.  One module runs every count in DEscending order (a
    window's rows beyond its count are the previous, fuller call's), then the two smallest again: the same bits."""
    net, gb = _inst_net(), _gb(R)
    counts = C.window_counts(K, R)
    first = {}
    for c in counts[::-1] + counts[:2]:
        mask = C.window_mask(K, R, c)
        near, far = C.instance_intervals(mask)
        got = _assert_instance_call(net, gb, mask, near, far, (K, R, c), "compact_sweep/instances/K%d_R%d_pairs%d" % (K, R, c))
        if c in first:            # after the full calls: the same bits as before them
            for white in (True, False):
                flat = lambda r: [t for part in (r["instances"], r["composite"]) for lv in part for t in lv]      # noqa: E731
                assert all(torch.equal(x, y) for x, y in zip(flat(got[white]), flat(first[c][white]))), (K, R, c)
        first[c] = got


def test_thirty_two_instances():
    """K = 32 (bit 31 of the membership mask), R = 65, Bernoulli(1/4) per pair, with rays on which instance 31 is the only hit, the
    nearest of several, ties with instance 0 in `near` (the id must be 0), and on which all 32 hit."""
    mask = C.k32_mask()
    near, far = C.instance_intervals(mask, designed=True)
    got = _assert_instance_call(_inst_net(), _gb(C.K32_R), mask, near, far, "k32", "compact_sweep/instances/K32_R65")
    for lv in range(2):
        ids = got[False]["composite"][lv][3].cpu()
        assert [int(ids[r]) for r in (C.ONLY31, C.NEAREST31, C.TIE31, C.ALL32)] == [31, 31, 0, 0], (lv, ids[:4])


def test_pair_compaction_over_258_workgroups():
    """K = 32, R = 2057: 65824 pairs, Bernoulli(1/128) per pair; the pair count and the rows of instances 0, 15 and 31."""
    mask = C.k32_big_mask()
    near, far = C.instance_intervals(mask)
    _assert_instance_call(_inst_net(), _gb(C.K32_BIG_R), mask, near, far, "k32_big", "compact_sweep/instances/K32_R2057",
                          rows=C.K32_BIG_ROWS, composite=False)


def test_instance_level0_builder_takes_a_second_trip():
    """K = 1, R = 16400, 256 + 1 samples, all hit: k_inst_level0's 4,214,800 rows x samples on a grid capped at 16384 blocks.  The
    rows are render_objects' (held to fp64 and to the piece loop by test_level0_builder_takes_a_second_trip)."""
    R, chunk = C.LEVEL0_R, C.LEVEL0_CHUNK
    near, far = (x.to(DEV) for x in C.intervals(torch.ones(R, dtype=torch.bool)))
    gb = _gb(R)
    net = _net(n_coarse=C.LEVEL0_N_COARSE, n_fine=C.LEVEL0_N_FINE)
    res, pairs = _instances(net, gb, near[None], far[None], chunk=chunk)
    assert pairs == R
    want, hits = _objects(net, gb, near, far, chunk=chunk)
    assert hits == R
    for lv in range(2):
        for k, x, y in zip(OUT, res["instances"][lv], want[lv]):
            assert x.shape[0] == 1 and torch.equal(x[0], y), (lv, k)
        for k, x, y in zip(OUT, res["composite"][lv][:3], want[lv]):       # K = 1: the composite IS the instance
            assert torch.equal(x, y), (lv, k)
        assert bool((res["composite"][lv][3] == 0).all())
    record_parity("compact_sweep/instances_grid/K1_R16400_N257_level0", pairs=pairs, bit_for_bit_render_objects=True)


def test_instance_miss_fill_takes_a_second_trip():
    """K = 32, R = 131073: 4,194,336 pairs against the 4,194,304 that 16384 blocks of k_inst_fill_misses cover in one trip; the
    last 32 pairs - rays of instance 31 - hold 31 misses and a hit.  Rows of instances 0 and 31 against render_objects."""
    mask = C.fill_mask()
    near, far = C.instance_intervals(mask)
    _assert_instance_call(_inst_net(), _gb(C.FILL_R), mask, near, far, "fill", "compact_sweep/instances_grid/K32_R131073_fill",
                          rows=C.FILL_ROWS, composite=False)


# ---- culling ---------------------------------------------------------------------------------------------------------------------
def _cull_net(precision=None, preproject=3):
    st = synth.nerf_tp_state(0)
    for k in ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias"):
        st[k] = st[k] + C.CULL_BIAS
    return _net(precision, preproject, state=st)


def _forward(net, batch, eps, fine_only=False):
    net.cull_background = eps
    try:
        out = net(batch, False, False, 0.0, 0.0, out_depth=True, fine_only=fine_only)
        net.check_flags()
    finally:
        net.cull_background = None
    return [None if lv is None else [t.clone() for t in lv] for lv in out]


def _cull_sweep(net, R, label, name, fine_only_kernel=None, fresh=None):
    """Every target survivor count of R: eps = the k-th largest max(lambda_0, lambda_1) of the UN-culled render keeps exactly k rays;
    the contract is test_gpu_cull_background._assert_contract, unchanged.  k = R directly before k = 1 (and repeated on `fresh`)."""
    batch = _gb(R)
    full = _forward(net, batch, None)
    m = torch.maximum(full[0][4].reshape(-1), full[1][4].reshape(-1))
    targets = C.cull_targets(R)
    order = [k for k in targets if k not in (1, R)] + [R, 1]
    ctx = net._context(torch.device(DEV))
    for k in order:
        eps, tie = C.cull_eps(m, k)
        assert not tie, (label, k, "max(lambda_0, lambda_1) ties at this rank")
        assert 0.0 < eps < 1.0, (label, k, eps)
        got = _forward(net, batch, eps)
        assert int(net.last_cull_survivors) == k, (label, k, int(net.last_cull_survivors))
        _assert_contract(net, full, got, eps)
        if fresh is not None and k in (R, 1):
            again = _forward(fresh, batch, eps)
            assert int(fresh.last_cull_survivors) == k
            for lv in range(2):
                for key, x, y in zip(CULL_NAMES, again[lv], got[lv]):
                    assert torch.equal(x, y), (label, k, lv, key)
        if fine_only_kernel is not None:
            # level 0 takes no colour or depth: the two compact background launches are density-only
            ctx.set_timing(True)
            try:
                fine = _forward(net, batch, eps, fine_only=True)
                torch.cuda.synchronize()
                launched = [n for _, n, _, _ in ctx.read_spans()]
            finally:
                ctx.set_timing(False)
            assert len(launched) == 4 and launched[2] == launched[3] == fine_only_kernel, launched
            assert fine[0] is None and int(net.last_cull_survivors) == k
            _assert_contract(net, full, [got[0], fine[1]], eps)
            assert int(net.last_cull_survivors) == k
        record_parity("%s_keep%d" % (name, k), rays=R, survivors=k, eps=eps, bit_for_bit_survivors=True,
                      tiles_level0=C.tiles(k, C.N0), tiles_level1=C.tiles(k, C.N1))


@pytest.mark.parametrize("R", [R for R in C.CULL_R if R != C.FIXED_R])
def test_cull_survivor_counts(R):
    """0, 1, 15, 16, 17, R - 1 and R survivors on the default configuration; the call history rule on a fresh module."""
    _cull_sweep(_cull_net(), R, ("cull", R), "compact_sweep/cull/R%d" % R, fresh=_cull_net())


@pytest.mark.parametrize("precision,preproject,kernel", CULL_EVALUATORS,
                         ids=["%s-pre%d-%s" % (p, int(m), k) for p, m, k in CULL_EVALUATORS])
def test_cull_survivor_counts_on_every_background_evaluator(precision, preproject, kernel):
    """R = 257: also 112, 128 and 129 survivors (7 and 8 tiles exact, 9 tiles at level 0)."""
    _cull_sweep(_cull_net(precision, preproject), C.FIXED_R, ("cull", precision, preproject),
                "compact_sweep/cull_evaluators/%s_pre%d_R257" % (precision, int(preproject)))


def test_cull_survivor_counts_with_density_only_background_launches():
    """R = 65 through the fine-only call: level 0 is NULL, so the coarse background launch is the compact density-only one
    (input_ch == 4)."""
    _cull_sweep(_cull_net(), 65, ("cull", "fine_only"), "compact_sweep/cull_fine_only/R65", fine_only_kernel="k_tp_mlp_hpp")
