"""GPU: the fused frame drivers of vanilla NeRF, PixelNeRF and Mip-NeRF 360 (neo_vanilla_render, neo_pix_render, neo_mip_render), case
by case of tests/frame_chain_cases.py (whose conditions tests/test_frame_chain_cases_cpu.py checks without a GPU).

Every case is run twice over.  (1) The frame is rebuilt from the PUBLIC stage operators - eval_mlp, ops.composite, ops.resample,
ops.mip_resample, ops.mip_composite, the level-0 row built on the host - and must be torch.equal to the fused call on every returned
tensor: the drivers are the only callers of the shared-row kernel forms (one row of level-0 positions for all rays), of the edge
table with a real near / far, and of the Mip-NeRF 360 level loop in C.  (2) The frame is held to the fp64 oracle evaluated at the
rows the chain produced, per ray and output, under the project's parity contract; no ray is exempt.  Then the call history: one
module through the table with ray and sample counts going down and up, against fresh modules, against the calls without overlap,
and ten consecutive calls against their single calls.  Every case lands in the parity report under frame_chain_sweep/<case>/<variant>."""
import pytest
import torch

import cases
import frame_chain_cases as F
from conftest import max_abs, record_parity
from neo360_amd import _lib, models, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NETS = {}


# ---- modules, frames and their stage chains ----------------------------------------------------------------------------------------
def _new(kind, overlap=None):
    if kind == "vanilla":
        net = models.NeRF().to(DEV)
    elif kind == "pix":
        net = models.PixelNeRF(num_src_views=cases.NV).to(DEV)
        sc = F.scene()
        net.set_scene(sc["latent"].to(DEV), sc["image_wh"])
    else:
        net = models.MipNeRF360().to(DEV)
    if overlap is not None:
        net.overlap_calls = overlap
    net._fc_state = None
    return net


def _shared(kind):
    """One module per renderer for the case-by-case tests: whichever cases ran before, a case's frame must equal its chain."""
    if kind not in _NETS:
        _NETS[kind] = _new(kind)
    return _NETS[kind]


def _configure(net, c, variant):
    if net._fc_state != c.state:
        net.load_state_dict(F.state_of(c.kind, c.state))
        net._fc_state = c.state
    if c.kind == "mip":
        net.num_prop_samples, net.num_nerf_samples = c.counts
        net.precision, net.layered = variant
    else:
        net.num_coarse_samples, net.num_fine_samples = c.counts
        if c.kind == "vanilla":
            net.precision = variant
        else:
            net.preproject = variant
    return net


def _rays(kind, R, _cache={}):
    if (kind, R) not in _cache:
        _cache[(kind, R)] = {k: v.to(DEV) for k, v in F.rays_of(kind, R).items()}
    return _cache[(kind, R)]


def _frame(net, c):
    """The fused call, its returned tensors by name."""
    rays = _rays(c.kind, c.R)
    if c.kind == "mip":
        rend, hist = net(rays, c.tf, False, False, c.near, c.far)
        out = {}
        for l in range(3):
            out.update({"rgb%d" % l: rend[l]["rgb"], "sdist%d" % l: hist[l]["sdist"], "w%d" % l: hist[l]["weights"],
                        "dens%d" % l: hist[l]["density"], "prgb%d" % l: hist[l]["rgb"]})
        return out
    if c.kind == "vanilla":
        res = net(rays, False, c.white, c.near, c.far)
    else:
        res = net(rays, False, c.white, c.near, c.far, chunk=c.chunk)
    return {"%s%d" % (k, lv): res[lv][j] for lv in (0, 1) for j, k in enumerate(("rgb", "acc", "depth"))}


def _chain(net, c):
    """The same frame from the public stage operators; also returns the sample rows it went through and (vanilla, PixelNeRF) the
    level-0 weights the resampler read."""
    rays = _rays(c.kind, c.R)
    if c.kind == "mip":
        dilation, anneal = F.mip_schedule(c)
        s_prev = torch.tensor([[0.0, 1.0]], device=DEV).repeat(c.R, 1)
        w_prev = torch.ones(c.R, 1, device=DEV)
        out = {}
        for l in range(3):
            n = c.counts[0] if l < 2 else c.counts[1]
            sdist, tdist = ops.mip_resample(s_prev, w_prev, n, c.near, c.far, dilate=l > 0, dilation=dilation[l], anneal=anneal)
            rd = net.eval_mlp(l, rays, tdist)
            w, rgb = ops.mip_composite(rd, tdist, rays["rays_d"])
            out.update({"rgb%d" % l: rgb, "sdist%d" % l: sdist, "w%d" % l: w, "dens%d" % l: rd[..., 3], "prgb%d" % l: rd[..., :3]})
            s_prev, w_prev = sdist, w
        return out, tuple(out["sdist%d" % l] for l in range(3)), None
    n_coarse, n_fine = c.counts
    t0 = F.host_edges(n_coarse, c.near, c.far).to(DEV)[None].expand(c.R, n_coarse + 1).contiguous()
    if c.kind == "vanilla":
        ev = lambda lv, t: net.eval_mlp(lv, rays["rays_o"], rays["viewdirs"], t)
    else:
        ev = lambda lv, t: net.eval_mlp(lv, rays, t, chunk=c.chunk)         # the chunk decides the direction rows
    c0 = ops.composite(0, ev(0, t0), t0, rays["rays_d"], white_bkgd=c.white)
    t1 = ops.resample(t0, c0["weights"], n_fine)
    c1 = ops.composite(0, ev(1, t1), t1, rays["rays_d"], white_bkgd=c.white)
    out = {"%s%d" % (k, lv): cc[k] for lv, cc in ((0, c0), (1, c1)) for k in ("rgb", "acc", "depth")}
    return out, (t0, t1), c0["weights"]


def _assert_equal(a, b, label):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape, (label, k)
        assert torch.equal(a[k], b[k]), (label, k, "max |difference| %.3e" % max_abs(a[k], b[k]))


ALL = [(c, v) for kind in ("vanilla", "pix", "mip") for c in F.table(kind) for v in c.variants]


@pytest.mark.parametrize("case,variant", ALL, ids=["%s-%s" % (F.case_id(c), F.variant_id(c, v)) for c, v in ALL])
def test_frame_equals_its_stage_chain_and_meets_fp64(case, variant):
    """torch.equal between the fused call and its stage chain on every returned tensor; then every ray and output of the frame inside
    TOL x max(1, |fp64 value|) (TOL_HIST on Mip-NeRF 360's weights and densities) of the fp64 oracle at the chain's rows."""
    label = "%s/%s" % (F.case_id(case), F.variant_id(case, variant))
    net = _configure(_shared(case.kind), case, variant)
    frame = _frame(net, case)
    chain, rows, w0 = _chain(net, case)
    net.check_flags()
    _assert_equal(frame, chain, label)
    if case.kind == "mip":
        assert float(frame["prgb0"].abs().max()) == 0.0 and float(frame["prgb1"].abs().max()) == 0.0       # proposal levels carry no colour
    else:
        assert rows[1].shape == (case.R, sum(case.counts) + 1) and bool((rows[1][:, 1:] >= rows[1][:, :-1]).all())
        if case.state == "empty":
            # the weights the resampler reads add up to less than 1e-5: its padded, uniform fallback.  PixelNeRF's density is a relu
            # and they are exactly 0.  Vanilla's is softplus(-101) = 1.4e-44, which the kernels keep as a subnormal, and the
            # compositing kernel's opacity of a tiny optical depth is that depth, not 0: weights of 1e-45 .. 2e-44, and 1e-34 on the
            # last sample, whose interval is 1e10.
            inner = float(w0[:, 1:-1].abs().max())
            assert inner == 0.0 if case.kind == "pix" else inner < 1e-40, inner
            assert float(frame["acc0"].abs().max()) < 1e-30 and float(frame["acc1"].abs().max()) < 1e-30
    ref64 = F.run_oracle(case, torch.float64, rows)
    ref32 = F.run_oracle(case, torch.float32, rows)
    checks = F.frame_checks(case, {k: v.cpu() for k, v in frame.items()}, ref64, ref32)
    record_parity("frame_chain_sweep/" + label, chain_bit_for_bit=True, rays=case.R, **F.summarize(checks))
    F.assert_inside(checks, label)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vanilla", "pix", "mip"])
def test_sample_counts_outside_the_limits_are_refused_before_any_launch(kind):
    """One step outside each limit of the drivers: an error from the host checks, no evaluator launch recorded, and the next
    accepted call is what it always is."""
    plain = F.find(kind, F.MIP_DEFAULT if kind == "mip" else F.LEVEL_MID)
    net = _configure(_new(kind), plain, plain.variants[0])
    want = _frame(net, plain)
    ctx = net._context(torch.device(DEV, torch.cuda.current_device()))
    ctx.set_timing(True)
    for counts in (F.MIP_REFUSED if kind == "mip" else F.LEVEL_REFUSED):
        bad = plain._replace(counts=counts)
        _configure(net, bad, plain.variants[0])
        with pytest.raises(_lib.NeoError, match="unsupported sample counts"):
            _frame(net, bad)
        assert ctx.read_timing()[1] == 0, counts
    ctx.set_timing(False)
    _configure(net, plain, plain.variants[0])
    _assert_equal(_frame(net, plain), want, kind)
    net.check_flags()


# ---- call history, lanes and tables ------------------------------------------------------------------------------------------------
def _size(c):
    return c.R * (sum(c.counts) + 1 if c.kind != "mip" else max(c.counts))


def _history_order(kind):
    """The table in an order that makes ray and sample counts go down and up: the largest case, the smallest counts at one ray, the
    ragged / largest ray count, the mid case, then the rest alternately from the big and the small end.  Ray counts repeat and
    alternate, so that the per-ray-count tables are both filled and hit."""
    tab = list(F.table(kind))
    if kind == "mip":
        head = [F.find(kind, F.MIP_LARGEST, R=3), F.find(kind, (2, 2)), F.find(kind, F.MIP_MID, R=201), F.find(kind, F.MIP_MID, R=1),
                F.find(kind, F.MIP_MID)]
    else:
        head = [F.find(kind, F.LEVEL_LARGEST), F.find(kind, (3, 1), R=1), F.find(kind, (3, 1), R=F.RAGGED_R), F.find(kind, F.LEVEL_MID)]
    rest = sorted((c for c in tab if c not in head), key=_size, reverse=True)
    order = list(head)
    while rest:
        order.append(rest.pop(0))
        if rest:
            order.append(rest.pop())
    assert len(order) == len(tab)
    return order


def _cpu(d):
    return {k: v.cpu() for k, v in d.items()}


@pytest.mark.parametrize("kind", ["vanilla", "pix", "mip"])
def test_one_module_through_the_table_with_counts_going_down_and_up(kind):
    """Workspaces per scratch lane grow under the calls and are never shrunk; consecutive calls alternate between two lanes.  One
    module through the whole table: six of the cases equal a fresh module's result bit for bit, equal it again on the first module
    after everything else has run, and every case equals the call of a module without overlap."""
    order = _history_order(kind)
    sizes = [_size(c) for c in order]
    assert any(a > b for a, b in zip(sizes, sizes[1:])) and any(a < b for a, b in zip(sizes, sizes[1:]))
    first = _new(kind)
    got = [_cpu(_frame(_configure(first, c, c.variants[0]), c)) for c in order]
    first.check_flags()
    six = [0, 1, 2, 3, len(order) // 2, len(order) - 1]
    for i in six:
        c = order[i]
        fresh = _new(kind)
        _assert_equal(_cpu(_frame(_configure(fresh, c, c.variants[0]), c)), got[i], ("fresh", F.case_id(c)))
        fresh.check_flags()
        fresh.close()
    for i in six:
        c = order[i]
        _assert_equal(_cpu(_frame(_configure(first, c, c.variants[0]), c)), got[i], ("again", F.case_id(c)))
    serial = _new(kind, overlap=False)
    for i, c in enumerate(order):
        _assert_equal(_cpu(_frame(_configure(serial, c, c.variants[0]), c)), got[i], ("no overlap", F.case_id(c)))
    first.check_flags()
    serial.check_flags()
    record_parity("frame_chain_sweep/history/%s" % kind, bit_for_bit=True, cases=len(order), fresh_modules=len(six))


@pytest.mark.parametrize("kind", ["vanilla", "pix", "mip"])
def test_ten_consecutive_calls_equal_their_single_calls(kind):
    """Ten calls on one module with nothing waited for in between, alternating two (near, far) pairs call by call and two ray counts
    every other call: two scratch lanes, two edge tables (vanilla, PixelNeRF), two seed histograms (Mip-NeRF 360) in flight."""
    mid = F.find(kind, F.MIP_MID if kind == "mip" else F.LEVEL_MID)
    pairs = (F.NEAR_FAR[kind], F.NEAR_FAR_MID[0])
    combos = [mid._replace(R=R, near=nf[0], far=nf[1]) for R in (5, 201) for nf in pairs]
    single = {}
    for c in combos:
        net = _configure(_new(kind), c, c.variants[0])
        single[c] = _cpu(_frame(net, c))
        net.check_flags()
        net.close()
    net = _configure(_new(kind), mid, mid.variants[0])
    calls = [mid._replace(R=(5, 201)[(i // 2) % 2], near=pairs[i % 2][0], far=pairs[i % 2][1]) for i in range(10)]
    outs = [_frame(net, c) for c in calls]
    net.check_flags()
    for i, (c, o) in enumerate(zip(calls, outs)):
        _assert_equal(_cpu(o), single[c], (kind, "call %d" % i, F.case_id(c)))
    record_parity("frame_chain_sweep/ten_calls/%s" % kind, bit_for_bit=True, calls=10)
