"""The case table of the boundary sweep (tests/test_boundary_cases_cpu.py, tests/test_gpu_boundary_sweep.py): one record per
Python entry point that hands caller tensors to the library, and two generators that work from a record.

A record holds the smallest valid call of its entry point (cases.small_scene() seen by cases.strided_rays(7), sample counts 3 + 4
as in compact_cases, K = 2 instances, every value rounded through fp16 so that fp16 / fp32 / fp64 copies hold the same numbers),
the list of its tensor arguments with their symbolic shapes and roles, and - for a differentiable entry - the scalar whose
backward is taken.  Everything here is plain CPU torch; `call(env, T)` is only run by the GPU test, which supplies `env` (the
package's modules and one shared instance per model class) and the tensors `T` on the device.

layout_variants(record, dev)    one argument at a time (and, for the ray tensors of the module calls, all at once) as a column
                                slice, in transposed storage, as a stride-0 expansion of its own first row, as a contiguous view
                                4 bytes into its allocation, and as an fp64 / fp16 copy - each equal in value to its dense twin.
mismatch_variants(record, dev)  one argument at a time with R -+ 1 rows, a trailing extent off by one, one rank too few / too
                                many, the wrong dtype class, on the CPU, and optional groups given in part.  EVERY tensor of such a
                                case is a leading contiguous view of a backing allocation that holds the largest extent any tensor
                                of the case implies in every dimension: a wrapper that misses a check still reads only memory the
                                test owns, and the case fails by "did not raise".

The views are built ON `dev`: `.to(device)` of a strided or offset view would hand the device a compact copy.
"""
import math

import numpy as np
import torch

import cases

R, N0, N1, K, NV = 7, 4, 8, 2, cases.NV       # rays; samples per ray at the two levels of a 3 + 4 module; instances; source views
N_COARSE, N_FINE = 3, 4
G = 8                                          # occupancy resolution
MIP_COUNTS = (16, 8)                           # proposal / NeRF samples of the shared Mip-NeRF 360 module
SIZES = dict(R=R, N=N0, M=N1, K=K, L=2, P=R * N0, NV=NV, I=12, O=8, T=10, HF=cases.LATENT_HW[0], WF=cases.LATENT_HW[1], Q=4, Y=NV * 4)


def q(x):
    """Rounded through fp16: the fp16, fp32 and fp64 copies of the result hold the same numbers."""
    return x.half().float()


def _rand(seed, *shape):
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed))


class Arg:
    """One tensor argument: its name in the record's tensor dict, its symbolic shape (str = a symbol of SIZES, optionally 'N+1';
    int = a literal extent), the other shapes the entry accepts (`alts`), its role - "input", or "output" for a caller-owned
    output the library writes through -, its dtype class ("float", "int", "bool"), whether fp64 / fp16 copies are part of the
    contract (`copies`), and whether it may live on any device (`any_device`).  free=True: the entry accepts any shape."""

    def __init__(self, name, shape, alts=(), role="input", kind="float", copies=True, any_device=False, free=False):
        self.name, self.shape, self.alts, self.role, self.kind = name, tuple(shape), tuple(tuple(a) for a in alts), role, kind
        self.copies, self.any_device, self.free = copies and kind == "float" and role == "input", any_device, free


def extent(e, sizes=SIZES):
    if isinstance(e, int):
        return e
    sym, _, add = e.partition("+")
    return sizes[sym] + (int(add) if add else 0)


def symbol(e):
    return None if isinstance(e, int) else e.partition("+")[0]


def resolve(shape, sizes=SIZES):
    return tuple(extent(e, sizes) for e in shape)


class Record:
    """entry: the dotted name the completeness test matches ("ops.composite", "models.NeRF_TP.render_objects"); several records
    may cover one entry (its modes).  build() -> {name: dense fp32 CPU tensor}; call(env, T) -> the entry's outputs, any nesting
    of tensors / dicts / tuples / None.  grad: the names of the inputs that receive gradients; scalar(outputs) -> the scalar whose
    backward is taken.  groups: tuples of optional arguments that go together (T[name] = None means "not given").
    together: the arguments the layout variants are also applied to all at once.  family: for the counts of the write-up.
    chain = (module attribute of env, parameter-name endings to leave out): the call is made with autograd on, so that the
    module takes its differentiable operator chain (the training drivers); outputs AND the gradients of the module's parameters
    are compared, except the named ones, whose accumulation order is not fixed (docs/boundary_sweep.md)."""

    def __init__(self, name, entry, family, args, build, call, grad=(), scalar=None, groups=(), together=(), chain=None, ties=()):
        self.ties = tuple(ties)     # symbols one argument alone carries that a scalar of the call still fixes (R of d_enc: x0 has R n rows)
        self.name, self.entry, self.family, self.args, self.build, self.call = name, entry, family, list(args), build, call
        self.grad, self.scalar, self.groups, self.together, self.chain = tuple(grad), scalar, tuple(groups), tuple(together), chain

    def arg(self, name):
        return next(a for a in self.args if a.name == name)


RECORDS = {}


def record(*a, **kw):
    r = Record(*a, **kw)
    assert r.name not in RECORDS, r.name
    RECORDS[r.name] = r
    return r


# ---- inputs -------------------------------------------------------------------------------------------------------------------

_cache = {}


def base():
    """The shared dense inputs (CPU fp32, fp16-exact); built once, never modified (every user clones)."""
    if _cache:
        return _cache
    rays = cases.strided_rays(R)
    o, d = q(rays["rays_o"]), q(rays["rays_d"])
    d1 = -(o * d).sum(-1) / (d * d).sum(-1)
    rho2 = ((o + d1[:, None] * d) ** 2).sum(-1)
    far = q((d1 + torch.sqrt(1.0 - rho2) / d.norm(dim=-1)) * 0.98)           # inside the unit sphere's exit of every ray
    frac = torch.linspace(0.1, 0.9, N0)
    frac1 = torch.linspace(0.1, 0.9, N0 + 1)
    _cache.update(
        rays_o=o, rays_d=d, viewdirs=q(rays["viewdirs"]), far=far,
        t=q(far[:, None] * frac[None, :] + 0.01 * _rand(1, R, 1)),             # ascending rows below far
        t1=q(far[:, None] * frac1[None, :]),                                    # N + 1 ascending edges
        s=q(torch.linspace(0.9, 0.1, N0)[None, :] - 0.05 * _rand(2, R, 1)),    # descending inverse radius
        s1=q(torch.linspace(0.0, 1.0, N0 + 1)[None, :].expand(R, N0 + 1).contiguous()),     # sdist edges of a Mip-NeRF 360 level
        rgbsigma=q(torch.cat([_rand(3, R, N0, 3), 4.0 * _rand(4, R, N0, 1)], dim=-1)),
        w=q(0.05 + _rand(5, R, N0)), w_env=q(0.05 + _rand(6, R, N1)),
        t_env=q(torch.linspace(0.0, 1.0, N1 + 1)[None, :].expand(R, N1 + 1).contiguous()),
        u=q(_rand(7, R, N0)), u2=q(_rand(8, R, N0)), u_new=q(torch.sort(0.999 * _rand(9, R, N1), dim=-1).values),
        radii=q(cases.mip_rays(R)["radii"]), lam=q(_rand(10, R)),
        near_inst=q(torch.stack([0.3 * far, 0.5 * far])), far_inst=q(torch.stack([0.6 * far, 0.9 * far])),
        key=q(torch.stack([0.4 * far, 0.7 * far])), lrgb=q(0.5 * _rand(11, 2, R, 3)), lacc=q(0.5 * _rand(12, 2, R)),
        ldepth=q(_rand(13, 2, R)), occ=(_rand(14, G, G, G) > 0.3), sigma=q(2.0 * _rand(15, G, G, G)),
        x=q(2.0 * _rand(16, R, 3) - 1.0), raw_rgb=q(2.0 * _rand(17, R * N0, 3) - 1.0), raw_sigma=q(2.0 * _rand(18, R * N0) - 1.0),
        noise=q(_rand(19, R * N0)),
        tdist_mip=q(torch.linspace(0.2, 3.0, 5)[None, :].expand(R, 5).contiguous()),
    )
    return _cache


def rts():
    """Two axis-aligned boxes in the reference's RTs format (K = 2)."""
    return dict(R=[np.eye(3), np.eye(3)], T=[np.array([0.05, -0.05, 0.0]), np.array([-0.25, 0.2, 0.05])],
                s=[np.array([[-0.2, -0.2, -0.2], [0.2, 0.2, 0.2]]), np.array([[-0.1, -0.1, -0.1], [0.1, 0.1, 0.1]])])


def pick(*names, **renamed):
    """A builder: the named entries of base(), cloned (renamed: argument name = base name)."""
    def build():
        b = base()
        out = {n: b[n].clone() for n in names}
        out.update({k: b[v].clone() for k, v in renamed.items()})
        return out
    return build


def with_none(build, *names):
    def wrapped():
        out = build()
        out.update({n: None for n in names})
        return out
    return wrapped


RAYS3 = [Arg("rays_o", ("R", 3)), Arg("rays_d", ("R", 3)), Arg("viewdirs", ("R", 3))]
RAY_NAMES = ("rays_o", "rays_d", "viewdirs")


def _o(name="rays_o"):
    return Arg(name, ("R", 3))


# ---- ops ------------------------------------------------------------------------------------------------------------------------

record("ops.bbox_intersection_batch", "ops.bbox_intersection_batch", "ops", [_o(), _o("rays_d")], pick("rays_o", "rays_d"),
       lambda env, T: env.ops.bbox_intersection_batch([[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]], T["rays_o"], T["rays_d"]))
record("ops.sample_rays_in_bbox", "ops.sample_rays_in_bbox", "ops", [_o(), _o("view_dirs")], pick("rays_o", view_dirs="viewdirs"),
       lambda env, T: env.ops.sample_rays_in_bbox(rts(), T["rays_o"], T["view_dirs"], return_per_box=True))
record("ops.sample_rays_in_bbox_list", "ops.sample_rays_in_bbox_list", "ops", [_o(), _o("view_dirs")], pick("rays_o", view_dirs="viewdirs"),
       lambda env, T: env.ops.sample_rays_in_bbox_list(rts(), T["rays_o"], T["view_dirs"]))
record("ops.intersect_sphere", "ops.intersect_sphere", "ops", [_o(), _o("rays_d")], pick("rays_o", "rays_d"),
       lambda env, T: env.ops.intersect_sphere(T["rays_o"], T["rays_d"]))
record("ops.pos_enc", "ops.pos_enc", "ops", [Arg("x", ("R", 3), free=True)], pick("x"), lambda env, T: env.ops.pos_enc(T["x"], 0, 4))
record("ops.resample", "ops.resample", "ops", [Arg("t_prev", ("R", "N")), Arg("weights", ("R", "N"))], pick(t_prev="t", weights="w"),
       lambda env, T: env.ops.resample(T["t_prev"], T["weights"], N_FINE))
_COMP = [Arg("rgbsigma", ("R", "N", 4)), Arg("t", ("R", "N")), Arg("rays_d", ("R", 3)), Arg("t_far", ("R",), alts=[("R", 1)])]
record("ops.composite[inside]", "ops.composite", "ops", _COMP, pick("rgbsigma", "t", "rays_d", t_far="far"),
       lambda env, T: env.ops.composite(1, T["rgbsigma"], T["t"], T["rays_d"], T["t_far"], True))
record("ops.composite[vanilla]", "ops.composite", "ops", _COMP[:3], pick("rgbsigma", "t", "rays_d"),
       lambda env, T: env.ops.composite(0, T["rgbsigma"], T["t"], T["rays_d"]))
record("ops.composite[outside]", "ops.composite", "ops", _COMP[:2], pick("rgbsigma", t="s"),
       lambda env, T: env.ops.composite(2, T["rgbsigma"], T["t"]))
record("ops.mip_resample", "ops.mip_resample", "ops", [Arg("s_prev", ("R", "N+1")), Arg("w_prev", ("R", "N"))], pick(s_prev="s1", w_prev="w"),
       lambda env, T: env.ops.mip_resample(T["s_prev"], T["w_prev"], 6, 0.2, 3.0, dilate=True, dilation=0.01, anneal=0.7))
record("ops.mip_composite", "ops.mip_composite", "ops", [Arg("rgbdens", ("R", "N", 4)), Arg("tdist", ("R", "N+1")), Arg("rays_d", ("R", 3))],
       pick("rays_d", rgbdens="rgbsigma", tdist="t1"), lambda env, T: env.ops.mip_composite(T["rgbdens"], T["tdist"], T["rays_d"]))
record("ops.mip_extras", "ops.mip_extras", "ops", [Arg("edges", ("R", "N+1")), Arg("w", ("R", "N"))], pick(edges="t1", w="w"),
       lambda env, T: env.ops.mip_extras(T["edges"], T["w"]))
_EXTRAS = [Arg("fg_t", ("R", "N")), Arg("fg_w", ("R", "N")), Arg("far", ("R",), alts=[("R", 1)]), _o(), _o("rays_d"),
           Arg("bg_s", ("R", "N")), Arg("bg_w", ("R", "N")), Arg("bg_lambda", ("R",), alts=[("R", 1)])]
record("ops.tp_extras", "ops.tp_extras", "ops", _EXTRAS,
       pick("far", "rays_o", "rays_d", fg_t="t", fg_w="w", bg_s="s", bg_w="u", bg_lambda="lam"),
       lambda env, T: env.ops.tp_extras(T["fg_t"], T["fg_w"], T["far"], T["rays_o"], T["rays_d"], T["bg_s"], T["bg_w"], T["bg_lambda"]),
       groups=[("bg_s", "bg_w", "bg_lambda")])
_INST = [Arg("near_inst", ("K", "R"), alts=[("K", "R", 1)]), Arg("far_inst", ("K", "R"), alts=[("K", "R", 1)])]
record("ops.edit_rgbsigma", "ops.edit_rgbsigma", "ops", [Arg("rgbsigma", ("R", "N", 4)), Arg("t", ("R", "N"))] + _INST,
       pick("rgbsigma", "t", "near_inst", "far_inst"),
       lambda env, T: env.ops.edit_rgbsigma(T["rgbsigma"], T["t"], T["near_inst"], T["far_inst"], [0.5, 2.0], [[1.0, 0.5, 0.25], [0.5, 1.0, 1.0]]))
record("ops.decompose_rows", "ops.decompose_rows", "ops",
       [Arg("rgbsigma", ("R", "N", 4)), Arg("t", ("R", "N")), Arg("weights", ("R", "N"))] + _INST + [Arg("bg_lambda", ("R",), alts=[("R", 1)])],
       pick("rgbsigma", "t", "near_inst", "far_inst", weights="w", bg_lambda="lam"),
       lambda env, T: env.ops.decompose_rows(T["rgbsigma"], T["t"], T["weights"], T["near_inst"], T["far_inst"], T["bg_lambda"]))
record("ops.composite_layers", "ops.composite_layers", "ops",
       _COMP + [Arg("key", ("L", "R")), Arg("rgb", ("L", "R", 3)), Arg("acc", ("L", "R")), Arg("depth", ("L", "R"))],
       pick("rgbsigma", "t", "rays_d", "key", t_far="far", rgb="lrgb", acc="lacc", depth="ldepth"),
       lambda env, T: env.ops.composite_layers(T["rgbsigma"], T["t"], T["rays_d"], T["t_far"],
                                               dict(key=T["key"], rgb=T["rgb"], acc=T["acc"], depth=T["depth"])))
record("ops.occupancy_keep", "ops.occupancy_keep", "ops",
       [Arg("occ", (G, G, G), kind="bool", any_device=True), _o(), _o("rays_d"), Arg("t", ("R", "N"))], pick("occ", "rays_o", "rays_d", "t"),
       lambda env, T: env.ops.occupancy_keep(T["occ"], T["rays_o"], T["rays_d"], T["t"]))
record("ops.occupancy_from_sigma", "ops.occupancy_from_sigma", "ops", [Arg("sigma", (G, G, G))], pick("sigma"),
       lambda env, T: env.ops.occupancy_from_sigma(T["sigma"], G, 1.0, probes=1, dilate=0))
record("ops.termination_stops", "ops.termination_stops", "ops",
       [Arg("rgbsigma", ("R", "N", 4)), Arg("t", ("R", "N")), Arg("rays_d", ("R", 3)), Arg("t_far", ("R",), alts=[("R", 1)])],
       pick("rgbsigma", "t", "rays_d", t_far="far"),
       lambda env, T: env.ops.termination_stops(T["rgbsigma"], T["t"], T["rays_d"], T["t_far"], 0.1))
record("ops.termination_stops_outside", "ops.termination_stops_outside", "ops",
       [Arg("rgbsigma", ("R", "N", 4)), Arg("s", ("R", "N")), Arg("bg_lambda", ("R",), alts=[("R", 1)])], pick("rgbsigma", "s", bg_lambda="lam"),
       lambda env, T: env.ops.termination_stops_outside(T["rgbsigma"], T["s"], T["bg_lambda"], 0.1))


def _raygen_out():
    return dict(out_rays_o=torch.zeros(R, 3), out_viewdirs=torch.zeros(R, 3), out_rays_d=torch.zeros(R, 3), out_radii=torch.zeros(R))


record("ops.get_ray_directions_and_rays[out]", "ops.get_ray_directions_and_rays", "ops",
       [Arg("out_rays_o", ("R", 3), role="output"), Arg("out_viewdirs", ("R", 3), role="output"), Arg("out_rays_d", ("R", 3), role="output"),
        Arg("out_radii", ("R",), role="output")], _raygen_out,
       lambda env, T: env.ops.get_ray_directions_and_rays(4, 8, 6.4, env.c2w, ray_range=(5, 5 + R),
                                                          out=(T["out_rays_o"], T["out_viewdirs"], T["out_rays_d"], T["out_radii"])))

# ---- training -------------------------------------------------------------------------------------------------------------------


def _wsum(outs):
    """A scalar over every floating-point output, each with its own fixed fp16-exact weights."""
    total = 0.0
    for i, o in enumerate(x for x in flatten(outs) if x.is_floating_point()):
        wts = q(0.25 + _rand(100 + i, *o.shape)).to(o.device)
        total = total + (o.float() * wts).sum()
    return total


record("training.sample_level0", "training.sample_level0", "training",
       [Arg("far", ("R",), alts=[("R", 1)]), Arg("u_fg", ("R", "N")), Arg("u_bg", ("R", "N"))], pick("far", u_fg="u", u_bg="u2"),
       lambda env, T: env.training.sample_level0(T["far"], N_COARSE, T["u_fg"], T["u_bg"]), groups=[("u_fg", "u_bg")])
record("training.resample_u", "training.resample_u", "training", [Arg("t_prev", ("R", "N")), Arg("weights", ("R", "N")), Arg("u", ("R", "M"))],
       pick(t_prev="t", weights="w", u="u_new"), lambda env, T: env.training.resample_u(T["t_prev"], T["weights"], T["u"]))


def _split_rgbsigma():
    b = base()
    return dict(rgb=b["rgbsigma"][..., :3].clone(), sigma=b["rgbsigma"][..., 3:].clone(), t=b["t"].clone(), rays_d=b["rays_d"].clone(),
                t_far=b["far"].clone())


record("training.composite", "training.composite", "training",
       [Arg("rgb", ("R", "N", 3)), Arg("sigma", ("R", "N", 1), alts=[("R", "N")]), Arg("t", ("R", "N")), Arg("rays_d", ("R", 3)),
        Arg("t_far", ("R",), alts=[("R", 1)])], _split_rgbsigma,
       lambda env, T: env.training.composite(1, T["rgb"], T["sigma"], T["t"], T["rays_d"], T["t_far"], True),
       grad=("rgb", "sigma"), scalar=_wsum)
record("training.composite[packed]", "training.composite", "training", _COMP, pick("rgbsigma", "t", "rays_d", t_far="far"),
       lambda env, T: env.training.composite(1, T["rgbsigma"], None, T["t"], T["rays_d"], T["t_far"], False), grad=("rgbsigma",), scalar=_wsum)
record("training.activate", "training.activate", "training",
       [Arg("raw_rgb", ("P", 3)), Arg("raw_sigma", ("P",), alts=[("P", 1)]), Arg("noise", ("P",), alts=[("P", 1)])],
       pick("raw_rgb", "raw_sigma", "noise"), lambda env, T: env.training.activate(T["raw_rgb"], T["raw_sigma"], T["noise"], 0.5),
       grad=("raw_rgb", "raw_sigma"), scalar=_wsum)
record("training.train_points", "training.train_points", "training",
       [_o(), _o("rays_d"), Arg("tvals", ("R", "N")), Arg("far", ("R",), alts=[("R", 1)]), Arg("src_poses", ("NV", 4, 4))],
       lambda: dict(pick("rays_o", "rays_d", "far", tvals="s")(), src_poses=q(cases.neo_batch({})["src_poses"].float())),
       lambda env, T: env.training.train_points(None, 1, T["rays_o"], T["rays_d"], T["tvals"], T["far"], T["src_poses"]))
record("training.eff_distloss", "training.eff_distloss", "training", [Arg("w", ("R", "N")), Arg("m", ("R", "N"))], pick("w", m="t"),
       lambda env, T: env.training.eff_distloss(T["w"], T["m"], 0.01), grad=("w",), scalar=_wsum)
record("training.mip_resample_u", "training.mip_resample_u", "training",
       [Arg("s_prev", ("R", "N+1")), Arg("w_prev", ("R", "N")), Arg("u", (6,), alts=[(1, 6)]), Arg("jitter", ("R", 1), alts=[("R",)])],
       lambda: dict(pick(s_prev="s1", w_prev="w")(), u=q(torch.linspace(1 / 12, 11 / 12, 6)), jitter=q(0.01 * _rand(20, R, 1))),
       lambda env, T: env.training.mip_resample_u(T["s_prev"], T["w_prev"], 6, 0.2, 3.0, True, 0.01, 0.7, T["u"], T["jitter"]))
record("training.mip_encode", "training.mip_encode", "training",
       [_o(), _o("rays_d"), Arg("radii", ("R", 1), alts=[("R",), (1, "R")]), Arg("tdist", ("R", "N+1")), Arg("pos_basis_t", (3, 21))],
       lambda: dict(pick("rays_o", "rays_d", "radii", tdist="tdist_mip")(), pos_basis_t=q(_basis())),
       lambda env, T: env.training.mip_encode(T["rays_o"], T["rays_d"], T["radii"], T["tdist"], T["pos_basis_t"]))
record("training.mip_composite", "training.mip_composite", "training",
       [Arg("rgb", ("R", "N", 3)), Arg("density", ("R", "N")), Arg("tdist", ("R", "N+1")), Arg("rays_d", ("R", 3))],
       lambda: dict(rgb=base()["rgbsigma"][..., :3].clone(), density=base()["rgbsigma"][..., 3].clone(), tdist=base()["t1"].clone(),
                    rays_d=base()["rays_d"].clone()),
       lambda env, T: env.training.mip_composite(T["rgb"], T["density"], T["tdist"], T["rays_d"], 1.0), grad=("rgb", "density"), scalar=_wsum)
record("training.lossfun_outer", "training.lossfun_outer", "training",
       [Arg("t", ("R", "N+1")), Arg("w", ("R", "N")), Arg("t_env", ("R", "M+1")), Arg("w_env", ("R", "M"))], pick("w", "t_env", "w_env", t="s1"),
       lambda env, T: env.training.lossfun_outer(T["t"], T["w"], T["t_env"], T["w_env"]), grad=("w", "w_env"), scalar=_wsum)
record("training.lossfun_distortion", "training.lossfun_distortion", "training", [Arg("t", ("R", "N+1")), Arg("w", ("R", "N"))], pick("w", t="s1"),
       lambda env, T: env.training.lossfun_distortion(T["t"], T["w"]), grad=("w",), scalar=_wsum)
record("training.mip_expected_distance", "training.mip_expected_distance", "training", [Arg("edges", ("R", "N+1")), Arg("w", ("R", "N"))],
       pick("w", edges="t1"), lambda env, T: env.training.mip_expected_distance(T["edges"], T["w"]), grad=("w",), scalar=_wsum)


def _basis():
    from neo360_amd import geopoly
    return geopoly.icosahedron_basis().float()


# ---- modules --------------------------------------------------------------------------------------------------------------------


def _batch(env, T, extra=None):
    b = dict(extra if extra is not None else env.src)
    b.update({k: T[k] for k in RAY_NAMES})
    return b


_RAYS = pick(*RAY_NAMES)
_INST_RAYS = pick("near_inst", "far_inst", *RAY_NAMES)


def _module(name, method, family, call, args=RAYS3, build=_RAYS, **kw):
    return record("models.%s.%s" % (name, method), "models.%s.%s" % (name, method.partition("[")[0]), family, args, build, call, together=RAY_NAMES, **kw)


_module("NeRF", "forward", "vanilla", lambda env, T: env.nerf(_batch(env, T, {}), False, True, 0.2, 3.0))
_module("NeRF", "eval_mlp", "vanilla", lambda env, T: env.nerf.eval_mlp(1, T["rays_o"], T["dirs"], T["t"]),
        args=[_o(), _o("dirs"), Arg("t", ("R", "N"))], build=pick("rays_o", "t", dirs="viewdirs")).together = ("rays_o", "dirs")
_module("NeRF_TP", "forward[eval]", "neo360", lambda env, T: env.tp(_batch(env, T), False, False, 0.0, 0.0, out_depth=True))
_module("NeRF_TP", "forward[train]", "neo360", lambda env, T: env.tp(_batch(env, T), False, True, 0.0, 0.0))
_module("NeRF_TP", "sample_positions", "neo360", lambda env, T: env.tp.sample_positions(_batch(env, T)))
_module("NeRF_TP", "eval_mlp[inside]", "neo360", lambda env, T: env.tp.eval_mlp(1, _batch(env, T), T["tvals"]),
        args=RAYS3 + [Arg("tvals", ("R", "N"))], build=pick(*RAY_NAMES, tvals="t"))
_module("NeRF_TP", "eval_mlp[outside]", "neo360", lambda env, T: env.tp.eval_mlp(2, _batch(env, T), T["tvals"], T["far"]),
        args=RAYS3 + [Arg("tvals", ("R", "N")), Arg("far", ("R",), alts=[("R", 1)])], build=pick("far", *RAY_NAMES, tvals="s"))
_module("NeRF_TP", "render_objects", "neo360",
        lambda env, T: env.tp.render_objects(_batch(env, T), T["near_obj"], T["far_obj"], return_samples=True),
        args=RAYS3 + [Arg("near_obj", ("R",), alts=[("R", 1)]), Arg("far_obj", ("R",), alts=[("R", 1)])],
        build=lambda: dict(_RAYS(), near_obj=base()["near_inst"][0].clone(), far_obj=base()["far_inst"][1].clone()))
_module("NeRF_TP", "render_instances", "neo360", lambda env, T: env.tp.render_instances(_batch(env, T), T["near_inst"], T["far_inst"]),
        args=RAYS3 + _INST, build=_INST_RAYS)
_module("NeRF_TP", "render_edited", "neo360",
        lambda env, T: env.tp.render_edited(_batch(env, T), T["near_inst"], T["far_inst"], [0.5, 2.0], [[1.0, 0.5, 0.25], [0.5, 1.0, 1.0]]),
        args=RAYS3 + _INST, build=_INST_RAYS)
_module("NeRF_TP", "render_decomposed", "neo360", lambda env, T: env.tp.render_decomposed(_batch(env, T), T["near_inst"], T["far_inst"]),
        args=RAYS3 + _INST, build=_INST_RAYS)
_module("NeRF_TP", "render_skipping", "neo360", lambda env, T: env.tp.render_skipping(_batch(env, T), return_samples=True))
_module("NeRF_TP", "render_terminating", "neo360", lambda env, T: env.tp.render_terminating(_batch(env, T), 0.05, return_samples=True))
_module("NeRF_TP", "render_accelerated", "neo360", lambda env, T: env.tp.render_accelerated(_batch(env, T), 0.05, return_samples=True))
_module("NeRF_TP", "render_marching", "neo360", lambda env, T: env.tp.render_marching(_batch(env, T), 0.05, return_samples=True))
_module("PixelNeRF", "forward", "pixelnerf", lambda env, T: env.pix(_batch(env, T), False, True, 0.2, 3.0))
_module("PixelNeRF", "eval_mlp", "pixelnerf", lambda env, T: env.pix.eval_mlp(1, _batch(env, T), T["tvals"]),
        args=RAYS3 + [Arg("tvals", ("R", "N"))], build=pick(*RAY_NAMES, tvals="t"))
_MIP = RAYS3 + [Arg("radii", ("R", 1), alts=[("R",), (1, "R")])]
_module("MipNeRF360", "forward", "mip360", lambda env, T: env.mip(dict(_batch(env, T, {}), radii=T["radii"]), 1.0, False, False, 0.2, 3.0),
        args=_MIP, build=pick("radii", *RAY_NAMES))
_module("MipNeRF360", "eval_mlp", "mip360", lambda env, T: env.mip.eval_mlp(2, dict(_batch(env, T, {}), radii=T["radii"]), T["tdist"]),
        args=_MIP + [Arg("tdist", ("R", "N+1"))], build=pick("radii", *RAY_NAMES, tdist="tdist_mip"))


# ---- the training drivers, reached as the modules reach them: a forward with autograd on -------------------------------------------

def _driver(name, family, net, unordered, call, args=RAYS3, build=_RAYS):
    return record("training.%s" % name, "training.%s" % name, family, args, build, call, scalar=_wsum, together=RAY_NAMES,
                  chain=(net, tuple(unordered)))


# The weight gradients of the chains are sums over rows in a fixed order at these sizes (train_mlp.hip: dw_gemm cuts K into slices
# of >= 1024 rows, k_dw_reduce adds up to 16 slices per element in one thread, in slice order, and adds the sum to the zeroed
# gradient once; every record here has fewer than 17 x 1024 rows).  What is NOT in a fixed order is the scatter-add of the lookups'
# backward (training.hip: one atomicAdd per tap and point into the map gradient, workgroups in any order): the gradient of a
# projected map, and with it the weight columns that made the map - pts_linears.0 (and .3, the skip) of the decoders that read
# the latent through project_latent_all / project_pixel_latent.
_driver("nerf_render_train", "vanilla", "nerf", (), lambda env, T: env.nerf(_batch(env, T, {}), False, True, 0.2, 3.0))
_driver("pix_render_train", "pixelnerf", "pix", ("pts_linears.0.weight",), lambda env, T: env.pix(_batch(env, T), False, True, 0.2, 3.0))
_driver("tp_render_train", "neo360", "tp", ("pts_linears.0.weight", "pts_linears.3.weight"), lambda env, T: env.tp(_batch(env, T), False, True, 0.0, 0.0))
_driver("mip_render_train", "mip360", "mip", (), lambda env, T: env.mip(dict(_batch(env, T, {}), radii=T["radii"]), 1.0, False, False, 0.2, 3.0),
        args=_MIP, build=pick("radii", *RAY_NAMES))
record("training.channels_last_rows", "training.channels_last_rows", "training", [Arg("map", (2, 8, 3, 5), free=True)],
       lambda: dict(map=q(_rand(30, 2, 8, 3, 5))), lambda env, T: env.training.channels_last_rows(T["map"]), grad=("map",), scalar=_wsum)

# ---- the GEMM operators, the projections and the lookups on caller rows ---------------------------------------------------------------

record("training.linear", "training.linear", "training", [Arg("x", ("T", "I")), Arg("W", ("O", "I")), Arg("b", ("O",))],
       lambda: dict(x=q(_rand(31, 10, 12) - 0.5), W=q(_rand(32, 8, 12) - 0.5), b=q(_rand(33, 8) - 0.5)),
       lambda env, T: env.training.linear(T["x"], T["W"], T["b"], relu=True), grad=("x", "W", "b"), scalar=_wsum)
record("training.weight_grad", "training.weight_grad", "training", [Arg("gy", ("R", "O")), Arg("x", ("R", "I"))],
       lambda: dict(gy=q(_rand(34, R, 8) - 0.5), x=q(_rand(35, R, 12) - 0.5)),
       lambda env, T: env.training.weight_grad(T["gy"], T["x"], bias=True))
# the projections are `linear` on a block of the decoder's first layer: their row argument is linear's `x`
_LATENT_ROWS = [Arg("x", ("T", 512))]
record("training.project_latent", "training.project_latent", "training", _LATENT_ROWS, lambda: dict(x=q(_rand(36, 10, 512) - 0.5)),
       lambda env, T: env.training.project_latent(env.tp.fg_coarse_mlp, T["x"]), grad=("x",), scalar=_wsum)
record("training.project_latent_all", "training.project_latent_all", "training", _LATENT_ROWS, lambda: dict(x=q(_rand(36, 10, 512) - 0.5)),
       lambda env, T: env.training.project_latent_all([env.tp.fg_coarse_mlp, env.tp.fg_fine_mlp], T["x"])[0], grad=("x",), scalar=_wsum)
record("training.project_pixel_latent", "training.project_pixel_latent", "training", _LATENT_ROWS, lambda: dict(x=q(_rand(36, 10, 512) - 0.5)),
       lambda env, T: env.training.project_pixel_latent(env.pix.coarse_mlp, T["x"]), grad=("x",), scalar=_wsum)


def _pts():
    return dict(pts=q(1.2 * _rand(37, R * N0, 3) - 0.6))


def _maps(env):
    return tuple(env.scene[k] for k in ("plane_xz", "plane_xy", "plane_yz", "latent"))


# the lookups' gradients go to the maps through the scatter-add above: outputs only
record("training.gather_features", "training.gather_features", "training", [Arg("pts", ("P", 3))], _pts,
       lambda env, T: env.training.gather_features(env.tp, T["pts"], *_maps(env), env.src))
record("training.gather_planes", "training.gather_planes", "training", [Arg("pts", ("P", 3))], _pts,
       lambda env, T: env.training.gather_planes(env.tp, T["pts"], *_maps(env), env.src))


def _latent_rows():
    if "latent_rows" not in _cache:
        base()
        _cache["latent_rows"] = q(cases.small_scene()["latent"].permute(0, 2, 3, 1).reshape(-1, 512).contiguous())
    return _cache["latent_rows"].clone()


_TEXELS = NV * cases.LATENT_HW[0] * cases.LATENT_HW[1]
record("training.gather_map", "training.gather_map", "training", [Arg("map", (_TEXELS, 512)), Arg("pts", ("P", 3))],
       lambda: dict(_pts(), map=_latent_rows()), lambda env, T: env.training.gather_map(env.tp, T["map"], T["pts"], env.src))

# ---- the MLP chains on caller rows: Q = 4 points seen by NV = 3 views (Y = NV Q view-major rows); 7 rays of 4 samples for the others --

def _rows(seed, *shape):
    return q(_rand(seed, *shape) - 0.5)


_XE = Arg("x_enc", ("NV", "Q", 63))
_COND = Arg("cond_rows", ("Y", 27))
record("training.nerfpp_mlp", "training.nerfpp_mlp", "training",
       [_XE, _COND, Arg("world_feat", ("Y", 128)), Arg("local_feat", ("Y", 512))],
       lambda: dict(x_enc=_rows(40, NV, 4, 63), cond_rows=_rows(41, 12, 27), world_feat=_rows(42, 12, 128), local_feat=_rows(43, 12, 512)),
       lambda env, T: env.training.nerfpp_mlp(env.tp.fg_coarse_mlp, T["x_enc"], T["cond_rows"], T["world_feat"], T["local_feat"], NV),
       grad=("x_enc", "world_feat", "local_feat"), scalar=_wsum)
record("training.nerfpp_mlp_projected", "training.nerfpp_mlp_projected", "training",
       [_XE, _COND, Arg("world_feat", ("Y", 128)), Arg("pre", ("Y", 256))],
       lambda: dict(x_enc=_rows(40, NV, 4, 63), cond_rows=_rows(41, 12, 27), world_feat=_rows(42, 12, 128), pre=_rows(44, 12, 256)),
       lambda env, T: env.training.nerfpp_mlp_projected(env.tp.fg_coarse_mlp, T["x_enc"], T["cond_rows"], T["world_feat"], T["pre"], NV),
       grad=("x_enc", "world_feat", "pre"), scalar=_wsum)
record("training.nerf_mlp", "training.nerf_mlp", "training", [Arg("x_enc", ("R", "N", 63)), Arg("dir_enc", ("R", 27))],
       lambda: dict(x_enc=_rows(45, R, N0, 63), dir_enc=_rows(46, R, 27)),
       lambda env, T: env.training.nerf_mlp(env.nerf.coarse_mlp, T["x_enc"], T["dir_enc"]), grad=("x_enc", "dir_enc"), scalar=_wsum)
for _f in ("pixel_mlp_fused", "pixel_mlp_projected"):
    record("training.%s" % _f, "training.%s" % _f, "training", [_XE, _COND, Arg("pre", ("Y", 128))],
           lambda: dict(x_enc=_rows(40, NV, 4, 63), cond_rows=_rows(41, 12, 27), pre=_rows(47, 12, 128)),
           lambda env, T, _f=_f: getattr(env.training, _f)(env.pix.coarse_mlp, T["x_enc"], T["cond_rows"], T["pre"], NV),
           grad=("x_enc", "pre"), scalar=_wsum)
# the fused Mip-NeRF 360 chain returns no input gradients (its parameters' are compared under mip_render_train): outputs only
record("training.mip_mlp", "training.mip_mlp", "training", [Arg("x0", ("P", 504)), Arg("d_enc", ("R", 27))],
       lambda: dict(x0=_rows(48, R * N0, 504), d_enc=_rows(49, R, 27)),
       lambda env, T: env.training.mip_mlp(env.mip.mlps[2], T["x0"], T["d_enc"], N0), grad=("x0", "d_enc"), scalar=_wsum, ties=("R",))
record("training.mip_mlp_fused", "training.mip_mlp_fused", "training", [Arg("x0", ("P", 504)), Arg("d_enc", ("R", 27))],
       lambda: dict(x0=_rows(48, R * N0, 504), d_enc=_rows(49, R, 27)),
       lambda env, T: env.training.mip_mlp_fused(env.mip.mlps[2], T["x0"], T["d_enc"], N0), ties=("R",))

# ---- GridEncoder: the pillar stage at grid (5, 7, 3); the cameras are read on the host and may live anywhere ---------------------------

PILLAR_GRID = (5, 7, 3)
_PILLAR = [Arg("latent", ("NV", 512, "HF", "WF")), Arg("poses", ("NV", 4, 4), any_device=True), Arg("focal", ("NV",), any_device=True),
           Arg("c", ("NV", 2), any_device=True)]


def _pillar_inputs():
    if "pillar" not in _cache:
        base()
        poses, focal, centre = cases.neo_batch({})["src_poses"], cases.neo_batch({})["src_focal"], cases.neo_batch({})["src_c"]
        _cache["pillar"] = dict(latent=q(cases.small_scene()["latent"]), poses=q(poses.float()), focal=q(focal.float()), c=q(centre.float()))
    return {k: v.clone() for k, v in _cache["pillar"].items()}


# floorplans_train is the same forward under autograd; its backward scatters the latent's gradient with atomics (pillar_train.hip),
# in no fixed order: outputs only
for _m in ("floorplans", "floorplans_train"):
    record("encoder.GridEncoder.%s" % _m, "encoder.GridEncoder.%s" % _m, "encoder", _PILLAR, _pillar_inputs,
           lambda env, T, _m=_m: getattr(env.enc, _m)(T["latent"], T["poses"], T["focal"], T["c"], env.scene["image_wh"]))

def _encoder_forward(env, T):
    """GridEncoder.forward, compared on what this library computes in it: the three floor-plans as they enter the torch
    convolutions.  The convolutions behind them are the backend's, not this library's, and two identical dense calls differ there
    by 2e-6 on the MI355X, so the planes they return cannot be held to a bitwise bound; their shapes are returned instead."""
    enc, seen = env.enc_full, []
    hooks = [m.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].contiguous()))
             for m in (enc.floorplan_convnet_xz, enc.floorplan_convnet_xy, enc.floorplan_convnet_yz)]
    try:
        planes = enc(T["images"], T["poses"], T["focal"], T["c"])
    finally:
        for h in hooks:
            h.remove()
    assert len(seen) == 3
    return seen, torch.tensor([list(p.shape) for p in planes])


# forward = a spatial encoder (here env.enc_full's stand-in, which emits the scene's latent) + the pillar stage + torch convolutions
record("encoder.GridEncoder.forward", "encoder.GridEncoder.forward", "encoder",
       [Arg("images", ("NV", 3, 6, 8), free=True)] + _PILLAR[1:],
       lambda: dict({k: v for k, v in _pillar_inputs().items() if k != "latent"}, images=q(_rand(50, NV, 3, 6, 8))),
       lambda env, T: _encoder_forward(env, T))

# ---- render.py: the frame helpers slice a batch and hand it to the module calls above -----------------------------------------------


def _frame(helper, call, args=RAYS3, build=_RAYS):
    return record("render.%s" % helper, "render.%s" % helper.partition("[")[0], "render", args, build, call, together=RAY_NAMES)


_frame("render_rays_test[NeRF_TP]", lambda env, T: env.render.render_rays_test(env.tp, _batch(env, T), chunk=4))
_frame("render_rays_test[MipNeRF360]", lambda env, T: env.render.render_rays_test(env.mip, dict(_batch(env, T, {}), radii=T["radii"])),
       args=_MIP, build=pick("radii", *RAY_NAMES))
_frame("render_frame_sharded", lambda env, T: env.render.render_frame_sharded(env.tp, _batch(env, T), 1, 0, chunk=4))
_frame("render_object_rays", lambda env, T: env.render.render_object_rays(env.tp, dict(_batch(env, T), near_obj=T["near_obj"], far_obj=T["far_obj"])),
       args=RAYS3 + [Arg("near_obj", ("R",), alts=[("R", 1)]), Arg("far_obj", ("R",), alts=[("R", 1)])],
       build=lambda: dict(_RAYS(), near_obj=base()["near_inst"][0].clone(), far_obj=base()["far_inst"][1].clone()))
for _h in ("render_instance_rays", "render_edited_rays", "render_decomposed_rays"):
    _frame(_h, lambda env, T, _h=_h: getattr(env.render, _h)(env.tp, dict(_batch(env, T), near_inst=T["near_inst"], far_inst=T["far_inst"])),
           args=RAYS3 + _INST, build=_INST_RAYS)
_frame("instance_layers", lambda env, T: env.render.instance_layers(
    env.tp, _batch(env, T), rts(), {1: [[1.0, 0.0, 0.0, 0.05], [0.0, 1.0, 0.0, -0.1], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]}))
_frame("render_skipping_rays", lambda env, T: env.render.render_skipping_rays(env.tp, _batch(env, T)))
for _h in ("render_terminating_rays", "render_accelerated_rays", "render_marching_rays"):
    _frame(_h, lambda env, T, _h=_h: getattr(env.render, _h)(env.tp, _batch(env, T), 0.05))


# Public entry points without a record, each with its reason: nothing of the tensor contract applies to them.
EXEMPT = {
    "models.NeRF_TP.build_occupancy": "reads only the device of rays['rays_o'] and the source cameras (host copies); the lattice it "
                                      "evaluates is its own, through eval_mlp and occupancy_from_sigma, which have records",
    "render.psnr": "plain torch on two images; no library call",
    "parallel.shard_counts": "integers in, integers out", "parallel.shard_bounds": "integers in, integers out",
    "parallel.clear_buffers": "takes no argument that is a tensor: drops the cached exchange buffers",
    "parallel.ray_patch_order": "integers in, a LongTensor of its own out (host mirror of the device's ray order)",
    "ops.edit_table": "host sequences or CPU tensors -> ctypes arrays; never touches a device pointer (tests/test_edit_cpu.py)",
    "ops.occupancy_resolution_ok": "a predicate on an int",
    "ops.pack_occupancy": "plain torch on the caller's device, no library call; .contiguous() before the reshape (tests/test_occupancy_cpu.py)",
    "ops.unpack_occupancy": "plain torch, no library call",
    "ops.occupancy_lattice": "takes no tensor",
    "training.rand_uniform": "takes no tensor",
    "training.shared_grad_group": "autograd bookkeeping on tensor identities; no pointer is read",
    "training.shared_grad_buffers": "autograd bookkeeping; no pointer is read",
    "training.mip_interlevel_loss": "torch.mean over lossfun_outer, which has a record",
    "training.mip_distortion_loss": "torch.mean over lossfun_distortion, which has a record",
    "training.mip_training_loss": "plain torch over the two losses above",
    "models.NeRF_TP.scene_matches": "compares tensor identities and versions; no pointer is read",
    "models.NeRF_TP.scene_image_wh": "reads a shape",
    "models.NeRF_TP.set_scene": "module state: tests/test_gpu_boundary_sweep.py::test_set_scene_* (layouts, dtypes, mismatches)",
    "models.PixelNeRF.set_scene": "module state: tests/test_gpu_boundary_sweep.py::test_pixelnerf_set_scene_layouts",
    "models.NeRF_TP.set_occupancy": "module state: tests/test_gpu_boundary_sweep.py::test_occupancy_grid_from_strided_bool_tensors_and_uint8_refused",
    "parallel.gather_tiles": "needs a process group: tests/test_parallel_cpu.py, tests/test_gpu_multirank.py; the `out=` refusals are in "
                             "tests/test_boundary_cases_cpu.py::test_gather_tiles_refuses_a_foreign_out",
    "parallel.alter_gather_cat": "torch.cat + one collective on .contiguous() rows; no library pointer",
}
DEFERRED = {}       # every entry the contract applies to has a record


# ---- helpers shared by the two test files ------------------------------------------------------------------------------------------

def flatten(x):
    """Every tensor of a nested result, in a fixed order."""
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in flatten(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in flatten(v)]
    return []


# ---- layout variants ----------------------------------------------------------------------------------------------------------------

def _column_slice(x):
    if x.dim() == 1:
        wide = torch.zeros(x.shape[0], 2, dtype=x.dtype, device=x.device)
        wide[:, 0] = x
        return wide[:, 0]
    wide = torch.zeros(*x.shape[:-1], x.shape[-1] + 2, dtype=x.dtype, device=x.device)
    wide[..., 1:-1] = x
    return wide[..., 1:-1]


def _transposed(x):
    if x.dim() < 2:
        return None
    if x.dim() == 2:
        return x.t().contiguous().t()
    back = (x.dim() - 1,) + tuple(range(x.dim() - 1))             # channels-first allocation of a channels-last tensor
    there = tuple(range(1, x.dim())) + (0,)
    return x.permute(*back).contiguous().permute(*there)


def _stride0(x):
    return x[:1].expand(x.shape) if x.dim() >= 1 and x.shape[0] > 1 else None


def _misaligned(x):
    buf = torch.zeros(x.numel() + 8, dtype=x.dtype, device=x.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    return v


LAYOUTS = {
    "column_slice": (_column_slice, lambda v: not v.is_contiguous()),
    "transposed": (_transposed, lambda v: not v.is_contiguous()),
    "stride0": (_stride0, lambda v: 0 in v.stride()),
    "misaligned": (_misaligned, lambda v: v.is_contiguous() and v.data_ptr() % 16 == v.element_size()),
    "float64": (lambda x: x.double(), lambda v: v.dtype == torch.float64),
    "float16": (lambda x: x.half(), lambda v: v.dtype == torch.float16),
}
VIEWS = ("column_slice", "transposed", "stride0", "misaligned")


def _variant(arg, x, layout):
    """The `layout` variant of the dense tensor x of `arg`, or None where it does not apply (a dtype copy outside the contract;
    a view that cannot have the property at this shape, e.g. the transposed storage of an (R,1) column, which is dense)."""
    if x is None or (layout in ("float64", "float16") and not arg.copies):
        return None
    make, has = LAYOUTS[layout]
    v = make(x)
    return v if v is not None and has(v) else None


def layout_variants(rec, dev="cpu"):
    """Yields (case id, argument name or "together", layout, T, twin): T holds the variant, twin the dense fp32 tensors of the same
    values (the materialised copy for a stride-0 argument); the other arguments are the SAME dense tensors in both."""
    dense = {k: (v.to(dev) if v is not None else None) for k, v in rec.build().items()}
    for layout in LAYOUTS:
        for group in [(a.name,) for a in rec.args] + ([rec.together] if rec.together and layout in VIEWS + ("float64",) else []):
            T, twin, hit = dict(dense), dict(dense), False
            for name in group:
                arg = rec.arg(name)
                if arg.kind != "float" and layout in ("float64", "float16"):
                    continue
                v = _variant(arg, dense[name], layout)
                if v is None:
                    continue
                hit = True
                T[name] = v
                twin[name] = v.contiguous() if layout == "stride0" else dense[name]
            if hit:
                who = group[0] if len(group) == 1 else "together"
                yield "%s/%s/%s" % (rec.name, who, layout), who, layout, T, twin


# ---- mismatch variants --------------------------------------------------------------------------------------------------------------

def _shared_symbols(rec):
    """Symbols that tie two arguments together: changing one of these extents in ONE argument is a mismatch."""
    count = {}
    for a in rec.args:
        for s in {symbol(e) for e in a.shape} - {None}:
            count[s] = count.get(s, 0) + 1
    return {s for s, n in count.items() if n > 1} | set(rec.ties)


def _accepted(arg, shape):
    return any(resolve(s) == tuple(shape) for s in (arg.shape,) + arg.alts)


def _bad_shapes(rec, arg):
    """(kind, shape) of every wrong shape of one argument."""
    if arg.free:
        return []
    true = resolve(arg.shape)
    shared = _shared_symbols(rec)
    out = []
    for i, e in enumerate(arg.shape):
        if symbol(e) == "R" and "R" in shared:
            out += [("rows-1", true[:i] + (true[i] - 1,) + true[i + 1:]), ("rows+1", true[:i] + (true[i] + 1,) + true[i + 1:])]
    last = arg.shape[-1]
    if isinstance(last, int) or (symbol(last) in shared and symbol(last) != "R"):
        out += [("last-1", true[:-1] + (true[-1] - 1,)), ("last+1", true[:-1] + (true[-1] + 1,))]
    out += [("rank-1", true[:-1]), ("rank+1", true + (2,))]
    seen, keep = set(), []
    for kind, shape in out:
        if shape not in seen and not _accepted(arg, shape) and all(e >= 0 for e in shape):
            seen.add(shape)
            keep.append((kind, shape))
    return keep


_DTYPE = {"float": torch.float32, "int": torch.int32, "bool": torch.bool}


def backing_numel(arg):
    """Elements of the allocation behind every view of `arg` in a mismatch case: every extent of its largest accepted shape plus
    one, times two for the extra dimension of the rank+1 variant."""
    return 2 * max(math.prod(e + 1 for e in resolve(s)) for s in (arg.shape,) + arg.alts)


def _leading_view(arg, x, shape, dtype, dev):
    """A contiguous view of `shape` at offset 0 of a fresh allocation of backing_numel(arg) elements, holding x where it fits."""
    buf = torch.zeros(backing_numel(arg), dtype=dtype, device=dev)
    v = buf[:math.prod(shape)].view(shape)
    if x is not None and len(shape) == x.dim():
        idx = tuple(slice(0, min(a, b)) for a, b in zip(shape, x.shape))
        v[idx] = x[idx].to(device=dev, dtype=dtype)
    elif x is not None and v.numel():
        flat = x.reshape(-1)[:v.numel()].to(device=dev, dtype=dtype)
        v.reshape(-1)[:flat.numel()] = flat
    return v


def mismatch_variants(rec, dev="cpu"):
    """Yields (case id, argument name, kind, T).  T[name] is wrong in exactly the way `kind` says, everything else is right, and
    every tensor is a leading view of its own backing allocation (see the module docstring)."""
    dense = rec.build()

    def good(skip=None):
        return {a.name: (None if dense[a.name] is None else
                         _leading_view(a, dense[a.name], tuple(dense[a.name].shape), dense[a.name].dtype, dev))
                for a in rec.args if a.name != skip}

    for arg in rec.args:
        x = dense[arg.name]
        if x is None:
            continue
        bad = [(kind, shape, x.dtype, dev) for kind, shape in _bad_shapes(rec, arg)]
        other = torch.int32 if arg.kind == "float" else torch.float32
        bad.append(("dtype", tuple(x.shape), other, dev))
        if not arg.any_device and str(dev) != "cpu":
            bad.append(("cpu", tuple(x.shape), x.dtype, "cpu"))
        for kind, shape, dtype, where in bad:
            T = good(arg.name)
            T[arg.name] = _leading_view(arg, x, shape, dtype, where)
            yield "%s/%s/%s" % (rec.name, arg.name, kind), arg.name, kind, T
    for group in rec.groups:
        for name in group:
            T = good()
            T[name] = None
            yield "%s/%s/missing" % (rec.name, name), name, "missing", T


# Mismatch cases whose message names, instead of the varied argument, the tensor that was checked against it: case id -> that
# argument.  In each of them the varied argument is the one the call takes its sizes (or its device) from.
_NAMED_INSTEAD = {      # (record, varied argument): {argument named instead: the kinds of mismatch it is named for}
    ("models.MipNeRF360.eval_mlp", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.MipNeRF360.forward", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF.eval_mlp", "rays_o"): {"dirs": "rows+1 rows-1"},
    ("models.NeRF.forward", "rays_o"): {"viewdirs": "rows+1 rows-1"},
    ("models.NeRF_TP.eval_mlp[inside]", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF_TP.eval_mlp[outside]", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF_TP.forward[eval]", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF_TP.forward[train]", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF_TP.render_accelerated", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF_TP.render_decomposed", "rays_o"): {"near_inst": "cpu rows+1 rows-1"},
    ("models.NeRF_TP.render_edited", "rays_o"): {"near_inst": "cpu rows+1 rows-1"},
    ("models.NeRF_TP.render_instances", "rays_o"): {"near_inst": "cpu rows+1 rows-1"},
    ("models.NeRF_TP.render_marching", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF_TP.render_objects", "rays_o"): {"near_obj": "rows+1 rows-1"},
    ("models.NeRF_TP.render_skipping", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF_TP.render_terminating", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.NeRF_TP.sample_positions", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.PixelNeRF.eval_mlp", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("models.PixelNeRF.forward", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("ops.bbox_intersection_batch", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("ops.composite[inside]", "t"): {"rgbsigma": "last+1 last-1 rows+1 rows-1"},
    ("ops.composite[outside]", "t"): {"rgbsigma": "last+1 last-1 rows+1 rows-1"},
    ("ops.composite[vanilla]", "t"): {"rgbsigma": "last+1 last-1 rows+1 rows-1"},
    ("ops.composite_layers", "t"): {"key": "cpu rows+1 rows-1", "rgbsigma": "last+1 last-1"},
    ("ops.decompose_rows", "t"): {"rgbsigma": "last+1 last-1 rows+1 rows-1"},
    ("ops.intersect_sphere", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("ops.mip_composite", "tdist"): {"rgbdens": "last+1 last-1 rows+1 rows-1"},
    ("ops.mip_resample", "w_prev"): {"s_prev": "last+1 last-1 rows+1 rows-1"},
    ("ops.resample", "t_prev"): {"weights": "last+1 last-1 rows+1 rows-1"},
    ("ops.sample_rays_in_bbox", "rays_o"): {"view_dirs": "rows+1 rows-1"},
    ("ops.sample_rays_in_bbox_list", "rays_o"): {"view_dirs": "rows+1 rows-1"},
    ("ops.tp_extras", "fg_t"): {"fg_w": "last+1 last-1 rows+1 rows-1"},
    ("render.render_accelerated_rays", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("render.render_decomposed_rays", "rays_o"): {"near_inst": "cpu rows+1 rows-1"},
    ("render.render_edited_rays", "rays_o"): {"near_inst": "cpu rows+1 rows-1"},
    ("render.render_instance_rays", "rays_o"): {"near_inst": "cpu rows+1 rows-1"},
    ("render.render_marching_rays", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("render.render_object_rays", "rays_o"): {"near_obj": "rows+1 rows-1"},
    ("render.render_rays_test[MipNeRF360]", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("render.render_rays_test[NeRF_TP]", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("render.render_skipping_rays", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("render.render_terminating_rays", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("training.composite", "t"): {"rgb": "last+1 last-1 rows+1 rows-1"},
    ("training.composite[packed]", "t"): {"rgbsigma": "last+1 last-1 rows+1 rows-1"},
    ("training.eff_distloss", "w"): {"m": "last+1 last-1 rank+1 rank-1 rows+1 rows-1"},
    ("training.mip_composite", "tdist"): {"rgb": "last+1 last-1 rows+1 rows-1"},
    ("training.mip_encode", "tdist"): {"rays_o": "rows+1 rows-1"},
    ("training.mip_render_train", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("training.mip_resample_u", "w_prev"): {"s_prev": "last+1 last-1 rows+1 rows-1"},
    ("training.nerf_render_train", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("training.pix_render_train", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("training.resample_u", "t_prev"): {"weights": "last+1 last-1 rows+1 rows-1"},
    ("training.sample_level0", "far"): {"u_fg": "rows+1 rows-1"},
    ("training.tp_render_train", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("render.instance_layers", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("render.render_frame_sharded", "rays_o"): {"rays_d": "rows+1 rows-1"},
    ("training.train_points", "rays_o"): {"rays_d": "rows+1 rows-1"},
}
NAMED_INSTEAD = {"%s/%s/%s" % (rec, who, kind): other for (rec, who), d in _NAMED_INSTEAD.items() for other, kinds in d.items()
                 for kind in kinds.split()}
