"""CPU half of the boundary sweep: the case table is complete and means what it says, and the contract helper
(`context.dense`, `context.owned_output`, `context.f32`) behaves as specified - its shape, dtype and alignment logic runs on CPU
tensors with the device requirement switched off.  The GPU half is tests/test_gpu_boundary_sweep.py."""
import inspect
import math

import pytest
import torch

import boundary_cases as B
from neo360_amd import _lib, context, encoder, models, ops, parallel, training

dense, owned = context.dense, context.owned_output


# ---- the registry ---------------------------------------------------------------------------------------------------------------

def _public_functions(mod, name):
    return {"%s.%s" % (name, k) for k, v in vars(mod).items()
            if not k.startswith("_") and inspect.isfunction(v) and v.__module__ == mod.__name__}


def _public_methods(cls, path):
    """The public methods a class itself (or a project base class) defines that take an argument besides self."""
    own = {}
    for klass in cls.__mro__:
        if klass.__module__.startswith("neo360_amd"):
            for k, v in vars(klass).items():
                own.setdefault(k, v)
    out = set()
    for k, v in own.items():
        f = v.__func__ if isinstance(v, (staticmethod, classmethod)) else v
        if k.startswith("_") and k != "__call__" or not inspect.isfunction(f):
            continue
        if len([p for p in inspect.signature(f).parameters.values() if p.name != "self"]) == 0:
            continue
        out.add("%s.%s" % (path, k))
    return out


def _entry_points():
    from neo360_amd import render
    names = (_public_functions(ops, "ops") | _public_functions(training, "training") | _public_functions(parallel, "parallel")
             | _public_functions(render, "render"))
    for cls in (models.NeRF, models.NeRF_TP, models.PixelNeRF, models.MipNeRF360):
        names |= _public_methods(cls, "models.%s" % cls.__name__)
    names |= _public_methods(encoder.GridEncoder, "encoder.GridEncoder")
    return names


def test_registry_is_complete():
    """Every public callable of ops / training / parallel and every public method of the module classes has a record, or stands in
    the exempt / deferred lists with its reason.  A new entry point without a record fails here."""
    covered = {r.entry for r in B.RECORDS.values()} | set(B.EXEMPT) | set(B.DEFERRED)
    unlisted = sorted(_entry_points() - covered)
    assert unlisted == [], unlisted
    stale = sorted(covered - _entry_points())
    assert stale == [], "listed but not (or no longer) public: %s" % stale
    both = sorted({r.entry for r in B.RECORDS.values()} & (set(B.EXEMPT) | set(B.DEFERRED)))
    assert both == [], both
    assert all(isinstance(v, str) and len(v) > 10 for v in list(B.EXEMPT.values()) + list(B.DEFERRED.values()))


def test_render_helpers_reach_the_modules_through_records():
    """render.py slices a batch and calls the modules' forward / render_* methods: each of those has a record, besides the
    records of the helpers themselves (enumerated by test_registry_is_complete)."""
    from neo360_amd import render
    src = inspect.getsource(render)
    for method in ("render_objects", "render_instances", "render_edited", "render_decomposed", "render_skipping", "render_terminating",
                   "render_accelerated", "render_marching"):
        assert "model.%s(" % method in src and "models.NeRF_TP.%s" % method in {r.entry for r in B.RECORDS.values()}, method


@pytest.mark.parametrize("name", sorted(B.RECORDS))
def test_record_is_consistent(name):
    rec = B.RECORDS[name]
    T = rec.build()
    assert set(T) == {a.name for a in rec.args}
    for a in rec.args:
        x = T[a.name]
        assert x.device.type == "cpu" and x.is_contiguous()
        assert tuple(x.shape) == B.resolve(a.shape), (a.name, tuple(x.shape), a.shape)
        assert x.dtype == {"float": torch.float32, "int": torch.int32, "bool": torch.bool}[a.kind]
        if a.kind == "float":
            assert torch.equal(x, x.half().float()), "%s is not fp16-exact" % a.name
    assert set(rec.grad) <= set(T) and (rec.scalar is not None) == (bool(rec.grad) or rec.chain is not None)
    assert all(set(g) <= set(T) for g in rec.groups) and set(rec.together) <= set(T)


# ---- layout variants ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(B.RECORDS))
def test_layout_variants_hold_the_dense_values_and_their_property(name):
    rec = B.RECORDS[name]
    seen = {}
    for cid, who, layout, T, twin in B.layout_variants(rec):
        has = B.LAYOUTS[layout][1]
        names = [who] if who != "together" else [k for k in rec.together if T[k] is not twin[k] and has(T[k])]
        assert names, cid
        for k in names:
            v, d = T[k], twin[k]
            assert has(v), (cid, k, v.stride(), v.dtype, v.data_ptr() % 16)
            assert d.dtype in (torch.float32, torch.bool, torch.int32) and d.is_contiguous() and tuple(d.shape) == tuple(v.shape)
            if layout == "stride0":
                assert torch.equal(v.contiguous(), d) and torch.equal(d, d[:1].expand_as(d))
            else:
                assert torch.equal(v.float().contiguous(), d.float()), (cid, k)
                assert torch.equal(d, rec.build()[k]), (cid, k)
        for k in T:
            if k not in names and T[k] is not None:
                assert T[k] is twin[k] and T[k].is_contiguous()
        seen.setdefault(who, set()).add(layout)
    for a in rec.args:      # every argument gets every view its shape can carry; an input of the float contract also both copies
        want = {"misaligned"} | ({"stride0", "column_slice"} if B.resolve(a.shape)[0] > 1 else set())
        if a.copies:
            want |= {"float64", "float16"}
        assert want <= seen.get(a.name, set()), (a.name, want - seen.get(a.name, set()))
    if rec.together:
        assert set(B.VIEWS) | {"float64"} <= seen["together"]


# ---- mismatch variants ----------------------------------------------------------------------------------------------------------

def _implied_numel(rec, a, T):
    """The most elements a wrapper that misses a check could read through `a`: its accepted shapes with every symbol at the largest
    extent any tensor of the case gives it (a literal extent: plus one)."""
    largest = dict(B.SIZES)
    for b in rec.args:
        t = T.get(b.name)
        if t is None:
            continue
        for shape in (b.shape,) + b.alts:
            if len(shape) == t.dim():
                for e, got in zip(shape, t.shape):
                    if B.symbol(e) is not None:
                        add = B.extent(e) - B.SIZES[B.symbol(e)]
                        largest[B.symbol(e)] = max(largest[B.symbol(e)], got - add)
    return max(math.prod((B.extent(e, largest) if B.symbol(e) else e + 1) for e in shape) for shape in (a.shape,) + a.alts)


@pytest.mark.parametrize("name", sorted(B.RECORDS))
def test_mismatch_variants_stay_inside_their_backing_allocations(name):
    rec = B.RECORDS[name]
    kinds = {}
    for cid, who, kind, T in B.mismatch_variants(rec):
        assert set(T) == {a.name for a in rec.args}
        for a in rec.args:
            t = T[a.name]
            if t is None:
                assert kind == "missing" and a.name == who or rec.build()[a.name] is None
                continue
            assert t.is_contiguous() and t.storage_offset() == 0, (cid, a.name)
            need = max(t.numel(), _implied_numel(rec, a, T)) * t.element_size()
            assert t.untyped_storage().nbytes() - t.storage_offset() * t.element_size() >= need, (cid, a.name, need)
            if a.name != who:       # the rest of the case is right
                assert tuple(t.shape) == B.resolve(a.shape) and torch.equal(t, rec.build()[a.name])
        bad, arg = T[who], rec.arg(who)
        if kind == "dtype":
            assert bad.is_floating_point() != (arg.kind == "float") and tuple(bad.shape) == B.resolve(arg.shape)
        elif kind != "missing":
            assert not any(B.resolve(s) == tuple(bad.shape) for s in (arg.shape,) + arg.alts), cid
        kinds.setdefault(who, set()).add(kind)
    for a in rec.args:
        want = {"dtype"} if a.free else {"dtype", "rank+1"}
        if not a.free and not any(B.resolve(s) == B.resolve(a.shape)[:-1] for s in a.alts):
            want |= {"rank-1"}
        if not a.free and isinstance(a.shape[-1], int):
            want |= {"last-1", "last+1"}
        if not a.free and len(rec.args) > 1 and "R" in {B.symbol(e) for e in a.shape}:
            want |= {"rows-1", "rows+1"}
        assert want <= kinds[a.name], (a.name, want - kinds[a.name])
    for g in rec.groups:
        assert all("missing" in kinds[n] for n in g)


def test_mismatch_variants_on_a_device_add_the_cpu_tensor():
    """The GPU test hands the generators its device; on any device but the CPU every argument also comes once as a CPU tensor.
    Checked here on the meta device, which allocates nothing."""
    rec = B.RECORDS["ops.resample"]
    assert not any(kind == "cpu" for _, _, kind, _ in B.mismatch_variants(rec, "cpu"))
    cases = [(who, T) for _, who, kind, T in B.mismatch_variants(rec, "meta") if kind == "cpu"]
    assert sorted(who for who, _ in cases) == ["t_prev", "weights"]
    for who, T in cases:
        assert T[who].device.type == "cpu" and all(t.device.type == "meta" for k, t in T.items() if k != who)


# ---- the helper -------------------------------------------------------------------------------------------------------------------

def _cpu(t, name="x", shape=None, **kw):
    return dense(t, name, shape, on_device=False, **kw)


def test_dense_returns_the_same_object_when_nothing_needs_fixing():
    x = torch.arange(24.0).reshape(2, 3, 4)
    assert x.data_ptr() % 16 == 0
    assert _cpu(x) is x and _cpu(x, shape=(2, 3, 4)) is x and _cpu(x, shape=(None, 3, None)) is x
    assert _cpu(x, shape=[(2,), (2, 3, 4)]) is x
    e = torch.zeros(0, 3)
    assert _cpu(e, shape=(0, 3)) is e
    i = torch.arange(6, dtype=torch.int32)
    assert _cpu(i, dtypes=(torch.int32,), to=torch.int32) is i


@pytest.mark.parametrize("layout", ["column_slice", "transposed", "stride0", "misaligned", "float64", "float16"])
def test_dense_copies_what_the_library_could_not_read(layout):
    x = B.q(torch.rand(5, 4, generator=torch.Generator().manual_seed(1)))
    v = B.LAYOUTS[layout][0](x)
    assert B.LAYOUTS[layout][1](v)
    before = v.clone()
    got = _cpu(v, "v", (5, 4))
    assert got is not v and got.dtype == torch.float32 and got.is_contiguous() and got.data_ptr() % 16 == 0
    want = v.contiguous().float()
    assert torch.equal(got, want) and got.numpy().tobytes() == want.numpy().tobytes()       # bitwise, not only ==
    assert torch.equal(v.contiguous(), before.contiguous())                                   # the input is not written


def test_dense_keeps_nan_payloads_and_signed_zeros_in_a_copy():
    x = torch.tensor([[0.0, -0.0, float("nan"), float("inf")], [1.0, 2.0, 3.0, 4.0]])
    v = B.LAYOUTS["misaligned"][0](x)
    got = _cpu(v)
    assert got.numpy().tobytes() == x.numpy().tobytes()


def test_dense_refuses_shapes_dtypes_and_non_tensors():
    x = torch.zeros(7, 3)
    with pytest.raises(ValueError, match=r"^rays_d must have shape \(7, 4\), got \(7, 3\)$"):
        _cpu(x, "rays_d", (7, 4))
    with pytest.raises(ValueError, match=r"^rays_d must have shape \(6, 3\), got \(7, 3\)$"):
        _cpu(x, "rays_d", (6, 3))
    with pytest.raises(ValueError, match=r"^far must have shape \(7,\) or \(7, 1\), got \(7, 3\)$"):
        _cpu(x, "far", [(7,), (7, 1)])
    with pytest.raises(ValueError, match=r"^t must have shape \(7, \*\), got \(7,\)$"):
        _cpu(x[:, 0], "t", (7, None))                       # one rank too few
    with pytest.raises(ValueError, match=r"must have shape \(7, 3\), got \(7, 3, 1\)"):
        _cpu(x[..., None], "x", (7, 3))                     # one too many
    with pytest.raises(ValueError, match="rays_o must be a floating-point tensor, got torch.int32"):
        _cpu(x.int(), "rays_o")
    with pytest.raises(ValueError, match="rays_o must be a floating-point tensor, got torch.bool"):
        _cpu(x.bool(), "rays_o")
    with pytest.raises(ValueError, match="idx must be an integer"):
        _cpu(x, "idx", dtypes=(torch.int32,), to=torch.int32)
    for bad in (None, [[1.0, 2.0, 3.0]], 1.0):
        with pytest.raises(TypeError, match="rays_o must be a torch.Tensor"):
            _cpu(bad, "rays_o")


def test_dense_on_a_device_refuses_cpu_tensors_with_both_exception_types():
    """With the device requirement on, a CPU tensor is refused before any library or device access: the project's NeoError (as
    ever, there is no CPU fallback) that is also a ValueError."""
    with pytest.raises(ValueError, match="rays_o is on cpu") as e:
        dense(torch.zeros(7, 3), "rays_o", (7, 3))
    assert isinstance(e.value, _lib.NeoError)
    with pytest.raises(ValueError, match="must have shape"):         # the shape comes first: it needs no device
        dense(torch.zeros(7, 2), "rays_o", (7, 3))
    with pytest.raises(_lib.NeoError) as e:
        context.f32(torch.zeros(3), "x")
    assert type(e.value) is _lib.NeoError                              # f32 keeps its exception as it was


def test_owned_output_is_checked_and_never_copied():
    out = torch.zeros(7, 3)
    assert owned(out, "out", (7, 3), on_device=False) is out
    wide = torch.zeros(7, 5)
    for bad, what in ((wide[:, 1:4], "dense"), (B.LAYOUTS["misaligned"][0](out), "aligned"), (out.double(), "float32"),
                      (torch.zeros(6, 3), "shape"), (torch.zeros(7, 3, 1), "shape"), (out.int(), "float32")):
        with pytest.raises(ValueError, match="^out must "):
            owned(bad, "out", (7, 3), on_device=False)
    with pytest.raises(TypeError):
        owned(None, "out", (7, 3), on_device=False)
    with pytest.raises(_lib.NeoError, match="out is on cpu"):
        owned(out, "out", (7, 3))


def test_gather_tiles_refuses_a_foreign_out():
    """`out=` of the frame gather is written by the collective: another dtype is refused before the process group is touched."""
    tile = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="out must be a torch.float32 tensor"):
        parallel.gather_tiles(tile, 4, 1, unit=4, out=torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(AssertionError, match="out must be a contiguous"):
        parallel.gather_tiles(tile, 4, 1, unit=4, out=torch.zeros(4, 5)[:, :3])


def test_wrappers_refuse_on_the_host_before_any_device_access():
    """What needs no device is refused before one is asked for: a non-tensor, a dtype class and the shape of a tensor come before
    its device, so the first argument of a call is judged completely on CPU tensors (the later ones need a GPU: the sweep)."""
    o = torch.zeros(7, 3)
    with pytest.raises(ValueError, match="rays_o must be a floating-point tensor"):
        ops.intersect_sphere(o.int(), o)
    with pytest.raises(ValueError, match=r"rays_o must have shape \(\*, 3\), got \(7, 4\)"):
        ops.intersect_sphere(torch.zeros(7, 4), o)
    with pytest.raises(TypeError, match="t_prev must be a torch.Tensor"):
        ops.resample([[0.0, 1.0]], o, 4)
    with pytest.raises(_lib.NeoError, match="rays_o is on cpu"):
        ops.intersect_sphere(o, o)
    net = models.NeRF_TP(num_coarse_samples=3, num_fine_samples=4, num_src_views=3)
    with pytest.raises(ValueError, match=r"rays_o must have shape \(\*, 3\), got \(7,\)"):
        net(dict(rays_o=o[:, 0], rays_d=o, viewdirs=o), False, False, 0.0, 0.0, out_depth=True)
    with pytest.raises(ValueError, match=r"plane_xz must have shape \(\*, \*, \*, \*\), got \(3, 128, 12\)"):
        net.set_scene(torch.zeros(3, 128, 12), o, o, o, (64.0, 48.0))


def test_named_instead_lists_real_cases_only():
    """The cases whose message may name the other tensor of a pair are listed one by one: each id is a generated case, and the
    listed argument is another argument of that record."""
    ids = {cid: who for rec in B.RECORDS.values() for cid, who, _, _ in B.mismatch_variants(rec, "meta")}
    assert B.NAMED_INSTEAD and set(B.NAMED_INSTEAD) <= set(ids), sorted(set(B.NAMED_INSTEAD) - set(ids))
    for cid, other in B.NAMED_INSTEAD.items():
        rec = B.RECORDS[cid.rsplit("/", 2)[0]]
        assert other != ids[cid] and other in {a.name for a in rec.args}, cid
