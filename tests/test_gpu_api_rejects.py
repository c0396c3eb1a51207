"""Argument errors of the training-side C entry points: the return code and the neo_last_error() text of every check the map
lookups and the (NV, P)-row training chains make, and the order of those checks where one call fails two of them.  Every call
here is refused (or returns at P == 0) BEFORE anything is launched: no kernel ever sees one of these pointers or shapes."""
import ctypes

import pytest
import torch

import cases
from neo360_amd import models

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -3
DENSE = "bad shape (C a multiple of 64, <= 1024)"
SLICE_FWD = "bad shape (C a multiple of 64, <= 1024; pitch >= C, a multiple of 4)"
SLICE_BWD = "bad shape (C a multiple of 64, <= 1024; pitch >= C)"
NULL = "null pointer"
ALIGN = "the slice must start at a 16-byte boundary"
NO_TP = "scene geometry not set (neo_tp_set_scene)"
NO_PIX = "scene geometry not set (neo_pix_set_scene)"
NV_DIFF = "NV differs from the uploaded scene"
ROWS = "map rows differ from NV*Hf*Wf of the uploaded scene geometry (stale scene, or a map of another resolution)"
INPUT_CH = "input_ch must be 3 (inside the sphere) or 4 (outside)"
SHAPE = "bad shape"
CAP = "at most 4.19 M rows (point-views) per call"
W_B = "null weight / bias pointer"
W_G = "null weight / gradient pointer"
CHAIN = "chain_mode must be the 0 / 1 the forward returned"
NO_CTX = "null context"

NV = cases.NV
TEXELS = NV * cases.LATENT_HW[0] * cases.LATENT_HW[1]


@pytest.fixture(scope="module")
def env():
    """A context without scenes, one with both scene geometries uploaded, a device buffer for every non-null pointer."""
    dev = torch.device("cuda:0")
    scene = cases.small_scene()
    tp = models.NeRF_TP(num_coarse_samples=32, num_fine_samples=64, num_src_views=NV).to(dev)
    tp.set_scene(*(scene[k].to(dev) for k in ("plane_xz", "plane_xy", "plane_yz", "latent")), scene["image_wh"])
    pix = models.PixelNeRF(num_src_views=NV).to(dev)
    pix.set_scene(scene["latent"].to(dev), scene["image_wh"])
    bare = models.NeRF().to(dev)
    buf = torch.zeros(1024, device=dev)
    torch.cuda.synchronize()
    poses = (ctypes.c_float * (16 * 8))(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] * 8))
    e = dict(tp=tp._context(dev), pix=pix._context(dev), bare=bare._context(dev), buf=buf.data_ptr(), poses=poses,
             keep=(tp, pix, bare, buf))
    assert e["buf"] % 16 == 0
    yield e
    for net in (tp, pix, bare):
        net.close()


def _table(env, n=9, hole=None):
    t = (ctypes.c_void_p * n)(*([env["buf"]] * n))
    if hole is not None:
        t[hole] = None
    return t


def _map_args(env, name, **bad):
    """Valid arguments of one of the six map lookups, with `bad` laid over them."""
    a = dict(ctx="pix" if name.startswith("neo_pix") else "tp", map=env["buf"], texels=TEXELS, pitch=256, C=64, pts=env["buf"], P=5,
             poses=env["poses"], NV=NV, out=env["buf"], g_out=env["buf"], g_map=env["buf"])
    a.update(bad)
    lead = [env[a["ctx"]].handle if a["ctx"] else None]
    if not name.endswith("backward"):
        lead.append(a["map"])
    lead.append(a["texels"])
    if "slice" in name:
        lead.append(a["pitch"])
    tail = [a["g_out"], a["g_map"]] if name.endswith("backward") else [a["out"]]
    return lead + [a["C"], a["pts"], a["P"], a["poses"], a["NV"], 50.0, 32.0, 24.0] + tail + [None]


MAP_FWD = ("neo_tp_gather_map", "neo_tp_gather_map_slice", "neo_pix_gather_map")
MAP_BWD = ("neo_tp_gather_map_backward", "neo_tp_gather_map_slice_backward", "neo_pix_gather_map_backward")


def _map_cases():
    out = []
    for name in MAP_FWD + MAP_BWD:
        fwd, sl, pix = name in MAP_FWD, "slice" in name, name.startswith("neo_pix")
        shape = (SLICE_FWD if fwd else SLICE_BWD) if sl else DENSE
        out += [(name, "no_context", dict(ctx=None), INVALID, NO_CTX),
                (name, "C_65", dict(C=65), INVALID, shape),
                (name, "C_32", dict(C=32), INVALID, shape),
                (name, "C_1088", dict(C=1088), INVALID, shape),
                (name, "P_negative", dict(P=-1), INVALID, shape),
                (name, "shape_before_null", dict(C=65, pts=None), INVALID, shape),
                (name, "P_0_nulls", dict(P=0, map=None, pts=None, poses=None, out=None, g_out=None, g_map=None), OK, None),
                (name, "null_pts", dict(pts=None), INVALID, NULL),
                (name, "null_poses", dict(poses=None), INVALID, NULL),
                (name, "null_before_scene", dict(ctx="bare", pts=None), INVALID, NULL),
                (name, "no_scene", dict(ctx="bare"), STATE, NO_PIX if pix else NO_TP),
                (name, "only_the_other_decoders_scene", dict(ctx="tp" if pix else "pix"), STATE, NO_PIX if pix else NO_TP),
                (name, "NV_differs", dict(NV=NV + 1), INVALID, NV_DIFF),
                (name, "NV_before_rows", dict(NV=NV + 1, texels=TEXELS + 1), INVALID, NV_DIFF),
                (name, "rows_differ", dict(texels=TEXELS + 1), INVALID, ROWS)]
        out += [(name, "null_map", dict(map=None), INVALID, NULL), (name, "null_out", dict(out=None), INVALID, NULL)] if fwd else \
               [(name, "null_g_out", dict(g_out=None), INVALID, NULL), (name, "null_g_map", dict(g_map=None), INVALID, NULL)]
        if sl:
            out += [(name, "pitch_below_C", dict(pitch=32), INVALID, shape)]
            # only the forward reads the slice in 16-byte pieces: the backward takes any pitch >= C and any start
            out += [(name, "pitch_odd", dict(pitch=257), INVALID, shape), (name, "misaligned", dict(map="+4"), INVALID, ALIGN),
                    (name, "null_before_alignment", dict(map="+4", pts=None), INVALID, NULL),
                    (name, "alignment_before_scene", dict(ctx="bare", map="+4"), INVALID, ALIGN)] if fwd else \
                   [(name, "pitch_odd_no_scene", dict(ctx="bare", pitch=257), STATE, NO_TP)]
    return out


@pytest.mark.parametrize("name,label,bad,rc,msg", _map_cases(), ids=lambda v: v if isinstance(v, str) and " " not in v else None)
def test_map_lookup_rejects(env, name, label, bad, rc, msg):
    if bad.get("map") == "+4":
        bad = dict(bad, map=env["buf"] + 4)
    lib = env["tp"].lib
    got = getattr(lib, name)(*_map_args(env, name, **bad))
    assert got == rc
    if rc != OK:
        assert lib.neo_last_error().decode() == msg


def _chain_args(env, name, **bad):
    """Valid arguments of one of the six (NV, P)-row training chains, with `bad` laid over them."""
    b = env["buf"]
    a = dict(ctx="bare", input_ch=3, w=_table(env), b=_table(env), gw=_table(env), gb=_table(env), x_enc=b, tape=b, NV=NV, P=7, g_pre=b,
             chain=0, chain_out=None)
    a.update(bad)
    h = env[a["ctx"]].handle if a["ctx"] else None
    tp, pre, fwd = name.startswith("neo_tp"), name.endswith("_pre"), "forward" in name
    lead = [h] + ([a["input_ch"]] if tp else [])
    feats = [b] * ((3 if tp else 2) - (1 if pre and not fwd else 0))    # local | pre (not in a projected backward), world (tp), cond
    if fwd:
        return lead + [a["w"], a["b"], a["x_enc"]] + feats + [a["NV"], a["P"], a["tape"], b, b] + ([a["chain_out"]] if pre else []) + [None]
    grads = [b, a["g_pre"]] + ([b] if tp else [])                    # g_x_enc, g_local | g_pre, g_world (tp)
    return (lead + [a["w"], a["x_enc"]] + feats + [a["NV"], a["P"], a["tape"], b, b, a["gw"], a["gb"]] + grads
            + ([a["chain"]] if pre else []) + [None])


CHAINS = ("neo_tp_mlp_train_forward", "neo_tp_mlp_train_backward", "neo_tp_mlp_train_forward_pre", "neo_tp_mlp_train_backward_pre",
          "neo_pix_mlp_train_forward_pre", "neo_pix_mlp_train_backward_pre")


def _chain_cases():
    out = []
    for name in CHAINS:
        tp, pre, fwd = name.startswith("neo_tp"), name.endswith("_pre"), "forward" in name
        out += [(name, "no_context", dict(ctx=None), INVALID, NO_CTX),
                (name, "NV_0", dict(NV=0), INVALID, SHAPE),
                (name, "P_negative", dict(P=-1), INVALID, SHAPE),
                (name, "P_0_nulls", dict(P=0, w=None, b=None, gw=None, gb=None, x_enc=None, tape=None, g_pre=None), OK, None),
                (name, "row_cap", dict(P=1400000), INVALID, CAP),
                (name, "cap_before_null", dict(P=1400000, x_enc=None), INVALID, CAP),
                (name, "null_x_enc", dict(x_enc=None), INVALID, NULL),
                (name, "null_tape", dict(tape=None), INVALID, NULL),
                (name, "null_w_table", dict(w=None), INVALID, NULL),
                (name, "null_before_table_entries", dict(tape=None, w=("hole", 0)), INVALID, NULL),
                (name, "null_w_3", dict(w=("hole", 3)), INVALID, W_B if fwd else W_G),
                (name, "null_w_8", dict(w=("hole", 8)), INVALID, W_B if fwd else W_G)]
        out += [(name, "null_b_table", dict(b=None), INVALID, NULL), (name, "null_b_5", dict(b=("hole", 5)), INVALID, W_B)] if fwd else \
               [(name, "null_gw_table", dict(gw=None), INVALID, NULL), (name, "null_gb_table", dict(gb=None), INVALID, NULL),
                (name, "null_gw_0", dict(gw=("hole", 0)), INVALID, W_G), (name, "null_gb_8", dict(gb=("hole", 8)), INVALID, W_G)]
        if tp:
            # the forwards judge input_ch before the shape, the backwards only after the P == 0 early-out
            out += [(name, "input_ch_5", dict(input_ch=5), INVALID, INPUT_CH),
                    (name, "input_ch_5_and_NV_0", dict(input_ch=5, NV=0), INVALID, INPUT_CH if fwd else SHAPE),
                    (name, "input_ch_5_and_P_0", dict(input_ch=5, P=0), INVALID if fwd else OK, INPUT_CH if fwd else None),
                    (name, "input_ch_before_cap", dict(input_ch=5, P=1400000), INVALID, INPUT_CH)]
        if pre and not fwd:
            out += [(name, "chain_mode_2", dict(chain=2), INVALID, CHAIN),
                    (name, "chain_mode_negative", dict(chain=-1), INVALID, CHAIN),
                    (name, "chain_mode_first", dict(chain=2, NV=0, input_ch=5), INVALID, CHAIN),
                    (name, "chain_mode_before_P_0", dict(chain=2, P=0), INVALID, CHAIN),
                    (name, "null_g_pre", dict(g_pre=None), INVALID, NULL)]
    return out


@pytest.mark.parametrize("name,label,bad,rc,msg", _chain_cases(), ids=lambda v: v if isinstance(v, str) and " " not in v else None)
def test_training_chain_rejects(env, name, label, bad, rc, msg):
    bad = {k: (_table(env, hole=v[1]) if isinstance(v, tuple) else v) for k, v in bad.items()}
    lib = env["bare"].lib
    got = getattr(lib, name)(*_chain_args(env, name, **bad))
    assert got == rc
    if rc != OK:
        assert lib.neo_last_error().decode() == msg


@pytest.mark.parametrize("name", ["neo_tp_mlp_train_forward_pre", "neo_pix_mlp_train_forward_pre"])
@pytest.mark.parametrize("bad", [dict(NV=0), dict(x_enc=None), dict(P=0)], ids=["rejected", "null_pointer", "P_0"])
def test_projected_forward_reports_chain_mode_before_any_check(env, name, bad):
    """The tape layout is written to *chain_mode before the arguments are judged: a caller reads it even from a refused call."""
    lib = env["bare"].lib
    chain = ctypes.c_int(-1)
    rc = getattr(lib, name)(*_chain_args(env, name, chain_out=ctypes.byref(chain), **bad))
    assert rc == (OK if bad.get("P") == 0 else INVALID)
    assert chain.value == lib.neo_train_chain_mode(-1) and chain.value in (0, 1)


def test_projected_forward_with_null_context_leaves_chain_mode_alone(env):
    lib = env["bare"].lib
    for name in ("neo_tp_mlp_train_forward_pre", "neo_pix_mlp_train_forward_pre"):
        chain = ctypes.c_int(-1)
        assert getattr(lib, name)(*_chain_args(env, name, ctx=None, chain_out=ctypes.byref(chain))) == INVALID
        assert lib.neo_last_error().decode() == NO_CTX and chain.value == -1


VIEWS = "1..8 source views supported"


def _view_count_args(env, entry, nv):
    """Valid arguments of a scene, PixelNeRF-scene or encoder entry point (every pointer non-null) with NV = nv."""
    b, h = env["buf"], env["bare"].handle
    cams = [env["poses"], 50.0, 32.0, 24.0]
    if entry == "neo_tp_set_scene":
        return [h, b, b, b, nv, 128, 2, 2, b, 512, 2, 2, 64.0, 48.0, None]
    if entry == "neo_pix_set_scene":
        return [h, b, nv, 512, 2, 2, 64.0, 48.0, None]
    geo = [b, nv, 2, 2, 64.0, 48.0] + cams + [1, 1, 1]
    if entry == "neo_enc_floorplans":
        return [h] + geo + [b, b, b, None]
    if entry == "neo_enc_floorplans_train":
        return [h] + geo + [b, b, b, b, None]
    return [h, _table(env), _table(env)] + geo + [b, b, b, b, _table(env), _table(env), b, None]


@pytest.mark.parametrize("nv", [0, 9])
@pytest.mark.parametrize("entry", ["neo_tp_set_scene", "neo_pix_set_scene", "neo_enc_floorplans", "neo_enc_floorplans_train",
                                   "neo_enc_floorplans_backward"])
def test_view_count_limits(env, entry, nv):
    """The library takes 1..8 source views: 0 and 9 are refused by the scene, PixelNeRF-scene and encoder entry points before
    anything is launched (on a context without scenes or encoder weights: the view count is judged first)."""
    lib = env["bare"].lib
    assert getattr(lib, entry)(*_view_count_args(env, entry, nv)) == INVALID
    assert lib.neo_last_error().decode() == VIEWS
