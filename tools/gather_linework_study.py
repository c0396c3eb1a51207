"""Host-side measurement (no GPU), round 6: how much cache-line work does the gather half of k_tp_mlp_hp present to a CU's
texture-address unit, and what would a per-tile-view dedup (each unique texel fetched once, blends from LDS) leave of it?

The energy budget (profiles/r06_energy_budget.log) prices the DIVERGENT part of the gathers - distinct cache lines per load
instruction and the L2 -> L1 traffic behind them - at 22 % of an inside-sphere launch (NEO_TP_ABLATE 256: every tap reads texel 0
of its map, loads kept).  A load instruction of the kernel covers 4 ADJACENT samples x one tap x 256 B; the address unit works
per distinct 128-B line.  Counted here on the bench geometry, per 64-point tile and source view:
  now        sum over the kernel's load instructions of the distinct texels among their 4 rows   (x lines per 256-B piece)
  unique     distinct texels of the whole tile-view                                              (x lines per texel)
  cells      runs of consecutive samples in one bilinear cell x 4 texels (the cheap dedup: no hashing, duplicates between
             neighbouring cells stay)
Same rays / camera / sample positions as tools/footprint_study.py.
`--quad`: the ray-major and the quad point order side by side for all four launches (quad_study below)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neo360_amd import synth            # noqa: E402
import oracle                           # noqa: E402
from oracle import gather, rays as rays_mod, sampling   # noqa: E402
from footprint_study import taps, H, W, NV, GROUPS, RAYS_PER_GROUP   # noqa: E402


def main():
    torch.manual_seed(0)
    state = synth.nerf_tp_state(0)
    scene = {k: torch.randn(NV, 128, 120, 160) * 0.1 for k in ("plane_xz", "plane_xy", "plane_yz")}
    scene["latent"] = torch.randn(NV, 512, 240, 320) * 0.1
    scene["image_wh"] = (float(W), float(H))
    poses, focal, centre = synth.source_views(NV, W, H)
    c2w = synth.look_at_origin(40.0)
    ro, vd, rd, _ = rays_mod.camera_rays(rays_mod.pixel_directions(H, W, 0.8 * W), c2w[:3, :4])
    rng = np.random.RandomState(0)
    starts = rng.randint(0, H * W - RAYS_PER_GROUP, GROUPS)
    idx = np.concatenate([np.arange(s, s + RAYS_PER_GROUP) for s in starts])
    batch = dict(rays_o=ro[idx], rays_d=rd[idx], viewdirs=vd[idx], src_poses=poses, src_focal=focal, src_c=centre)
    _, extra = oracle.neo360.render(state, batch, scene, keep=True)
    o, d = batch["rays_o"], batch["rays_d"]
    res = {}
    for level in range(2):
        tv = extra[level]["fg_t"]
        pts = sampling.points_on_rays(tv, o, d)
        B, N, _ = pts.shape
        cam = gather.world_to_camera(pts.reshape(-1, 3), poses)
        f = focal[0].repeat(2).clone()
        f[1] *= -1
        uv = gather.project(cam, f, centre[0][None])
        g = (uv * (gather.latent_scaling(240, 320) / torch.tensor([float(W), float(H)])) - 1.0).numpy()
        camn = cam.numpy()
        maps = {"latent": (taps(g[..., 0], g[..., 1], 320, 240), 1024),          # projected latent: 1 KB per texel
                "plane_xz": (taps(camn[..., 0], camn[..., 2], 160, 120), 512),
                "plane_xy": (taps(camn[..., 0], camn[..., 1], 160, 120), 512),
                "plane_yz": (taps(camn[..., 1], camn[..., 2], 160, 120), 512)}
        key = "fg_%s" % ("coarse" if level == 0 else "fine")
        tot = dict(now=0.0, unique=0.0, cells=0.0, requested=0.0)
        per = {}
        ntv = 0
        for name, (t, texel_bytes) in maps.items():
            lines = texel_bytes // 128
            now = uniq = cells = 0
            n = 0
            for gi in range(GROUPS):
                lo, hi = gi * RAYS_PER_GROUP * N, (gi + 1) * RAYS_PER_GROUP * N
                for t0 in range(lo, hi - 63, 64):
                    for v in range(NV):
                        tt = t[v, t0:t0 + 64]                                     # (64 rows, 4 taps)
                        n += 1
                        # the kernel's instruction: rows {4w..4w+3} + 16q, one tap
                        for q in range(4):
                            for w in range(4):
                                rows = tt[16 * q + 4 * w:16 * q + 4 * w + 4]
                                for k in range(4):
                                    now += len(np.unique(rows[:, k]))
                        uniq += len(np.unique(tt))
                        change = np.ones(64, bool)
                        change[1:] = (tt[1:] != tt[:-1]).any(axis=1)
                        cells += 4 * int(change.sum())
            per[name] = dict(now_texels=now / n, unique_texels=uniq / n, cell_run_texels=cells / n, lines_per_texel=lines)
            tot["now"] += now / n * lines
            tot["unique"] += uniq / n * lines
            tot["cells"] += cells / n * lines
            tot["requested"] += 256 * lines
            ntv = n
        res[key] = dict(per_map=per, lines_per_tile_view=tot, tile_views=ntv,
                        ratio_now_over_unique=tot["now"] / tot["unique"], ratio_now_over_cells=tot["now"] / tot["cells"])
        print(key, json.dumps(res[key], indent=1))
    with open(os.path.join(ROOT, "profiles", "r06_gather_linework.json"), "w") as fh:
        json.dump(dict(note=__doc__, result=res), fh, indent=1)


# ---- quad order (csrc/point_order.h:quad_point): both point orders, all four launches ------------------------------------------
def taps_ok(gx, gy, Wd, Hd):
    """Texel ids (invalid taps: the placeholder texel 0, as in the kernels) and which taps are inside the map."""
    x = (gx + 1) / 2 * (Wd - 1)
    y = (gy + 1) / 2 * (Hd - 1)
    x0, y0 = np.floor(x), np.floor(y)
    ids, oks = [], []
    for yy in (y0, y0 + 1):
        for xx in (x0, x0 + 1):
            ok = (xx >= 0) & (xx <= Wd - 1) & (yy >= 0) & (yy <= Hd - 1)
            ids.append(np.where(ok, yy * Wd + xx, 0).astype(np.int64))
            oks.append(ok)
    return np.stack(ids, -1), np.stack(oks, -1)


def tile_view_lines(ids, oks, lines, work_list):
    """128-B lines one 64-point tile presents / touches for one source view.  ids / oks: per map (64 rows, 4 taps); lines: per map,
    lines per texel.  One load instruction = rows {4 w .. 4 w + 3} + 16 q, one tap, 256 B of the texel: its distinct texels among
    the four rows x the texel's lines is what all pieces of that texel present together.
    work_list = False (k_tp_mlp_hp): every (row group, map) is gathered; the latent's as a whole only when some row of the tile has a
    weighted latent tap.  True (k_tp_mlp_hpp): only the pairs in which some row carries weight are listed, an empty row group
    keeps the latent's, the list is padded to a multiple of 3 with all-zero entries (texel 0), and a tile-view without any
    weighted tap gathers nothing.  Returns (presented, unique, listed pairs, skipped pairs)."""
    names = list(ids)
    weighted = {m: oks[m].reshape(4, 16, 4).any(axis=(1, 2)) for m in names}          # per map: row group q has a weighted tap
    if work_list:
        if not any(w.any() for w in weighted.values()):
            return 0.0, 0.0, 0, 16
        listed = {m: weighted[m].copy() for m in names}
        for q in range(4):
            if not any(weighted[m][q] for m in names):
                listed[names[0]][q] = True
    else:
        listed = {m: np.ones(4, bool) for m in names}
        if not weighted[names[0]].any():
            listed[names[0]][:] = False
    presented, touched, n = 0.0, 0.0, 0
    for m in names:
        seen = []
        for q in range(4):
            if not listed[m][q]:
                continue
            n += 1
            rows = ids[m][16 * q:16 * q + 16]
            for w in range(4):
                for k in range(4):
                    presented += len(np.unique(rows[4 * w:4 * w + 4, k])) * lines[m]
            seen.append(rows.reshape(-1))
        if seen:
            touched += len(np.unique(np.concatenate(seen))) * lines[m]
    if work_list:
        presented += (-n % 3) * 16 * lines[names[0]]                                 # padding entries: 16 instructions on texel 0
    return presented, touched, n, 16 - n


QUAD_BLOCKS, BLOCK_RAYS = 12, 16


def quad_study():
    """Lines per tile-view in ray-major order and with the samples of 4 (a quad), 8 and 16 consecutive launch-order rays interleaved
    (64 / G samples x G rays per tile, the instruction rows being four consecutive rays of the group) for the four evaluator launches
    of the bench frame, at the oracle's coarse and fine positions.  Rays: 12 random blocks of 16 launch-order rays as the launches
    see them under the pixel-grid hint - four 2 x 2 pixel patches in a row inside the sphere, two rows of an 8 x 8 patch outside; a
    quad is the first / second / .. four of a block (a 2 x 2 patch inside, four adjacent pixels outside).
    Writes profiles/quad_order_linework.json."""
    torch.manual_seed(0)
    state = synth.nerf_tp_state(0)
    scene = {k: torch.randn(NV, 128, 120, 160) * 0.1 for k in ("plane_xz", "plane_xy", "plane_yz")}
    scene["latent"] = torch.randn(NV, 512, 240, 320) * 0.1
    scene["image_wh"] = (float(W), float(H))
    poses, focal, centre = synth.source_views(NV, W, H)
    c2w = synth.look_at_origin(40.0)
    ro, vd, rd, _ = rays_mod.camera_rays(rays_mod.pixel_directions(H, W, 0.8 * W), c2w[:3, :4])
    rng = np.random.RandomState(0)
    px, py = 8 * rng.randint(0, W // 8, QUAD_BLOCKS), 2 * rng.randint(0, H // 2, QUAD_BLOCKS)
    inside = np.concatenate([[y * W + x + 2 * p, y * W + x + 2 * p + 1, (y + 1) * W + x + 2 * p, (y + 1) * W + x + 2 * p + 1]
                             for x, y in zip(px, py) for p in range(4)])
    qx, qy = 8 * rng.randint(0, W // 8, QUAD_BLOCKS), 2 * rng.randint(0, H // 2, QUAD_BLOCKS)
    outside = np.concatenate([np.concatenate([np.arange(y * W + x, y * W + x + 8), np.arange((y + 1) * W + x, (y + 1) * W + x + 8)])
                              for x, y in zip(qx, qy)])
    idx = np.concatenate([inside, outside])
    nb = QUAD_BLOCKS * BLOCK_RAYS
    batch = dict(rays_o=ro[idx], rays_d=rd[idx], viewdirs=vd[idx], src_poses=poses, src_focal=focal, src_c=centre)
    _, extra = oracle.neo360.render(state, batch, scene, keep=True)
    o, d, far = batch["rays_o"], batch["rays_d"], extra[0]["far"]
    res = {}
    for region in ("fg", "bg"):
        for level in range(2):
            sel = slice(0, nb) if region == "fg" else slice(nb, 2 * nb)
            tv = extra[level]["fg_t" if region == "fg" else "bg_s"][sel]
            pts = sampling.points_on_rays(tv if region == "fg" else far[sel] * (1.0 - tv) + 3.0 * tv, o[sel], d[sel])
            B, N, _ = pts.shape
            cam = gather.world_to_camera(pts.reshape(-1, 3), poses)
            f = focal[0].repeat(2).clone()
            f[1] *= -1
            uv = gather.project(cam, f, centre[0][None])
            g = (uv * (gather.latent_scaling(240, 320) / torch.tensor([float(W), float(H)])) - 1.0).numpy()
            camn = cam.numpy()
            maps = {"latent": taps_ok(g[..., 0], g[..., 1], 320, 240), "plane_xz": taps_ok(camn[..., 0], camn[..., 2], 160, 120),
                    "plane_xy": taps_ok(camn[..., 0], camn[..., 1], 160, 120), "plane_yz": taps_ok(camn[..., 1], camn[..., 2], 160, 120)}
            # bytes per texel: the projected latent 1 KB; the planes raw (512 B) inside, projected (1 KB) outside the sphere
            lines = {m: (1024 if m == "latent" or region == "bg" else 512) // 128 for m in maps}
            v_idx = np.arange(BLOCK_RAYS * N)
            out = {}
            for order, G in (("ray_major", 1), ("quad", 4), ("group_8", 8), ("group_16", 16)):
                # virtual index inside a block -> ray-major index (point_order.h:quad_point; G = 1: identity)
                grp, within = v_idx // (G * N), v_idx % (G * N)
                perm = (G * grp + within % G) * N + within // G
                acc = np.zeros(4)
                n = 0
                for bi in range(QUAD_BLOCKS):
                    at = bi * BLOCK_RAYS * N + perm
                    for t0 in range(0, BLOCK_RAYS * N - 63, 64):
                        rows = at[t0:t0 + 64]
                        for v in range(NV):
                            acc += tile_view_lines({m: maps[m][0][v, rows] for m in maps}, {m: maps[m][1][v, rows] for m in maps},
                                                   lines, region == "bg")
                            n += 1
                out[order] = dict(presented_lines=acc[0] / n, unique_lines=acc[1] / n, gathered_pairs_of_16=acc[2] / n,
                                  skipped_pairs_of_16=acc[3] / n, tile_views=n)
            key = "%s %s (N = %d)" % ("inside" if region == "fg" else "outside", "coarse" if level == 0 else "fine", N)
            for order in ("quad", "group_8", "group_16"):
                out[order]["presented_change"] = out[order]["presented_lines"] / out["ray_major"]["presented_lines"] - 1.0
            res[key] = out
            print(key, json.dumps(out, indent=1))
    with open(os.path.join(ROOT, "profiles", "quad_order_linework.json"), "w") as fh:
        json.dump(dict(note=quad_study.__doc__ + "  " + tile_view_lines.__doc__, result=res), fh, indent=1)


if __name__ == "__main__":
    if "--quad" in sys.argv:
        quad_study()
    else:
        main()
