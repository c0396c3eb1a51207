"""CPU: the point order of a NeO-360 evaluator launch (csrc/point_order.h), compiled into a stand-alone host program.

The header maps a launch's virtual (tile-order) point index to the (ray, sample) pair it stands for: quad_point interleaves the
samples of G consecutive launch-order rays (G = 4: a quad; 8 and 16 as well), patch_point (moved there unchanged from tp_common.h) sends a launch-order ray to its
pixel under the pixel-grid hint, launch_point is the composition the kernels use for BOTH the row they set up and the row they
write.  Checked for R in {0, 1, 2, 3, 4, 5, 7, 9} x N in {1, 2, 129} (no quad, a partial last quad, one and two whole quads) without
a grid, with a grid of whole bands and with ragged ends, all with quads of four; larger launches with the patch shapes the library
uses and with groups of 4, 8 and 16 rays (R with no, a partial last, one and several whole groups):

* quad off is the identity; quad on is a bijection on [0, R * N), and so is the composition with the patch order;
* ranks 0..3 of a quad at one sample index s are the quad's four rays at s (virtual index quad * 4 N + 4 s + r -> ray 4 quad + r),
  in general ranks 0..G-1 of a group its G rays; the last R % G rays keep ray-major order;
* through the patch order those four are the rays parallel.ray_patch_order (the host mirror of patch_point) lists at 4 quad + r, and
  with 2 x 2 patches inside whole bands they are one 2 x 2 pixel patch.

The program is built with -fsanitize=undefined,address where the host compiler has the runtimes (its own main, no preloading); a
failed sanitized build is reported as a warning with the compiler's message before the plain build is tried, and which build ran is
printed and carried by the assertion messages."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from neo360_amd import parallel

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neo-360_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "point_order.h"
// argv: groups of R N quad grid_w grid_first pw ph; per group three lines: quad_point, patch_point, launch_point of every gv
int main(int argc, char** argv) {
    for (int a = 1; a + 6 < argc; a += 7) {
        const int R = atoi(argv[a]), N = atoi(argv[a + 1]), quad = atoi(argv[a + 2]), gw = atoi(argv[a + 3]);
        const long first = atol(argv[a + 4]);
        const int pw = atoi(argv[a + 5]), ph = atoi(argv[a + 6]);
        const long P = (long)R * N;
        for (long g = 0; g < P; ++g) printf("%ld ", neo::tp::quad_point(g, N, R, quad));
        printf("\n");
        for (long g = 0; g < P; ++g) printf("%ld ", neo::tp::patch_point(g, N, R, gw, first, pw, ph));
        printf("\n");
        for (long g = 0; g < P; ++g) printf("%ld ", neo::tp::launch_point(g, N, R, quad, gw, first, pw, ph));
        printf("\n");
    }
    return 0;
}
"""

RS = (0, 1, 2, 3, 4, 5, 7, 9)
NS = (1, 2, 129)
# (grid_w, grid_first, pw, ph): no grid; 2-pixel-wide image in 2 x 2 patches, bands of 4 rays: whole bands from ray 0; ragged ends
GRIDS = ((0, 0, 1, 1), (2, 0, 1, 1), (2, 1, 1, 1), (2, 6, 1, 1))
# the library's shapes on a 16- / 8-pixel-wide image: 2 x 2 (inside the sphere) and 8 x 8 (outside), whole and ragged
LARGE = ((64, 3, (16, 0, 1, 1)), (70, 3, (16, 32, 1, 1)), (77, 2, (16, 5, 1, 1)), (128, 2, (8, 0, 3, 3)), (150, 2, (8, 8, 3, 3)),
         (150, 1, (8, 3, 3, 3)))
WIDE = ((5, 2), (8, 2), (15, 2), (16, 2), (17, 129), (33, 3), (40, 1))   # (R, N) for groups of 8 and 16 without a grid
CONFIGS = [(R, N, quad, g) for R in RS for N in NS for quad in (0, 4) for g in GRIDS] + \
          [(R, N, quad, g) for R, N, g in LARGE for quad in (0, 4, 8, 16)] + \
          [(R, N, quad, GRIDS[0]) for R, N in WIDE for quad in (8, 16)]


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (set CXX)")
    d = tmp_path_factory.mktemp("point_order")
    src, exe = str(d / "point_order_main.cpp"), str(d / "point_order_main")
    with open(src, "w") as f:
        f.write(PROGRAM)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    build = "with -fsanitize=undefined,address"
    if r.returncode != 0:        # a compiler without the sanitizer runtimes: the plain program checks the same values
        warnings.warn("point_order host program: the sanitized build failed, checking the plain build instead:\n" + r.stderr[-1500:])
        build = "WITHOUT sanitizers"
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, (build, r.stderr)
    print("point_order host program built %s (%s)" % (build, cxx))
    args = []
    for R, N, quad, (gw, first, pw, ph) in CONFIGS:
        args += [R, N, quad, gw, first, pw, ph]
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (build, r.stderr[-2000:])
    lines = r.stdout.split("\n")
    assert len(lines) >= 3 * len(CONFIGS)
    out = {}
    for i, cfg in enumerate(CONFIGS):
        out[cfg] = tuple(np.array(lines[3 * i + j].split(), dtype=np.int64) for j in range(3))
    return out


def test_every_config_has_all_its_points(maps):
    for (R, N, quad, g), (qp, pp, lp) in maps.items():
        assert qp.size == pp.size == lp.size == R * N, (R, N, quad, g)


def test_off_is_the_identity(maps):
    for (R, N, quad, g), (qp, pp, lp) in maps.items():
        if quad == 0:
            assert np.array_equal(qp, np.arange(R * N)), (R, N, g)
            assert np.array_equal(lp, pp), (R, N, g)


def test_bijection_with_and_without_the_grid(maps):
    for (R, N, quad, g), (qp, pp, lp) in maps.items():
        ident = np.arange(R * N)
        assert np.array_equal(np.sort(qp), ident), (R, N, quad, g)
        assert np.array_equal(np.sort(pp), ident), (R, N, quad, g)
        assert np.array_equal(np.sort(lp), ident), (R, N, quad, g)
        assert np.array_equal(lp, pp[qp]), ("launch_point is patch_point after quad_point", R, N, quad, g)


def test_ranks_of_a_quad_are_its_four_rays_at_one_sample(maps):
    seen = set()
    for (R, N, G, g), (qp, pp, lp) in maps.items():
        if G == 0:
            continue
        ng = R // G
        v = qp[:ng * G * N].reshape(ng, N, G)                      # [group, s, rank]
        want = (G * np.arange(ng)[:, None, None] + np.arange(G)[None, None, :]) * N + np.arange(N)[None, :, None]
        assert np.array_equal(v, want), (R, N, G, g)
        tail = np.arange(ng * G * N, R * N)
        assert np.array_equal(qp[tail], tail), ("the last R % G rays keep ray-major order", R, N, G, g)
        seen.add((G, "none" if ng == 0 else "partial" if R % G else "whole", min(ng, 2)))
    for G in (4, 8, 16):                                           # no group, a partial last group, one and several whole groups
        assert {(G, "none", 0), (G, "partial", 1), (G, "whole", 1), (G, "whole", 2)} <= seen, (G, sorted(seen))


def test_through_the_patch_order_a_quad_is_four_neighbouring_pixels(maps):
    checked_2x2 = 0
    for (R, N, G, g), (qp, pp, lp) in maps.items():
        gw, first, pw, ph = g
        if G == 0 or gw == 0:
            continue
        order = parallel.ray_patch_order(R, gw, first, pw, ph).numpy()      # launch-order ray -> the ray it stands for
        ng = R // G
        v = lp[:ng * G * N].reshape(ng, N, G)
        assert np.array_equal(v % N, np.broadcast_to(np.arange(N)[None, :, None], v.shape)), (R, N, G, g)   # one sample index per row group
        rays = v // N
        assert np.array_equal(rays, np.broadcast_to(order[:ng * G].reshape(ng, 1, G), rays.shape)), (R, N, G, g)
        if (pw, ph) == (1, 1) and first % 4 == 0:
            band = gw << ph
            for q in range(R // 4):                                        # every aligned four of a group is one 2 x 2 pixel patch
                if q // (G // 4) >= ng:
                    break
                Gf = first + 4 * q
                b = Gf // band
                if b * band < first or (b + 1) * band > first + R:
                    continue                                               # ragged end: the caller's order
                px = first + rays[q // (G // 4), 0, 4 * (q % (G // 4)):4 * (q % (G // 4)) + 4]      # pixels of the frame
                x0, y0 = px[0] % gw, px[0] // gw
                assert x0 % 2 == 0 and y0 % 2 == 0
                assert [(int(p % gw), int(p // gw)) for p in px] == [(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)], (R, N, G, g, q)
                checked_2x2 += 1
    assert checked_2x2 >= 16


def test_documented_defaults_are_the_shipped_ones():
    """The per-launch defaults live in ONE place, api_tp.hip:quad_default; DESIGN.md 4.1 states them in one marked sentence and
    every other document points there.  The two must agree."""
    root = os.path.dirname(CSRC.rstrip(os.sep)).rsplit(os.sep, 1)[0]
    api = open(os.path.join(CSRC, "api_tp.hip")).read()
    m = re.search(r"quad_default\[4\] = \{(\d+), (\d+), (\d+), (\d+)\};", api)
    assert m, "api_tp.hip:quad_default not found"
    design = open(os.path.join(root, "DESIGN.md")).read()
    d = re.search(r"Shipped defaults \(`api_tp\.hip:quad_default`; rays per group, 0 = ray-major\): inside coarse (\d+), inside fine (\d+), "
                  r"outside coarse (\d+), outside fine (\d+)", design)
    assert d, "DESIGN.md 4.1 does not state the shipped defaults in the marked sentence"
    assert d.groups() == m.groups(), (d.groups(), m.groups())
