"""CPU: who writes which position of the outside-sphere positional encoding (csrc/pe_schedule.h), compiled into a stand-alone
host program.

Outside the unit sphere the point evaluator k_tp_mlp_hpp<4> encodes (x, y, z, 1/r) into 96 positions per row: 40 (sin, cos) pairs
in the pair order launch_tp_pack_hp packs (pair = octave * 4 + coordinate), the four identity features, 12 zeros.  1/r does not depend
on the source view, so its 10 pairs, identity position 83 and the padding are written once per tile and the view loop writes the
30 pairs of x, y, z and identity positions 80..82.  The header says which wave writes what; the kernel follows it.  Checked here:

* the per-tile and the per-view assignments together write each of the 96 positions exactly once;
* the feature every position holds is the column of pts_linears.0 that launch_tp_pack_hp packs at that position (px.col);
* the pairs of a view differ by at most one between the waves (8 / 8 / 7 / 7), and so do the per-tile ones (3 / 3 / 2 / 2).

The program is built with -fsanitize=undefined,address where the host compiler has the runtimes (its own main, no preloading); a
failed sanitized build is reported as a warning before the plain build is tried."""
import os
import re
import shutil
import subprocess
import warnings

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neo-360_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "pe_schedule.h"
// one line per written position: <when> <wave> <position> <octave> <coordinate> <kind>; kind s = sine, c = cosine, i = identity, z = zero
int main() {
    namespace ps = neo::pe_sched;
    printf("consts %d %d %d %d %d %d %d %d\n", ps::WAVES, ps::OCTAVES, ps::COORDS, ps::WIDTH, ps::IDENT_POS, ps::PAD_POS, ps::VIEW_SLOTS,
           ps::TILE_SLOTS);
    for (int q = 0; q < ps::WAVES; ++q) {
        for (int slot = 0; slot < ps::VIEW_SLOTS; ++slot)
            if (slot < ps::view_pairs(q)) {
                const int oct = ps::view_octave(q, slot), a = ps::view_coord(q, slot), pos = ps::pair_pos(oct, a);
                printf("view %d %d %d %d s\nview %d %d %d %d c\n", q, pos, oct, a, q, pos + 1, oct, a);
            }
        if (q == ps::VIEW_IDENT_WAVE)
            for (int a = 0; a < 3; ++a) printf("view %d %d -1 %d i\n", q, ps::IDENT_POS + a, a);
        for (int slot = 0; slot < ps::TILE_SLOTS; ++slot)
            if (slot < ps::tile_pairs(q)) {
                const int oct = ps::tile_octave(q, slot), pos = ps::pair_pos(oct, 3);
                printf("tile %d %d %d 3 s\ntile %d %d %d 3 c\n", q, pos, oct, q, pos + 1, oct);
            }
        if (q == ps::TILE_IDENT_WAVE) {
            printf("tile %d %d -1 3 i\n", q, ps::IDENT_POS + 3);
            for (int e = 0; e < 4; ++e) printf("tile %d %d -1 -1 z\n", q, ps::PAD_POS + e);
        }
        if (q == ps::TILE_PAD_WAVE)
            for (int e = 4; e < 12; ++e) printf("tile %d %d -1 -1 z\n", q, ps::PAD_POS + e);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def schedule(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (set CXX)")
    d = tmp_path_factory.mktemp("pe_schedule")
    src, exe = str(d / "pe_schedule_main.cpp"), str(d / "pe_schedule_main")
    with open(src, "w") as f:
        f.write(PROGRAM)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    build = "with -fsanitize=undefined,address"
    if r.returncode != 0:        # a compiler without the sanitizer runtimes: the plain program prints the same values
        warnings.warn("pe_schedule host program: the sanitized build failed, checking the plain build instead:\n" + r.stderr[-1500:])
        build = "WITHOUT sanitizers"
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, (build, r.stderr)
    print("pe_schedule host program built %s (%s)" % (build, cxx))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (build, r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert lines[0][0] == "consts"
    consts = dict(zip(("waves", "octaves", "coords", "width", "ident", "pad", "view_slots", "tile_slots"), map(int, lines[0][1:])))
    recs = [(w, int(q), int(pos), int(o), int(a), k) for w, q, pos, o, a, k in lines[1:]]
    return consts, recs


def test_constants_are_the_kernels(schedule):
    consts, _ = schedule
    assert consts == dict(waves=4, octaves=10, coords=4, width=96, ident=80, pad=84, view_slots=8, tile_slots=3)


def test_every_position_is_written_exactly_once(schedule):
    consts, recs = schedule
    pos = sorted(r[2] for r in recs)
    assert pos == list(range(consts["width"])), pos
    per_view = sorted(r[2] for r in recs if r[0] == "view")
    per_tile = sorted(r[2] for r in recs if r[0] == "tile")
    assert len(per_view) == 63 and len(per_tile) == 33
    # the per-tile positions are exactly the ones that do not depend on the view: coordinate 3 (1/r) and the padding
    assert all(r[4] == 3 or r[5] == "z" for r in recs if r[0] == "tile")
    assert all(r[4] in (0, 1, 2) and r[5] != "z" for r in recs if r[0] == "view")


def test_positions_hold_the_columns_the_weights_are_packed_for(schedule):
    """launch_tp_pack_hp packs, at stage position 128 + j, column C + (j odd: 10 C) + j / 2 of pts_linears.0 for j < 20 C, then the C
    identity columns, then nothing.  The reference's columns: [x (C) | sin, octave-major (10 C) | cos (10 C)]."""
    consts, recs = schedule
    C = consts["coords"]
    src = open(os.path.join(CSRC, "mlp_tp_hp.hip")).read()
    assert re.search(r"for \(int j = 0; j < 20 \* C; \+\+j\) px\.col\[128 \+ j\] = \(short\)\(C \+ \(\(j & 1\) \? 10 \* C : 0\) \+ \(j >> 1\)\);", src)
    assert re.search(r"for \(int a = 0; a < C; \+\+a\) px\.col\[128 \+ 20 \* C \+ a\] = \(short\)a;", src)
    col = [-1] * consts["width"]
    for j in range(20 * C):
        col[j] = C + (10 * C if j & 1 else 0) + (j >> 1)
    for a in range(C):
        col[20 * C + a] = a
    for _, _, pos, oct_, a, kind in recs:
        want = {"s": C + oct_ * C + a, "c": C + 10 * C + oct_ * C + a, "i": a, "z": -1}[kind]
        assert col[pos] == want, (pos, oct_, a, kind, col[pos], want)
    assert sorted(c for c in col if c >= 0) == list(range(21 * C))       # all 84 features, each once


def test_pairs_are_balanced_over_the_waves(schedule):
    consts, recs = schedule
    for when, total in (("view", 30), ("tile", 10)):
        n = [sum(1 for r in recs if r[0] == when and r[1] == q and r[5] == "s") for q in range(consts["waves"])]
        assert sum(n) == total and max(n) - min(n) <= 1, (when, n)
    n_view = [sum(1 for r in recs if r[0] == "view" and r[1] == q and r[5] == "s") for q in range(4)]
    assert n_view == [8, 8, 7, 7] and max(n_view) <= consts["view_slots"]
    # the identity features ride on a wave with the smaller number of pairs
    ident = {r[1] for r in recs if r[0] == "view" and r[5] == "i"}
    assert len(ident) == 1 and n_view[ident.pop()] == min(n_view)
