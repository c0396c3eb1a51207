"""CPU: the conditions of the case table of tests/train_matrix_cases.py, on the very inputs tests/test_gpu_train_matrix_sweep.py hands
to the kernels.  For every case: the fp64 references are finite, the fp32 oracle - torch's own fp32 arithmetic - is inside the bounds
with nothing lifted, the kink filter rejected no more than its cap and the case has exactly the rows the table names.  Planted errors
show that the bounds would see a subtly wrong kernel, and the geometry assertions that the table reaches the branches it was built
for (from the constants of the sources, which are read back here)."""
import os
import re

import pytest
import torch

import train_matrix_cases as M

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neo-360_amd", "csrc")


def _finite(d):
    return all(bool(torch.isfinite(v).all()) for v in d.values() if isinstance(v, torch.Tensor))


def _fp32_inside(checks, label):
    M.assert_inside({k: dict(v, ratio=v["fp32_ratio"]) for k, v in checks.items()}, label)
    return max(v["fp32_ratio"] for v in checks.values())


def _broken_share(wrong, ref64, bound):
    """Share of the entries that are non-zero in either reference on which `wrong` misses the bound."""
    live = (wrong != 0) | (ref64 != 0)
    return float((((wrong - ref64).abs() > bound) & live).sum()) / max(int(live.sum()), 1)


# ---- the constants the tables are derived from -------------------------------------------------------------------------------------
def test_constants_mirror_the_sources():
    src = open(os.path.join(CSRC, "train_mlp.hip")).read()
    chain = open(os.path.join(CSRC, "train_chain.h")).read()
    kern = open(os.path.join(CSRC, "kernels.h")).read()
    api = open(os.path.join(CSRC, "api_train.hip")).read()
    const = lambda text, name: int(re.search(r"constexpr (?:int|long) %s = (\d+);" % name, text).group(1))
    assert (const(src, "GTM"), const(src, "GTN"), const(src, "GK")) == (M.GTM, M.GTN, M.GK)
    assert const(src, "DW_ZG") == M.DW_ZG and const(src, "DW_PART_TILES") == M.DW_PART_TILES
    assert const(chain, "CH_ROWS") == M.CH_ROWS and const(kern, "TP_MAX_VIEWS") == M.TP_MAX_VIEWS
    assert "M <= %d && N >= 1 && N <= %d" % (M.MAX_M, M.MAX_N) in api and "in_f <= %d" % M.MAX_F in api
    assert "K / %d > 0 ? K / %d : 1" % (M.DW_MIN_SLICE, M.DW_MIN_SLICE) in src
    assert "const int NT = N > 64 ? 128 : 64;" in src and "(lin & 7)" in src


def test_no_launch_sets_the_epilogue_scale():
    """GemmEpi::scale (the result multiplied by it before the bias) is 1 in every launch: epi() is never called with its sixth argument.
    No entry point can reach another value, so no case of the sweep can tell a kernel that ignores it from one that applies it
    (docs/train_matrix_sweep.md, variant `noscale`).  The day a launch passes a scale, the sweep needs a case that reaches it."""
    src = open(os.path.join(CSRC, "train_mlp.hip")).read()
    calls = []
    for m in re.finditer(r"[ (]epi\(", src):
        depth, args, i = 1, 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            args += src[i] == "," and depth == 1
            i += 1
        if "float scale" not in src[m.end():i - 1]:              # the definition of epi() itself
            calls.append((src[m.end():i - 1], args))
    assert len(calls) > 20 and max(n for _, n in calls) == 5, [a for a, n in calls if n > 5]      # 5: bias, relu, accumulate, mask, ldm
    assert "GemmEpi{bias, mask, ldm, relu, accumulate, scale}" in src and src.count("GemmEpi{") == 1


def test_weight_gradient_scratch_clamp_never_yields_zero_slices():
    """dw_gemm clamps slices x tiles to DW_PART_TILES: with the entry's limits (M <= 1024, N <= 4096: 8 x 32 = 256 tiles of 128 x 128) the
    clamp leaves >= 1 slice, and no shape asks for more partial tiles than the scratch holds."""
    most_tiles = (M.MAX_M // 128) * (M.MAX_N // 128)
    assert most_tiles == 256 and M.DW_PART_TILES // most_tiles >= 1
    for m in (1, 128, 129, 640, M.MAX_M):
        for n in (1, 64, 65, 128, 129, 2048, M.MAX_N):
            for k in (1, 1024, 5000, 70001, 600000, 2000000000):
                nt, tx, ty, slices = M.dw_slices(m, n, k)
                assert slices >= 1 and slices * tx * ty <= M.DW_PART_TILES, (m, n, k, slices)


# ---- primitives ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fwd", "dx"])
def test_linear_cases_fp32_oracle_inside_bounds_and_a_dropped_term_is_seen(kind):
    worst = 0.0
    for case in M.linear_table(kind):
        assert (kind, M.linear_id(case)) not in M.SEQ_LIFT or case[2] >= M.LIFT_MIN_K
        c = M.linear_case(kind, *case)
        assert _finite(c) and tuple(c["ref64"].shape) == case[:2], case
        worst = max(worst, _fp32_inside(M.linear_checks(c, c["ref32"]), (kind, case)))
        if c["ref64_k_dropped"] is not None:
            # the last K element left out of every sum
            assert _broken_share(c["ref64_k_dropped"], c["ref64"], M.linear_bound(kind, c["ref64"])) > 0.9, case
    print(kind, "largest share of a bound the fp32 oracle uses: %.2f" % worst)


def test_weight_gradient_cases_fp32_oracle_inside_bounds_and_a_dropped_row_is_seen():
    worst = 0.0
    for case in M.dw_table():
        assert ("dw", M.dw_id(case)) not in M.SEQ_LIFT or case[2] >= M.LIFT_MIN_K
        c = M.dw_case(*case)
        assert _finite(c["ref64"]) and tuple(c["ref64"]["dw"].shape) == case[:2] and c["gy"].shape[0] == case[2], case
        worst = max(worst, _fp32_inside(M.dw_checks(c, c["ref32"]["dw"], c["ref32"]["db"]), ("dw", case)))
        if c["dw64_row_dropped"] is not None:
            # the last row left out of the reduction (its scale is 10^U(-4, 0): most entries, not all)
            assert _broken_share(c["dw64_row_dropped"], c["ref64"]["dw"], M.dw_bounds(c)["dw"]) > 0.5, case
    print("dw largest share of a bound the fp32 oracle uses: %.2f" % worst)


def test_no_case_with_a_short_reduction_carries_a_lift():
    """A lift is 3 x the error of the sequential fp32 emulation against fp64 - a yardstick computed here on the CPU - and belongs to a
    case of the table with more than 512 terms; the emulation itself is a correct evaluation (a dropped term is still seen)."""
    ids = {("fwd", M.linear_id(c)): c for c in M.linear_table("fwd")}
    assert len(M.SEQ_LIFT) <= 1
    for key in M.SEQ_LIFT:
        case = ids[key]
        assert case[2] >= M.LIFT_MIN_K, key
        c = M.linear_case("fwd", *case)
        emul, err = M.sequential_fp32_forward("fwd", *case)
        lift = M.linear_lift("fwd", case)
        bound = M.linear_bound("fwd", c["ref64"])
        print(key, "sequential emulation error %.3e, lift %.3e, constant bound %.3e" % (err, lift, bound))
        assert lift == 3.0 * err and 0.0 < err < 10 * bound
        assert _broken_share(c["ref64_k_dropped"], c["ref64"], bound + lift) > 0.9
    for case in M.linear_table("fwd") + M.linear_table("dx"):
        if case[2] < M.LIFT_MIN_K:
            assert M.linear_lift("fwd", case) == 0.0 and M.linear_lift("dx", case) == 0.0


def test_tables_reach_the_geometry_they_were_built_for():
    for kind in ("fwd", "dx"):
        t = M.linear_table(kind)
        steps = {(M.full_k_steps(r, n, k)) for r, n, k, _ in t}
        for s in range(1, 8):                       # every prologue / drain arm of the pipelined path, with and without a partial last step
            assert (s, False) in steps and (s, True) in steps, (kind, s)
        assert any(r >= M.GTM and n >= M.GTN and k < M.GK for r, n, k, _ in t)                      # remainder-only reduction
        blocks = {(r + M.GTM - 1) // M.GTM for r, _, _, _ in t}
        assert any(b > M.XCD and b % M.XCD for b in blocks) and M.XCD in blocks and 2 * M.XCD + 4 in blocks
        assert any(n == M.MAX_F for _, n, _, _ in t) and any(k == M.MAX_F for _, _, k, _ in t)
    d = M.dw_table()
    assert any(M.dw_slices(m, n, k)[3] > M.DW_ZG for m, n, k, _ in d)
    assert any(M.dw_slices(m, n, k)[1] * M.dw_slices(m, n, k)[2] == 256 for m, n, k, _ in d)          # the largest grid
    assert {M.dw_slices(m, n, k)[0] for m, n, k, _ in d} == set(M.DW_NT)
    rows = [P * NV for P, NV in M.POINT_VIEWS]
    assert 1 in rows and any(1 < r < M.CH_ROWS for r in rows) and any(r % M.CH_ROWS == 0 for r in rows)
    assert any(r > M.CH_ROWS and r % M.CH_ROWS == 1 for r in rows) and any(r > M.CH_ROWS and r % M.CH_ROWS == 33 for r in rows)
    assert any(r % M.CH_ROWS == 32 for r in rows) and any(NV == M.TP_MAX_VIEWS for _, NV in M.POINT_VIEWS)
    assert any(NV > 1 and P % M.CH_ROWS for P, NV in M.POINT_VIEWS)                                  # a tile that straddles two views
    widths = {c[1] for c in M.chain_table("mip")}
    depths = {c[2] for c in M.chain_table("mip")}
    assert {64, 1024} <= widths and {1, 8} <= depths and any(M.skip_columns(c) for c in M.chain_table("mip"))
    assert {c[5] for c in M.chain_table("mip")} == {1, 2, 7}


# ---- chains --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nerfpp", "nerfpp_proj", "pix_proj", "vanilla", "mip"])
def test_chain_cases_conditions(kind):
    worst, worst_rej = 0.0, 0.0
    for case in M.chain_table(kind):
        c = M.chain_case(case)
        assert _finite(c["ref64"]) and _finite(c["ref32"]), case
        worst = max(worst, _fp32_inside(M.chain_checks(c["ref32"], c["ref64"], c["ref32"]), case))
        assert c["rejected"] <= M.KINK_CAP[kind] * c["candidates"], (case, c["rejected"], c["candidates"])
        worst_rej = max(worst_rej, c["rejected"] / c["candidates"])
        keep, rows = M.chain_rows(case)
        inp = c["inputs"]
        if kind == "mip":
            assert tuple(inp["x0"].shape) == (case[4], case[5], 504) and inp["x0"].shape[0] * inp["x0"].shape[1] == rows
        elif kind == "vanilla":
            assert tuple(inp["x_enc"].shape) == (rows, 1, 63)
        else:
            assert inp["x_enc"].shape[:2] == (case[2], keep) and inp["cond"].shape[0] == rows
            if "pre" in inp:
                assert tuple(inp["pre"].shape) == (rows, 256 if kind == "nerfpp_proj" else 128)
    print(kind, "fp32 oracle's largest share of a bound %.2f, largest rejected share %.3f" % (worst, worst_rej))


@pytest.mark.parametrize("case", [("nerfpp_proj", 33, 3, 4), ("pix_proj", 33, 3)])
def test_projected_reference_is_the_ordinary_mlp_on_the_local_features(case):
    """The reference of a projected chain takes `pre` through selector blocks; it is the ordinary oracle MLP on the local features
    `pre` was formed from (up to the fp32 rounding of `pre`), for the outputs and every gradient both have."""
    c = M.chain_case(case)
    plain = M.chain_oracle(case, c["inputs"], c["state"], torch.float64, selectors=False)
    pe = 21 * case[3] if case[0] == "nerfpp_proj" else 63
    for k, v in c["ref64"].items():
        if k == "g_pre":
            continue
        w = plain[k].clone()
        if k.startswith("gw/"):
            for layer, col in M.local_blocks(case[0], pe):
                if k == "gw/" + layer + ".weight":
                    w[:, col:col + 512] = 0
        assert float((v - w).abs().max()) <= 1e-6 * max(1.0 if k in M.OUTPUT_NAMES else 0.0, float(w.abs().max())), k
    # ... and the gradient of pre carries on into the local features through the weight blocks
    blocks = torch.cat([c["state"][l + ".weight"][:, col:col + 512].double() for l, col in M.local_blocks(case[0], pe)], 0)
    want = plain["g_local"]
    assert float((c["ref64"]["g_pre"] @ blocks - want).abs().max()) <= 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("case", [("nerfpp", 33, 3, 4), ("nerfpp_proj", 65, 2, 4), ("pix_proj", 33, 3), ("nerfpp_proj", 21, 8, 4)])
def test_a_view_left_out_of_the_mean_breaks_a_bound(case):
    assert case in M.chain_table(case[0])
    c = M.chain_case(case)
    wrong = M.chain_oracle(case, c["inputs"], c["state"], torch.float64, variant="view0_weightless")
    assert max(v["ratio"] for v in M.chain_checks(wrong, c["ref64"]).values()) > 1.0


@pytest.mark.parametrize("case", [("nerfpp", 33, 3, 4), ("nerfpp_proj", 65, 2, 4), ("vanilla", 65), ("mip", 192, 6, 1, 147, 7), ("mip", 1024, 8, 1, 65, 1)])
def test_a_skip_segment_left_out_breaks_a_bound(case):
    assert case in M.chain_table(case[0])
    c = M.chain_case(case)
    wrong = M.chain_oracle(case, c["inputs"], c["state"], torch.float64, variant="no_skip")
    assert max(v["ratio"] for v in M.chain_checks(wrong, c["ref64"]).values()) > 1.0
