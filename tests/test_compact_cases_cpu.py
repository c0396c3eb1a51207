"""CPU: the conditions of the compact-launch case table (tests/compact_cases.py) that tests/test_gpu_compact_sweep.py relies on:
masks and counts, the tile edges the counts were chosen for, the CPU models of the compaction and of the instance windows, the call
order, the fp32 oracle's own distance from its fp64 twin on the table's rays, and the visibility margins behind the id rule."""
import pytest
import torch

import compact_cases as C
import object_cases as oc


def test_every_mask_and_its_intervals():
    seen = set()
    for kind, R, what in C.table():
        m = C.case_mask(kind, R, what)
        assert m.dtype == torch.bool and m.shape == (R,)
        near, far = C.intervals(m)
        assert near.dtype == far.dtype == torch.float32
        lo, hi, hit = oc.hit_rule(near, far)
        assert torch.equal(hit, m), (kind, R, what)                  # every miss encoding is a miss, every hit a hit
        assert bool((lo[m] >= 0.3).all()) and bool((hi[m] <= 0.9).all()) and bool((hi[m] - lo[m] > 0.58).all())
        misses = int((~m).sum())
        if misses >= len(C.MISSES):                                  # every table with six misses mixes all six encodings
            n, f = near[~m], far[~m]
            kinds = [((n == 0) & (f == 0)).any(), torch.isnan(n).any(), torch.isnan(f).any(), torch.isinf(n).any(),
                     ((n == 0) & (f == lo[~m]) & (f > 0)).any(), ((f < n) & (f > 0.1)).any()]
            assert all(bool(k) for k in kinds), (kind, R, what, kinds)
        seen.add((kind, R, what))
    assert len(seen) == len(C.table())
    # the patterns are what their names say
    for R in C.R_LIST:
        count = {p: (None if C.pattern_mask(R, p) is None else int(C.pattern_mask(R, p).sum())) for p in C.PATTERNS}
        assert count["none"] == 0 and count["all"] == R and count["first"] == 1 and count["last"] == 1
        assert count["even"] == (R + 1) // 2 and count["odd"] == R // 2
        assert count["wave1"] == (64 if R >= 128 else None)
        assert count["not_wg0"] == (R - 256 if R > 256 else None)
        assert count["last_wg"] == ({257: 1, 513: 1}.get(R))
        assert bool(C.pattern_mask(R, "last")[R - 1]) and bool(C.pattern_mask(R, "first")[0])
        if R >= 255:
            assert 0.35 * R < count["half"] < 0.65 * R and 0 < count["sparse"] < R // 16, (R, count)
        assert torch.equal(C.pattern_mask(R, "half"), C.pattern_mask(R, "half"))       # a fixed generator
    assert {R for _, R, _ in C.table()} == set(C.R_LIST)
    assert sum(1 for k, _, _ in C.table() if k == "pattern") == 8 * 8 + 4 + 2 + 2       # wave1 at four counts, the two workgroup patterns at two
    w = C.pattern_mask(513, "wave1")
    assert bool(w[64:128].all()) and int(w.sum()) == 64
    lw = C.pattern_mask(513, "last_wg")
    assert bool(lw[512]) and not bool(lw[:512].any())


def test_fixed_counts_and_tile_edges():
    prev = torch.zeros(C.FIXED_R, dtype=torch.bool)
    for k in C.FIXED_COUNTS:
        m = C.fixed_mask(k)
        assert int(m.sum()) == k and bool((m | ~prev).all())       # nested prefixes of one permutation
        prev = m
    assert sorted(C.FIXED_ORDER) == sorted(C.FIXED_COUNTS) and sorted(C.PATTERN_ORDER) == sorted(C.PATTERNS)
    aligned = [k for k in C.FIXED_COUNTS if k * C.N0 % C.TM == 0]
    # 256 rows x 4 = 16 whole tiles as well: the list's fourth aligned count (the 3 + 1 pair runs on the first three, where its
    # level 1 is never aligned; 256 x 5 = 20 tiles would be)
    assert aligned == list(C.ALIGNED_COUNTS) == [16, 112, 128, 256] and C.TILE_EDGE_COUNTS == C.ALIGNED_COUNTS[:3]
    assert [C.tiles(k, C.N0) for k in C.FIXED_COUNTS] == [1, 1, 1, 2, 7, 7, 8, 8, 8, 9, 16]
    assert C.tiles(16, C.N1) == 2 and 16 * C.N1 % C.TM == 0
    # 3 + 1: level 1 ends 16 and 48 points into a tile at 16 and 112 rows; 128 rows x 5 = 10 whole tiles, aligned at both levels
    assert [k * C.N1_ODD % C.TM for k in C.TILE_EDGE_COUNTS] == [16, 48, 0]
    assert (C.N0, C.N1, C.N1_ODD) == (4, 8, 5) and C.N0 >= 4         # the resampler's n_prev >= 4
    assert set(C.CHUNK_COUNTS) <= set(C.FIXED_COUNTS) and C.FIXED_R == 4 * C.CHUNK + 1


def test_compaction_model_inverts_on_every_case():
    masks = [C.case_mask(*c) for c in C.table()] + [C.big_wg_mask(), C.scatter_mask(), C.k32_mask(), C.k32_big_mask()]
    masks += [C.window_mask(K, R, c) for K in C.WINDOW_K for R in C.WINDOW_R for c in C.window_counts(K, R)]
    for m in masks:
        mp, slot, totals, prefix = C.compaction_model(m)
        flat = m.reshape(-1)
        n = int(flat.sum())
        assert mp.shape == (n,) and bool((mp[1:] > mp[:-1]).all())
        r = torch.arange(flat.shape[0])
        assert torch.equal(mp[slot[flat]], r[flat]) and bool((slot[~flat] == -1).all())
        assert int(totals.sum()) == n and totals.shape[0] == (flat.shape[0] + C.BLOCK - 1) // C.BLOCK
        # a workgroup's first survivor sits at its prefix
        for b in range(totals.shape[0]):
            if int(totals[b]):
                first = int(flat[b * C.BLOCK:(b + 1) * C.BLOCK].nonzero()[0]) + b * C.BLOCK
                assert int(slot[first]) == int(prefix[b])


def test_call_order_puts_few_after_many():
    tab = C.table()
    counts = [int(C.case_mask(*c).sum()) for c in tab]
    at = {c: i for i, c in enumerate(tab)}
    assert tab[at[("pattern", 1, "all")] - 1][1] == 513, "R = 513 comes directly before R = 1"
    assert counts[at[("pattern", 1, "all")] - 1] == 256
    for R in (257, 513):
        i = at[("pattern", R, "all")]
        assert counts[i] == R and counts[i + 1] == 1
        j = at[("pattern", R, "half")]
        assert counts[j] > 8 * counts[j + 1]
    f = [at[("fixed", 257, k)] for k in C.FIXED_ORDER]
    assert f == list(range(f[0], f[0] + len(f)))
    assert [counts[i] for i in f[:6]] == [256, 1, 129, 15, 128, 16]
    assert len(C.REPEATED) == 6 and all(c in at for c in C.REPEATED)
    assert ("pattern", 1, "all") in C.REPEATED and ("fixed", 257, 16) in C.REPEATED


def test_grid_stride_cases_reach_what_they_are_for():
    m = C.big_wg_mask()
    _, slot, totals, prefix = C.compaction_model(m)
    assert totals.shape[0] == 258 and all(int(totals[b]) > 0 for b in (0, 254, 255, 256, 257))
    # workgroup 257 sums 257 totals: thread 0 reads totals[0] and, on its SECOND trip, totals[256] - which is not zero
    assert int(totals[256]) > 0 and int(prefix[257]) == int(totals[:257].sum()) > int(totals[:256].sum())
    assert all(bool(m[r]) for r in C.BIG_WG_FORCED) and 150 < int(m.sum()) < 400
    assert C.SCATTER_R * (C.N_COARSE + 1 + C.SCATTER_N_FINE) == 4195323 > C.GRID_CAP == 4194304
    assert C.N_COARSE + 1 + C.SCATTER_N_FINE == 1023 and int(C.scatter_mask().sum()) == 5
    assert sorted({h // C.SCATTER_CHUNK for h in C.SCATTER_HITS}) == [0, 1, 2]
    assert C.LEVEL0_R * (C.LEVEL0_N_COARSE + 1) == 4214800 > C.GRID_CAP
    assert C.LEVEL0_R % C.LEVEL0_CHUNK == 16
    assert C.K32 * C.K32_BIG_R == 65824 and (65824 + 255) // 256 == 258
    big = C.k32_big_mask()
    assert 350 < int(big.sum()) < 700 and all(int(big[i].sum()) > 0 for i in C.K32_BIG_ROWS)
    assert int(C.compaction_model(big)[2][256:].sum()) > 0
    fill = C.fill_mask()
    assert C.K32 * C.FILL_R == 4194336 > C.GRID_CAP and 31 * C.FILL_R < C.GRID_CAP          # the second trip lies in instance 31's row
    second = fill.reshape(-1)[C.GRID_CAP:]
    assert second.shape[0] == 32 and int(second.sum()) == 1 and bool(second[-1])
    assert 500 < int(fill.sum()) < 1500 < C.FILL_R and all(int(fill[i].sum()) > 0 for i in C.FILL_ROWS)      # one window


def test_instance_window_masks():
    for K in C.WINDOW_K:
        for R in C.WINDOW_R:
            counts = C.window_counts(K, R)
            assert counts[0] == 0 and counts[-1] == K * R and R in counts and (1 in counts)
            assert (R + 1 in counts) == (K >= 2) and (K < 2 or 2 * R in counts) and (R - 1 in counts)
            for c in counts:
                m = C.window_mask(K, R, c)
                assert m.shape == (K, R) and int(m.sum()) == c
                rows = C.windows_model(c, K, R)
                # the windows partition the pair list: consecutive, at most R rows each, empty ones at the end only
                assert sum(rows) == c and all(0 <= n <= R for n in rows)
                assert all(rows[p] == R for p in range(K) if sum(rows[p + 1:]) > 0)
                w = C.window_of_pairs(m)
                assert [int((w == p).sum()) for p in range(K)] == rows
                if c > R:        # a second window exists: some ray has one instance in window 0 and another in window 1
                    split = C.split_rays(m)
                    assert split.numel() >= 1, (K, R, c)
                    ray = int(split[0])
                    pairs = [i * R + ray for i in range(K) if bool(m[i, ray])]
                    cs = torch.cumsum(m.reshape(-1).long(), 0) - 1
                    assert {int(cs[p]) // R for p in pairs} >= {0, 1}
                near, far = C.instance_intervals(m)
                assert torch.equal(oc.hit_rule(near, far)[2], m)
                if K >= 2:
                    both = m[0] & m[1]
                    tie = both & (near[0] == near[1])
                    assert torch.equal(tie, both & (torch.arange(R) % C.TIE_EVERY == 0))
            full = C.window_mask(K, R, K * R)
            assert bool(full.all())
            near, _ = C.instance_intervals(full)
            if K >= 2 and R >= 5:
                assert int((near[0] == near[1]).sum()) == (R + 2) // 3
            if K == 3:           # otherwise distinct and in index order
                assert bool((near[2] > near[1]).all()) and bool((near[1] >= near[0]).all())
    assert C.windows_model(5, 3, 5) == [5, 0, 0] and C.windows_model(6, 3, 5) == [5, 1, 0] and C.windows_model(4, 3, 5) == [4, 0, 0]


def test_k32_designed_rays():
    m = C.k32_mask()
    near, far = C.instance_intervals(m, designed=True)
    lo, hi, hit = oc.hit_rule(near, far)
    assert torch.equal(hit, m) and m.shape == (32, 65)
    assert m[:, C.ONLY31].nonzero().reshape(-1).tolist() == [31]
    assert m[:, C.NEAREST31].nonzero().reshape(-1).tolist() == [3, 17, 31]
    assert float(lo[31, C.NEAREST31]) < float(lo[3, C.NEAREST31]) < float(lo[17, C.NEAREST31])
    assert m[:, C.TIE31].nonzero().reshape(-1).tolist() == [0, 31] and float(lo[0, C.TIE31]) == float(lo[31, C.TIE31])
    assert bool(m[:, C.ALL32].all()) and bool((lo[1:, C.ALL32] >= lo[:-1, C.ALL32]).all())
    assert 0.2 * 32 * 65 < int(m.sum()) < 0.3 * 32 * 65 and int(m[31].sum()) >= 4
    assert float(far.nan_to_num(0.0, 0.0, 0.0).max()) < 2.1                     # the depth bound K 2^-22 assumes d_i <= far < 2.1


ORACLE_SHARES = {}


@pytest.mark.parametrize("R", C.R_LIST)
def test_fp32_oracle_stays_below_the_tolerance_on_the_tables_rays(R):
    """Truth 4's bound is 1e-4 with no exempt rays; a row whose own fp32-vs-fp64 noise reaches 1e-4 would get 1e-4 + 3 x it.  On
    these inputs no row needs that (the cap is one ray a case)."""
    near, far = C.intervals(torch.ones(R, dtype=torch.bool))
    for n_fine in ((C.N_FINE, C.N_FINE_ODD) if R == C.FIXED_R else (C.N_FINE,)):
        o32, o64 = C.oracle_pair(R, near, far, n_fine)
        hit = torch.ones(R, dtype=torch.bool)
        b = C.oracle_bounds(o32, o64, hit)
        worst = {k: float(v[0].max()) for k, v in b.items()}
        print("R %d, 3 + %d: fp32 oracle against fp64, largest per quantity" % (R, n_fine), {k: "%.2e" % v for k, v in worst.items()})
        assert C.lifted_rays(b) <= C.MAX_LIFTED_RAYS
        assert max(worst.values()) < C.TOL
        # a hit ray's oracle rows do not depend on the pattern: every second ray as a miss leaves the others' rows unchanged
        if R >= 63 and n_fine == C.N_FINE:
            m = C.pattern_mask(R, "even")
            n2, f2 = C.intervals(m)
            thin = oc.oracle_render(oc.state(), C.rays(R), n2, f2, C.N_COARSE, n_fine)
            assert all(torch.equal(thin[k][m], o32[k][m]) for k in ("t0", "t1", "rgb0", "rgb1", "acc1", "depth1"))


def _margin_frac(near, far, mask, rows, K):
    p, a, d = rows
    z = ~mask
    p, a, d = p.clone(), a.clone(), d.clone()
    p[z], a[z], d[z] = 0.0, 0.0, 0.0
    c = C.composite64(near, far, p, a, d, white=False)
    close = ((c["best"] - c["second"]) <= K * 2.0 ** -22) & c["any_hit"]
    return float(close.float().mean()), c


def test_visibility_margins_on_the_fp32_oracles_rows():
    """The id rule is exact where best and second-best visibility differ by more than K 2^-22: at most 2 % of a case's rays may
    fall inside that margin (on the CPU oracle's fp32 per-instance rows)."""
    for R in C.WINDOW_R:
        full = torch.ones(3, R, dtype=torch.bool)
        near3, far3 = C.instance_intervals(full)
        rows = C.oracle_instance_rows(near3, far3, ("windows", R))
        for K in C.WINDOW_K:
            for c in C.window_counts(K, R):
                m = C.window_mask(K, R, c)
                near, far = C.instance_intervals(m)
                frac, c64 = _margin_frac(near, far, m, tuple(x[:K] for x in rows), K)
                assert frac <= C.MARGIN_MAX_FRAC, (K, R, c, frac)
                assert torch.equal(c64["id"] >= 0, m.any(dim=0))                   # every hit instance is visible at bias + 6
    m = C.k32_mask()
    near, far = C.instance_intervals(m, designed=True)
    full = torch.ones_like(m)
    nf, ff = C.instance_intervals(full, designed=True)
    rows = C.oracle_instance_rows(nf, ff, ("k32", C.K32_R))
    frac, c64 = _margin_frac(near, far, m, rows, C.K32)
    print("K = 32, R = 65: %.3f of the rays inside the id margin" % frac)
    assert frac <= C.MARGIN_MAX_FRAC
    ids = c64["id"]
    assert int(ids[C.ONLY31]) == 31 and int(ids[C.NEAREST31]) == 31 and int(ids[C.TIE31]) == 0 and int(ids[C.ALL32]) == 0


def test_cull_targets_and_threshold():
    assert C.cull_targets(65) == [0, 1, 15, 16, 17, 64, 65]
    assert C.cull_targets(257) == [0, 1, 15, 16, 17, 256, 257, 112, 128, 129]
    m = torch.rand(65, generator=C._gen(65)) * 0.5 + 0.01
    for k in C.cull_targets(65):
        eps, tie = C.cull_eps(m, k)
        assert not tie and 0 < eps < 1
        assert int((~(m < eps)).sum()) == k                                      # the keep rule !(lambda < eps)
    m[3] = m[7]
    rank = int((m >= m[3]).sum())
    assert C.cull_eps(m, rank - 1)[1] and not C.cull_eps(m, rank)[1]
