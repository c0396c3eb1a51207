"""GPU: the rank merge of k_resample against the full bitonic network, bitwise.

k_resample merges the (monotone) previous samples with the new ones by rank and sorts the new samples alone where they are
not in order; a ray whose t_prev is not monotone takes the full network over the whole row.  $NEO_RESAMPLE_FULL_SORT=1 sends
EVERY ray through the full network - what the kernel did before the merge existed.  The variable is read once per process,
so the full-network results come from ONE fresh child process (this file run as a script) that evaluates the same cases;
every case is compared with torch.equal.  No case holds a NaN.

Cases per (n_prev, n_new, R): ascending rows with peaked / flat weights, descending rows (the new samples are a sawtooth:
the segment sort), all-zero weights (the 1e-5 padding), all weight in one bin, ties across the two lists (a zero-width heavy
bin: every new sample equals three previous ones; and a dyadic grid), one shuffled row (fallback next to merged rows), and
per-ray quantiles through training.resample_u, sorted and unsorted.  n_prev / n_new = 129 / 256 (n_out 385: SORT_N 512),
65 / 128 (193: 256), 9 / 16 (25: 256) and 129 / 512 (641: 1024) reach all three instantiations with n_out no power of two;
R = 1, 4, 7 covers a partial last workgroup (4 rays per workgroup).
"""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "NEO_RESAMPLE_FULL_SORT"
SIZES = [(129, 256), (65, 128), (9, 16), (129, 512)]
ROWS = [1, 4, 7]


def _asc(g, R, n):
    return torch.sort(torch.rand(R, n, generator=g) * 2.9 + 0.1, dim=-1).values


def _peaked(g, R, n):
    c = torch.rand(R, 1, generator=g) * n
    k = torch.arange(n, dtype=torch.float32)[None]
    return torch.exp(-0.5 * ((k - c) / (0.03 * n + 1.0)) ** 2) + 1e-3 * torch.rand(R, n, generator=g)


def build_cases():
    """name -> (kind, t_prev, weights, n_new or u, descending); CPU tensors, deterministic."""
    out = {}
    for n_prev, n_new in SIZES:
        for R in ROWS:
            g = torch.Generator().manual_seed(1000 * n_prev + 10 * n_new + R)
            tag = "%d+%d/R%d/" % (n_prev, n_new, R)
            t = _asc(g, R, n_prev)
            td = torch.flip(_asc(g, R, n_prev) / 3.0, dims=[-1]).contiguous()
            out[tag + "asc_peaked"] = ("r", t, _peaked(g, R, n_prev), n_new, False)
            out[tag + "asc_flat"] = ("r", t, torch.full((R, n_prev), 0.01), n_new, False)
            out[tag + "desc_peaked"] = ("r", td, _peaked(g, R, n_prev), n_new, True)
            out[tag + "desc_flat"] = ("r", td, torch.full((R, n_prev), 0.01), n_new, True)
            out[tag + "asc_zero_weights"] = ("r", t, torch.zeros(R, n_prev), n_new, False)
            out[tag + "desc_zero_weights"] = ("r", td, torch.zeros(R, n_prev), n_new, True)
            hot = torch.zeros(R, n_prev)
            j = n_prev // 2
            hot[:, j] = 1.0
            out[tag + "asc_one_bin"] = ("r", t, hot, n_new, False)
            out[tag + "desc_one_bin"] = ("r", td, hot, n_new, True)
            # ties across the lists: pdf weight j sits on bins j - 1, j; with t[j-2] = t[j-1] = t[j] = t[j+1] those bins have
            # zero width at a previous sample, and every new sample is that value
            tt, ttd = t.clone(), td.clone()
            tt[:, j - 2:j + 2] = tt[:, j:j + 1]
            ttd[:, j - 2:j + 2] = ttd[:, j:j + 1]
            out[tag + "asc_ties_zero_width_bin"] = ("r", tt, hot, n_new, False)
            out[tag + "desc_ties_zero_width_bin"] = ("r", ttd, hot, n_new, True)
            grid = (torch.arange(n_prev, dtype=torch.float32) / 64.0 + 0.25)[None].repeat(R, 1).contiguous()
            out[tag + "asc_dyadic_grid"] = ("r", grid, torch.full((R, n_prev), 1.0 / 64.0), n_new, False)
            out[tag + "desc_dyadic_grid"] = ("r", torch.flip(grid, dims=[-1]).contiguous(), torch.full((R, n_prev), 1.0 / 64.0), n_new, True)
            # one row out of order: that row takes the full network, its neighbours the merge
            ts = t.clone()
            ts[R - 1] = ts[R - 1][torch.randperm(n_prev, generator=g)]
            out[tag + "shuffled_row"] = ("r", ts, _peaked(g, R, n_prev), n_new, False)
            tsd = td.clone()
            tsd[0] = tsd[0][torch.randperm(n_prev, generator=g)]
            out[tag + "shuffled_row_desc"] = ("r", tsd, _peaked(g, R, n_prev), n_new, True)
            # per-ray quantiles (training.resample_u)
            u = torch.rand(R, n_new, generator=g) * 0.999
            us = torch.sort(u, dim=-1).values
            out[tag + "u_sorted_asc"] = ("u", t, _peaked(g, R, n_prev), us, False)
            out[tag + "u_unsorted_asc"] = ("u", t, _peaked(g, R, n_prev), u, False)
            out[tag + "u_sorted_desc"] = ("u", td, _peaked(g, R, n_prev), us, True)
            out[tag + "u_unsorted_desc"] = ("u", td, _peaked(g, R, n_prev), u, True)
    for name, (_, t, w, _, _) in out.items():
        assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(w).all()), name
    return out


def run_case(case):
    sys.path.insert(0, ROOT)
    from neo360_amd import ops, training
    kind, t, w, x, desc = case
    t, w = t.cuda(), w.cuda()
    if kind == "r":
        got = ops.resample(t, w, x, descending=desc)
    else:
        got = training.resample_u(t, w, x.cuda(), descending=desc)
    torch.cuda.synchronize()
    return got.cpu()


if __name__ == "__main__":          # the child: every case through the full network
    assert os.environ.get(ENV) == "1"
    torch.save({name: run_case(c) for name, c in build_cases().items()}, sys.argv[1])
    sys.exit(0)


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def all_cases():
    return build_cases()


@pytest.fixture(scope="module")
def full_sort(tmp_path_factory):
    assert not os.environ.get(ENV), "this process must run the merge: unset %s" % ENV
    path = str(tmp_path_factory.mktemp("resample") / "full_sort.pt")
    env = dict(os.environ)
    env[ENV] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return torch.load(path)


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("n_prev,n_new", SIZES, ids=["%d+%d" % s for s in SIZES])
def test_merge_is_bitwise_the_full_network(all_cases, full_sort, n_prev, n_new, R):
    tag = "%d+%d/R%d/" % (n_prev, n_new, R)
    names = [n for n in all_cases if n.startswith(tag)]
    assert len(names) == 18
    for name in names:
        got, want = run_case(all_cases[name]), full_sort[name]
        assert got.shape == want.shape == (R, n_prev + n_new), name
        assert bool(torch.isfinite(want).all()), name
        desc = all_cases[name][4]
        d = want[:, 1:] - want[:, :-1]
        assert bool((d <= 0).all() if desc else (d >= 0).all()), ("the full network's row is not sorted", name)
        assert torch.equal(got, want), (name, int((got != want).sum()), float((got - want).abs().max()))


def test_every_case_was_compared(all_cases, full_sort):
    assert set(all_cases) == set(full_sort) and len(all_cases) == len(SIZES) * len(ROWS) * 18
