"""CPU: the content of the decomposed-render fixture and the restatements of tests/decompose_cases.py (no GPU).

The oracle's level-0 rows of the 96 strided rays (17 samples each) against the seven instances [A, B, F, G, D, A, G]: who owns
what under the DECOMPOSITION RULE.  The counts are computed here, by the restatement, and pinned: tests/test_gpu_decompose.py
relies on the fixture holding samples inside two DISTINCT boxes (A and G), an empty instance and two exact duplicates."""
import torch

import decompose_cases as dc
import edit_cases as ec
import instance_cases as ic

OWNED_96 = [45, 13, 6, 9, 0, 0, 0, 1559]           # A, B, F, G, D, second A, second G, rest
OWNED_96_G_FIRST = [30, 13, 6, 24, 0, 0, 0, 1559]  # the list with A and G swapped: G, B, F, A, D, A, G, rest


def _level0():
    L = ec.oracle_level0(96)
    return L["fg_t"], L["near"], L["far"]


def test_every_sample_has_one_owner_and_the_counts_are_pinned():
    t, near, far = _level0()
    assert tuple(t.shape) == (96, 17) and tuple(near.shape) == (dc.K7, 96)
    own = dc.owners(t, near, far)
    counts = [int((own == s).sum()) for s in range(dc.K7 + 1)]
    assert counts == OWNED_96
    assert sum(counts) == 1632 == t.numel()
    # the duplicates at index 5 and 6 and the empty D own nothing
    assert counts[5] == counts[6] == counts[ic.D] == 0
    inside = ec.inside_mask(t.float(), near, far)
    assert int(inside[5].sum()) == int(inside[ic.A].sum()) > 0 and int(inside[6].sum()) == int(inside[ic.G].sum()) > 0
    assert int(inside[ic.D].sum()) == 0
    # the owned counts of A, B, F, G are the size of the union of the intervals: a sample inside two boxes counts once
    union = int(inside.any(dim=0).sum())
    assert counts[ic.A] + counts[ic.B] + counts[ic.F] + counts[ic.G] == union == 73
    assert int(inside[:5].sum()) == 94 > union
    # samples inside two DISTINCT boxes: A and G, and only them
    two = inside[:5].sum(dim=0) >= 2
    assert int(two.sum()) == 21 and torch.equal(two, inside[ic.A] & inside[ic.G])
    # an owner is a hit pair that holds the sample; the rest is inside nothing
    for i in range(dc.K7):
        assert bool(inside[i][own == i].all())
    assert not bool(inside.any(dim=0)[own == dc.K7].any())


def test_swapping_a_and_g_moves_exactly_the_shared_samples():
    t, near, far = _level0()
    own = dc.owners(t, near, far)
    perm = [ic.G, ic.B, ic.F, ic.A, ic.D, 5, 6]
    swapped = dc.owners(t, near[perm], far[perm])
    assert [int((swapped == s).sum()) for s in range(dc.K7 + 1)] == OWNED_96_G_FIRST
    back = torch.tensor(perm + [dc.K7])            # slot of the swapped list -> instance of the original one
    moved = back[swapped] != own
    inside = ec.inside_mask(t.float(), near, far)
    assert torch.equal(moved, inside[ic.A] & inside[ic.G]) and int(moved.sum()) == 21
    assert bool((own[moved] == ic.A).all()) and bool((back[swapped][moved] == ic.G).all())


def test_the_fp64_restatement_adds_up_and_respects_the_edges():
    g = torch.Generator().manual_seed(3)
    R, N, K = 6, 9, 3
    t = torch.sort(torch.rand(R, N, generator=g) + 0.1, dim=-1).values
    rs = torch.rand(R, N, 4, generator=g)
    w = torch.rand(R, N, generator=g) / N
    near = torch.stack([t[:, 2], t[:, 1], torch.full((R,), float("nan"))])      # closed ends: on lo and on hi
    far = torch.stack([t[:, 4], t[:, 6], torch.full((R,), 2.0)])
    near[1, 0], far[1, 0] = 0.7, 0.2                                            # reversed: a miss
    far[0, 1] = float("inf")                                                    # infinite: a miss
    d = dc.decompose_f64(rs, t, w, near, far)
    own = d["own"]
    assert bool((own[2:, 2:5] == 0).all()) and bool((own[2:, 1] == 1).all()) and bool((own[2:, 5:7] == 1).all())
    assert bool((own[2:, 0] == K).all()) and bool((own[2:, 7:] == K).all())
    assert bool((own[0] != 1).all()) and bool((own[1] != 0).all()) and bool((own != 2).all())
    assert torch.equal(d["count"].sum(dim=0), torch.full((R,), N))
    assert bool((d["acc"][2] == 0).all()) and bool((d["rgb"][2] == 0).all())
    assert torch.allclose(d["acc"].sum(dim=0), w.double().sum(dim=1), rtol=0, atol=1e-14)
    assert torch.allclose(d["rgb"].sum(dim=0), (w.double()[..., None] * rs.double()[..., :3]).sum(dim=1), rtol=0, atol=1e-14)
    assert torch.allclose(d["depth"].sum(dim=0), (w.double() * t.double()).sum(dim=1), rtol=0, atol=1e-14)
    assert torch.equal(d["S_acc"], d["acc"]) and torch.equal(d["S_depth"], d["depth"])      # non-negative rows


def test_the_id_rule():
    nan = float("nan")
    #                    ray: 0     1     2     3     4     5     6     7
    acc = torch.tensor([[0.50, 0.20, 0.00, 0.30, nan, 0.40, 0.25, 0.0],      # instance 0
                        [0.50, 0.30, 0.00, 0.10, 0.2, 0.10, 0.25, -0.1],     # instance 1
                        [0.10, 0.30, 0.00, 0.30, 0.1, 0.45, 0.25, 0.0]])     # the rest
    # ties go to the lower index; the winner must reach the rest; zero mass is nobody's; a NaN never wins; equality is enough
    assert dc.id_rule(acc).tolist() == [0, 1, -1, 0, 1, -1, 0, -1]
    lam = torch.tensor([0.3, 0.1, 0.0, 0.0, nan, 0.0, 0.01, 0.0])
    assert dc.id_rule(acc, lam).tolist() == [0, -1, -1, 0, -1, -1, -1, -1]
    assert dc.id_rule(acc, lam[:, None]).tolist() == dc.id_rule(acc, lam).tolist()
    assert dc.id_rule(acc[2:]).tolist() == [-1] * 8                             # K = 0
    nan_rest = torch.tensor([[0.5], [nan]])
    assert dc.id_rule(nan_rest).tolist() == [-1]
