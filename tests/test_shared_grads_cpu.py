"""CPU checks of the shared-gradient bookkeeping of the training call (training.shared_grad_group / shared_grad_buffers /
_SharedGradSink): several lookups in the same tensors scatter their backward into ONE set of buffers, which a sink node hands to
autograd once per backward pass.  A stand-in lookup (weighted sum, scattered in place like the library's lookup backward) uses the
helpers exactly as training._Gather does; every case is checked against plain autograd through the same weighted sums.

The cases are the ones the first scheme (a counter of the lookups still to report) got wrong: an extra gradient term on the shared
tensors, two groups in one loss, and a partial backward pass over a retained graph followed by a full one."""
import pytest
import torch

from neo360_amd import training


@pytest.fixture(autouse=True)
def _grad_on():
    with torch.enable_grad():              # the suite's conftest turns autograd off
        yield


class _Lookup(torch.autograd.Function):
    """out = sum_i w * x_i[idx] for the group's tensors; backward scatters g * w into the group's shared buffers and returns None
    for them (or, without a group, private buffers returned to autograd)."""

    @staticmethod
    def forward(ctx_, idx, w, shared, *xs):
        ctx_.meta = (idx, w, shared, [x.shape for x in xs])
        return sum((x.reshape(-1)[idx] * w).sum() for x in xs).reshape(1)

    @staticmethod
    def backward(ctx_, g):
        idx, w, shared, shapes = ctx_.meta
        make = lambda: [torch.zeros(s, dtype=torch.float64) for s in shapes]
        bufs = training.shared_grad_buffers(shared, make) if shared is not None else make()
        for b in bufs:                                   # scatter in place, as the library's lookup backward does
            b.view(-1).index_add_(0, idx, (g * w).expand(len(idx)))
        if shared is not None:
            return (None, None, None) + (None,) * len(bufs)
        return (None, None, None) + tuple(bufs)


def lookup(xs, idx, w, shared):
    if shared is None:
        return _Lookup.apply(idx, w, None, *xs)
    return _Lookup.apply(idx, w, shared, *training.shared_grad_group(shared, xs))


def _tensors():
    g = torch.Generator().manual_seed(0)
    return [torch.randn(4, 6, dtype=torch.float64, generator=g).requires_grad_() for _ in range(3)]


IDX = [torch.tensor([0, 5, 7]), torch.tensor([5, 11, 23]), torch.tensor([1, 1, 2, 19]), torch.tensor([23, 0])]
W = [1.0, 2.0, 3.0, 4.0]


def _plain(xs, which, extra=None):
    """The same loss through plain autograd (a private gradient per lookup)."""
    loss = sum(lookup(xs, IDX[i], W[i], None).sum() for i in which)
    if extra is not None:
        loss = loss + extra(xs)
    return torch.autograd.grad(loss, xs)


def test_all_lookups():
    xs = _tensors()
    sh = {}
    outs = [lookup(xs, IDX[i], W[i], sh) for i in range(4)]
    got = torch.autograd.grad(sum(o.sum() for o in outs), xs)
    for a, b in zip(got, _plain(xs, range(4))):
        assert torch.equal(a, b)


def test_extra_gradient_term_on_the_shared_tensors():
    xs = _tensors()
    sh = {}
    reg = lambda ts: 0.1 * sum((t ** 2).sum() for t in ts)
    outs = [lookup(xs, IDX[i], W[i], sh) for i in range(4)]
    got = torch.autograd.grad(sum(o.sum() for o in outs) + reg(xs), xs)
    for a, b in zip(got, _plain(xs, range(4), reg)):
        assert torch.allclose(a, b, rtol=0, atol=1e-12)


def test_two_groups_in_one_loss_backward_into_grad():
    xs = _tensors()
    sh1, sh2 = {}, {}
    o1 = [lookup(xs, IDX[i], W[i], sh1) for i in range(4)]
    o2 = [lookup(xs, IDX[i], 2 * W[i], sh2) for i in range(4)]
    (sum(o.sum() for o in o1) + sum(o.sum() for o in o2)).backward()
    want = [a + b for a, b in zip(_plain(xs, range(4)), [2 * t for t in _plain(xs, range(4))])]
    for x, b in zip(xs, want):
        assert torch.allclose(x.grad, b, rtol=0, atol=1e-12)


def test_partial_pass_retained_then_full_pass():
    xs = _tensors()
    sh = {}
    outs = [lookup(xs, IDX[i], W[i], sh) for i in range(4)]
    g1 = torch.autograd.grad(outs[2].sum() + outs[3].sum(), xs, retain_graph=True)
    kept = [t.clone() for t in g1]
    g2 = torch.autograd.grad(sum(o.sum() for o in outs), xs)
    for a, b in zip(g1, _plain(xs, (2, 3))):
        assert torch.equal(a, b)
    for a, b in zip(g1, kept):                       # pass 2 must not write into what pass 1 returned
        assert torch.equal(a, b)
    for a, b in zip(g2, _plain(xs, range(4))):
        assert torch.equal(a, b)
    assert sh["box"]["bufs"] is None                 # released by the sink after each pass


def test_a_group_serves_one_set_of_tensors():
    xs, ys = _tensors(), _tensors()
    sh = {}
    lookup(xs, IDX[0], 1.0, sh)
    with pytest.raises(ValueError):
        lookup(ys, IDX[0], 1.0, sh)


def test_no_reference_cycle_through_the_sink():
    """The group's dict holds the sink's outputs; the sink must not hold the dict (a cycle would keep the shared tensors - an
    encoder's 100s of MB of planes - alive after the step)."""
    import gc
    import weakref
    xs = _tensors()
    sh = {}
    out = lookup(xs, IDX[0], 1.0, sh)
    ref = weakref.ref(sh["sunk"][0])
    del out, sh
    gc.disable()
    try:
        assert ref() is None
    finally:
        gc.enable()
