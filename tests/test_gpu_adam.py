"""GPU: ``pob_adam_step`` (k_adam_step and k_adam_advance) against ``adam_step_ref`` of
po-brax_amd/csrc/pob_mlp.h (tests/host/adam_host.cpp), bit for bit over three carried steps, and
``training.optim.FusedAdam`` on device leaves.

Every segment is a view into a larger buffer filled with a sentinel: the elements on both sides of it
must keep their bits.  Offsets are in floats from a 16-byte aligned base: 4 keeps the segment aligned
(all of it 16-byte groups but the tail), 1 leaves it 4-byte aligned only (a head of three scalar
elements when theta, grad, m and v agree, an all-scalar segment when they do not).  Lengths 1 .. 1 027
cross the 256-lane block and every head / body / tail split; the last case is the parameter counts of
the reference's networks (``make_models(16, 114)``: 7 376 and 292 865)."""
import numpy as np
import pytest
import torch

from test_adam_host import BETA1, BETA2, EPS, LR, bits, build_adam_host, ref_step

pytestmark = pytest.mark.gpu

PAD = 8  # sentinel floats on each side of a segment
SENTINEL = 12345.0
ALIGNED, OFF1 = (4, 4, 4, 4), (1, 1, 1, 1)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_adam_host(tmp_path_factory.mktemp("adam_host_gpu"))


def _real_pair():
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    return tuple(int(m.init(jumpy.random_prngkey(0)).theta.numel()) for m in networks.make_models(16, 114))


class Segment:
    """theta, grad, m, v of n floats at the given float offsets inside sentinel-filled device buffers."""

    def __init__(self, rng, n, offsets):
        self.n, self.offsets = n, offsets
        self.bufs = [torch.full((n + 2 * PAD + 4,), SENTINEL, device="cuda") for _ in range(4)]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)
        self.views = [b[PAD + o:PAD + o + n] for b, o in zip(self.bufs, offsets)]
        assert all(v.data_ptr() % 16 == 4 * (o % 4) for v, o in zip(self.views, offsets))
        self.host = [(0.5 * rng.standard_normal(n)).astype(np.float32), None, np.zeros(n, np.float32), np.zeros(n, np.float32)]
        for k in (0, 2, 3):
            self.views[k].copy_(torch.from_numpy(self.host[k]))

    def set_grad(self, g):
        self.host[1] = g
        self.views[1].copy_(torch.from_numpy(g))

    def check(self, tag):
        for k, name in ((0, "theta"), (2, "m"), (3, "v")):
            assert np.array_equal(bits(self.views[k].cpu().numpy()), bits(self.host[k])), (tag, name)
        for b, o in zip(self.bufs, self.offsets):
            outside = torch.cat([b[:PAD + o], b[PAD + o + self.n:]])
            assert bool((outside == SENTINEL).all()), (tag, "an element outside the segment changed")


def device_step(segments, state):
    from po_brax_amd import _lib
    segs = (_lib.pob_adam_seg * len(segments))()
    for s, seg in zip(segs, segments):
        s.theta, s.grad, s.m, s.v = (v.data_ptr() for v in seg.views)
        s.n = seg.n
    _lib.check(_lib.lib.pob_adam_step(segs, len(segments), state.data_ptr(), LR, BETA1, BETA2, EPS,
                                      _lib.stream_handle(state.device)))


CASES = [([n], [ALIGNED]) for n in (1, 3, 63, 64, 65, 255, 1027)]
CASES += [([n], [OFF1]) for n in (1, 3, 64, 1027)]           # a view at offset 1: head of three, then 16-byte groups
CASES += [([65], [(1, 4, 4, 4)]), ([1027], [(4, 2, 4, 3)])]  # the four bases disagree modulo 16: all scalar
CASES += [([65, 1027], [ALIGNED, OFF1]), ([1027, 3, 255, 64], [OFF1, ALIGNED, (4, 1, 4, 4), ALIGNED]), ("real", None)]


@pytest.mark.parametrize("lengths,offsets", CASES, ids=[f"{c[0]}-{c[1]}".replace(" ", "") for c in CASES])
def test_kernel_is_the_restatement(host, lengths, offsets):
    if lengths == "real":
        lengths = list(_real_pair())
        assert lengths == [7376, 292865]
        offsets = [ALIGNED, OFF1]
    rng = np.random.default_rng(sum(lengths))
    segments = [Segment(rng, n, o) for n, o in zip(lengths, offsets)]
    state = torch.ones(2, dtype=torch.float64, device="cuda")
    state_host = np.ones(2, np.float64)
    for step in range(3):
        for seg in segments:
            seg.set_grad((0.1 * rng.standard_normal(seg.n)).astype(np.float32))
        device_step(segments, state)
        ref_step(host, *[[seg.host[k] for seg in segments] for k in range(4)], state_host)
        torch.cuda.synchronize()
        for i, seg in enumerate(segments):
            seg.check((step, i))
        assert np.array_equal(state.cpu().numpy(), state_host), step


def test_arguments_are_checked_before_any_launch():
    from po_brax_amd import _lib
    seg = Segment(np.random.default_rng(0), 8, ALIGNED)
    seg.set_grad(np.zeros(8, np.float32))
    state = torch.ones(2, dtype=torch.float64, device="cuda")
    segs = (_lib.pob_adam_seg * 5)()
    for s in segs:
        s.theta, s.grad, s.m, s.v = (v.data_ptr() for v in seg.views)
        s.n = 8
    call = lambda n_seg, st: _lib.lib.pob_adam_step(segs, n_seg, st, LR, BETA1, BETA2, EPS, None)  # noqa: E731
    for n_seg in (0, 5):
        with pytest.raises(ValueError):
            _lib.check(call(n_seg, state.data_ptr()))
    with pytest.raises(ValueError):
        _lib.check(call(1, None))
    segs[0].n = 0
    with pytest.raises(ValueError):
        _lib.check(call(1, state.data_ptr()))
    segs[0].n, segs[0].m = 8, seg.views[2].data_ptr() + 2
    with pytest.raises(ValueError):
        _lib.check(call(1, state.data_ptr()))
    torch.cuda.synchronize()
    seg.check("refused calls")
    assert state.tolist() == [1.0, 1.0]


def _leaves(rng, lengths):
    base = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    grads = [[(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lengths] for _ in range(3)]
    return base, grads


@pytest.mark.parametrize("lengths", [(7376, 1027), (1, 63, 64, 255, 1027)], ids=["two", "five"])
def test_fused_adam_on_device_leaves(host, lengths):
    """``FusedAdam.step`` on CUDA leaves against the restatement (five leaves: two launches under the
    same bias corrections), storage in place, and the state dict round trip."""
    from po_brax_amd.training import FusedAdam
    rng = np.random.default_rng(len(lengths))
    base, grads = _leaves(rng, lengths)
    leaves = [torch.from_numpy(b.copy()).cuda().requires_grad_(True) for b in base]
    opt = FusedAdam(leaves, lr=LR)
    ptrs = [p.data_ptr() for p in leaves]
    ref = [[b.copy() for b in base], [np.zeros_like(b) for b in base], [np.zeros_like(b) for b in base]]
    state = np.ones(2, np.float64)
    for step in range(3):
        for p, g in zip(leaves, grads[step]):
            p.grad = torch.from_numpy(g).cuda()
        opt.step()
        for lo in range(0, len(lengths), 4):
            s = state.copy()
            ref_step(host, ref[0][lo:lo + 4], grads[step][lo:lo + 4], ref[1][lo:lo + 4], ref[2][lo:lo + 4], s)
        state = s
        for k, p in enumerate(leaves):
            assert np.array_equal(bits(p.detach().cpu().numpy()), bits(ref[0][k])), (step, k)
            assert np.array_equal(bits(opt.m[k].cpu().numpy()), bits(ref[1][k])), (step, k)
            assert np.array_equal(bits(opt.v[k].cpu().numpy()), bits(ref[2][k])), (step, k)
        assert np.array_equal(opt.bias.cpu().numpy(), state)
        opt.zero_grad(set_to_none=True)
    assert [p.data_ptr() for p in leaves] == ptrs
    other = FusedAdam([torch.zeros_like(p).requires_grad_(True) for p in leaves])
    other.load_state_dict(opt.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.m + other.v + [other.bias], opt.m + opt.v + [opt.bias]))


def test_a_captured_step_counts_on_the_device():
    """One ``step()`` captured into a ``torch.cuda.graph`` and replayed three times equals three eager
    steps bit for bit: the bias corrections advance with no host counter."""
    from po_brax_amd.training import FusedAdam
    rng = np.random.default_rng(3)
    base, grads = _leaves(rng, (7376, 1027))
    eager = [torch.from_numpy(b.copy()).cuda().requires_grad_(True) for b in base]
    graphed = [torch.from_numpy(b.copy()).cuda().requires_grad_(True) for b in base]
    for pe, pg, g in zip(eager, graphed, grads[0]):
        pe.grad = torch.from_numpy(g).cuda()
        pg.grad = pe.grad.clone()  # static: every replay reads this storage
    opt_e, opt_g = FusedAdam(eager, lr=LR), FusedAdam(graphed, lr=LR)
    for step in range(3):
        opt_e.step()  # (the kernels are loaded by now: nothing lazy is left for the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()
    torch.cuda.synchronize()
    assert opt_g.bias.tolist() == [1.0, 1.0] and all(torch.equal(p.detach().cpu(), torch.from_numpy(b))
                                                      for p, b in zip(graphed, base))  # a capture runs nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    b1 = float(np.float32(BETA1))
    assert torch.equal(opt_g.bias, opt_e.bias) and opt_e.bias[0].item() == ((1.0 * b1) * b1) * b1
    for k in range(2):
        for a, b in ((graphed[k], eager[k]), (opt_g.m[k], opt_e.m[k]), (opt_g.v[k], opt_e.v[k])):
            assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), k
    assert not torch.equal(eager[0].detach().cpu(), torch.from_numpy(base[0]))
