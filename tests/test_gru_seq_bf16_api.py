"""CPU: the bf16 recurrent window's definition (``apply_sequence(kernel="bf16")`` in torch ops against a float64
statement), its keyword checks and its workspace query.  The GPU tests import ``NETS``, ``case``, ``rows_of``,
``reference``, ``metric`` and ``TOL`` from here."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

# DESIGN.md "Bf16 recurrent window": 4 x the torch-op path's largest error over the cases below: h_out 1.721e-4 (114 -> GRU 64
# -> 1, S = 3, M = 200 without idx: one flipped bf16 tie of a carried h), y 5.97e-5 (30 -> GRU 64 -> 1, S = 3, M = 200 without idx)
TOL = 6.9e-4

# (pre widths from the observation's, H, post widths, activation)
NETS = [([30], 64, [1], "swish"), ([114], 64, [1], "swish"), ([114, 32], 33, [16, 1], "tanh"), ([7], 1, [1], "swish"),
        ([5, 17], 128, [3, 1], "relu")]
B_ALL, CLIP = 256, 2.5
VARIANTS = [(M, use_idx) for M in (1, 33, 65, 200) for use_idx in (False, True)]  # 65: one full tile of 64 plus one row


def reference(pre, H, post, act, theta, obs, h0, reset, table):
    """The definition in float64 over every env of obs (S, B, D): ``(y (S, B, out), [h after the reset of step 0,
    h after step 1, .., h after step S])``.  Matrix-product operands are rounded through f32 to bf16."""
    fn = (torch.relu, torch.nn.functional.silu, torch.tanh)[act]
    r = lambda t: t.float().to(torch.bfloat16).double()  # noqa: E731
    I, h, ys, hs = pre[-1], h0.double(), [], []
    for s in range(obs.shape[0]):
        off = 0

        def dense(v, n_in, n_out):
            nonlocal off
            W, b = theta[off:off + n_in * n_out].view(n_in, n_out), theta[off + n_in * n_out:off + (n_in + 1) * n_out]
            off += (n_in + 1) * n_out
            return b.double() + v @ r(W)

        x = r(torch.clamp((obs[s] - table[0]) * table[1], -CLIP, CLIP))  # pob_obsnorm_apply's f32 arithmetic
        for n_in, n_out in zip(pre[:-1], pre[1:]):
            x = r(fn(dense(x, n_in, n_out)))
        h = torch.where(reset[s].reshape(-1, 1) != 0, torch.zeros_like(h), h)
        if s == 0:
            hs.append(h)
        hb = r(h)
        rz = torch.sigmoid(dense(torch.cat([x, hb], dim=-1), I + H, 2 * H))
        cx, ch = dense(x, I, H), dense(hb, H, H)
        n = torch.tanh(cx + rz[:, :H] * ch)
        h = n + rz[:, H:] * (h - n)  # the unrounded h
        hs.append(h)
        y, widths = r(h), [H] + list(post)
        for i, (n_in, n_out) in enumerate(zip(widths[:-1], widths[1:])):
            y = dense(y, n_in, n_out)
            if i != len(post) - 1:
                y = r(fn(y))
        ys.append(y)
    return torch.stack(ys), hs


def metric(y, want):
    return float((y.double() - want).abs().max() / max(1.0, float(want.abs().max())))


def case(net, S):
    """The model, theta, and the inputs over B_ALL envs of one (network, S): reset on about a quarter of the entries."""
    from po_brax_amd.training import networks
    pre, H, post, act = NETS[net]
    model = networks.make_recurrent_model(pre[1:], H, post, pre[0], activation=act)
    g = torch.Generator().manual_seed(100 * net + S)
    theta = model.init(torch.tensor([net, S], dtype=torch.uint32)).theta
    theta = (theta + 0.1 * torch.randn(theta.shape, generator=g)).contiguous()  # the biases too
    obs = torch.randn((S, B_ALL, pre[0]), generator=g)
    h0 = torch.rand((B_ALL, H), generator=g) - 0.5
    reset = (torch.rand((S, B_ALL), generator=g) < 0.25).float()
    table = torch.stack([torch.rand(pre[0], generator=g) - 0.5, 0.5 + 2 * torch.rand(pre[0], generator=g), torch.ones(pre[0])])
    return model, theta, obs, h0, reset, table


def rows_of(M, use_idx):
    """The envs a variant's sequences are: the first M, or M of a fixed permutation of B_ALL."""
    return torch.from_numpy(np.random.default_rng(M).permutation(B_ALL)[:M].copy()) if use_idx else torch.arange(M)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("net", range(len(NETS)))
def test_apply_sequence_bf16_is_the_definition(net, S):
    model, theta, obs, h0, reset, table = case(net, S)
    pre, H, post, _ = NETS[net]
    want_y, want_h = reference(pre, H, post, model.activation, theta, obs, h0, reset, table)
    p = types.SimpleNamespace(theta=theta)
    xn = torch.clamp((obs - table[0]) * table[1], -CLIP, CLIP)
    for M, use_idx in VARIANTS:
        rows = rows_of(M, use_idx)
        y, h = model.apply_sequence(p, xn[:, rows], h0[rows], reset[:, rows], kernel="bf16")
        ey, eh = metric(y, want_y[:, rows]), metric(h, want_h[S][rows])
        print(f"bf16 window torch ops {NETS[net]} S={S} M={M} idx={use_idx}: y {ey:.3e} h {eh:.3e}")
        assert ey <= TOL and eh <= TOL, (M, use_idx, ey, eh)
    y_t, h_t = model.apply_sequence(p, xn, h0, reset, kernel="tile")
    y_d, h_d = model.apply_sequence(p, xn, h0, reset)
    assert torch.equal(y_t, y_d) and torch.equal(h_t, h_d)  # the default, bit for bit
    assert not torch.equal(y, y_t[:, rows])  # not silently f32


def exact_case():
    """relu [114, 32] -> GRU 33 -> [16, 1] on small integers whose gates saturate: biases of +-1000 put every r and z at
    exactly 0 or 1 and +-50 every candidate at exactly +-1, in f32 and in float64, so h' is h or +-1 and every value is
    an integer that bf16 holds and f32 sums in any order."""
    from po_brax_amd.training import networks
    pre, H, post, S = [114, 32], 33, [16, 1], 3
    model = networks.make_recurrent_model(pre[1:], H, post, pre[0], activation="relu")
    rng = np.random.default_rng(33)

    def sparse(n_in, n_out, bias):
        W = np.zeros((n_in, n_out))
        for j in range(n_out):
            W[rng.integers(0, n_in, 2), j] = rng.choice([-1.0, 1.0], 2)
        return [W.ravel(), bias(n_out)]

    small = lambda n: rng.integers(-2, 3, n)  # noqa: E731
    parts = sparse(pre[0], pre[1], small)
    parts += sparse(pre[1] + H, 2 * H, lambda n: rng.choice([-1000.0, 1000.0], n))
    parts += sparse(pre[1], H, lambda n: rng.choice([-50.0, 50.0], n)) + sparse(H, H, small)
    parts += sparse(H, post[0], small) + sparse(post[0], post[1], small)
    theta = torch.from_numpy(np.concatenate(parts).astype(np.float32))
    obs = torch.from_numpy(rng.integers(-3, 4, (S, B_ALL, pre[0])).astype(np.float32))
    h0 = torch.from_numpy(rng.integers(-3, 4, (B_ALL, H)).astype(np.float32))
    reset = torch.from_numpy((rng.random((S, B_ALL)) < 0.25).astype(np.float32))
    # even observations under a mean of 0 and a scale of 1 / 2: the normalised rows are integers inside the clip
    table = torch.stack([torch.zeros(pre[0]), torch.full((pre[0],), 0.5), torch.ones(pre[0])])
    return model, theta, 2 * obs.clamp(-2, 2), h0, reset, table, (pre, H, post)


def test_exact_case_is_exact_in_the_reference():
    model, theta, obs, h0, reset, table, (pre, H, post) = exact_case()
    y, hs = reference(pre, H, post, 0, theta, obs, h0, reset, table)
    for t in (y, *hs):
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= 200
    assert len(hs[-1].unique()) > 2 and len(y.unique()) > 4  # not a constant
    xn = torch.clamp((obs - table[0]) * table[1], -CLIP, CLIP)
    y32, h32 = model.apply_sequence(types.SimpleNamespace(theta=theta), xn, h0, reset, kernel="bf16")
    assert torch.equal(y32.double(), y) and torch.equal(h32.double(), hs[-1])


def test_kernel_keyword_errors_before_any_hip_call():
    from po_brax_amd.training import RecurrentValueFunction, networks
    key = torch.tensor([0, 3], dtype=torch.uint32)
    gru = networks.make_recurrent_model([], 8, [1], 5)
    lstm = networks.make_recurrent_model([], 8, [1], 5, cell="lstm")
    x, h = torch.zeros((2, 3, 5)), torch.zeros((3, 8))
    for bad in ("resident", "mixed"):
        with pytest.raises(ValueError, match="tile.*bf16"):
            gru.apply_sequence(gru.init(key), x, h, kernel=bad)
        with pytest.raises(ValueError, match="tile.*bf16"):
            RecurrentValueFunction(gru, gru.init(key), kernel=bad)
    with pytest.raises(ValueError, match="lstm"):
        lstm.apply_sequence(lstm.init(key), x, torch.zeros((3, 16)), kernel="bf16")
    for kernel in ("tile", "bf16"):
        with pytest.raises(ValueError, match="cell='lstm'"):
            RecurrentValueFunction(lstm, lstm.init(key), kernel=kernel)


def test_workspace_query_and_argument_checks_without_gpu():
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import GRUHandle
    n = C.c_longlong()
    g = GRUHandle([114, 32], 33, [16, 1], 1)
    _lib.check(_lib.lib.pob_gru_sequence_bf16_workspace_bytes(g.handle, C.byref(n)))
    frags = lambda a, b: -(-a // 16) * -(-b // 32)  # noqa: E731
    assert n.value == 1024 * (frags(114, 32) + 3 * (2 + 3) * 2 + frags(33, 16) + frags(16, 1))
    lstm = GRUHandle([5], 8, [1], 1, "lstm")
    for bad in ((None, C.byref(n)), (g.handle, None), (lstm.handle, C.byref(n))):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib.pob_gru_sequence_bf16_workspace_bytes(*bad))
    assert b"lstm" in _lib.lib.pob_last_error()
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    good = [g.handle, 2, 4, 4, p, None, p, None, p, p, None, None, 2, None, 0.0, p, None]
    for at, value in ((0, None), (0, lstm.handle), (1, 0), (2, 0), (3, 5), (4, None), (6, None), (8, None), (9, None), (12, 0),
                      (12, 3), (15, None)):
        args = list(good)
        args[at] = value
        with pytest.raises(ValueError):
            _lib.check(_lib.lib.pob_gru_sequence_forward_bf16(*args))
