"""CPU: the LSTM cell of make_recurrent_model(..., cell="lstm") through its torch-op definition and
the C ABI's host side (DESIGN.md "LSTM cell").  No HIP call is made here."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import pob_np
from po_brax_amd import _lib
from po_brax_amd.training import networks

D, H, O = 7, 5, 4


def _key(seed):
    return torch.from_numpy(np.asarray(pob_np.prngkey(seed), np.uint32))


@pytest.fixture(scope="module")
def model():
    return networks.make_recurrent_model([], H, [O], D, cell="lstm")


def test_param_count_and_views_alias_theta(model):
    p = model.init(_key(1))
    assert model.cell == "lstm" and model.state_size == 2 * H
    assert model.gru.param_count == p.theta.numel() == 4 * H * (D + H) + 4 * H + (H + 1) * O
    assert "gru" not in p and p["lstm"]["kernel"].shape == (D + H, 4 * H) and p["lstm"]["bias"].shape == (4 * H,)
    p["lstm"]["bias"][H] = 7.0  # the first f-gate bias sits right behind W
    assert p.theta[4 * H * (D + H) + H] == 7.0
    assert tuple(model.initial_state(3).shape) == (3, 2 * H) and not model.initial_state(3).any()


def test_apply_equals_lstmcell_float64(model):
    gen = torch.Generator().manual_seed(0)
    theta = (torch.rand(model.gru.param_count, generator=gen, dtype=torch.float64) - 0.5)
    p = networks.RecurrentParams(theta, model.pre_sizes, H, model.post_sizes, "lstm")
    x = torch.rand((9, D), generator=gen, dtype=torch.float64) * 6 - 3
    s = torch.rand((9, 2 * H), generator=gen, dtype=torch.float64) * 2 - 1
    W, b = p["lstm"]["kernel"], p["lstm"]["bias"]
    cell = torch.nn.LSTMCell(D, H, dtype=torch.float64)
    with torch.no_grad():
        cell.weight_ih.copy_(W[:D].T); cell.weight_hh.copy_(W[D:].T)
        cell.bias_ih.copy_(b); cell.bias_hh.zero_()
        h1, c1 = cell(x, (s[:, :H], s[:, H:]))
        y1 = torch.addmm(p["post_0"]["bias"], h1, p["post_0"]["kernel"])
    y, s1 = model.apply(p, x, s)
    assert float((y - y1).abs().max()) <= 1e-12 and float((s1 - torch.cat([h1, c1], -1)).abs().max()) <= 1e-12


def test_apply_sequence_equals_chained_apply_with_grad(model):
    gen = torch.Generator().manual_seed(1)
    theta = model.init(_key(2)).theta.clone().requires_grad_(True)
    p = types.SimpleNamespace(theta=theta)
    x = torch.rand((3, 6, D), generator=gen) * 2 - 1
    s0 = torch.rand((6, 2 * H), generator=gen) - 0.5
    reset = (torch.rand((3, 6), generator=gen) < 0.3).float()
    y, s_last = model.apply_sequence(p, x, s0, reset)
    s = s0
    for t in range(3):
        yt, s = model.apply(p, x[t], s, reset[t])
        assert torch.equal(yt, y[t])
    assert torch.equal(s, s_last)
    (y.square().sum() + s_last.sum()).backward()
    assert bool(torch.isfinite(theta.grad).all()) and bool(theta.grad.any())


def test_value_errors_before_any_hip_call(model):
    from po_brax_amd.training import RecurrentPPOLearner, RecurrentValueFunction, ValueFunction
    with pytest.raises(ValueError, match="'gru' or 'lstm'"):
        networks.make_recurrent_model([], H, [O], D, cell="rnn")
    p = model.init(_key(3))
    with pytest.raises(ValueError, match=f"h \\(B, {2 * H}\\)"):
        model.apply(p, torch.zeros((2, D)), torch.zeros((2, H)))
    with pytest.raises(ValueError, match="apply_sequence_native"):
        model.apply_sequence_native(p, torch.zeros((2, 2, D)), torch.zeros((2, 2 * H)))
    vmodel = networks.make_recurrent_model([], H, [1], D, cell="lstm")
    with pytest.raises(ValueError, match="lstm"):
        RecurrentValueFunction(vmodel, vmodel.init(_key(4)))
    policy = networks.RecurrentTanhPolicy.__new__(networks.RecurrentTanhPolicy)  # the native actor needs a GPU
    policy.model = networks.make_recurrent_model([], H, [2 * O], D, cell="lstm")
    value_fn = ValueFunction.__new__(ValueFunction)
    for backward in ("native", ("native", "torch")):
        with pytest.raises(ValueError, match="cell='gru'"):
            RecurrentPPOLearner(policy, value_fn, backward=backward)


def test_sequence_entry_points_refuse_the_handle(model):
    g, n = model.gru.handle, C.c_longlong()
    calls = [lambda: _lib.lib.pob_gru_sequence_saved_bytes(g, 2, 4, C.byref(n)),
             lambda: _lib.lib.pob_gru_sequence_backward_workspace_bytes(g, 2, 4, C.byref(n)),
             lambda: _lib.lib.pob_gru_sequence_forward_train(g, 2, 4, 4, *[None] * 9, 0.0, None),
             lambda: _lib.lib.pob_gru_sequence_backward(g, 2, 4, 4, *[None] * 10),
             lambda: _lib.lib.pob_gru_sequence_forward(g, 2, 4, 4, *[None] * 8, 1, None, 0.0, None)]
    for call in calls:
        assert call() == _lib.POB_EINVAL and b"lstm" in _lib.lib.pob_last_error()


def test_gru_keyword_changes_nothing():
    a = networks.make_recurrent_model([8], H, [O], D).init(_key(5))
    b = networks.make_recurrent_model([8], H, [O], D, cell="gru").init(_key(5))
    assert torch.equal(a.theta, b.theta) and "gru" in b and "lstm" not in b
