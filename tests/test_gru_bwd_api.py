"""CPU: the public side of the recurrent backward pass: ``RecurrentModel.apply_sequence``,
``apply_sequence_native`` off the kernel path, their argument checks, and the checks of
``RecurrentPPOLearner``'s constructor and ``update``."""
import types

import numpy as np
import pytest
import torch


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32)


def _model(pre=(6,), H=7, post=(5, 4), D=5, act="tanh"):
    from po_brax_amd.training import make_recurrent_model
    model = make_recurrent_model(list(pre), H, list(post), D, act)
    params = model.init(_key(0))
    with torch.no_grad():  # biases away from their zero init
        params.theta.add_(0.05 * torch.from_numpy(np.random.default_rng(9).standard_normal(params.theta.numel())).float())
    return model, params


def _inputs(T, B, D, H, dtype, seed=0):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((T, B, D))).to(dtype)
    h0 = torch.from_numpy(rng.uniform(-1, 1, (B, H))).to(dtype)
    reset = torch.from_numpy((rng.uniform(size=(T, B)) < 0.3).astype(np.float32))
    return x, h0, reset


class StubNormalizer:
    """``apply`` alone: what the torch path reads of an ``ObservationNormalizer``."""

    def __init__(self, D):
        rng = np.random.default_rng(3)
        self.mean = torch.from_numpy(0.5 * rng.standard_normal(D))
        self.scale = torch.from_numpy(rng.uniform(0.5, 2.0, D))

    def apply(self, obs):
        return torch.clamp((obs - self.mean.to(obs.dtype)) * self.scale.to(obs.dtype), -2.0, 2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_apply_sequence_is_a_loop_over_apply(dtype):
    model, params = _model()
    T, B = 4, 9
    x, h0, reset = _inputs(T, B, 5, 7, dtype)
    p = types.SimpleNamespace(theta=params.theta.to(dtype))
    y, h_last = model.apply_sequence(p, x, h0, reset)
    assert y.shape == (T, B, 4) and h_last.shape == (B, 7) and y.dtype == dtype
    h = h0
    for t in range(T):
        yt, h = model.apply(p, x[t], h, reset[t])
        assert torch.equal(y[t], yt)
    assert torch.equal(h_last, h)
    y2, _ = model.apply_sequence(p, x, h0)  # reset=None
    assert torch.equal(y2[0], model.apply(p, x[0], h0)[0]) and not torch.equal(y2, y)
    # differentiable in theta, x and h0
    th = p.theta.clone().requires_grad_(True)
    xx, hh = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    y3, hl = model.apply_sequence(types.SimpleNamespace(theta=th), xx, hh, reset)
    (y3.sum() + hl.sum()).backward()
    assert all(t.grad is not None and bool(t.grad.abs().sum() > 0) for t in (th, xx, hh))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_apply_sequence_native_off_the_kernel_path(dtype):
    """CPU tensors: ``apply_sequence`` on the gathered, normalised rows, under autograd."""
    model, params = _model()
    T, B, M = 3, 11, 6
    x, h0, reset = _inputs(T, B, 5, 7, dtype, 1)
    idx = torch.from_numpy(np.random.default_rng(2).permutation(B)[:M].astype(np.int32))
    norm = StubNormalizer(5)
    dy = torch.from_numpy(np.random.default_rng(4).standard_normal((T, M, 4))).to(dtype)
    th_a, th_b = (params.theta.to(dtype).clone().requires_grad_(True) for _ in range(2))
    h_a, h_b = (h0.clone().requires_grad_(True) for _ in range(2))
    y, h_last = model.apply_sequence_native(types.SimpleNamespace(theta=th_a), x, h_a, reset, idx, norm)
    assert y.shape == (T, M, 4) and h_last.shape == (M, 7) and y.dtype == dtype and y.requires_grad
    j = idx.long()
    y_w, h_w = model.apply_sequence(types.SimpleNamespace(theta=th_b), norm.apply(x[:, j]), h_b[j], reset[:, j])
    assert torch.equal(y, y_w) and torch.equal(h_last, h_w)
    ((y * dy).sum() + h_last.sum()).backward()
    ((y_w * dy).sum() + h_w.sum()).backward()
    assert torch.equal(th_a.grad, th_b.grad) and torch.equal(h_a.grad, h_b.grad)
    assert bool((h_a.grad[j] != 0).any()) and not bool(h_a.grad[[k for k in range(B) if k not in set(j.tolist())]].any())
    # without idx, reset or normaliser, and without a needed gradient
    with torch.no_grad():
        y0, _ = model.apply_sequence_native(params if dtype == torch.float32 else types.SimpleNamespace(theta=th_a), x, h0)
    assert y0.shape == (T, B, 4) and not y0.requires_grad


def test_apply_sequence_argument_errors():
    model, params = _model()
    T, B = 3, 4
    x, h0, reset = _inputs(T, B, 5, 7, torch.float32)
    idx = torch.arange(2, dtype=torch.int32)
    seq, nat = model.apply_sequence, model.apply_sequence_native
    for fn in (seq, nat):
        with pytest.raises(ValueError, match=r"\(T, [MB], 5\)"):
            fn(params, x[0], h0)
        with pytest.raises(ValueError, match=r"\(T, [MB], 5\)"):
            fn(params, x[:, :, :4], h0)
        with pytest.raises(ValueError, match="h0 must be"):
            fn(params, x, h0[:, :6])
        with pytest.raises(ValueError, match="reset must be"):
            fn(params, x, h0, reset[:2])
        with pytest.raises(ValueError, match="theta has"):
            fn(types.SimpleNamespace(theta=params.theta[:-1]), x, h0)
    with pytest.raises(TypeError, match="obs must be a torch.Tensor"):
        nat(params, x.numpy(), h0)
    with pytest.raises(TypeError, match="obs must be a floating-point"):
        nat(params, x.long(), h0)
    with pytest.raises(TypeError, match="h0 is"):
        nat(params, x, h0.double())
    with pytest.raises(TypeError, match="params.theta is"):
        nat(types.SimpleNamespace(theta=params.theta.double()), x, h0)
    with pytest.raises(TypeError, match="params.theta must be"):
        nat(types.SimpleNamespace(theta=None), x, h0)
    with pytest.raises(TypeError, match="reset must be a torch.Tensor"):
        nat(params, x, h0, reset.numpy())
    for bad in (idx.long(), idx.reshape(1, 2), idx[:0], [0, 1]):
        with pytest.raises(ValueError, match="idx must be"):
            nat(params, x, h0, None, bad)
    with pytest.raises(TypeError, match="normalizer must be"):
        nat(params, x, h0, None, None, object())
    bad_table = types.SimpleNamespace(apply=lambda o: o, table=torch.zeros(3, 4), clip=0.0)
    with pytest.raises(ValueError, match="normalizer.table"):
        nat(params, x, h0, None, None, bad_table)


class _Roll:
    """The buffers of a RecurrentActorRollout(..., critic=) replay, as far as update() reads them."""

    def __init__(self, T, B, D, A, H, seed=0):
        rng = np.random.default_rng(seed)
        f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
        self.obs, self.raw = f(T, B, D), f(T, B, A)
        self.logp, self.advantages, self.vs = -2.0 + 0.3 * f(T, B), f(T, B), f(T, B)
        self.hidden = torch.full((T, B, H), float("nan"))
        self.hidden[0] = torch.from_numpy(rng.uniform(-1, 1, (B, H)).astype(np.float32))
        self.done = torch.from_numpy((rng.uniform(size=(T, B)) < 0.2).astype(np.float32))


def test_recurrent_learner_checks():
    from po_brax_amd.training import PPOLearner, RecurrentPPOLearner
    from test_recurrent_learner_host import A, D, H, stub_actors
    policy, value_fn = stub_actors(0, None, None)
    for bad in ("hip", None, ("native",), ("native", "torch", "torch"), ("native", "cuda"), 1):
        with pytest.raises(ValueError, match="backward"):
            RecurrentPPOLearner(policy, value_fn, key=_key(0), backward=bad)
    with pytest.raises(TypeError, match="RecurrentTanhPolicy"):
        RecurrentPPOLearner(object(), value_fn, key=_key(2), backward="torch")
    with pytest.raises(TypeError, match="RecurrentTanhPolicy"):  # the feed-forward actor is PPOLearner's
        from test_learner_host import stub_actors as ff_actors
        RecurrentPPOLearner(ff_actors(0, None, None)[0], value_fn, key=_key(2), backward="torch")
    with pytest.raises(TypeError, match="NormalTanhPolicy"):  # and PPOLearner still refuses the recurrent one
        PPOLearner(policy, value_fn, key=_key(2))
    with pytest.raises(TypeError, match="ValueFunction"):
        RecurrentPPOLearner(policy, object(), key=_key(2), backward="torch")
    with pytest.raises(ValueError, match="key"):
        RecurrentPPOLearner(policy, value_fn, backward="torch")
    with pytest.raises(ValueError, match="positive"):
        RecurrentPPOLearner(policy, value_fn, num_update_epochs=0, key=_key(2), backward="torch")
    value_fn.obs_size = D + 1
    with pytest.raises(ValueError, match="observation width"):
        RecurrentPPOLearner(policy, value_fn, key=_key(2), backward="torch")
    value_fn.obs_size = D
    learner = RecurrentPPOLearner(policy, value_fn, num_minibatches=4, num_update_epochs=1, key=_key(2), backward="torch")
    assert learner.backward == ("torch", "torch")
    with pytest.raises(ValueError, match="not divisible"):
        learner.update(_Roll(4, 6, D, A, H))  # T B = 24 divides by 4, B = 6 does not: minibatches are envs
    for missing in ("obs", "raw", "logp", "advantages", "vs", "hidden", "done"):
        roll = _Roll(3, 8, D, A, H)
        delattr(roll, missing)
        with pytest.raises(ValueError, match=f"no {missing}.*RecurrentActorRollout.*critic="):
            learner.update(roll)
    # host tensors run the whole loop in torch ops, "native" too: the same steps bit for bit
    thetas = []
    for backward in ("torch", "native"):
        policy, value_fn = stub_actors(0, None, None)
        learner = RecurrentPPOLearner(policy, value_fn, num_minibatches=4, num_update_epochs=2, key=_key(2),
                                      backward=backward)
        before, ptrs = policy.theta.clone(), (policy.theta.data_ptr(), value_fn.theta.data_ptr())
        metrics = learner.update(_Roll(3, 8, D, A, H))
        assert sorted(metrics) == ["entropy_loss", "policy_loss", "total_loss", "value_loss"]
        assert all(bool(torch.isfinite(v)) for v in metrics.values())
        assert not torch.equal(policy.theta, before) and (policy.theta.data_ptr(), value_fn.theta.data_ptr()) == ptrs
        assert not policy.theta.requires_grad
        thetas.append((policy.theta.clone(), value_fn.theta.clone()))
    assert torch.equal(thetas[0][0], thetas[1][0]) and torch.equal(thetas[0][1], thetas[1][1])
