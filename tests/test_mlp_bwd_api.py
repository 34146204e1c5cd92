"""CPU: the public side of the native MLP backward pass: ``apply_native`` off the kernel path,
``PPOLearner(backward=...)`` and the argument checks of pob_mlp_forward_train / pob_mlp_backward."""
import ctypes as C
import types

import numpy as np
import pytest
import torch


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_apply_native_off_the_kernel_path_is_apply_under_autograd(dtype):
    from po_brax_amd.training import make_model
    model = make_model([7, 4], 5, "tanh")
    assert callable(model.apply_native)
    params = model.init(_key(0))
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((9, 5))).to(dtype)
    dy = torch.from_numpy(np.random.default_rng(1).standard_normal((9, 4))).to(dtype)
    grads = []
    for fn in (model.apply_native, model.apply):
        th = params.theta.detach().to(dtype).requires_grad_(True)
        xx = x.clone().requires_grad_(True)
        y = fn(types.SimpleNamespace(theta=th), xx)
        assert y.dtype == dtype and y.requires_grad
        (y * dy).sum().backward()
        grads.append((y.detach(), th.grad, xx.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    # the dict-of-views form and the no-grad call
    views = {k: {n: t.detach().clone().requires_grad_(True) for n, t in v.items()} for k, v in params.items()}
    y = model.apply_native(views, x.float())
    y.sum().backward()
    assert views["hidden_0"]["kernel"].grad is not None
    with torch.no_grad():
        assert torch.equal(model.apply_native(params, x.float()), model.apply(params, x.float()))


def test_learner_backward_keyword():
    from po_brax_amd.training import PPOLearner
    for bad in ("hip", None, ("native",), ("native", "torch", "torch"), ("native", "cuda"), 1):
        with pytest.raises(ValueError, match="backward"):
            PPOLearner(None, None, key=_key(0), backward=bad)
    for good in ("torch", "native", ("native", "torch"), ["torch", "native"]):
        with pytest.raises(TypeError, match="NormalTanhPolicy"):  # past the keyword's check
            PPOLearner(None, None, key=_key(0), backward=good)


def test_native_learner_on_host_tensors_is_the_torch_learner():
    """Off the kernel path ``backward="native"`` takes the same torch ops: the same steps, bit for bit."""
    from po_brax_amd.training import NormalTanhPolicy, PPOLearner, ValueFunction, make_model
    from test_ppo_api import _Roll
    D, A = 5, 2
    rng = np.random.default_rng(0)
    roll = _Roll(4, 8, D, A)
    roll.obs = torch.from_numpy(rng.standard_normal((4, 8, D)).astype(np.float32))
    roll.raw = torch.from_numpy(rng.standard_normal((4, 8, A)).astype(np.float32))
    roll.logp = torch.from_numpy((-2.0 + 0.3 * rng.standard_normal((4, 8))).astype(np.float32))
    roll.advantages = torch.from_numpy(rng.standard_normal((4, 8)).astype(np.float32))
    roll.vs = torch.from_numpy(rng.standard_normal((4, 8)).astype(np.float32))
    left = []
    for backward in ("torch", "native", ("torch", "native")):
        policy = NormalTanhPolicy.__new__(NormalTanhPolicy)  # the native actor needs a GPU: only what the learner reads
        model = make_model([7, 2 * A], D)
        policy.model, policy.params = model, model.init(_key(0))
        policy.theta, policy.obs_size, policy.action_size, policy.normalizer = policy.params.theta, D, A, None
        value_fn = ValueFunction.__new__(ValueFunction)
        vmodel = make_model([7, 1], D)
        value_fn.model, value_fn.params = vmodel, vmodel.init(_key(1))
        value_fn.theta, value_fn.obs_size, value_fn.normalizer = value_fn.params.theta, D, None
        learner = PPOLearner(policy, value_fn, num_minibatches=4, num_update_epochs=1, key=_key(2), backward=backward)
        assert learner.backward == ((backward, backward) if isinstance(backward, str) else backward)
        learner.update(roll)
        left.append((policy.theta.clone(), value_fn.theta.clone()))
    for other in left[1:]:
        assert torch.equal(other[0], left[0][0]) and torch.equal(other[1], left[0][1])


def test_new_symbols_and_argument_checks_without_a_gpu():
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import MLPHandle
    lib = _lib.lib
    new = {"pob_mlp_saved_bytes", "pob_mlp_forward_train", "pob_mlp_backward_workspace_bytes", "pob_mlp_backward"}
    assert new <= set(_lib.EXPORTS) and all(hasattr(lib, n) for n in new)
    assert _lib.ABI_VERSION == 8 and lib.pob_abi_version() == 8
    sizes = [27, 33, 16]
    P = (27 + 1) * 33 + (33 + 1) * 16
    h = MLPHandle(sizes, 1, False)
    n = C.c_longlong()
    assert lib.pob_mlp_saved_bytes(h.handle, 1025, C.byref(n)) == 0 and n.value == 1025 * 33 * 4
    assert lib.pob_mlp_backward_workspace_bytes(h.handle, 1025, C.byref(n)) == 0
    assert n.value == ((1025 * 49 * 4 + 7) & ~7) + 2 * P * 8
    fin = MLPHandle(sizes, 1, True)
    assert lib.pob_mlp_saved_bytes(fin.handle, 10, C.byref(n)) == 0 and n.value == 10 * 49 * 4
    one = MLPHandle([3, 1], 1, False)
    assert lib.pob_mlp_saved_bytes(one.handle, 10, C.byref(n)) == 0 and n.value == 0
    # the value network at M = 40 960: about 0.3 GB
    big = MLPHandle([114, 256, 256, 256, 256, 256, 1], 1, False)
    assert lib.pob_mlp_backward_workspace_bytes(big.handle, 40960, C.byref(n)) == 0
    assert 0.29e9 < n.value < 0.32e9 and n.value == 40960 * 1281 * 4 + 40 * big.param_count * 8
    a = np.zeros(64, np.float32)
    p = a.ctypes.data_as(C.c_void_p)  # never dereferenced: every call below is rejected before any HIP call
    ok = dict(h=h.handle, M=4, x=p, theta=p, y=p, saved=p, dy=p, dtheta=p, dx=None, ws=p)

    def forward(**kw):
        k = {**ok, **kw}
        return lib.pob_mlp_forward_train(k["h"], k["M"], k["x"], k["theta"], k["y"], k["saved"], None)

    def backward(**kw):
        k = {**ok, **kw}
        return lib.pob_mlp_backward(k["h"], k["M"], k["x"], k["theta"], k["saved"], k["dy"], k["dtheta"], k["dx"], k["ws"], None)

    for kw in (dict(h=None), dict(M=0), dict(M=-3), dict(M=2 ** 31 // 33 + 1), dict(M=2 ** 31 // 33 - 1000), dict(M=2 ** 40),
               dict(x=None), dict(theta=None), dict(saved=None)):
        assert forward(**kw) == _lib.POB_EINVAL, kw
        assert lib.pob_last_error().decode().startswith("mlp"), kw
        assert backward(**kw) == _lib.POB_EINVAL, kw
        with pytest.raises(ValueError, match="mlp"):
            _lib.check(backward(**kw))
    # (M + 1024) times the widest layer (33) stays below 2^31: the largest M and the one after it
    assert lib.pob_mlp_saved_bytes(h.handle, 2 ** 31 // 33 - 1025, C.byref(n)) == 0
    assert lib.pob_mlp_saved_bytes(h.handle, 2 ** 31 // 33 - 1024, C.byref(n)) == _lib.POB_EINVAL
    assert "(M + 1024)" in lib.pob_last_error().decode()
    assert forward(y=None) == _lib.POB_EINVAL
    for kw in (dict(dy=None), dict(dtheta=None), dict(ws=None)):
        assert backward(**kw) == _lib.POB_EINVAL, kw
    assert lib.pob_mlp_saved_bytes(h.handle, 4, None) != 0 and lib.pob_mlp_backward_workspace_bytes(h.handle, 0, C.byref(n)) != 0
