"""CPU: the Python surface of po_brax_amd.training.networks (the reference's
po_brax/training/networks.py: FeedForwardModel, make_model, make_models) and the argument
checks of the pob_mlp_* / pob_policy_act entry points, none of which needs a GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pob_np


def _key(seed):
    return torch.from_numpy(np.asarray(pob_np.prngkey(seed), np.uint32))


def test_make_models_shapes_and_param_counts():
    from po_brax_amd.training import networks
    policy, value = networks.make_models(16, 114)
    assert policy.layer_sizes == (114, 32, 32, 32, 32, 16) and value.layer_sizes == (114, 256, 256, 256, 256, 256, 1)
    # policy: (114 + 1) 32 + 3 (32 + 1) 32 + (32 + 1) 16 = 3 680 + 3 168 + 528; value: (114 + 1) 256
    # + 4 (256 + 1) 256 + (256 + 1) 1 = 29 440 + 263 168 + 257
    assert policy.mlp.param_count == 7376 and value.mlp.param_count == 292865
    p, v = policy.init(_key(0)), value.init(_key(1))
    assert p.theta.shape == (7376,) and v.theta.shape == (292865,) and p.theta.dtype == torch.float32
    assert list(p) == [f"hidden_{i}" for i in range(5)]
    assert p["hidden_0"]["kernel"].shape == (114, 32) and p["hidden_4"]["kernel"].shape == (32, 16)
    assert p["hidden_4"]["bias"].shape == (16,) and v["hidden_5"]["kernel"].shape == (256, 1)
    x = torch.zeros((3, 5, 114))
    assert policy.apply(p, x).shape == (3, 5, 16) and value.apply(v, x).shape == (3, 5, 1)
    assert isinstance(policy, networks.FeedForwardModel)


def test_theta_views_alias():
    from po_brax_amd.training import networks
    model = networks.make_model([4, 3], 5)
    p = model.init(_key(2))
    assert p.theta.numel() == 5 * 4 + 4 + 4 * 3 + 3
    p["hidden_1"]["kernel"][2, 1] = 7.0
    assert p.theta[5 * 4 + 4 + 2 * 3 + 1] == 7.0  # row-major (in, out)
    p.theta[5 * 4 + 1] = -2.0
    assert p["hidden_0"]["bias"][1] == -2.0
    assert p["hidden_0"]["kernel"].data_ptr() == p.theta.data_ptr()


def test_lecun_uniform_init_from_the_key():
    from po_brax_amd.training import networks
    model = networks.make_model([64, 8], 114, activation="tanh")
    p = model.init(_key(3))
    key = pob_np.prngkey(3)
    for i, n_in in enumerate((114, 64)):
        W = p[f"hidden_{i}"]["kernel"]
        lim = math.sqrt(3.0 / n_in)
        assert float(W.abs().max()) <= np.float32(lim) and float(W.abs().max()) > 0.95 * lim
        assert abs(float(W.mean())) < 4 * lim / math.sqrt(3 * W.numel())  # 4 sigma of the mean
        assert abs(float(W.var()) - lim * lim / 3) < 0.1 * lim * lim / 3
        assert not p[f"hidden_{i}"]["bias"].any()
        # the draw: key, sub = split(key); uniform(sub, (in * out,), -lim, lim) of the test oracle
        key, sub = pob_np.split(key)
        want = pob_np.uniform(sub, (W.numel(),), np.float32(-lim), np.float32(lim))
        assert np.array_equal(W.reshape(-1).numpy(), np.asarray(want, np.float32))
    assert not torch.equal(p.theta, model.init(_key(4)).theta)
    assert torch.equal(p.theta, model.init(_key(3)).theta)


@pytest.mark.parametrize("activation", ["relu", "swish", "tanh"])
def test_apply_torch_path_and_gradient(activation):
    from po_brax_amd.training import networks
    model = networks.make_model([7, 6, 2], 5, activation=activation)
    p = model.init(_key(5))
    p.theta.add_(0.01)  # nonzero biases
    x = torch.linspace(-2, 2, 4 * 5).reshape(4, 5)
    fn = {"relu": torch.relu, "swish": torch.nn.functional.silu, "tanh": torch.tanh}[activation]
    h = x
    for i in range(3):
        h = h @ p[f"hidden_{i}"]["kernel"] + p[f"hidden_{i}"]["bias"]
        if i < 2:
            h = fn(h)
    assert torch.allclose(model.apply(p, x), h, atol=1e-6)
    assert torch.allclose(model.apply(dict(p), x), h, atol=1e-6)  # a plain mapping works too
    p.theta.requires_grad_(True)
    model.apply(p, x).square().sum().backward()
    assert p.theta.grad is not None and p.theta.grad.shape == p.theta.shape
    assert (p.theta.grad != 0).sum() > p.theta.numel() // 2  # every layer's kernel and bias take part
    assert p.theta.grad[-2:].abs().min() > 0  # the last bias


def test_spectral_norm_is_refused():
    from po_brax_amd.training import networks
    with pytest.raises(NotImplementedError, match="spectral"):
        networks.make_model([32, 8], 10, spectral_norm=True)


def test_bad_shapes_are_einval_without_gpu():
    from po_brax_amd import _lib
    from po_brax_amd.training import networks
    lib = _lib.lib

    def create(sizes, act=1):
        h = C.c_void_p()
        rc = lib.pob_mlp_create(len(sizes) - 1, (C.c_int * len(sizes))(*sizes), act, 0, C.byref(h))
        return rc, h

    for sizes in ([0, 4], [4, 257], [257, 4], [4, 0, 4], [4] * 10, [4]):
        rc, h = create(sizes)
        assert rc == _lib.POB_EINVAL and not h.value, sizes
        assert b"mlp" in lib.pob_last_error()
    assert create([4, 4], act=3)[0] == _lib.POB_EINVAL
    assert lib.pob_mlp_create(1, None, 0, 0, C.byref(C.c_void_p())) == _lib.POB_EINVAL
    assert lib.pob_mlp_create(1, (C.c_int * 2)(4, 4), 0, 0, None) == _lib.POB_EINVAL
    with pytest.raises(ValueError, match="1 .. 256"):
        networks.make_model([300, 2], 10)
    with pytest.raises(ValueError, match="layers"):
        networks.make_model([8] * 9, 10)

    rc, odd = create([6, 8, 5])
    assert rc == 0
    rc, even = create([6, 8, 4])
    assert rc == 0 and create([256] * 9)[0] == 0 and create([1, 1])[0] == 0
    n = C.c_longlong()
    assert lib.pob_mlp_param_count(even, C.byref(n)) == 0 and n.value == 6 * 8 + 8 + 8 * 4 + 4
    assert lib.pob_mlp_param_count(None, C.byref(n)) == _lib.POB_EINVAL
    p = 64  # a non-NULL pointer value: every call below is refused before anything is read
    assert lib.pob_mlp_forward(None, 4, p, p, p, None) == _lib.POB_EINVAL
    assert lib.pob_mlp_forward(even, 0, p, p, p, None) == _lib.POB_EINVAL
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.pob_mlp_forward(even, 4, *args, None) == _lib.POB_EINVAL
        assert b"NULL" in lib.pob_last_error()

    def act(m, B=4, total=4, first=0, obs=p, theta=p, key=p, det=0, action=p):
        return lib.pob_policy_act(m, B, total, first, obs, theta, key, det, action, None, None, None, None, None)

    assert act(None) == _lib.POB_EINVAL
    assert act(odd) == _lib.POB_EINVAL and b"even" in lib.pob_last_error()
    assert act(even, B=4, total=8, first=5) == _lib.POB_EINVAL and b"first + B <= total" in lib.pob_last_error()
    assert act(even, first=-1) == _lib.POB_EINVAL and act(even, B=0) == _lib.POB_EINVAL
    for kw in ({"obs": None}, {"theta": None}, {"action": None}, {"key": None}):
        assert act(even, **kw) == _lib.POB_EINVAL, kw
    with pytest.raises(ValueError):
        _lib.check(act(even, obs=None))
    for h in (odd, even):
        lib.pob_mlp_destroy(h)
    lib.pob_mlp_destroy(None)
