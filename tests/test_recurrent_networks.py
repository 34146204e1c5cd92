"""CPU: the Python surface of the recurrent actor (po_brax_amd.training.networks:
make_recurrent_model, RecurrentParams, RecurrentTanhPolicy) and the argument checks of the
pob_gru_* entry points, none of which needs a GPU.  The torch-op ``apply`` is compared with the
plain-C restatement (tests/host/gru_host.cpp)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pob_np
from test_gru_host import build_gru_host, ref_forward


def _key(seed):
    return torch.from_numpy(np.asarray(pob_np.prngkey(seed), np.uint32))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_gru_host(tmp_path_factory.mktemp("gru_host_net"))


def test_param_counts_and_shapes():
    from po_brax_amd.training import networks
    m = networks.make_recurrent_model([], 64, [16], 114)
    assert m.gru.param_count == 3 * 64 * 114 + 3 * 64 ** 2 + 4 * 64 + 65 * 16
    assert m.pre_sizes == (114,) and m.hidden_size == 64 and m.post_sizes == (16,)
    p = m.init(_key(0))
    assert p.theta.shape == (m.gru.param_count,) and p.theta.dtype == torch.float32
    assert list(p) == ["gru", "post_0"] and list(p["gru"]) == ["rz", "xn", "hn"]
    assert p["gru"]["rz"]["kernel"].shape == (178, 128) and p["gru"]["rz"]["bias"].shape == (128,)
    assert p["gru"]["xn"]["kernel"].shape == (114, 64) and p["gru"]["hn"]["kernel"].shape == (64, 64)
    assert p["post_0"]["kernel"].shape == (64, 16)
    m2 = networks.make_recurrent_model([32], 64, [32, 16], 114)
    assert m2.gru.param_count == 115 * 32 + 3 * 64 * 32 + 3 * 64 ** 2 + 4 * 64 + 65 * 32 + 33 * 16
    assert list(m2.init(_key(0))) == ["pre_0", "gru", "post_0", "post_1"]
    h0 = m.initial_state(5, "cpu")
    assert h0.shape == (5, 64) and h0.dtype == torch.float32 and not h0.any()
    y, h1 = m.apply(p, torch.zeros((5, 114)), h0)
    assert y.shape == (5, 16) and h1.shape == (5, 64)
    assert isinstance(m, networks.RecurrentModel)


def test_theta_views_alias():
    from po_brax_amd.training import networks
    I, H = 5, 3
    m = networks.make_recurrent_model([], H, [2], I)
    p = m.init(_key(2))
    n_rz = (I + H) * 2 * H
    assert p.theta.numel() == 3 * H * I + 3 * H * H + 4 * H + (H + 1) * 2
    p["gru"]["rz"]["kernel"][I + 1, H + 2] = 7.0  # h feature 1 -> z[2]
    assert p.theta[(I + 1) * 2 * H + H + 2] == 7.0
    p.theta[n_rz + 2 * H + 4 * H + 1] = -2.0  # W_xn[4][1], row-major (I, H)
    assert p["gru"]["xn"]["kernel"][4, 1] == -2.0
    off_hn = n_rz + 2 * H + I * H + H
    p["gru"]["hn"]["bias"][2] = 3.0
    assert p.theta[off_hn + H * H + 2] == 3.0
    assert p["gru"]["rz"]["kernel"].data_ptr() == p.theta.data_ptr()
    assert p["post_0"]["bias"].data_ptr() == p.theta[-2:].data_ptr()


def test_init_key_schedule():
    from po_brax_amd.training import networks
    m = networks.make_recurrent_model([8], 6, [4], 10, activation="tanh")
    p = m.init(_key(3))
    assert torch.equal(p.theta, m.init(_key(3)).theta) and not torch.equal(p.theta, m.init(_key(4)).theta)
    key = pob_np.prngkey(3)
    leaves = [p["pre_0"], p["gru"]["rz"], p["gru"]["xn"], p["gru"]["hn"], p["post_0"]]
    for leaf, n_in in zip(leaves, (10, 14, 8, 6, 6)):
        W = leaf["kernel"]
        assert W.shape[0] == n_in and not leaf["bias"].any()
        lim = math.sqrt(3.0 / n_in)
        key, sub = pob_np.split(key)
        want = pob_np.uniform(sub, (W.numel(),), np.float32(-lim), np.float32(lim))
        assert np.array_equal(W.reshape(-1).numpy(), np.asarray(want, np.float32))


@pytest.mark.parametrize("activation,act", [("relu", 0), ("swish", 1), ("tanh", 2)])
def test_apply_torch_path_against_restatement(host, activation, act):
    from po_brax_amd.training import networks
    pre, H, post, D, B = [12], 9, [7, 4], 11, 37
    m = networks.make_recurrent_model(pre, H, post, D, activation=activation)
    p = m.init(_key(5))
    p.theta.add_(0.01)  # nonzero biases
    rng = np.random.default_rng(8)
    h = torch.from_numpy(rng.uniform(-1, 1, (B, H)).astype(np.float32))
    h_ref = h.numpy().copy()
    for step in range(3):
        x = rng.uniform(-2, 2, (B, D)).astype(np.float32)
        reset = ((np.arange(B) + step) % 3 == 0).astype(np.float32)
        y, h = m.apply(p, torch.from_numpy(x), h, torch.from_numpy(reset))
        y_ref, h_ref, _ = ref_forward(host, [D] + pre, H, post, act, x, p.theta.numpy(), reset, h_ref)
        assert torch.allclose(y, torch.from_numpy(y_ref), atol=1e-5), step
        assert torch.allclose(h, torch.from_numpy(h_ref), atol=1e-5), step
    # no reset array: the state is kept
    y0, _ = m.apply(p, torch.from_numpy(x), h)
    y0_ref, _, _ = ref_forward(host, [D] + pre, H, post, act, x, p.theta.numpy(), None, h_ref)
    assert torch.allclose(y0, torch.from_numpy(y0_ref), atol=1e-5)


def test_autograd_reaches_theta_and_h():
    from po_brax_amd.training import networks
    m = networks.make_recurrent_model([6], 5, [4], 7)
    p = m.init(_key(6))
    p.theta.add_(0.01)
    x = torch.linspace(-2, 2, 3 * 7).reshape(3, 7)
    h = torch.linspace(-1, 1, 3 * 5).reshape(3, 5).clone().requires_grad_(True)
    p.theta.requires_grad_(True)
    y, h1 = m.apply(p, x, h, torch.tensor([0.0, 1.0, 0.0]))
    (y.square().sum() + h1.sum()).backward()
    assert p.theta.grad is not None and (p.theta.grad != 0).sum() > p.theta.numel() // 2
    assert h.grad is not None and h.grad[0].abs().min() > 0 and h.grad[2].abs().min() > 0
    assert not h.grad[1].any()  # the reset env's old state takes no part


def test_limits_are_refused_with_their_message():
    from po_brax_amd.training import networks
    mk = networks.make_recurrent_model
    with pytest.raises(ValueError, match="hidden width must be in 1 .. 128"):
        mk([], 129, [4], 10)
    with pytest.raises(ValueError, match="together must be at most 256"):
        mk([], 128, [4], 129)  # I + H = 257
    with pytest.raises(ValueError, match="together must be at most 256"):
        mk([200], 57, [4], 10)
    with pytest.raises(ValueError, match="every width must be in 1 .. 256"):
        mk([300], 16, [4], 10)
    with pytest.raises(ValueError, match="every width must be in 1 .. 256"):
        mk([], 16, [300, 4], 10)
    with pytest.raises(ValueError, match="every width must be in 1 .. 256"):
        mk([], 16, [4], 257)
    with pytest.raises(ValueError, match="at most 8 layers"):
        mk([8] * 4, 16, [8] * 4, 10)  # 9 layers
    with pytest.raises(ValueError, match="at most 8 layers"):
        mk([], 16, [8] * 5, 10)
    with pytest.raises(ValueError, match="at most 8 layers"):
        mk([], 16, [], 10)
    with pytest.raises(ValueError, match="activation"):
        mk([], 16, [4], 10, activation="gelu")
    assert mk([8] * 3, 128, [8] * 4, 10).gru.param_count > 0  # 8 layers, H = 128, I + H = 136
    assert mk([], 128, [2], 128).gru.param_count == 3 * 128 * 128 * 2 + 4 * 128 + 129 * 2
    odd = mk([], 16, [5], 10)
    with pytest.raises(ValueError, match="even"):
        networks.RecurrentTanhPolicy(odd, odd.init(_key(0)), _key(1))


def test_c_abi_checks_without_gpu():
    from po_brax_amd import _lib
    lib = _lib.lib

    def create(pre, H, post, act=1):
        h = C.c_void_p()
        rc = lib.pob_gru_create(len(pre) - 1, (C.c_int * len(pre))(*pre), H, len(post), (C.c_int * max(1, len(post)))(*post),
                                act, C.byref(h))
        return rc, h

    for pre, H, post in (([0], 4, [4]), ([4], 0, [4]), ([4], 129, [4]), ([200], 57, [4]), ([4, 257], 4, [4]),
                         ([4], 4, [0]), ([4], 4, []), ([4] * 5, 4, [4]), ([4], 4, [4] * 5)):
        rc, h = create(pre, H, post)
        assert rc == _lib.POB_EINVAL and not h.value, (pre, H, post)
        assert b"gru" in lib.pob_last_error()
    assert create([4], 4, [4], act=3)[0] == _lib.POB_EINVAL
    one = (C.c_int * 1)(4)
    assert lib.pob_gru_create(0, None, 4, 1, one, 0, C.byref(C.c_void_p())) == _lib.POB_EINVAL
    assert lib.pob_gru_create(0, one, 4, 1, None, 0, C.byref(C.c_void_p())) == _lib.POB_EINVAL
    assert lib.pob_gru_create(0, one, 4, 1, one, 0, None) == _lib.POB_EINVAL
    rc, odd = create([6], 8, [5])
    assert rc == 0
    rc, even = create([6, 7], 8, [4])
    assert rc == 0
    n = C.c_longlong()
    assert lib.pob_gru_param_count(even, C.byref(n)) == 0
    assert n.value == 7 * 7 + 3 * 8 * 7 + 3 * 8 * 8 + 4 * 8 + 9 * 4
    assert lib.pob_gru_param_count(None, C.byref(n)) == _lib.POB_EINVAL
    assert lib.pob_gru_param_count(even, None) == _lib.POB_EINVAL
    p = 64  # a non-NULL pointer value: every call below is refused before anything is read

    def fwd(g, B=4, x=p, theta=p, h_io=p, y=p):
        return lib.pob_gru_forward(g, B, x, theta, None, h_io, y, None, None)

    assert fwd(None) == _lib.POB_EINVAL and fwd(even, B=0) == _lib.POB_EINVAL
    for kw in ({"x": None}, {"theta": None}, {"y": None}):
        assert fwd(even, **kw) == _lib.POB_EINVAL and b"NULL" in lib.pob_last_error(), kw
    assert fwd(even, h_io=None) == _lib.POB_EINVAL and b"h_io is NULL" in lib.pob_last_error()

    def act(g, B=4, total=4, first=0, obs=p, theta=p, key=p, det=0, h_io=p, action=p):
        return lib.pob_gru_policy_act(g, B, total, first, obs, theta, key, det, None, h_io, action, None, None, None,
                                      None, None, None)

    assert act(None) == _lib.POB_EINVAL
    assert act(odd) == _lib.POB_EINVAL and b"even" in lib.pob_last_error()
    assert act(even, B=4, total=8, first=5) == _lib.POB_EINVAL and b"first + B <= total" in lib.pob_last_error()
    assert act(even, first=-1) == _lib.POB_EINVAL and act(even, B=0) == _lib.POB_EINVAL
    for kw in ({"obs": None}, {"theta": None}, {"action": None}, {"key": None}, {"h_io": None}):
        assert act(even, **kw) == _lib.POB_EINVAL, kw
    with pytest.raises(ValueError, match="h_io is NULL"):
        _lib.check(act(even, h_io=None))
    for h in (odd, even):
        lib.pob_gru_destroy(h)
    lib.pob_gru_destroy(None)
