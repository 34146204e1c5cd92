"""GPU: the MLP training forward and backward kernels (pob_mlp_forward_train / pob_mlp_backward)
against the plain-C restatement (mlp_forward_train_ref / mlp_backward_ref of csrc/pob_mlp.h, built
for the host by tests/host/mlp_bwd_host.cpp), bit for bit; ``apply_native`` and
``PPOLearner(backward="native")`` on top of them."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from test_mlp_bwd_host import (POLICY, RELU, SWISH, TANH, build_mlp_bwd_host, check_against_float64, integer_problem,
                               make_problem, param_count, ref_train_and_back, within_bound)

pytestmark = pytest.mark.gpu

NETS = {"single": [3, 1], "small": [5, 7, 4], "odd": [27, 33, 16], "wide": [40, 256, 255, 1], "policy": POLICY,
        "deep": [4, 3, 3, 3, 3, 3, 3, 3, 2]}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_mlp_bwd_host(tmp_path_factory.mktemp("mlp_bwd_host"))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(got, want, what):
    want = _cuda(np.ascontiguousarray(want, np.float32))
    assert got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())


class Buffers:
    """The device buffers of one forward_train + backward of a network at M rows."""

    def __init__(self, sizes, act, fin, M, want_dx=True):
        from po_brax_amd._lib import check, lib
        from po_brax_amd.training.networks import MLPHandle
        self.mlp, self.M, self.sizes = MLPHandle(sizes, act, fin), M, sizes
        n = C.c_longlong()
        check(lib.pob_mlp_saved_bytes(self.mlp.handle, M, C.byref(n)))
        self.saved = torch.full((n.value // 4,), float("nan"), device="cuda")
        check(lib.pob_mlp_backward_workspace_bytes(self.mlp.handle, M, C.byref(n)))
        self.workspace_bytes = n.value
        self.workspace = torch.full((n.value // 8,), float("nan"), dtype=torch.float64, device="cuda")
        self.x = torch.zeros((M, sizes[0]), device="cuda")
        self.theta = torch.zeros(param_count(sizes), device="cuda")
        self.dy = torch.zeros((M, sizes[-1]), device="cuda")
        self.y = torch.full((M, sizes[-1]), float("nan"), device="cuda")
        self.dtheta = torch.full((param_count(sizes),), float("nan"), device="cuda")
        self.dx = torch.full((M, sizes[0]), float("nan"), device="cuda") if want_dx else None

    def load(self, x, theta, dy):
        self.x.copy_(_cuda(x)); self.theta.copy_(_cuda(theta)); self.dy.copy_(_cuda(dy))

    def run(self):
        from po_brax_amd import _lib
        from po_brax_amd._lib import check, lib, ptr
        st = _lib.stream_handle(self.x.device)
        check(lib.pob_mlp_forward_train(self.mlp.handle, self.M, ptr(self.x), ptr(self.theta), ptr(self.y),
                                        ptr(self.saved) if self.saved.numel() else None, st))
        check(lib.pob_mlp_backward(self.mlp.handle, self.M, ptr(self.x), ptr(self.theta),
                                   ptr(self.saved) if self.saved.numel() else None, ptr(self.dy), ptr(self.dtheta),
                                   ptr(self.dx), ptr(self.workspace), st))

    def check(self, want, what):
        torch.cuda.synchronize()
        _same_bits(self.y, want["y"], (what, "y"))
        _same_bits(self.saved, want["saved"], (what, "saved"))
        _same_bits(self.dtheta, want["dtheta"], (what, "dtheta"))
        if self.dx is not None:
            _same_bits(self.dx, want["dx"], (what, "dx"))


def _run_and_check(host, sizes, act, fin, x, theta, dy, what, want_dx=True):
    b = Buffers(sizes, act, fin, x.shape[0], want_dx)
    b.load(x, theta, dy)
    b.run()
    want = ref_train_and_back(host, sizes, act, fin, x, theta, dy, want_dx)
    b.check(want, what)
    return b, want


@pytest.mark.parametrize("M", [1, 31, 32, 33, 65, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("net", list(NETS))
def test_kernels_equal_restatement(host, net, M):
    sizes = NETS[net]
    for act in (RELU, SWISH, TANH):
        x, theta, dy = make_problem(np.random.default_rng(100 * M + act), sizes, M)
        b, _ = _run_and_check(host, sizes, act, 0, x, theta, dy, (net, M, act))
        # y is pob_mlp_forward's
        from po_brax_amd import _lib
        from po_brax_amd._lib import check, lib, ptr
        y = torch.empty_like(b.y)
        check(lib.pob_mlp_forward(b.mlp.handle, M, ptr(b.x), ptr(b.theta), ptr(y), _lib.stream_handle(y.device)))
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(b.y))


@pytest.mark.parametrize("act", [RELU, SWISH, TANH])
@pytest.mark.parametrize("M", [33, 1025])
def test_activate_final(host, M, act):
    sizes = NETS["odd"]
    x, theta, dy = make_problem(np.random.default_rng(7 * M + act), sizes, M)
    _run_and_check(host, sizes, act, 1, x, theta, dy, ("activate_final", M, act))


def test_subnormal_and_zero_input_columns(host):
    sizes, M = NETS["odd"], 67
    x, theta, dy = make_problem(np.random.default_rng(11), sizes, M)
    x[:, 1] = (x[:, 1] * np.float32(1e-39)).astype(np.float32)
    x[:, 2] = 0.0
    assert (np.abs(x[:, 1]) < 1.2e-38).all() and (x[:, 1] != 0).any()
    for act in (RELU, SWISH, TANH):
        _, want = _run_and_check(host, sizes, act, 0, x, theta, dy, ("subnormal", act))
        n_out = sizes[1]
        assert (want["dtheta"][2 * n_out:3 * n_out].view(np.uint32) == 0).all()  # the zero column's row of dW_0


@pytest.mark.parametrize("net", ["single", "odd"])
def test_null_dx(host, net):
    sizes, M = NETS[net], 65
    x, theta, dy = make_problem(np.random.default_rng(12), sizes, M)
    _run_and_check(host, sizes, SWISH, 0, x, theta, dy, ("null dx", net), want_dx=False)


@pytest.mark.parametrize("n_in,n_out,M", [(3, 5, 7), (35, 37, 70), (6, 4, 1100)])
def test_integer_layout(host, n_in, n_out, M):
    x, theta, dy, want_y, want_dtheta, want_dx = integer_problem(np.random.default_rng(n_in), n_in, n_out, M)
    b = Buffers([n_in, n_out], SWISH, 0, M)
    b.load(x, theta, dy)
    b.run()
    torch.cuda.synchronize()
    _same_bits(b.y, want_y, "y")
    _same_bits(b.dtheta, want_dtheta, "dtheta")
    _same_bits(b.dx, want_dx, "dx")


def test_workspace_formula_and_bad_arguments():
    from po_brax_amd._lib import check, lib, ptr
    b = Buffers(NETS["odd"], SWISH, 0, 1025)
    n_delta = 1025 * (33 + 16) * 4
    assert b.workspace_bytes == ((n_delta + 7) & ~7) + 2 * param_count(NETS["odd"]) * 8
    assert b.saved.numel() == 1025 * 33
    h, n = b.mlp.handle, C.c_longlong()
    good = dict(x=ptr(b.x), theta=ptr(b.theta), saved=ptr(b.saved), dy=ptr(b.dy), dtheta=ptr(b.dtheta), ws=ptr(b.workspace),
                y=ptr(b.y))
    for M in (0, -1, 2 ** 31 // 33 + 1):
        with pytest.raises(ValueError):
            check(lib.pob_mlp_saved_bytes(h, M, C.byref(n)))
        with pytest.raises(ValueError):
            check(lib.pob_mlp_backward_workspace_bytes(h, M, C.byref(n)))
        with pytest.raises(ValueError):
            check(lib.pob_mlp_forward_train(h, M, good["x"], good["theta"], good["y"], good["saved"], None))
        with pytest.raises(ValueError):
            check(lib.pob_mlp_backward(h, M, good["x"], good["theta"], good["saved"], good["dy"], good["dtheta"], None,
                                       good["ws"], None))
    for missing in ("x", "theta", "y", "saved"):
        a = dict(good, **{missing: None})
        with pytest.raises(ValueError):
            check(lib.pob_mlp_forward_train(h, 1025, a["x"], a["theta"], a["y"], a["saved"], None))
    for missing in ("x", "theta", "saved", "dy", "dtheta", "ws"):
        a = dict(good, **{missing: None})
        with pytest.raises(ValueError):
            check(lib.pob_mlp_backward(h, 1025, a["x"], a["theta"], a["saved"], a["dy"], a["dtheta"], None, a["ws"], None))
    with pytest.raises(ValueError):
        check(lib.pob_mlp_saved_bytes(None, 4, C.byref(n)))
    torch.cuda.synchronize()  # nothing was launched, nothing failed


def test_captured_in_one_graph(host):
    sizes, M = NETS["odd"], 1057
    rng = np.random.default_rng(13)
    b = Buffers(sizes, SWISH, 0, M)
    b.load(*make_problem(rng, sizes, M))
    b.run()  # outside the capture once: modules loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.run()
    for rep in range(2):
        x, theta, dy = make_problem(rng, sizes, M)
        b.load(x, theta, dy)  # in place: the graph reads the same addresses
        for t in (b.y, b.saved, b.dtheta, b.dx):
            t.fill_(float("nan"))
        graph.replay()
        b.check(ref_train_and_back(host, sizes, SWISH, 0, x, theta, dy), ("graph", rep))


def test_apply_native_equals_the_c_call(host):
    from po_brax_amd.training import make_model
    sizes, M = [27, 33, 16], 257
    model = make_model(sizes[1:], sizes[0], "tanh")
    x, theta, dy = make_problem(np.random.default_rng(14), sizes, M)
    want = ref_train_and_back(host, sizes, TANH, 0, x, theta, dy)
    th = _cuda(theta).requires_grad_(True)
    xx = _cuda(x).reshape(1, M, sizes[0]).requires_grad_(True)
    y = model.apply_native(types.SimpleNamespace(theta=th), xx)
    assert y.shape == (1, M, 16) and y.requires_grad
    (y * _cuda(dy).reshape(1, M, 16)).sum().backward()
    torch.cuda.synchronize()
    _same_bits(y.reshape(M, 16), want["y"], "y")
    _same_bits(th.grad, want["dtheta"], "theta.grad")
    _same_bits(xx.grad.reshape(M, sizes[0]), want["dx"], "x.grad")
    # x without grad: theta.grad alone, the same bits; no grad at all: apply
    th2 = _cuda(theta).requires_grad_(True)
    model.apply_native(types.SimpleNamespace(theta=th2), _cuda(x)).backward(_cuda(dy))
    assert torch.equal(_bits(th2.grad), _bits(th.grad))
    with torch.no_grad():
        y0 = model.apply_native(types.SimpleNamespace(theta=th), _cuda(x))
    assert not y0.requires_grad and torch.equal(_bits(y0), _bits(y.reshape(M, 16)))
    # against float64 torch autograd, the host test's bound
    check_against_float64(sizes, TANH, 0, x, theta, dy, th.grad.cpu().numpy(), xx.grad.reshape(M, -1).cpu().numpy(),
                          "apply_native")


def test_apply_native_is_once_differentiable():
    """The kernels are invisible to autograd: a double backward raises instead of returning nothing."""
    from po_brax_amd.training import make_model
    model = make_model([7, 4], 5)
    th = model.init(torch.tensor([1, 2], dtype=torch.uint32)).theta.cuda().requires_grad_(True)
    y = model.apply_native(types.SimpleNamespace(theta=th), torch.ones((9, 5), device="cuda"))
    w = torch.ones_like(y).requires_grad_(True)  # the incoming gradient is part of the graph
    (g,) = torch.autograd.grad((y * w).sum(), th, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_backward_through_ppo_loss():
    """theta.grad of a [5 -> 7 -> 2 A] policy and a [5 -> 7 -> 1] value through apply_native and the
    loss kernel's head gradient, within the bound of the all-torch float64 result (the yardstick: the
    same all-torch spelling in float32)."""
    from po_brax_amd.training import make_model, networks, ppo_loss
    from test_gpu_ppo import _draws, _key, _loss_inputs
    from test_ppo_host import brax_loss, make_inputs
    M, A, D = 257, 2, 5
    rng = np.random.default_rng(10)
    d = make_inputs(rng, M, A)
    obs = rng.standard_normal((M, D)).astype(np.float32)
    key = _key(17)
    u = _draws(key, M, A)
    models = [make_model([7, 2 * A], D), make_model([7, 1], D)]
    thetas = [m.init(_key(20 + i)).theta for i, m in enumerate(models)]

    def all_torch(dtype):
        th = [t.detach().cpu().to(dtype).requires_grad_(True) for t in thetas]
        x = torch.from_numpy(obs).to(dtype)
        logits = networks._forward_torch(models[0].layer_sizes, models[0].activation, types.SimpleNamespace(theta=th[0]), x)
        values = networks._forward_torch(models[1].layer_sizes, models[1].activation, types.SimpleNamespace(theta=th[1]), x)
        c = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
        total = brax_loss(logits, values.reshape(M), c(d["raw"]), c(d["old_logp"]), c(d["adv"]), c(d["vs"]), c(u), 1e-4, 0.3)[0]
        total.backward()
        return [t.grad.numpy() for t in th]

    th = [t.detach().clone().requires_grad_(True) for t in thetas]
    x = _cuda(obs)
    logits = models[0].apply_native(types.SimpleNamespace(theta=th[0]), x)
    values = models[1].apply_native(types.SimpleNamespace(theta=th[1]), x).reshape(M)
    t, _ = _loss_inputs(d)
    total, _ = ppo_loss(logits, values, t["raw"], t["old_logp"], t["adv"], t["vs"], key)
    total.backward()
    torch.cuda.synchronize()
    f64, f32 = all_torch(torch.float64), all_torch(torch.float32)
    for i, name in enumerate(("policy", "value")):
        assert th[i].grad is not None and bool(th[i].grad.abs().sum() > 0)
        within_bound(th[i].grad.cpu().numpy(), f32[i], f64[i], f"{name} theta.grad")


# ---------------------------------------------------------------------------- learner
B_ROLL, T_ROLL = 64, 4
N_MINI = 4


class _Recorder:
    """Wraps a model's ``apply_native``: every call's input rows, the theta it ran under and its output."""

    def __init__(self, model):
        self.inner, self.calls = model.apply_native, []
        model.apply_native = self

    def __call__(self, params, x):
        y = self.inner(params, x)
        self.calls.append(dict(x=x.detach().clone(), theta=params.theta.detach().clone(), y=y.detach().clone(),
                               with_grad=y.requires_grad))
        return y


@functools.lru_cache(maxsize=None)
def _learning_rounds(backward, repeat=0):
    """Two rounds of replay(); update(roll) on ant_heavenhell from fixed keys: what each round left, the
    calls update() made to either model's apply_native, and the first minibatch's rows as update() drew
    them (``repeat`` only tells a rerun from the same keys apart)."""
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import PPOLearner, ValueFunction, networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    from test_gpu_parity import _keys
    env = envs.create("ant_heavenhell", batch_size=B_ROLL, episode_length=3)
    state = env.reset(torch.from_numpy(_keys(B_ROLL, 3)).cuda())
    D = env.observation_size
    norm = ObservationNormalizer(D)
    p_model, v_model = networks.make_models(2 * env.action_size, D)
    p_params = p_model.init(jumpy.random_prngkey(5))
    p_params.theta.mul_(3.0)
    policy = networks.NormalTanhPolicy(p_model, p_params, jumpy.random_prngkey(6), normalizer=norm)
    critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)), normalizer=norm)
    roll = ActorRollout(env, state, policy, T_ROLL, update_normalizer=True, critic=critic)
    learner = PPOLearner(policy, critic, learning_rate=1e-2, num_minibatches=N_MINI, num_update_epochs=1,
                         key=jumpy.random_prngkey(7), backward=backward)
    p_rec, v_rec = _Recorder(p_model), _Recorder(v_model)
    ptrs = (policy.theta.data_ptr(), critic.theta.data_ptr())
    N = T_ROLL * B_ROLL
    out = []
    for _ in range(2):
        theta0 = (policy.theta.clone(), critic.theta.clone())
        roll.replay()
        # the first minibatch's rows as update() will draw them (the generator's state is put back)
        gen_state = learner._generator.get_state()
        idx = torch.randperm(N, device="cuda", generator=learner._generator).to(torch.int32)[:N // N_MINI]
        learner._generator.set_state(gen_state)
        rows = norm.apply(roll.obs.reshape(N, D).index_select(0, idx))
        p_rec.calls, v_rec.calls = [], []
        metrics = learner.update(roll)
        torch.cuda.synchronize()
        with torch.no_grad():  # pob_mlp_forward of the same rows under the theta the round started from
            alone = p_model.apply(types.SimpleNamespace(theta=theta0[0]), rows).clone()
        out.append(dict(logp=roll.logp.clone(), values=roll.values.clone(), obs=roll.obs.clone(),
                        metrics={k: v.clone() for k, v in metrics.items()}, rows=rows, alone=alone,
                        p_calls=p_rec.calls, v_calls=v_rec.calls,
                        theta=(policy.theta.clone(), critic.theta.clone()), theta0=theta0))
    assert (policy.theta.data_ptr(), critic.theta.data_ptr()) == ptrs
    return out


@pytest.mark.parametrize("backward", ["native", ("native", "torch")], ids=["native", "native-torch"])
def test_learner_with_the_native_backward(backward):
    rounds = _learning_rounds(backward)
    for r in rounds:
        assert sorted(r["metrics"]) == ["entropy_loss", "policy_loss", "total_loss", "value_loss"]
        assert all(bool(torch.isfinite(v)) for v in r["metrics"].values())
        for k in range(2):  # both parameter vectors moved
            assert not torch.equal(r["theta"][k], r["theta0"][k]) and bool(torch.isfinite(r["theta"][k]).all())
        # update() itself went through apply_native, under grad, once a minibatch: for the policy, and
        # for the value network only when it was asked to
        assert len(r["p_calls"]) == N_MINI and all(c["with_grad"] for c in r["p_calls"])
        assert len(r["v_calls"]) == (N_MINI if backward == "native" else 0)
        # the learner's own first-minibatch logits: its rows and theta are the minibatch's, and the
        # logits are a standalone pob_mlp_forward's of those rows, bit for bit (the rollout's stored
        # logits were made under the normaliser table of before the replay's update)
        first = r["p_calls"][0]
        assert torch.equal(_bits(first["x"]), _bits(r["rows"])) and torch.equal(_bits(first["theta"]), _bits(r["theta0"][0]))
        assert first["y"].shape == (B_ROLL * T_ROLL // N_MINI, 16)
        assert torch.equal(_bits(first["y"]), _bits(r["alone"]))
    assert not torch.equal(rounds[1]["logp"], rounds[0]["logp"])
    # from the same keys: both rounds again, bit for bit
    again = _learning_rounds(backward, repeat=1)
    for a, b in zip(rounds, again):
        for k in ("logp", "values", "obs"):
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
        for k in range(2):
            assert torch.equal(_bits(a["theta"][k]), _bits(b["theta"][k])), k
        for k, v in a["metrics"].items():
            assert torch.equal(_bits(v.reshape(1)), _bits(b["metrics"][k].reshape(1))), k
    # against the torch-op learner from the same keys: the native pass sums in another order, so the
    # first round leaves other bits in the policy's theta; the value network's theta of that round
    # depends on its own gradient only, so it differs exactly when its pass was the native one
    torch_rounds = _learning_rounds("torch")
    assert not torch_rounds[0]["p_calls"] and not torch_rounds[0]["v_calls"]
    assert torch.equal(_bits(rounds[0]["theta0"][0]), _bits(torch_rounds[0]["theta0"][0]))
    assert not torch.equal(_bits(rounds[0]["theta"][0]), _bits(torch_rounds[0]["theta"][0]))
    same_value = torch.equal(_bits(rounds[0]["theta"][1]), _bits(torch_rounds[0]["theta"][1]))
    assert same_value == (backward != "native")
