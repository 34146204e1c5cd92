"""GPU: k_ppo_loss and its two reduction launches against their restatement (ppo_loss_ref of
po-brax_amd/csrc/pob_mlp.h: integer-view equality of dlogits, dvalues, the chunk partials and the
four scalars, no tolerance), ``ppo_loss`` on device tensors (key advance, capture, backward through
the networks' torch-op apply) and the learner on a captured rollout."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from test_ppo_host import CHUNK, brax_loss, build_ppo_host, make_inputs, ref_ppo, within_bound

pytestmark = pytest.mark.gpu

KEYS = ("logits", "values", "raw", "old_logp", "adv", "vs")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_ppo_host(tmp_path_factory.mktemp("ppo_host_gpu"))


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(got, want, what):
    want = want if isinstance(want, torch.Tensor) else _cuda(want)
    assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want)), what


def _key(seed, hi=0):
    return torch.tensor([hi, seed], dtype=torch.uint32).cuda()


def _draws(key, M, A):
    """uniform(split(key)[1], (M, A), -1, 1) of the device threefry, on the host."""
    from po_brax_amd import jumpy
    return jumpy.random_uniform(jumpy.random_split(key)[1], (M, A), -1.0, 1.0).cpu().numpy()


def _pob_ppo(d, key, ec=1e-4, eps=0.3, want_dlogits=True, want_dvalues=True):
    """One pob_ppo_loss call on device copies; outputs pre-filled with NaN.  dict like ref_ppo's."""
    from po_brax_amd import _lib
    t = {k: _cuda(np.asarray(d[k], np.float32)) for k in KEYS}
    idx = None if d.get("idx") is None else _cuda(np.asarray(d["idx"], np.int32))
    M, W = d["logits"].shape
    n_chunks = (M + CHUNK - 1) // CHUNK
    need = C.c_longlong()
    _lib.check(_lib.lib.pob_ppo_loss_workspace_bytes(M, C.byref(need)))
    assert need.value % 8 == 0 and need.value >= n_chunks * 24 + 12 * M
    ws = torch.full((need.value // 8,), float("nan"), dtype=torch.float64, device="cuda")
    dl = torch.full((M, W), float("nan"), device="cuda") if want_dlogits else None
    dv = torch.full((M,), float("nan"), device="cuda") if want_dvalues else None
    losses = torch.full((4,), float("nan"), device="cuda")
    _lib.check(_lib.lib.pob_ppo_loss(M, W // 2, _lib.ptr(t["logits"]), _lib.ptr(t["values"]), _lib.ptr(idx), _lib.ptr(t["raw"]),
                                     _lib.ptr(t["old_logp"]), _lib.ptr(t["adv"]), _lib.ptr(t["vs"]), _lib.ptr(key), ec, eps,
                                     _lib.ptr(dl), _lib.ptr(dv), _lib.ptr(losses), _lib.ptr(ws), _lib.stream_handle()))
    torch.cuda.synchronize()
    return dict(dlogits=dl, dvalues=dv, losses=losses, partials=ws[:3 * n_chunks].reshape(n_chunks, 3))


def _check(host, d, key, ec=1e-4, eps=0.3, what=None, **kw):
    M, W = d["logits"].shape
    d = dict(d, u=_draws(key, M, W // 2))
    want = ref_ppo(host, d, ec, eps, **kw)
    got = _pob_ppo(d, key, ec, eps, **kw)
    for k in ("dlogits", "dvalues", "partials", "losses"):
        if want[k] is None:
            assert got[k] is None
        else:
            _same_bits(got[k], want[k], (what, k))
    return got, want


def _variants(rng, M, A):
    """idx NULL; a permutation with the minibatch rows permuted; idx with repeats into N > M rows."""
    d = make_inputs(rng, M, A)
    yield "null", d
    perm = rng.permutation(M).astype(np.int32)
    yield "permutation", dict(d, logits=d["logits"][perm], values=d["values"][perm], idx=perm)
    yield "repeats", make_inputs(rng, M, A, N=M + M // 2 + 3)


def test_header_constants(host):
    """The shapes below straddle the chunk and include the largest action size."""
    assert int(host.ppo_ref_chunk()) == CHUNK == 1024 and int(host.ppo_ref_max_a()) == 128


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1000, 1025, 2049])
def test_kernel_equals_restatement(host, M):
    # A = 5: a tile of 204 rows whose components do not fill the block; A = 128: 8 rows a tile
    for A in (1, 3, 5, 8, 128):
        rng = np.random.default_rng(1000 * M + A)
        for name, d in _variants(rng, M, A):
            key = _key(M + A)
            before = key.clone()
            _check(host, d, key, what=(M, A, name))
            assert torch.equal(key, before), "the C call leaves the key alone"


@pytest.mark.parametrize("ec,eps", [(1e-4, 0.0), (0.0, 0.3), (0.0, 0.0)])
def test_other_coefficients(host, ec, eps):
    rng = np.random.default_rng(3)
    for A in (3, 8):
        d = make_inputs(rng, 257, A, N=400)
        got, _ = _check(host, d, _key(11), ec, eps, what=(A, ec, eps))
        if ec == 0.0:
            assert float(got["losses"][3]) == 0.0


def test_nan_row(host):
    M, A = 257, 8
    d = make_inputs(np.random.default_rng(4), M, A)
    key = _key(12)
    clean, _ = _check(host, d, key)
    e = dict(d, adv=d["adv"].copy())
    e["adv"][130] = np.nan
    got, _ = _check(host, e, key)
    others = torch.arange(M, device="cuda") != 130
    _same_bits(got["dlogits"][others], clean["dlogits"][others], "other rows")
    _same_bits(got["dvalues"], clean["dvalues"], "dvalues")
    assert bool(torch.isnan(got["losses"][0])) and bool(torch.isnan(got["losses"][1]))
    _same_bits(got["losses"][2:], clean["losses"][2:], "value and entropy losses")


def test_subnormal_old_logp(host):
    M, A = 65, 3
    d = make_inputs(np.random.default_rng(5), M, A)
    d["old_logp"] = (d["old_logp"] * np.float32(1e-40)).astype(np.float32)
    nz = d["old_logp"][d["old_logp"] != 0]
    assert nz.size and (np.abs(nz) < 1.2e-38).all()
    _check(host, d, _key(13))


def test_u_at_the_clamp(host):
    """Key [0, 705]: element (1972, 2) of the (2049, 8) draw is exactly -1."""
    M, A = 2049, 8
    key = _key(705)
    u = _draws(key, M, A)
    assert u[1972, 2] == -1.0 and u.min() == -1.0
    d = make_inputs(np.random.default_rng(6), M, A)
    got, _ = _check(host, d, key)
    assert bool(torch.isfinite(got["dlogits"][1972]).all())


def test_null_outputs(host):
    d = make_inputs(np.random.default_rng(7), 1025, 3, N=1500)
    key = _key(14)
    full, _ = _check(host, d, key)
    no_dl, _ = _check(host, d, key, want_dlogits=False)
    no_dv, _ = _check(host, d, key, want_dvalues=False)
    _same_bits(no_dl["losses"], full["losses"], "losses without dlogits")
    _same_bits(no_dv["losses"], full["losses"], "losses without dvalues")


def _loss_inputs(d, requires_grad=False):
    t = {k: _cuda(np.asarray(d[k], np.float32)) for k in KEYS}
    if requires_grad:
        t["logits"].requires_grad_(True)
        t["values"].requires_grad_(True)
    idx = None if d.get("idx") is None else _cuda(np.asarray(d["idx"], np.int32))
    return t, idx


def test_ppo_loss_takes_the_kernel_and_advances_the_key(host):
    from po_brax_amd import jumpy
    from po_brax_amd.training import ppo_loss
    M, A = 257, 3
    d = make_inputs(np.random.default_rng(8), M, A, N=300)
    key = _key(15)
    before = key.clone()
    d["u"] = _draws(key, M, A)
    want = ref_ppo(host, d, 1e-3, 0.2)
    t, idx = _loss_inputs(d, requires_grad=True)
    total, metrics = ppo_loss(t["logits"], t["values"], t["raw"], t["old_logp"], t["adv"], t["vs"], key, idx=idx,
                              entropy_cost=1e-3, ppo_epsilon=0.2)
    (total * 2.0).backward()
    torch.cuda.synchronize()
    losses = torch.stack([total.detach(), metrics["policy_loss"], metrics["value_loss"], metrics["entropy_loss"]])
    _same_bits(losses, want["losses"], "losses")
    _same_bits(t["logits"].grad, want["dlogits"] * np.float32(2.0), "dlogits x 2")
    _same_bits(t["values"].grad, want["dvalues"] * np.float32(2.0), "dvalues x 2")
    assert torch.equal(key, jumpy.random_split(before)[0]) and not torch.equal(key, before)
    # a non-contiguous logits takes the torch-op spelling on the device: the same numbers to rounding
    wide = torch.zeros((M, 2 * A + 1), device="cuda")
    wide[:, :2 * A] = t["logits"].detach()
    total_t, _ = ppo_loss(wide[:, :2 * A], t["values"].detach(), t["raw"], t["old_logp"], t["adv"], t["vs"], before.clone(),
                          idx=idx, entropy_cost=1e-3, ppo_epsilon=0.2)
    torch.testing.assert_close(total_t, total.detach(), rtol=1e-5, atol=1e-6)


def test_ppo_loss_is_capturable(host):
    from po_brax_amd.training import ppo_loss
    M, A = 257, 8
    rng = np.random.default_rng(9)
    d = make_inputs(rng, M, A)
    t, _ = _loss_inputs(d)
    key = _key(16)
    keys = [key.clone()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total, metrics = ppo_loss(t["logits"], t["values"], t["raw"], t["old_logp"], t["adv"], t["vs"], key)
    for rep in range(2):
        if rep:  # new inputs in place; the key is the one the first replay left
            d = make_inputs(rng, M, A)
            for k in KEYS:
                t[k].copy_(_cuda(np.asarray(d[k], np.float32)))
        keys.append(key.clone())
        graph.replay()
        torch.cuda.synchronize()
        want = ref_ppo(host, dict(d, u=_draws(keys[-1], M, A)), 1e-4, 0.3)
        losses = torch.stack([total, metrics["policy_loss"], metrics["value_loss"], metrics["entropy_loss"]])
        _same_bits(losses, want["losses"], ("losses", rep))
        assert not torch.equal(key, keys[-1])


def test_backward_through_the_networks(host):
    """theta.grad of a [5 -> 7 -> 2 A] policy and a [5 -> 7 -> 1] value through their torch-op apply
    and the kernel's head gradient, within the host test's bound of the all-torch float64 result
    (the yardstick: the same all-torch spelling in float32)."""
    from po_brax_amd.training import make_model, networks, ppo_loss
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
    logits = models[0].apply(types.SimpleNamespace(theta=th[0]), x)
    values = models[1].apply(types.SimpleNamespace(theta=th[1]), x).reshape(M)
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


def _learning_rounds():
    """Two rounds of replay(); update(roll) on ant_heavenhell from fixed keys: what each round left."""
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
    learner = PPOLearner(policy, critic, learning_rate=1e-2, num_minibatches=4, num_update_epochs=1,
                         key=jumpy.random_prngkey(7))
    ptrs = (policy.theta.data_ptr(), critic.theta.data_ptr())
    out = []
    for _ in range(2):
        theta0 = (policy.theta.clone(), critic.theta.clone())
        roll.replay()
        metrics = learner.update(roll)
        torch.cuda.synchronize()
        out.append(dict(logp=roll.logp.clone(), values=roll.values.clone(), obs=roll.obs.clone(),
                        final_obs=roll.final_obs.clone(), metrics={k: v.clone() for k, v in metrics.items()},
                        theta=(policy.theta.clone(), critic.theta.clone()), theta0=theta0))
    assert (policy.theta.data_ptr(), critic.theta.data_ptr()) == ptrs
    return out, roll, critic


def test_learner_on_a_captured_rollout():
    from test_gpu_gae import _standalone_values
    rounds, roll, critic = _learning_rounds()
    for r in rounds:
        assert sorted(r["metrics"]) == ["entropy_loss", "policy_loss", "total_loss", "value_loss"]
        assert all(bool(torch.isfinite(v)) for v in r["metrics"].values())
        for k in range(2):  # both parameter vectors moved
            assert not torch.equal(r["theta"][k], r["theta0"][k]) and bool(torch.isfinite(r["theta"][k]).all())
    # the captured graph saw the update: the second replay acted and valued under the first round's theta
    assert not torch.equal(rounds[1]["logp"], rounds[0]["logp"])
    assert torch.equal(rounds[1]["theta0"][1], rounds[0]["theta"][1])
    D = roll.obs.shape[-1]
    rows = torch.cat([rounds[1]["obs"], rounds[1]["final_obs"][None]]).reshape((T_ROLL + 1) * B_ROLL, D)
    keep = critic.theta.clone()
    critic.theta.copy_(rounds[1]["theta0"][1])  # the parameters the second replay ran under (the table is unchanged since)
    want = _standalone_values(critic, rows)
    critic.theta.copy_(keep)
    assert torch.equal(_bits(rounds[1]["values"].reshape(-1)), _bits(want))
    # from the same keys: both rounds again, bit for bit
    again, _, _ = _learning_rounds()
    for a, b in zip(rounds, again):
        for k in ("logp", "values", "obs"):
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
        for k in range(2):
            assert torch.equal(_bits(a["theta"][k]), _bits(b["theta"][k])), k
        for k, v in a["metrics"].items():
            assert torch.equal(_bits(v.reshape(1)), _bits(b["metrics"][k].reshape(1))), k


def test_learner_rejects_an_indivisible_batch():
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import PPOLearner, ValueFunction, networks
    from test_gpu_parity import _keys
    env = envs.create("ant_heavenhell", batch_size=B_ROLL, episode_length=3)
    state = env.reset(torch.from_numpy(_keys(B_ROLL, 3)).cuda())
    D = env.observation_size
    p_model, v_model = networks.make_models(2 * env.action_size, D)
    policy = networks.NormalTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6))
    critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)))
    roll = ActorRollout(env, state, policy, 3, critic=critic)
    learner = PPOLearner(policy, critic, num_minibatches=5, key=jumpy.random_prngkey(7))
    with pytest.raises(ValueError, match="not divisible"):
        learner.update(roll)
