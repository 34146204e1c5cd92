"""CPU: the public PPO-loss interface (po_brax_amd.training.ppo) and the argument checks of
pob_ppo_loss.

``ppo_loss`` on CPU float32 tensors takes the torch-op spelling with the header's scalar functions
spelled out; its four scalars and both gradients equal ``ppo_loss_ref`` bit for bit (the entropy
draws are the host threefry's).  On float64 tensors the same operation order runs with torch's own
functions: its backward agrees with float64 autograd of brax's spelling to rounding (the gradients
are analytic, the same formulas), and the float32 path stays within test_ppo_host.py's bound of it."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_ppo_host import brax_ppo, build_ppo_host, make_inputs, ref_ppo, same_bits, within_bound, kept_rows


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_ppo_host(tmp_path_factory.mktemp("ppo_host_api"))


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32)


def _draws(key, M, A):
    """uniform(split(key)[1], (M, A), -1, 1) of the host threefry."""
    from po_brax_amd.training import networks
    return networks._host_uniform(networks._host_split(key)[1], M * A, -1.0, 1.0).reshape(M, A).numpy()


def _call(d, key, dtype=torch.float32, **kw):
    from po_brax_amd.training import ppo_loss
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    logits, values = t(d["logits"]).requires_grad_(True), t(d["values"]).requires_grad_(True)
    idx = None if d.get("idx") is None else torch.from_numpy(np.asarray(d["idx"], np.int32))
    total, metrics = ppo_loss(logits, values, t(d["raw"]), t(d["old_logp"]), t(d["adv"]), t(d["vs"]), key, idx=idx, **kw)
    total.backward()
    losses = torch.stack([total.detach(), metrics["policy_loss"], metrics["value_loss"], metrics["entropy_loss"]])
    return dict(dlogits=logits.grad.numpy(), dvalues=values.grad.numpy(), losses=losses.numpy(), total=total, metrics=metrics)


@pytest.mark.parametrize("M,A,N,ec,eps", [(1, 1, None, 1e-4, 0.3), (257, 3, None, 1e-4, 0.3), (1025, 8, 1500, 1e-2, 0.3),
                                          (65, 2, 80, 0.0, 0.0)])
def test_torch_path_equals_the_restatement(host, M, A, N, ec, eps):
    d = make_inputs(np.random.default_rng(M + A), M, A, N)
    key = _key(M)
    before = key.clone()
    d["u"] = _draws(key, M, A)
    got = _call(d, key, entropy_cost=ec, ppo_epsilon=eps)
    want = ref_ppo(host, d, ec, eps)
    for k in ("dlogits", "dvalues", "losses"):
        assert got[k].dtype == np.float32 and same_bits(got[k], want[k]), k
    assert got["total"].dim() == 0 and all(v.dim() == 0 and not v.requires_grad for v in got["metrics"].values())
    assert sorted(got["metrics"]) == ["entropy_loss", "policy_loss", "value_loss"]
    # the key advanced: key <- split(key)[0]
    from po_brax_amd.training import networks
    assert torch.equal(key.to(torch.int64), networks._host_split(before)[0]) and not torch.equal(key, before)


def test_backward_scales_with_the_upstream_gradient():
    from po_brax_amd.training import ppo_loss
    d = make_inputs(np.random.default_rng(3), 65, 3)
    t = torch.from_numpy
    grads = []
    for factor in (1.0, -2.5):
        logits, values = t(d["logits"]).requires_grad_(True), t(d["values"]).requires_grad_(True)
        total, _ = ppo_loss(logits, values, t(d["raw"]), t(d["old_logp"]), t(d["adv"]), t(d["vs"]), _key(3))
        (total * factor).backward()
        grads.append((logits.grad, values.grad))
    assert torch.equal(grads[1][0], grads[0][0] * -2.5) and torch.equal(grads[1][1], grads[0][1] * -2.5)
    # raw, old_logp, advantages and vs take no gradient
    raw = t(d["raw"]).requires_grad_(True)
    total, _ = ppo_loss(t(d["logits"]).requires_grad_(True), t(d["values"]), raw, t(d["old_logp"]), t(d["adv"]), t(d["vs"]),
                        _key(3))
    total.backward()
    assert raw.grad is None


@pytest.mark.parametrize("M,A", [(257, 3), (4096, 8)])
def test_backward_against_the_float64_spelling(M, A):
    d = make_inputs(np.random.default_rng(7 * M + A), M, A)
    key = _key(M)
    d["u"] = _draws(key, M, A)
    f64 = brax_ppo(d, 1e-4, 0.3, torch.float64)
    f32 = brax_ppo(d, 1e-4, 0.3, torch.float32)
    keep = kept_rows(f64["rho"], 0.3, M)
    ours64 = _call(d, key.clone(), torch.float64)
    ours32 = _call(d, key.clone())
    # float64 tensors: analytic gradients in torch's own float64 functions against autograd
    for k in ("dlogits", "dvalues"):
        assert ours64[k].dtype == np.float64
        a, b = (ours64[k][keep], f64[k][keep]) if k == "dlogits" else (ours64[k], f64[k])
        err = float(np.abs(a - b).max())
        print(f"M {M} A {A} {k}: float64 path against float64 autograd {err:.3e}, largest gradient {np.abs(b).max():.3e}")
        assert err <= 1e-12 * max(1.0, float(np.abs(b).max()))
    np.testing.assert_allclose(ours64["losses"], f64["losses"], rtol=1e-12, atol=1e-15)
    # float32 tensors: within the host test's bound of the float64 result
    within_bound(ours32["dlogits"][keep], f32["dlogits"][keep], f64["dlogits"][keep], f"M {M} A {A} float32 path dlogits")
    within_bound(ours32["dvalues"], f32["dvalues"], f64["dvalues"], f"M {M} A {A} float32 path dvalues")


def test_argument_errors():
    from po_brax_amd.training import ppo_loss
    d = make_inputs(np.random.default_rng(4), 9, 2)
    t = torch.from_numpy
    ok = dict(logits=t(d["logits"]), values=t(d["values"]), raw=t(d["raw"]), old_logp=t(d["old_logp"]),
              advantages=t(d["adv"]), vs=t(d["vs"]), key=_key(1))

    def call(**kw):
        return ppo_loss(**{**ok, **kw})

    with pytest.raises(ValueError, match="logits"):
        call(logits=ok["logits"][:, :3])
    with pytest.raises(ValueError, match="logits"):
        call(logits=ok["logits"][0])
    with pytest.raises(ValueError, match="values"):
        call(values=ok["values"][:8])
    with pytest.raises(ValueError, match="raw"):
        call(raw=ok["raw"][:, :1])
    with pytest.raises(ValueError, match="old_logp"):
        call(old_logp=ok["old_logp"][:8])
    with pytest.raises(ValueError, match="without idx"):
        call(raw=torch.cat([ok["raw"], ok["raw"]]), old_logp=ok["old_logp"].repeat(2), advantages=ok["advantages"].repeat(2),
             vs=ok["vs"].repeat(2))
    with pytest.raises(ValueError, match="idx"):
        call(idx=torch.arange(9))  # int64
    with pytest.raises(ValueError, match="idx"):
        call(idx=torch.arange(8, dtype=torch.int32))
    with pytest.raises(TypeError, match="advantages"):
        call(advantages=ok["advantages"].double())
    with pytest.raises(TypeError, match="vs"):
        call(vs=d["vs"])
    with pytest.raises(TypeError, match="logits"):
        call(logits=ok["logits"].to(torch.int32))
    with pytest.raises(TypeError, match="key"):
        call(key=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="action size"):
        call(logits=torch.zeros(9, 2 * 129), raw=torch.zeros(9, 129))


def test_pob_ppo_loss_rejects_bad_arguments_without_a_gpu():
    from po_brax_amd import _lib
    lib = _lib.lib
    a = np.zeros(64, np.float32)
    p = a.ctypes.data_as(C.c_void_p)  # never dereferenced: every call below is rejected before any HIP call
    ok = dict(M=4, A=2, logits=p, values=p, idx=None, raw=p, old=p, adv=p, vs=p, key=p, dl=p, dv=p, losses=p, ws=p)

    def call(**kw):
        k = {**ok, **kw}
        return lib.pob_ppo_loss(k["M"], k["A"], k["logits"], k["values"], k["idx"], k["raw"], k["old"], k["adv"], k["vs"],
                                k["key"], 1e-4, 0.3, k["dl"], k["dv"], k["losses"], k["ws"], None)

    for kw, word in ((dict(M=0), "M"), (dict(M=-1), "M"), (dict(A=0), "A"), (dict(A=129), "128"), (dict(M=2 ** 31, A=2), "2^32"),
                     (dict(M=2 ** 33, A=1), "2^32"), (dict(logits=None), "NULL"), (dict(values=None), "NULL"),
                     (dict(raw=None), "NULL"), (dict(old=None), "NULL"), (dict(adv=None), "NULL"), (dict(vs=None), "NULL"),
                     (dict(key=None), "key"), (dict(losses=None), "NULL"), (dict(ws=None), "NULL")):
        assert call(**kw) != 0, kw
        msg = lib.pob_last_error().decode()
        assert msg.startswith("ppo_loss:") and word in msg, (kw, msg)
        with pytest.raises(ValueError, match="ppo_loss:"):
            _lib.check(call(**kw))
    need = C.c_longlong()
    assert lib.pob_ppo_loss_workspace_bytes(1025, C.byref(need)) == 0 and need.value == 2 * 3 * 8 + 3 * 1025 * 4 + 4
    assert need.value % 8 == 0
    assert lib.pob_ppo_loss_workspace_bytes(0, C.byref(need)) != 0 and lib.pob_ppo_loss_workspace_bytes(4, None) != 0
    assert {"pob_ppo_loss", "pob_ppo_loss_workspace_bytes"} <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 8 and lib.pob_abi_version() == 8


class _Roll:
    """The buffers of an ActorRollout(..., critic=) replay, as far as update() reads them."""

    def __init__(self, T, B, D, A):
        self.obs, self.raw = torch.zeros(T, B, D), torch.zeros(T, B, A)
        self.logp = self.advantages = self.vs = torch.zeros(T, B)


def test_learner_checks():
    from po_brax_amd.training import NormalTanhPolicy, PPOLearner, ValueFunction, make_model
    D, A = 5, 2
    policy = NormalTanhPolicy.__new__(NormalTanhPolicy)  # the native actor needs a GPU: only what the learner reads
    model = make_model([7, 2 * A], D)
    policy.model, policy.params = model, model.init(_key(0))
    policy.theta, policy.obs_size, policy.action_size, policy.normalizer = policy.params.theta, D, A, None
    value_fn = ValueFunction.__new__(ValueFunction)
    vmodel = make_model([7, 1], D)
    value_fn.model, value_fn.params = vmodel, vmodel.init(_key(1))
    value_fn.theta, value_fn.obs_size, value_fn.normalizer = value_fn.params.theta, D, None
    with pytest.raises(TypeError, match="NormalTanhPolicy"):
        PPOLearner(object(), value_fn, key=_key(2))
    with pytest.raises(TypeError, match="ValueFunction"):
        PPOLearner(policy, object(), key=_key(2))
    with pytest.raises(ValueError, match="key"):
        PPOLearner(policy, value_fn)
    with pytest.raises(ValueError, match="positive"):
        PPOLearner(policy, value_fn, num_minibatches=0, key=_key(2))
    learner = PPOLearner(policy, value_fn, num_minibatches=4, num_update_epochs=1, key=_key(2))
    with pytest.raises(ValueError, match="not divisible"):
        learner.update(_Roll(3, 7, D, A))
    with pytest.raises(ValueError, match="critic="):
        learner.update(types_only_obs(D))
    # a divisible T B on host tensors runs the whole loop in torch ops: in-place steps, finite metrics
    rng = np.random.default_rng(0)
    roll = _Roll(4, 8, D, A)
    roll.obs, roll.raw = torch.from_numpy(rng.standard_normal((4, 8, D)).astype(np.float32)), torch.from_numpy(
        rng.standard_normal((4, 8, A)).astype(np.float32))
    roll.logp = torch.from_numpy((-2.0 + 0.3 * rng.standard_normal((4, 8))).astype(np.float32))
    roll.advantages = torch.from_numpy(rng.standard_normal((4, 8)).astype(np.float32))
    roll.vs = torch.from_numpy(rng.standard_normal((4, 8)).astype(np.float32))
    before = [policy.theta.clone(), value_fn.theta.clone()]
    ptrs = [policy.theta.data_ptr(), value_fn.theta.data_ptr()]
    metrics = learner.update(roll)
    assert sorted(metrics) == ["entropy_loss", "policy_loss", "total_loss", "value_loss"]
    assert all(bool(torch.isfinite(v)) for v in metrics.values())
    assert not torch.equal(policy.theta, before[0]) and not torch.equal(value_fn.theta, before[1])
    assert [policy.theta.data_ptr(), value_fn.theta.data_ptr()] == ptrs
    assert not policy.theta.requires_grad and not value_fn.theta.requires_grad


def types_only_obs(D):
    class R:
        obs = torch.zeros(2, 4, D)
    return R()
