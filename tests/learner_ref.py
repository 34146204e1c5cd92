"""An independent float64 learner to hold ``PPOLearner.update`` against (a helper of
test_learner_host.py and test_gpu_learner.py: no tests here).

Plain torch / numpy on the host.  ``record_steps`` keeps what every optimiser step of one ``update``
saw and left; ``reference_minibatches`` redraws the permutation slices and the entropy draws from the
generator state and the key saved before the update; ``reference_grads`` recomputes one minibatch in
a chosen dtype (gather, normalise, both networks in torch ops, brax's loss in brax's spelling,
autograd); ``Adam64`` is the textbook optimiser in float64.  ``check_update`` ties them together:
DESIGN.md "Learner against a float64 learner" has the bounds and the measured ratios."""
import types

import numpy as np
import torch

from test_ppo_host import U_MIN, brax_loss, ulp32, within_bound

EDGE = 1e-4  # no row's float64 rho may lie within this (relative) of 1 +- epsilon


def record_steps(learner):
    """Wrap ``learner.optimizer.step`` (an instance attribute: no product code changes).  Returns the
    record: ``steps`` grows by one dict a minibatch (clones of both thetas before the step, both
    gradients, both thetas after), next to the generator state, the key and the actors' ``data_ptr``
    as they stand now, i.e. before the ``update`` that follows."""
    rec = dict(steps=[], generator_state=learner._generator.get_state(), key=learner.key.clone(),
               ptrs=(learner.policy.theta.data_ptr(), learner.value_fn.theta.data_ptr()))
    inner = learner.optimizer.step

    def step(*args, **kw):
        before = [t.detach().clone() for t in learner._theta]
        grad = [t.grad.detach().clone() for t in learner._theta]
        out = inner(*args, **kw)
        rec["steps"].append(dict(before=before, grad=grad, after=[t.detach().clone() for t in learner._theta]))
        return out

    learner.optimizer.step = step
    return rec


def _draws_and_next(key, M, A):
    """(uniform(split(key)[1], (M, A), -1, 1) on the host, split(key)[0]): the public device threefry
    on a device key, the host's on a host key."""
    if key.is_cuda:
        from po_brax_amd import jumpy
        halves = jumpy.random_split(key)
        return jumpy.random_uniform(halves[1], (M, A), -1.0, 1.0).cpu(), halves[0].clone()
    from po_brax_amd.training import networks
    halves = networks._host_split(key)
    return networks._host_uniform(halves[1], M * A, -1.0, 1.0).reshape(M, A), halves[0].to(torch.uint32)


def reference_minibatches(generator_state, key, N, num_minibatches, num_epochs, A, device):
    """[(idx (M,) int64, u (M, A) float32)] on the host, one pair a minibatch in ``update``'s order:
    per epoch one ``randperm`` from a generator put into the saved state, sliced; per minibatch the
    draws of the key's second half, then key <- its first half."""
    gen = torch.Generator(device=device)
    gen.set_state(generator_state)
    key = key.clone()
    M = N // num_minibatches
    out = []
    for _ in range(num_epochs):
        perm = torch.randperm(N, device=device, generator=gen).to(torch.int32)
        for m in range(num_minibatches):
            u, key = _draws_and_next(key, M, A)
            out.append((perm[m * M:(m + 1) * M].cpu().long(), u))
    return out


def random_table(rng, width, mean_sd=0.5, lo=0.5, hi=2.0):
    """(mean, scale) float32 of a made-up normaliser table: mean_sd N(0, 1) and U(lo, hi)."""
    return (mean_sd * rng.standard_normal(width)).astype(np.float32), rng.uniform(lo, hi, width).astype(np.float32)


def table_of(normalizer):
    """(mean, scale, clip) of a normaliser as plain host tensors read now, or None."""
    if normalizer is None:
        return None
    return normalizer.mean.detach().cpu().clone(), normalizer.scale.detach().cpu().clone(), float(normalizer.clip)


def normalise(x, table):
    """clip((x - mean) scale, +-clip) in x's dtype."""
    if table is None:
        return x
    mean, scale, clip = table
    t = (x - mean.to(x.dtype)) * scale.to(x.dtype)
    return torch.clamp(t, -clip, clip) if clip > 0.0 else t


def forward(model, theta, x):
    from po_brax_amd.training import networks
    return networks._forward_torch(model.layer_sizes, model.activation, types.SimpleNamespace(theta=theta), x)


def reference_grads(dtype, models, thetas, tables, obs, raw, logp, adv, vs, idx, u, entropy_cost, eps):
    """One minibatch at ``thetas`` (policy, value) cast to ``dtype``; every array a host tensor in
    trajectory order, ``idx`` the minibatch's rows.  dict of ``grads`` (policy, value), ``losses``
    (total, policy, value, entropy), ``rho`` and ``logp``."""
    th = [t.detach().cpu().to(dtype).requires_grad_(True) for t in thetas]
    x = obs[idx].to(dtype)
    logits = forward(models[0], th[0], normalise(x, tables[0]))
    values = forward(models[1], th[1], normalise(x, tables[1])).reshape(idx.numel())
    c = lambda a: a[idx].to(dtype)  # noqa: E731
    u = torch.maximum(u, torch.tensor(float(U_MIN))).to(dtype)
    total, parts, new_logp, rho = brax_loss(logits, values, c(raw), c(logp), c(adv), c(vs), u, entropy_cost, eps)
    assert total.dtype == dtype
    total.backward()
    return dict(grads=[t.grad.numpy() for t in th], losses=torch.stack([total, *parts]).detach().numpy(),
                rho=rho.detach().numpy(), logp=new_logp.detach().numpy())


class Adam64:
    """Textbook Adam on one parameter vector: beta = (0.9, 0.999), epsilon 1e-8, bias-corrected; the
    moments are float64 and live as long as the object."""

    def __init__(self, lr, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.beta1, self.beta2, self.epsilon = float(lr), beta1, beta2, epsilon
        self.m = self.v = 0.0
        self.t = 0

    def step(self, theta, grad):
        theta, g = np.asarray(theta, np.float64), np.asarray(grad, np.float64)
        self.t += 1
        self.m = self.beta1 * self.m + (1.0 - self.beta1) * g
        self.v = self.beta2 * self.v + (1.0 - self.beta2) * g * g
        m_hat = self.m / (1.0 - self.beta1 ** self.t)
        v_hat = self.v / (1.0 - self.beta2 ** self.t)
        return theta - self.lr * m_hat / (np.sqrt(v_hat) + self.epsilon)


def adam64(lr):
    """One ``Adam64`` a network: (policy's, value's)."""
    return Adam64(lr), Adam64(lr)


def _softplus(x):
    return torch.logaddexp(x, torch.zeros_like(x))


def policy_logp(model, theta, table, obs, raw, dtype):
    """(logp (N,), loc, scale (N, A)) of brax's tanh-normal ``log_prob`` of ``raw`` in ``dtype``."""
    A = raw.shape[1]
    logits = forward(model, theta.detach().cpu().to(dtype), normalise(obs.to(dtype), table))
    zero = torch.zeros(raw.shape[0], dtype=dtype)
    logp = brax_loss(logits, zero, raw.to(dtype), zero, zero, zero, torch.zeros(raw.shape, dtype=dtype), 0.0, 0.3)[2]
    return logp, logits[:, :A], _softplus(logits[:, A:]) + 0.001


def make_roll(rng, T, B, D, A, policy, normalizer, noise, device="cpu"):
    """Synthetic rollout buffers: obs ~ N(0, 1); raw = loc + scale N(0, 1) from the float64 logits of
    ``policy`` as built (its ``model`` and ``theta``, the observations through ``normalizer``);
    advantages ~ N(0, 1); vs ~ 3 N(0, 1); logp = the float64 log-probability of the float32 raw plus
    ``noise`` N(0, 1)."""
    N = T * B
    obs = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32))
    table = table_of(normalizer)
    logits = forward(policy.model, policy.theta.detach().cpu().double(), normalise(obs.double(), table))
    loc, scale = logits[:, :A], _softplus(logits[:, A:]) + 0.001
    raw = (loc + scale * torch.from_numpy(rng.standard_normal((N, A)))).float()
    logp64 = policy_logp(policy.model, policy.theta, table, obs, raw, torch.float64)[0]
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(device)  # noqa: E731
    return types.SimpleNamespace(
        obs=obs.reshape(T, B, D).to(device), raw=raw.reshape(T, B, A).to(device),
        logp=f((logp64.numpy() + noise * rng.standard_normal(N)).reshape(T, B)),
        advantages=f(rng.standard_normal((T, B))), vs=f(3.0 * rng.standard_normal((T, B))))


def host_buffers(roll):
    """The five buffers ``update`` reads, flattened to trajectory rows on the host."""
    T, B = roll.logp.shape
    h = lambda t, *s: t.detach().cpu().reshape(T * B, *s)  # noqa: E731
    return dict(obs=h(roll.obs, roll.obs.shape[-1]), raw=h(roll.raw, roll.raw.shape[-1]), logp=h(roll.logp),
                adv=h(roll.advantages), vs=h(roll.vs))


def full_batch_losses(learner, roll):
    """(policy loss, value loss) of the whole batch in float64 at the actors' present parameters (the
    clipped surrogate and mean((vs - v)^2) / 4; no entropy term)."""
    b = host_buffers(roll)
    N = b["logp"].numel()
    zero_u = torch.zeros(b["raw"].shape)
    ref = reference_grads(torch.float64, (learner.policy.model, learner.value_fn.model),
                          (learner.policy.theta, learner.value_fn.theta),
                          (table_of(learner.policy.normalizer), table_of(learner.value_fn.normalizer)), b["obs"], b["raw"],
                          b["logp"], b["adv"], b["vs"], torch.arange(N), zero_u, 0.0, learner.ppo_epsilon)
    return float(ref["losses"][1]), float(ref["losses"][2])


def check_update(learner, roll, rec, metrics, case, tag):
    """Every recorded minibatch of the one ``update(roll)`` that followed ``record_steps`` against the
    float64 learner.  ``case``: "live" (10 % .. 60 % of the update's rows outside the clip range) or
    "on-policy" (every float64 rho in [0.9, 1.1]).  The conditions are computed from the float64
    reference alone and asserted before anything is compared.  Returns the metrics' triple (ours,
    float32, float64), each (4,): the caller holds them to the bound over the case's seeds."""
    policy, value_fn = learner.policy, learner.value_fn
    b = host_buffers(roll)
    N, A = b["logp"].numel(), policy.action_size
    eps, ec = learner.ppo_epsilon, learner.entropy_cost
    lr = float(learner.optimizer.param_groups[0]["lr"])
    models = (policy.model, value_fn.model)
    tables = (table_of(policy.normalizer), table_of(value_fn.normalizer))
    batches = reference_minibatches(rec["generator_state"], rec["key"], N, learner.num_minibatches,
                                    learner.num_update_epochs, A, policy.theta.device)
    steps = rec["steps"]
    assert len(steps) == len(batches) == learner.num_minibatches * learner.num_update_epochs
    refs = []
    for step, (idx, u) in zip(steps, batches):
        refs.append({dt: reference_grads(dt, models, step["before"], tables, b["obs"], b["raw"], b["logp"], b["adv"],
                                         b["vs"], idx, u, ec, eps) for dt in (torch.float64, torch.float32)})
    # ---- the conditions, from float64 alone
    rho = np.concatenate([r[torch.float64]["rho"] for r in refs])
    near = (np.abs(rho - (1.0 - eps)) <= EDGE * (1.0 - eps)) | (np.abs(rho - (1.0 + eps)) <= EDGE * (1.0 + eps))
    outside = float(((rho < 1.0 - eps) | (rho > 1.0 + eps)).mean())
    print(f"{tag}: rho64 in [{rho.min():.4f}, {rho.max():.4f}], {100.0 * outside:.1f} % outside the clip range, "
          f"{int(near.sum())} rows within {EDGE} of an edge")
    assert near.sum() == 0, "a row at a clip edge: take the next seed"
    if case == "live":
        assert 0.1 <= outside <= 0.6
    else:
        assert case == "on-policy" and rho.min() >= 0.9 and rho.max() <= 1.1
    # ---- gradients, per network: kept for check_case, which takes the maxima over all minibatches of the case
    grads, ratios = {}, {}
    for k, name in enumerate(("policy", "value")):
        got = np.concatenate([s["grad"][k].cpu().numpy().astype(np.float64) for s in steps])
        f32 = np.concatenate([r[torch.float32]["grads"][k] for r in refs]).astype(np.float64)
        f64 = np.concatenate([r[torch.float64]["grads"][k] for r in refs])
        assert np.isfinite(got).all() and np.abs(f64).max() > 0
        e, yard = np.abs(got - f64).max(), np.abs(f32 - f64).max()
        ratios[f"{name} grad"] = e / (4.0 * yard + ulp32(np.abs(f64).max()))
        print(f"{tag} {name} theta.grad: ours {e:.3e} float32 torch {yard:.3e}, this update alone at "
              f"{ratios[f'{name} grad']:.2f} of the bound")
        grads[name] = (got, f32, f64)
    # ---- the Adam steps, elementwise, and that step i + 1 started where step i ended
    opt = adam64(lr)
    worst = 0.0
    for i, step in enumerate(steps):
        for k in range(2):
            before, after = (step[w][k].cpu().numpy() for w in ("before", "after"))
            if i:
                assert np.array_equal(before.view(np.uint32), steps[i - 1]["after"][k].cpu().numpy().view(np.uint32))
            want = opt[k].step(before, step["grad"][k].cpu().numpy())
            bound = np.spacing(np.abs(before)).astype(np.float64) + 1e-6 * lr
            r = np.abs(after.astype(np.float64) - want) / bound
            worst = max(worst, float(r.max()))
            assert (r <= 1.0).all(), (tag, "Adam step", i, k, float(r.max()))
    print(f"{tag}: Adam steps at {worst:.2f} of ulp32(theta) + 1e-6 lr")
    ratios["adam"] = worst
    # ---- in place: the actors' own storage holds the last step's bits and never moved
    for k, actor in enumerate((policy, value_fn)):
        assert actor.theta.data_ptr() == rec["ptrs"][k]
        assert torch.equal(actor.theta.view(torch.int32), steps[-1]["after"][k].view(torch.int32))
        assert not actor.theta.requires_grad
    # ---- the returned metrics are the last minibatch's
    assert sorted(metrics) == ["entropy_loss", "policy_loss", "total_loss", "value_loss"]
    ours = np.array([float(metrics[k]) for k in ("total_loss", "policy_loss", "value_loss", "entropy_loss")], np.float64)
    last = refs[-1]
    return dict(metrics=(ours, last[torch.float32]["losses"].astype(np.float64), last[torch.float64]["losses"]),
                grads=grads, ratios=ratios)


def check_case(results, tag):
    """``check_update``'s results of every seed of a case: both gradients within the bound with the
    maxima taken over all minibatches of the case, the four returned scalars with the maxima over the
    seeds (one update gives ONE sample of each scalar, and a value network's float32 yardstick of one
    update varies several-fold from seed to seed: test_ppo_host.check_against_float64)."""
    out = {}
    for name in ("policy", "value"):
        cols = [np.concatenate([r["grads"][name][j] for r in results]) for j in range(3)]
        e, _, bound = within_bound(cols[0], cols[1], cols[2], f"{tag} {name} theta.grad")
        out[f"{name} grad"] = e / bound
    for i, name in enumerate(("total_loss", "policy_loss", "value_loss", "entropy_loss")):
        cols = [np.array([r["metrics"][j][i] for r in results]) for j in range(3)]
        e, _, bound = within_bound(cols[0], cols[1], cols[2], f"{tag} {name}")
        out[name] = e / bound
    out["adam"] = max(r["ratios"]["adam"] for r in results)
    print(f"{tag}: Adam steps at {out['adam']:.2f} of the bound over the case")
    return out


def logp_bound(raw, logp64, logp32, loc64, scale64):
    """Per row: R_row + 4 max_rows |L32 - L64| + ulp32(max |L64|), with R_row = sum_a |e_a| d_a +
    d_a^2 / 2 and d_a = ulp32(|raw_a| + |loc_a|) / scale_a: the first-order effect of raw's own float32
    rounding on -e^2 / 2 (the actor's term is made from eps itself, the loss's from the stored raw)."""
    raw, loc, scale = (np.asarray(a, np.float64) for a in (raw, loc64, scale64))
    d = np.spacing((np.abs(raw) + np.abs(loc)).astype(np.float32)).astype(np.float64) / scale
    e = np.abs(raw - loc) / scale
    R = (e * d + 0.5 * d * d).sum(axis=1)
    logp64, logp32 = np.asarray(logp64, np.float64), np.asarray(logp32, np.float64)
    return R + 4.0 * float(np.abs(logp32 - logp64).max()) + ulp32(np.abs(logp64).max())
