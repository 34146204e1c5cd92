"""An independent float64 learner to hold ``RecurrentPPOLearner.update`` against (a helper of
test_recurrent_learner_host.py and test_gpu_recurrent_learner.py: no tests here), in the manner of
learner_ref.py, whose recorder, Adam, bounds and problem conditions it reuses.

What differs from the feed-forward learner: minibatches are slices of a permutation of the B ENVS;
a minibatch is the T-step window of its envs, unrolled here in plain torch ops written out in this
file (pre-MLP, GRU cell, post-MLP: brax-style formulas, not the product's ``_recurrent_torch``) from
``hidden[0]`` with the state zeroed where ``done[t - 1]`` is set; the loss rows are ``t B + idx[m]``
in (t, m) order."""
import types

import numpy as np
import torch

import learner_ref as ref
from test_ppo_host import U_MIN, brax_loss, ulp32

ACT = {0: torch.relu, 1: torch.nn.functional.silu, 2: torch.tanh}


def unroll(model, theta, x, h, reset):
    """y (T, M, out) of the recurrent network on x (T, M, D) from h (M, H); reset (T, M)."""
    pre, H, post, fn = list(model.pre_sizes), model.hidden_size, list(model.post_sizes), ACT[model.activation]
    I, off, mats = pre[-1], 0, []
    shapes = list(zip(pre[:-1], pre[1:])) + [(I + H, 2 * H), (I, H), (H, H)] + list(zip([H] + post[:-1], post))
    for a, b in shapes:
        mats.append((theta[off:off + a * b].reshape(a, b), theta[off + a * b:off + (a + 1) * b]))
        off += (a + 1) * b
    assert off == theta.numel()
    n_pre = len(pre) - 1
    ys = []
    for t in range(x.shape[0]):
        v = x[t]
        for W, b in mats[:n_pre]:
            v = fn(v @ W + b)
        h = h * (reset[t] == 0).to(h.dtype)[:, None]
        (W_rz, b_rz), (W_xn, b_xn), (W_hn, b_hn) = mats[n_pre:n_pre + 3]
        rz = torch.sigmoid(torch.cat([v, h], dim=1) @ W_rz + b_rz)
        r, z = rz[:, :H], rz[:, H:]
        n = torch.tanh(v @ W_xn + b_xn + r * (h @ W_hn + b_hn))
        h = (1.0 - z) * n + z * h
        v = h
        for i, (W, b) in enumerate(mats[n_pre + 3:]):
            v = v @ W + b
            if i != len(post) - 1:
                v = fn(v)
        ys.append(v)
    return torch.stack(ys)


def reference_minibatches(generator_state, key, B, num_minibatches, num_epochs, T, A, device):
    """[(idx (M,) int64 env indices, u (T M, A) float32)] on the host, in ``update``'s order."""
    gen = torch.Generator(device=device)
    gen.set_state(generator_state)
    key = key.clone()
    M = B // num_minibatches
    out = []
    for _ in range(num_epochs):
        perm = torch.randperm(B, device=device, generator=gen).to(torch.int32)
        for m in range(num_minibatches):
            u, key = ref._draws_and_next(key, T * M, A)
            out.append((perm[m * M:(m + 1) * M].cpu().long(), u))
    return out


def reference_grads(dtype, models, thetas, tables, roll, idx, u, entropy_cost, eps):
    """One minibatch (the envs ``idx``) at ``thetas`` (policy, value) cast to ``dtype``; ``roll`` holds
    host tensors (T, B, ...).  dict of ``grads``, ``losses``, ``rho``."""
    th = [t.detach().cpu().to(dtype).requires_grad_(True) for t in thetas]
    T, B = roll["logp"].shape
    M = idx.numel()
    x = roll["obs"][:, idx].to(dtype)  # (T, M, D)
    reset = torch.cat([torch.zeros(1, M), roll["done"][:-1, idx]])
    logits = unroll(models[0], th[0], ref.normalise(x, tables[0]), roll["hidden"][0, idx].to(dtype), reset)
    logits = logits.reshape(T * M, -1)
    values = ref.forward(models[1], th[1], ref.normalise(x, tables[1]).reshape(T * M, -1)).reshape(T * M)
    c = lambda a: a[:, idx].reshape(T * M, *a.shape[2:]).to(dtype)  # noqa: E731
    u = torch.maximum(u, torch.tensor(float(U_MIN))).to(dtype)
    total, parts, new_logp, rho = brax_loss(logits, values, c(roll["raw"]), c(roll["logp"]), c(roll["advantages"]),
                                            c(roll["vs"]), u, entropy_cost, eps)
    assert total.dtype == dtype
    total.backward()
    return dict(grads=[t.grad.numpy() for t in th], losses=torch.stack([total, *parts]).detach().numpy(),
                rho=rho.detach().numpy())


def make_roll(rng, T, B, D, A, H, policy, normalizer, noise, done_p=0.1, device="cpu"):
    """Synthetic buffers of a ``RecurrentActorRollout(..., critic=)`` replay: obs ~ N(0, 1), done on
    about ``done_p`` of the entries, hidden[0] ~ U(-1, 1) (hidden[t > 0] is not read and stays NaN), raw
    = loc + scale N(0, 1) from the float64 logits of ``policy`` as built, unrolled over the window;
    advantages ~ N(0, 1); vs ~ 3 N(0, 1); logp = the float64 log-probability of the float32 raw plus
    ``noise`` N(0, 1)."""
    obs = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32))
    done = torch.from_numpy((rng.uniform(size=(T, B)) < done_p).astype(np.float32))
    hidden = torch.full((T, B, H), float("nan"))
    hidden[0] = torch.from_numpy(rng.uniform(-1, 1, (B, H)).astype(np.float32))
    table = ref.table_of(normalizer)
    reset = torch.cat([torch.zeros(1, B), done[:-1]])
    logits = unroll(policy.model, policy.theta.detach().cpu().double(), ref.normalise(obs.double(), table),
                    hidden[0].double(), reset).reshape(T * B, 2 * A)
    loc, scale = logits[:, :A], ref._softplus(logits[:, A:]) + 0.001
    raw = (loc + scale * torch.from_numpy(rng.standard_normal((T * B, A)))).float()
    zero = torch.zeros(T * B, dtype=torch.float64)
    logp64 = brax_loss(logits, zero, raw.double(), zero, zero, zero, torch.zeros(raw.shape, dtype=torch.float64), 0.0, 0.3)[2]
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(device)  # noqa: E731
    return types.SimpleNamespace(
        obs=obs.to(device), raw=raw.reshape(T, B, A).to(device), done=done.to(device), hidden=hidden.to(device),
        logp=f((logp64.detach().numpy() + noise * rng.standard_normal(T * B)).reshape(T, B)),
        advantages=f(rng.standard_normal((T, B))), vs=f(3.0 * rng.standard_normal((T, B))))


def check_update(learner, roll, rec, metrics, tag):
    """Every recorded minibatch of the one ``update(roll)`` that followed ``learner_ref.record_steps``
    against the float64 learner: the problem's conditions (learner_ref's: no float64 rho within 1e-4 of
    a clip edge, 10 % .. 60 % of the rows outside the clip range) from float64 alone and asserted
    first; every Adam step within ulp32(theta) + 1e-6 lr of the float64 textbook Adam; storage stepped
    in place.  Returns what ``learner_ref.check_case`` takes: the gradients' and the metrics' triples
    (ours, float32, float64), held to 4 x the float32 torch error + ulp32 over the case's seeds."""
    policy, value_fn = learner.policy, learner.value_fn
    host = {k: getattr(roll, k).detach().cpu() for k in ("obs", "raw", "logp", "advantages", "vs", "hidden", "done")}
    T, B = host["logp"].shape
    A, eps, ec = policy.action_size, learner.ppo_epsilon, learner.entropy_cost
    lr = float(learner.optimizer.param_groups[0]["lr"])
    models = (policy.model, value_fn.model)
    tables = (ref.table_of(policy.normalizer), ref.table_of(value_fn.normalizer))
    batches = reference_minibatches(rec["generator_state"], rec["key"], B, learner.num_minibatches,
                                    learner.num_update_epochs, T, A, policy.theta.device)
    steps = rec["steps"]
    assert len(steps) == len(batches) == learner.num_minibatches * learner.num_update_epochs
    refs = [{dt: reference_grads(dt, models, step["before"], tables, host, idx, u, ec, eps)
             for dt in (torch.float64, torch.float32)} for step, (idx, u) in zip(steps, batches)]
    rho = np.concatenate([r[torch.float64]["rho"] for r in refs])
    near = (np.abs(rho - (1.0 - eps)) <= ref.EDGE * (1.0 - eps)) | (np.abs(rho - (1.0 + eps)) <= ref.EDGE * (1.0 + eps))
    outside = float(((rho < 1.0 - eps) | (rho > 1.0 + eps)).mean())
    print(f"{tag}: rho64 in [{rho.min():.4f}, {rho.max():.4f}], {100.0 * outside:.1f} % outside the clip range, "
          f"{int(near.sum())} rows within {ref.EDGE} of an edge")
    assert near.sum() == 0, "a row at a clip edge: take the next seed"
    assert 0.1 <= outside <= 0.6
    # ---- gradients, per network: kept for learner_ref.check_case, which takes the maxima over the case
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
    opt = ref.adam64(lr)
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
    for k, actor in enumerate((policy, value_fn)):
        assert actor.theta.data_ptr() == rec["ptrs"][k]
        assert torch.equal(actor.theta.view(torch.int32), steps[-1]["after"][k].view(torch.int32))
        assert not actor.theta.requires_grad
    assert sorted(metrics) == ["entropy_loss", "policy_loss", "total_loss", "value_loss"]
    ours = np.array([float(metrics[k]) for k in ("total_loss", "policy_loss", "value_loss", "entropy_loss")], np.float64)
    last = refs[-1]
    return dict(metrics=(ours, last[torch.float32]["losses"].astype(np.float64), last[torch.float64]["losses"]),
                grads=grads, ratios=ratios)
