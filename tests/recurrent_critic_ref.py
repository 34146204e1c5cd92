"""An independent float64 learner to hold ``RecurrentPPOLearner.update`` with a RECURRENT critic against
(a helper of test_recurrent_critic_learner_host.py and test_gpu_recurrent_critic_learner.py: no tests
here).  recurrent_learner_ref.py with the value half changed: the value network is unrolled over the
minibatch's windows too (``recurrent_learner_ref.unroll``, the formulas written out there), from
``roll.value_hidden0`` with the policy's reset rows, and its (T, M, 1) output read as the loss's T M rows.
The recorder, the minibatch redraw, the Adam check, the problem's conditions and the bounds are
learner_ref's and recurrent_learner_ref's, unchanged."""
import numpy as np
import torch

import learner_ref as ref
import recurrent_learner_ref as rref
from test_ppo_host import U_MIN, brax_loss, ulp32

KEYS = ("obs", "raw", "logp", "advantages", "vs", "hidden", "done", "value_hidden0")


def reference_grads(dtype, models, thetas, tables, roll, idx, u, entropy_cost, eps):
    """One minibatch (the envs ``idx``) at ``thetas`` (policy, value) cast to ``dtype``; ``roll`` holds host
    tensors.  dict of ``grads``, ``losses``, ``rho``."""
    th = [t.detach().cpu().to(dtype).requires_grad_(True) for t in thetas]
    T, B = roll["logp"].shape
    M = idx.numel()
    x = roll["obs"][:, idx].to(dtype)  # (T, M, D)
    reset = torch.cat([torch.zeros(1, M), roll["done"][:-1, idx]])
    logits = rref.unroll(models[0], th[0], ref.normalise(x, tables[0]), roll["hidden"][0, idx].to(dtype), reset)
    logits = logits.reshape(T * M, -1)
    values = rref.unroll(models[1], th[1], ref.normalise(x, tables[1]), roll["value_hidden0"][idx].to(dtype), reset)
    assert values.shape == (T, M, 1)
    values = values.reshape(T * M)
    c = lambda a: a[:, idx].reshape(T * M, *a.shape[2:]).to(dtype)  # noqa: E731
    u = torch.maximum(u, torch.tensor(float(U_MIN))).to(dtype)
    total, parts, new_logp, rho = brax_loss(logits, values, c(roll["raw"]), c(roll["logp"]), c(roll["advantages"]),
                                            c(roll["vs"]), u, entropy_cost, eps)
    assert total.dtype == dtype
    total.backward()
    return dict(grads=[t.grad.numpy() for t in th], losses=torch.stack([total, *parts]).detach().numpy(),
                rho=rho.detach().numpy())


def make_roll(rng, T, B, D, A, H, Hv, policy, normalizer, noise, done_p=0.1, device="cpu"):
    """``recurrent_learner_ref.make_roll`` plus ``value_hidden0`` (B, Hv) ~ U(-1, 1), zero exactly where the
    replay before this one ended an episode (about ``done_p`` of the envs), as the critic's kernel leaves
    it."""
    roll = rref.make_roll(rng, T, B, D, A, H, policy, normalizer, noise, done_p, device)
    h = rng.uniform(-1, 1, (B, Hv)).astype(np.float32)
    h[rng.uniform(size=B) < done_p] = 0.0
    roll.value_hidden0 = torch.from_numpy(h).to(device)
    return roll


def check_update(learner, roll, rec, metrics, tag):
    """``recurrent_learner_ref.check_update`` with the recurrent value half: the conditions from float64
    alone and asserted first, every Adam step within ulp32(theta) + 1e-6 lr of the float64 textbook
    Adam, storage stepped in place; returns what ``learner_ref.check_case`` takes."""
    policy, value_fn = learner.policy, learner.value_fn
    host = {k: getattr(roll, k).detach().cpu() for k in KEYS}
    T, B = host["logp"].shape
    A, eps, ec = policy.action_size, learner.ppo_epsilon, learner.entropy_cost
    lr = float(learner.optimizer.param_groups[0]["lr"])
    models = (policy.model, value_fn.model)
    tables = (ref.table_of(policy.normalizer), ref.table_of(value_fn.normalizer))
    batches = rref.reference_minibatches(rec["generator_state"], rec["key"], B, learner.num_minibatches,
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
