"""GPU: ``PPOLearner.update`` on the device against the independent float64 learner of learner_ref.py,
for ``backward`` in "torch", "native" and ("native", "torch"), with the real ``NormalTanhPolicy``,
``ValueFunction`` and ``ObservationNormalizer`` (its table loaded with a random mean and scale).

For every minibatch of one update: both ``theta.grad`` within test_ppo_host.py's bound of float64
autograd through gather, normaliser, both networks and brax's loss at the recorded parameters; every
Adam step within ulp32(theta) + 1e-6 lr of a float64 textbook Adam; the actors' storage stepped in
place; the metrics the last minibatch's; and ``apply_native`` called exactly by the networks that
were asked to.  Then the ratio at the acting parameters (the actor kernel's log-probability against
the loss's spelling of the same rows) and descent on a fixed batch.  Bounds, conditions and the
measured ratios: DESIGN.md "Learner against a float64 learner"."""
import functools

import numpy as np
import pytest
import torch

import learner_ref as ref

pytestmark = pytest.mark.gpu

BACKWARDS = ["torch", "native", ("native", "torch")]
IDS = ["torch", "native", "native-torch"]
D, A, HIDDEN = 35, 3, [33]  # 33: one past the 32-row / 32-column MFMA tile
B_ROLL, T_ROLL = 64, 4
DEVICE = "cuda"
# The synthetic cases' table: means 0.2 N(0, 1), scales in [0.1, 0.3], clamp at 0.5 (live for entries
# 1.7 .. 5 from the mean).  With the host test's table (scales up to 2, clamp 5) the 35-wide rows give
# logits of order 1, scale = softplus(p) + 0.001 down to 0.05, and three Adam steps at lr 3e-4 move the
# float64 rho of the 4 x 1028 on-policy rows to [0.06, 2.5] (host path, seeds 0 .. 3); with this one it
# stays in [0.96, 1.04] on the device.
TABLE, CLIP = dict(mean_sd=0.2, lo=0.1, hi=0.3), 0.5
LIVE_SEEDS = (0, 1, 3, 4)


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32).to(DEVICE)


def _loaded_normalizer(rng, width, clip=CLIP, **table):
    """An ``ObservationNormalizer`` whose table is loaded with a random mean and scale."""
    from po_brax_amd.training.normalization import ObservationNormalizer
    norm = ObservationNormalizer(width)
    mean, scale = ref.random_table(rng, width, **(table or TABLE))
    norm.load_state_dict({"table": torch.from_numpy(np.stack([mean, scale, np.ones_like(mean)])),
                          "count": torch.tensor([1000.0], dtype=torch.float64), "clip": clip})
    return norm


def _actors(seed, norm):
    from po_brax_amd.training import NormalTanhPolicy, ValueFunction, make_model
    p_model, v_model = make_model(HIDDEN + [2 * A], D), make_model(HIDDEN + [1], D)
    policy = NormalTanhPolicy(p_model, p_model.init(_key(100 + seed)), _key(150 + seed), normalizer=norm)
    return policy, ValueFunction(v_model, v_model.init(_key(200 + seed)), normalizer=norm)


def _recorded_update(learner, roll, case, tag):
    """One ``update`` under ``record_steps`` with both models' ``apply_native`` wrapped; the check of
    learner_ref, and which path ran."""
    from test_gpu_mlp_bwd import _Recorder
    p_rec, v_rec = _Recorder(learner.policy.model), _Recorder(learner.value_fn.model)
    rec = ref.record_steps(learner)
    metrics = learner.update(roll)
    torch.cuda.synchronize()
    n = learner.num_minibatches * learner.num_update_epochs
    for calls, how in ((p_rec.calls, learner.backward[0]), (v_rec.calls, learner.backward[1])):
        assert len(calls) == (n if how == "native" else 0) and all(c["with_grad"] for c in calls)
    return ref.check_update(learner, roll, rec, metrics, case, tag)


def _synthetic(backward, seed, T, B, minibatches, epochs, lr, noise, case, tag):
    from po_brax_amd.training import PPOLearner
    rng = np.random.default_rng(seed)
    norm = _loaded_normalizer(rng, D)
    policy, value_fn = _actors(seed, norm)
    roll = ref.make_roll(rng, T, B, D, A, policy, norm, noise, DEVICE)
    learner = PPOLearner(policy, value_fn, learning_rate=lr, num_minibatches=minibatches, num_update_epochs=epochs,
                         key=_key(300 + seed), backward=backward)
    return _recorded_update(learner, roll, case, f"{tag} {backward} seed {seed}")


@pytest.mark.parametrize("backward", BACKWARDS, ids=IDS)
def test_update_with_clipping_live(backward):
    """T x B = 3 x 33 in 3 minibatches of M = 33 rows (one row past the 32-row tile), 2 epochs, lr 3e-3,
    behaviour log-probabilities off by N(0, 0.3^2).  Seed 2 is passed over: on the device it puts one
    row's float64 rho within 1e-4 of a clip edge."""
    ref.check_case([_synthetic(backward, seed, 3, 33, 3, 2, 3e-3, 0.3, "live", "live") for seed in LIVE_SEEDS],
                   f"live {backward}")


@pytest.mark.parametrize("backward", BACKWARDS, ids=IDS)
def test_update_on_policy_across_the_chunk(backward):
    """T x B = 4 x 1028 in 4 minibatches of M = 1028 = 1024 + 4 rows, one epoch, lr 3e-4, exact behaviour
    log-probabilities: crosses the 1024-row chunks of ``k_ppo_loss`` and of the weight-gradient kernel."""
    ref.check_case([_synthetic(backward, seed, 4, 1028, 4, 1, 3e-4, 0.0, "on-policy", "chunk") for seed in range(4)],
                   f"chunk {backward}")


# ---------------------------------------------------------------------------- the real rollout
def real_rollout(seed, update_normalizer, loaded, clip=CLIP, **table):
    """ant_heavenhell, B = 64, T = 4, the ``make_models`` pair with ``init`` as drawn, one normaliser for
    actor and critic: (roll, policy, critic) before any replay."""
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import ValueFunction, networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    from test_gpu_parity import _keys
    env = envs.create("ant_heavenhell", batch_size=B_ROLL, episode_length=3)
    state = env.reset(torch.from_numpy(_keys(B_ROLL, 3 + seed)).cuda())
    width = env.observation_size
    norm = (_loaded_normalizer(np.random.default_rng(50 + seed), width, clip, **table) if loaded
            else ObservationNormalizer(width))
    p_model, v_model = networks.make_models(2 * env.action_size, width)
    policy = networks.NormalTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5 + 10 * seed)),
                                       jumpy.random_prngkey(6 + 10 * seed), normalizer=norm)
    critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9 + 10 * seed)), normalizer=norm)
    return ActorRollout(env, state, policy, T_ROLL, update_normalizer=update_normalizer, critic=critic), policy, critic


# The on-policy rollout: the table is loaded and the replay leaves it alone.  With update_normalizer=True
# on a fresh normaliser the replay acts under the identity table and the learner reads the updated one:
# measured float64 rho in [0.10, 2.51] (seed 0) and [0.26, 3.33] (seed 1), 16 % .. 18 % of the rows
# outside the clip range: not on-policy, so that configuration runs as a "clipping live" case below.
REAL = dict(update_normalizer=False, loaded=True)
UPDATED = dict(update_normalizer=True, loaded=False)
UPDATED_SEEDS = (0, 1, 2, 3)


def real_update(backward, seed, config=None, case="on-policy"):
    from po_brax_amd import jumpy
    from po_brax_amd.training import PPOLearner
    roll, policy, critic = real_rollout(seed, **(REAL if config is None else config))
    learner = PPOLearner(policy, critic, learning_rate=3e-4, num_minibatches=4, num_update_epochs=1,
                         key=jumpy.random_prngkey(7 + 10 * seed), backward=backward)
    roll.replay()
    torch.cuda.synchronize()
    # the reference reads the normaliser's table as it stands after the replay
    return _recorded_update(learner, roll, case, f"rollout {backward} seed {seed}")


@pytest.mark.parametrize("backward", BACKWARDS, ids=IDS)
def test_update_on_a_real_rollout(backward):
    """One replay of ``ActorRollout(..., critic=)``, then one update of 4 minibatches x 1 epoch at lr 3e-4."""
    ref.check_case([real_update(backward, seed) for seed in range(4)], f"rollout {backward}")


@pytest.mark.parametrize("backward", BACKWARDS, ids=IDS)
def test_update_after_the_replay_updated_the_normaliser(backward):
    """The same with ``update_normalizer=True`` on a fresh normaliser: the learner and the reference read
    the table the replay LEFT, the actor acted under the one it found, so the clipping is live."""
    ref.check_case([real_update(backward, seed, UPDATED, "live") for seed in UPDATED_SEEDS],
                   f"updated table {backward}")


# ---------------------------------------------------------------------------- the ratio at the acting parameters
@functools.lru_cache(maxsize=None)
def _acted():
    """One replay with the normaliser loaded and not updated: the host buffers, the actor's logp, the
    loss's spelling of the same log-probability in float64 and float32, and the per-row bound."""
    roll, policy, _ = real_rollout(0, update_normalizer=False, loaded=True)
    roll.replay()
    torch.cuda.synchronize()
    b = ref.host_buffers(roll)
    table = ref.table_of(policy.normalizer)
    L64, loc, scale = ref.policy_logp(policy.model, policy.theta, table, b["obs"], b["raw"], torch.float64)
    L32 = ref.policy_logp(policy.model, policy.theta, table, b["obs"], b["raw"], torch.float32)[0]
    bound = ref.logp_bound(b["raw"].numpy(), L64.numpy(), L32.numpy(), loc.numpy(), scale.numpy())
    return roll, policy, b, L64.numpy(), bound, float(scale.min())


def test_actor_logp_against_the_loss_spelling():
    """Per row, rows with |raw| > 4 included: |roll.logp - L64| <= R_row + 4 max |L32 - L64| + ulp32(max |L64|)
    (learner_ref.logp_bound): the actor makes its term from eps, the loss from the stored float32 raw."""
    _, _, b, L64, bound, min_scale = _acted()
    err = np.abs(b["logp"].numpy().astype(np.float64) - L64)
    print(f"actor logp against the loss's float64 spelling: max error {err.max():.3e}, largest ratio to the row's bound "
          f"{(err / bound).max():.2f}, min scale {min_scale:.4f}, max |raw| {float(b['raw'].abs().max()):.2f}, "
          f"{100.0 * (err > 1e-3).mean():.2f} % of the rows off by more than 1e-3")
    assert np.isfinite(err).all() and (err <= bound).all()


def test_ratio_is_one_through_ppo_loss():
    """``ppo_loss`` of the whole batch at the acting parameters with positive advantages and no entropy
    term: policy_loss = -mean(rho adv) with every rho = 1 up to the same per-row bound."""
    from po_brax_amd.training import ppo_loss
    roll, policy, b, _, bound, _ = _acted()
    N = b["logp"].numel()
    rows = policy.normalizer.apply(roll.obs.reshape(N, -1))
    with torch.no_grad():
        logits = policy.model.apply(policy.params, rows)
    adv = torch.from_numpy(np.random.default_rng(0).uniform(0.5, 1.5, N).astype(np.float32)).cuda()
    zero = torch.zeros(N, device="cuda")
    _, metrics = ppo_loss(logits, zero, roll.raw.reshape(N, -1), roll.logp.reshape(N), adv, zero, _key(1),
                          entropy_cost=0.0)
    a64 = adv.double().cpu().numpy()
    got, want, tol = float(metrics["policy_loss"]), -a64.mean(), float((bound * a64).sum() / N)
    print(f"policy_loss {got:.9f} against -mean(adv) {want:.9f}: off by {abs(got - want):.3e}, bound {tol:.3e}, "
          f"ratio {abs(got - want) / tol:.2f}")
    assert abs(got - want) <= tol


# ---------------------------------------------------------------------------- descent
@pytest.mark.parametrize("backward", BACKWARDS, ids=IDS)
def test_descent_on_a_fixed_batch(backward):
    """Ten updates on one synthetic batch of T x B = 8 x 33 (minibatches of 66 rows): the float64 value
    loss falls to half or less, the float64 clipped surrogate loss falls."""
    from test_learner_host import descent
    for seed in range(2):
        norm = _loaded_normalizer(np.random.default_rng(1000 + seed), D)
        policy, value_fn = _actors(seed, norm)
        (p0, v0), (p1, v1) = descent(policy, value_fn, norm, seed, 8, 33, backward, DEVICE)
        assert v1 <= 0.5 * v0
        assert p1 < p0
