"""CPU: ``PPOLearner.update`` on host tensors (``backward="torch"``: the same wiring as on the device,
every kernel replaced by its torch-op spelling) against the independent float64 learner of
learner_ref.py.

For every minibatch of one update: both ``theta.grad`` within test_ppo_host.py's bound (4 x the
all-torch float32 error against float64, plus one ulp32) of float64 autograd through gather,
normaliser, both networks and brax's loss at the recorded parameters; every Adam step within
ulp32(theta) + 1e-6 lr of a float64 textbook Adam fed the recorded gradients; the actors' own storage
stepped in place; the returned metrics the last minibatch's.  The conditions on the problem (no row
at a clip edge, 10 % .. 60 % of the rows outside the clip range) come from the float64 reference
alone.  Inputs are unit scale and ``init`` is not multiplied: DESIGN.md "Learner against a float64
learner" says why, and holds the measured ratios.

The policy and value objects are the stubs of test_ppo_api.test_learner_checks (the native actors need
a GPU); the normaliser is a stub with ``mean``, ``scale``, ``clip`` and ``apply``."""
import numpy as np
import pytest
import torch

import learner_ref as ref

D, A, HIDDEN = 5, 2, [7]


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32)


class StubNormalizer:
    """What the learner and the reference read of an ``ObservationNormalizer``; ``apply`` in its ops.
    Means of 0.5 N(0, 1) and scales in [0.5, 2] put some unit-scale entries past the clamp."""

    def __init__(self, rng, width, clip=5.0, **table):
        self.mean, self.scale = map(torch.from_numpy, ref.random_table(rng, width, **table))
        self.clip = clip

    def apply(self, obs):
        return torch.clamp((obs - self.mean) * self.scale, -self.clip, self.clip)


def stub_actors(seed, p_norm, v_norm, d=D, a=A, hidden=HIDDEN):
    from po_brax_amd.training import NormalTanhPolicy, ValueFunction, make_model
    policy = NormalTanhPolicy.__new__(NormalTanhPolicy)  # the native actor needs a GPU: only what the learner reads
    model = make_model(hidden + [2 * a], d)
    policy.model, policy.params = model, model.init(_key(100 + seed))
    policy.theta, policy.obs_size, policy.action_size, policy.normalizer = policy.params.theta, d, a, p_norm
    value_fn = ValueFunction.__new__(ValueFunction)
    vmodel = make_model(hidden + [1], d)
    value_fn.model, value_fn.params = vmodel, vmodel.init(_key(200 + seed))
    value_fn.theta, value_fn.obs_size, value_fn.normalizer = value_fn.params.theta, d, v_norm
    return policy, value_fn


def _one_update(seed, T, B, minibatches, epochs, norms, tag, lr=3e-3, noise=0.3, case="live"):
    from po_brax_amd.training import PPOLearner
    rng = np.random.default_rng(seed)
    if norms == "shared":
        p_norm = v_norm = StubNormalizer(rng, D)
    else:
        p_norm = StubNormalizer(rng, D) if norms in ("policy", "both") else None
        v_norm = StubNormalizer(rng, D) if norms in ("value", "both") else None
    policy, value_fn = stub_actors(seed, p_norm, v_norm)
    roll = ref.make_roll(rng, T, B, D, A, policy, p_norm, noise)
    learner = PPOLearner(policy, value_fn, learning_rate=lr, num_minibatches=minibatches, num_update_epochs=epochs,
                         key=_key(300 + seed))
    rec = ref.record_steps(learner)
    metrics = learner.update(roll)
    return ref.check_update(learner, roll, rec, metrics, case, f"{tag} seed {seed}")


def test_update_with_clipping_live():
    """D 5, A 2, hidden [7], T x B = 8 x 32, 4 minibatches x 2 epochs, lr 3e-3, one normaliser for both
    networks, behaviour log-probabilities off by N(0, 0.3^2)."""
    ref.check_case([_one_update(seed, 8, 32, 4, 2, "shared", "live") for seed in range(4)], "live")


def test_update_without_a_normaliser():
    """T x B = 3 x 11 in 3 minibatches of M = 11 rows, one epoch."""
    ref.check_case([_one_update(seed, 3, 11, 3, 1, None, "no normaliser") for seed in range(4)],
                   "no normaliser")


@pytest.mark.parametrize("norms,seeds", [("policy", (1, 2, 3, 4)), ("value", (0, 1, 2, 3)), ("both", (0, 1, 2, 3))],
                         ids=["policy", "value", "both"])
def test_update_with_separate_normalisers(norms, seeds):
    """``v_norm is not norm``: only the policy's rows normalised, only the value network's, or each
    network with a table of its own.  T x B = 4 x 16, 2 minibatches x 2 epochs.  "policy" starts at
    seed 1: seed 0 puts one row's float64 rho within 1e-4 of a clip edge."""
    ref.check_case([_one_update(seed, 4, 16, 2, 2, norms, f"normalised: {norms}") for seed in seeds],
                   f"normalised: {norms}")


def descent(policy, value_fn, norm, seed, T, B, backward="torch", device="cpu"):
    """Ten updates (4 minibatches x 4 epochs, lr 3e-3) on one synthetic batch with vs = obs . w and
    on-policy logp: (value loss, policy loss) of the whole batch in float64, before and after."""
    from po_brax_amd.training import PPOLearner
    rng = np.random.default_rng(seed)
    d, a = policy.obs_size, policy.action_size
    roll = ref.make_roll(rng, T, B, d, a, policy, norm, 0.0, device)
    w = torch.from_numpy(rng.standard_normal(d).astype(np.float32)).to(device)
    roll.vs = (roll.obs @ w).contiguous()
    learner = PPOLearner(policy, value_fn, learning_rate=3e-3, num_minibatches=4, num_update_epochs=4,
                         key=_key(300 + seed).to(device), backward=backward)
    p0, v0 = ref.full_batch_losses(learner, roll)
    for _ in range(10):
        learner.update(roll)
    p1, v1 = ref.full_batch_losses(learner, roll)
    print(f"descent seed {seed} backward {backward}: value loss {v0:.4f} -> {v1:.4f} ({v1 / v0:.3f} of the start), "
          f"clipped surrogate loss {p0:+.4f} -> {p1:+.4f}")
    return (p0, v0), (p1, v1)


@pytest.mark.parametrize("seed", range(4))
def test_descent_on_a_fixed_batch(seed):
    norm = StubNormalizer(np.random.default_rng(1000 + seed), D)
    policy, value_fn = stub_actors(seed, norm, norm)
    (p0, v0), (p1, v1) = descent(policy, value_fn, norm, seed, 8, 32)
    assert v1 <= 0.5 * v0
    assert p1 < p0
