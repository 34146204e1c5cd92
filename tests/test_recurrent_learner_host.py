"""CPU: ``RecurrentPPOLearner.update`` on host tensors (``backward="torch"``: the same wiring as on the
device, every kernel replaced by its torch-op spelling) against the independent float64 learner of
recurrent_learner_ref.py.

For every minibatch of one update: both ``theta.grad`` within test_ppo_host.py's bound (4 x the
all-torch float32 error against float64, plus one ulp32) of float64 autograd through the gather, the
normaliser, the unrolled recurrent network, the value network and brax's loss at the recorded
parameters; every Adam step within ulp32(theta) + 1e-6 lr of a float64 textbook Adam fed the recorded
gradients; the actors' own storage stepped in place; the returned metrics the last minibatch's.  The
conditions on the problem (no row at a clip edge, 10 % .. 60 % of the rows outside the clip range)
come from the float64 reference alone.  ``done`` is set on about a tenth of the entries, so resets
fall inside the windows.

The policy and value objects are stubs (the native actors need a GPU); the normaliser is
test_learner_host's stub.  Seeds passed over, each because it puts one row's float64 rho within 1e-4
of a clip edge: seed 3 of the shared-normaliser case and seed 2 of the case without one."""
import numpy as np
import torch

import learner_ref as ref
import recurrent_learner_ref as rref
from test_learner_host import StubNormalizer

D, A, H = 5, 2, 7  # 5 -> GRU 7 -> 4


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32)


def stub_actors(seed, p_norm, v_norm, pre=(), post=None, device="cpu"):
    from po_brax_amd.training import RecurrentTanhPolicy, ValueFunction, make_model, make_recurrent_model
    policy = RecurrentTanhPolicy.__new__(RecurrentTanhPolicy)  # the native actor needs a GPU: only what the learner reads
    model = make_recurrent_model(list(pre), H, [2 * A] if post is None else post, D)
    policy.model, policy.params = model, model.init(_key(100 + seed).to(device))
    policy.theta, policy.obs_size, policy.action_size = policy.params.theta, D, A
    policy.hidden_size, policy.normalizer = H, p_norm
    value_fn = ValueFunction.__new__(ValueFunction)
    vmodel = make_model([7, 1], D)
    value_fn.model, value_fn.params = vmodel, vmodel.init(_key(200 + seed).to(device))
    value_fn.theta, value_fn.obs_size, value_fn.normalizer = value_fn.params.theta, D, v_norm
    return policy, value_fn


def _one_update(seed, T, B, minibatches, epochs, shared_norm, tag, pre=(), lr=3e-3, noise=0.3):
    from po_brax_amd.training import RecurrentPPOLearner
    rng = np.random.default_rng(seed)
    norm = StubNormalizer(rng, D) if shared_norm else None
    policy, value_fn = stub_actors(seed, norm, norm, pre)
    roll = rref.make_roll(rng, T, B, D, A, H, policy, norm, noise)
    assert 0 < float(roll.done[:-1].mean()) < 0.3
    learner = RecurrentPPOLearner(policy, value_fn, learning_rate=lr, num_minibatches=minibatches, num_update_epochs=epochs,
                                  key=_key(300 + seed), backward="torch")
    rec = ref.record_steps(learner)
    metrics = learner.update(roll)
    return rref.check_update(learner, roll, rec, metrics, f"{tag} seed {seed}")


def test_update_with_a_shared_normaliser():
    """5 -> GRU 7 -> 4, T x B = 8 x 32 in 4 minibatches of 8 envs x 2 epochs, lr 3e-3, one normaliser for
    both networks, behaviour log-probabilities off by N(0, 0.3^2)."""
    ref.check_case([_one_update(seed, 8, 32, 4, 2, True, "shared") for seed in (0, 1, 2, 4)], "recurrent, shared")


def test_update_without_a_normaliser():
    """T x B = 3 x 12 in 3 minibatches of 4 envs, one epoch."""
    ref.check_case([_one_update(seed, 3, 12, 3, 1, False, "plain") for seed in (0, 1, 3, 4)], "recurrent, plain")


def test_update_with_a_pre_mlp():
    """[5 -> 6] -> GRU 7 -> 4: the window's gradient reaches the layers in front of the cell."""
    ref.check_case([_one_update(seed, 8, 32, 4, 2, True, "pre-MLP", pre=(6,)) for seed in range(4)], "recurrent, pre-MLP")
