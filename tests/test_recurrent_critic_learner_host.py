"""CPU: ``RecurrentPPOLearner.update`` with a recurrent critic on host tensors (``backward="torch"``: the
device's wiring, every kernel replaced by its torch-op spelling) against the independent float64
learner of recurrent_critic_ref.py, which unrolls BOTH networks over the minibatch's windows -- the
value network from ``roll.value_hidden0``.

Bounds and conditions are learner_ref's, unchanged: both ``theta.grad`` within 4 x the all-torch
float32 error against float64 plus one ulp32, maxima over the case's seeds (``check_case``); every Adam
step within ulp32(theta) + 1e-6 lr of a float64 textbook Adam; storage stepped in place; no float64 rho
within 1e-4 of a clip edge and 10 % .. 60 % of the rows outside the clip range, from float64 alone and
asserted first.

The policy and the critic are stubs (the native objects need a GPU); the normaliser is
test_learner_host's stub.  Four seeds a case from the first six.  Seeds passed over, each because it
puts a row's float64 rho within 1e-4 of a clip edge: seed 3 of the shared-normaliser case, seed 2 of
the case without a normaliser, and seed 3 of the case with a pre-MLP and a two-layer post-MLP."""
import numpy as np
import torch

import learner_ref as ref
import recurrent_critic_ref as cref
from test_learner_host import StubNormalizer

D, A, H = 5, 2, 7  # the actor: 5 -> GRU 7 -> 4


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32)


def stub_actors(seed, norm, v_pre=(), v_hidden=6, v_post=(1,), device="cpu"):
    from po_brax_amd.training import RecurrentTanhPolicy, RecurrentValueFunction, make_recurrent_model
    policy = RecurrentTanhPolicy.__new__(RecurrentTanhPolicy)  # the native actor needs a GPU: only what the learner reads
    model = make_recurrent_model([], H, [2 * A], D)
    policy.model, policy.params = model, model.init(_key(100 + seed).to(device))
    policy.theta, policy.obs_size, policy.action_size = policy.params.theta, D, A
    policy.hidden_size, policy.normalizer = H, norm
    value_fn = RecurrentValueFunction.__new__(RecurrentValueFunction)
    vmodel = make_recurrent_model(list(v_pre), v_hidden, list(v_post), D)
    value_fn.model, value_fn.params = vmodel, vmodel.init(_key(200 + seed).to(device))
    value_fn.theta, value_fn.obs_size, value_fn.hidden_size = value_fn.params.theta, D, v_hidden
    value_fn.normalizer = norm
    return policy, value_fn


def one_update(seed, T, B, minibatches, epochs, shared_norm, tag, critic=None, lr=3e-3, noise=0.3, backward="torch",
               device="cpu", normalizer=None):
    from po_brax_amd.training import RecurrentPPOLearner
    rng = np.random.default_rng(seed)
    norm = (normalizer or StubNormalizer)(rng, D) if shared_norm else None
    policy, value_fn = stub_actors(seed, norm, device=device, **(critic or {}))
    roll = cref.make_roll(rng, T, B, D, A, H, value_fn.hidden_size, policy, norm, noise, device=device)
    assert 0 < float(roll.done[:-1].mean()) < 0.3
    learner = RecurrentPPOLearner(policy, value_fn, learning_rate=lr, num_minibatches=minibatches, num_update_epochs=epochs,
                                  key=_key(300 + seed).to(device), backward=backward)
    rec = ref.record_steps(learner)
    metrics = learner.update(roll)
    return cref.check_update(learner, roll, rec, metrics, f"{tag} seed {seed}")


PRE_POST = dict(v_pre=(6,), v_hidden=7, v_post=(4, 1))
CASES = {  # name: (T, B, minibatches, epochs, shared normaliser, critic, seeds)
    "shared": (8, 32, 4, 2, True, None, (0, 1, 2, 4)),
    "plain": (3, 12, 3, 1, False, None, (0, 1, 3, 4)),
    "pre-post": (8, 32, 4, 2, True, PRE_POST, (0, 1, 2, 4)),
}


def run_case(name, **kw):
    T, B, mb, ep, shared, critic, seeds = CASES[name]
    return ref.check_case([one_update(s, T, B, mb, ep, shared, name, critic, **kw) for s in seeds],
                          f"recurrent critic, {name}")


def test_update_with_a_shared_normaliser():
    """5 -> GRU 7 -> 4 actor, 5 -> GRU 6 -> 1 critic, T x B = 8 x 32 in 4 minibatches of 8 envs x 2 epochs, lr
    3e-3, one normaliser for both networks, behaviour log-probabilities off by N(0, 0.3^2)."""
    run_case("shared")


def test_update_without_a_normaliser():
    """T x B = 3 x 12 in 3 minibatches of 4 envs, one epoch."""
    run_case("plain")


def test_update_with_a_pre_mlp_and_a_two_layer_post_mlp():
    """The critic [5 -> 6] -> GRU 7 -> [4 -> 1]: the window's gradient reaches the layers on both sides of
    the cell."""
    run_case("pre-post")


def test_the_value_half_reads_value_hidden0():
    """Another ``value_hidden0`` changes the value network's gradient and leaves the policy's alone (the
    loss couples the two halves only through the sum)."""
    from po_brax_amd.training import RecurrentPPOLearner
    grads = []
    for flip in (False, True):
        rng = np.random.default_rng(0)
        policy, value_fn = stub_actors(0, None)
        roll = cref.make_roll(rng, 3, 12, D, A, H, value_fn.hidden_size, policy, None, 0.3)
        if flip:
            roll.value_hidden0 = -roll.value_hidden0
        learner = RecurrentPPOLearner(policy, value_fn, num_minibatches=1, num_update_epochs=1, key=_key(300), backward="torch")
        rec = ref.record_steps(learner)
        learner.update(roll)
        grads.append(rec["steps"][0]["grad"])
    assert torch.equal(grads[0][0], grads[1][0]) and not torch.equal(grads[0][1], grads[1][1])
