"""GPU: ``RecurrentPPOLearner.update`` with a recurrent critic and the native kernels for both halves
(``backward="native"``: ``apply_sequence_native`` for the policy and for the value network, the trajectory
read in place) against the float64 learner of recurrent_critic_ref.py, on the host cases of
test_recurrent_critic_learner_host.py with the real ``RecurrentTanhPolicy``, ``RecurrentValueFunction`` and
a loaded ``ObservationNormalizer``; then one "replay, update, replay" on the env of
test_gpu_recurrent_critic.py.

Bounds and conditions are learner_ref's, unchanged.  The actor, its keys, the synthetic buffers and the
learner's key are those of test_gpu_recurrent_learner.py seed for seed, and the two halves of the loss
share nothing but the sum, so the float64 rho of every row is that test's: the first four seeds meet the
conditions there (seeds 0 .. 7 all do on the device), so none is passed over here."""
import numpy as np
import pytest
import torch

import learner_ref as ref
import recurrent_critic_ref as cref
from test_recurrent_critic_learner_host import CASES

pytestmark = pytest.mark.gpu

D, A, H = 5, 2, 7  # the actor: 5 -> GRU 7 -> 4
DEVICE = "cuda"
SEEDS = (0, 1, 2, 3)


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32).to(DEVICE)


def _actors(seed, norm, v_pre=(), v_hidden=6, v_post=(1,)):
    from po_brax_amd.training import RecurrentTanhPolicy, RecurrentValueFunction, make_recurrent_model
    p_model = make_recurrent_model([], H, [2 * A], D)
    v_model = make_recurrent_model(list(v_pre), v_hidden, list(v_post), D)
    policy = RecurrentTanhPolicy(p_model, p_model.init(_key(100 + seed)), _key(150 + seed), normalizer=norm)
    return policy, RecurrentValueFunction(v_model, v_model.init(_key(200 + seed)), normalizer=norm)


def _synthetic(seed, name):
    from po_brax_amd.training import RecurrentPPOLearner
    from test_gpu_learner import _loaded_normalizer
    T, B, minibatches, epochs, shared_norm, critic, _ = CASES[name]
    rng = np.random.default_rng(seed)
    norm = _loaded_normalizer(rng, D, 5.0, mean_sd=0.5, lo=0.5, hi=2.0) if shared_norm else None
    policy, value_fn = _actors(seed, norm, **(critic or {}))
    roll = cref.make_roll(rng, T, B, D, A, H, value_fn.hidden_size, policy, norm, 0.3, device=DEVICE)
    learner = RecurrentPPOLearner(policy, value_fn, learning_rate=3e-3, num_minibatches=minibatches,
                                  num_update_epochs=epochs, key=_key(300 + seed), backward="native")
    assert learner.backward == ("native", "native")
    rec = ref.record_steps(learner)
    metrics = learner.update(roll)
    torch.cuda.synchronize()
    return cref.check_update(learner, roll, rec, metrics, f"{name} native seed {seed}")


@pytest.mark.parametrize("name", list(CASES))
def test_update_with_the_native_kernels(name):
    ref.check_case([_synthetic(seed, name) for seed in SEEDS], f"recurrent critic {name} native")


def test_replay_update_replay():
    """Both ``theta`` storages stay in place and change, and the next replay's values differ on the same
    kind of rows: the captured graph read the critic's parameters at launch time."""
    from po_brax_amd import jumpy
    from po_brax_amd.training import RecurrentPPOLearner
    from test_gpu_recurrent_critic import B, _build
    roll, critic, _, _ = _build(True)
    policy = roll.policy
    learner = RecurrentPPOLearner(policy, critic, learning_rate=3e-3, num_minibatches=2, num_update_epochs=2,
                                  key=jumpy.random_prngkey(7))
    assert learner.backward == ("native", "native")
    ptrs = (policy.theta.data_ptr(), critic.theta.data_ptr())
    before = (policy.theta.clone(), critic.theta.clone())
    roll.replay()
    torch.cuda.synchronize()
    values = roll.values.clone()
    metrics = learner.update(roll)
    torch.cuda.synchronize()
    assert (policy.theta.data_ptr(), critic.theta.data_ptr()) == ptrs
    assert not torch.equal(policy.theta, before[0]) and not torch.equal(critic.theta, before[1])
    assert all(bool(torch.isfinite(v)) for v in metrics.values())
    assert bool(torch.isfinite(policy.theta).all()) and bool(torch.isfinite(critic.theta).all())
    # an eager critic holding the new parameters reproduces the next replay's first value row; one holding the
    # old ones does not
    h0, reset0 = critic.hidden.clone(), critic.reset.clone()
    roll.replay()
    torch.cuda.synchronize()
    assert roll.values.shape == values.shape and not torch.equal(roll.values, values)
    x0 = critic.normalizer.apply(roll.obs[0])
    for theta, same in ((critic.theta, True), (before[1], False)):
        params = type("P", (), {"theta": theta.clone()})
        y, _ = critic.model.apply(params, x0, h0, reset0)
        assert torch.equal(y.reshape(B), roll.values[0]) == same
