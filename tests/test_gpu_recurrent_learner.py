"""GPU: ``RecurrentPPOLearner.update`` on the device against the independent float64 learner of
recurrent_learner_ref.py, for ``backward`` in "native" and ("native", "torch") (and "torch", the
torch ops on device tensors), with the real ``RecurrentTanhPolicy``, ``ValueFunction`` and
``ObservationNormalizer`` (its table loaded with a random mean and scale); then "replay, learn,
replay" on a real ``RecurrentActorRollout``.

For every minibatch of one update: both ``theta.grad`` within test_ppo_host.py's bound of float64
autograd through the gather, the normaliser, the unrolled network, the value network and brax's loss
at the recorded parameters; every Adam step within ulp32(theta) + 1e-6 lr of a float64 textbook Adam;
the actors' storage stepped in place; the metrics the last minibatch's.  The problem's conditions are
learner_ref.py's and come from the float64 reference alone; the permutation is the device
generator's, so the seeds are chosen on the device: see SEEDS."""
import types

import numpy as np
import pytest
import torch

import learner_ref as ref
import recurrent_learner_ref as rref

pytestmark = pytest.mark.gpu

BACKWARDS = ["torch", "native", ("native", "torch")]
IDS = ["torch", "native", "native-torch"]
D, A, H = 5, 2, 7  # 5 -> GRU 7 -> 4
DEVICE = "cuda"
# Per case the first four seeds of 0, 1, 2, .. that meet the conditions for every ``backward``: on the
# device seeds 0 .. 7 all do, so none is passed over.
SEEDS = {"shared": (0, 1, 2, 3), "plain": (0, 1, 2, 3)}


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32).to(DEVICE)


def _actors(seed, norm):
    from po_brax_amd.training import RecurrentTanhPolicy, ValueFunction, make_model, make_recurrent_model
    p_model, v_model = make_recurrent_model([], H, [2 * A], D), make_model([7, 1], D)
    policy = RecurrentTanhPolicy(p_model, p_model.init(_key(100 + seed)), _key(150 + seed), normalizer=norm)
    return policy, ValueFunction(v_model, v_model.init(_key(200 + seed)), normalizer=norm)


def _synthetic(backward, seed, T, B, minibatches, epochs, shared_norm, tag):
    from po_brax_amd.training import RecurrentPPOLearner
    from test_gpu_learner import _loaded_normalizer
    rng = np.random.default_rng(seed)
    norm = _loaded_normalizer(rng, D, 5.0, mean_sd=0.5, lo=0.5, hi=2.0) if shared_norm else None
    policy, value_fn = _actors(seed, norm)
    roll = rref.make_roll(rng, T, B, D, A, H, policy, norm, 0.3, device=DEVICE)
    learner = RecurrentPPOLearner(policy, value_fn, learning_rate=3e-3, num_minibatches=minibatches,
                                  num_update_epochs=epochs, key=_key(300 + seed), backward=backward)
    rec = ref.record_steps(learner)
    metrics = learner.update(roll)
    torch.cuda.synchronize()
    return rref.check_update(learner, roll, rec, metrics, f"{tag} {backward} seed {seed}")


@pytest.mark.parametrize("backward", BACKWARDS, ids=IDS)
def test_update_with_a_shared_normaliser(backward):
    """T x B = 8 x 32 in 4 minibatches of 8 envs x 2 epochs, lr 3e-3, one loaded normaliser for both
    networks, ``done`` on about a tenth of the entries."""
    ref.check_case([_synthetic(backward, seed, 8, 32, 4, 2, True, "shared") for seed in SEEDS["shared"]],
                   f"recurrent shared {backward}")


@pytest.mark.parametrize("backward", BACKWARDS, ids=IDS)
def test_update_without_a_normaliser(backward):
    """T x B = 3 x 12 in 3 minibatches of 4 envs, one epoch."""
    ref.check_case([_synthetic(backward, seed, 3, 12, 3, 1, False, "plain") for seed in SEEDS["plain"]],
                   f"recurrent plain {backward}")


# ---------------------------------------------------------------------------- replay, learn, replay
def _loop(backward, masked, rounds=2):
    """ant_heavenhell, B = 64, T = 8, episodes of 3 steps: ``rounds`` of replay(); update(roll).  Returns
    what a second run from the same keys has to reproduce bit for bit."""
    from po_brax_amd import envs, jumpy
    from po_brax_amd import standard_observability_masks as masks
    from po_brax_amd.rollout import RecurrentActorRollout
    from po_brax_amd.training import RecurrentPPOLearner, ValueFunction, networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    from test_gpu_parity import _keys
    B, T = 64, 8
    name = "ant_heavenhell"
    kw = dict(obs_mask=masks.po_env_mask(name, cfrc=False)) if masked else {}
    env = envs.create(name, batch_size=B, episode_length=3, **kw)
    state = env.reset(torch.from_numpy(_keys(B, 3)).cuda())
    width = env.masked_observation_size if masked else env.observation_size
    norm = ObservationNormalizer(width)
    p_model = networks.make_recurrent_model([], 64, [2 * env.action_size], width)
    v_model = networks.make_model([64, 64, 1], width)
    policy = networks.RecurrentTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6),
                                          normalizer=norm)
    critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)), normalizer=norm)
    roll = RecurrentActorRollout(env, state, policy, T, masked=masked, critic=critic)
    learner = RecurrentPPOLearner(policy, critic, learning_rate=3e-3, num_minibatches=2, num_update_epochs=2,
                                  key=jumpy.random_prngkey(7), backward=backward)
    ptr0, out = policy.theta.data_ptr(), []
    for _ in range(rounds):
        before = policy.theta.clone()
        roll.replay()
        torch.cuda.synchronize()
        acted = (roll.actions.clone(), roll.logp.clone(), roll.hidden.clone())
        metrics = learner.update(roll)
        torch.cuda.synchronize()
        assert policy.theta.data_ptr() == ptr0 and not torch.equal(policy.theta, before)  # stepped in place
        assert all(bool(torch.isfinite(v)) for v in metrics.values()) and bool(torch.isfinite(policy.theta).all())
        out.append(dict(acted=acted, theta=policy.theta.clone(), v_theta=critic.theta.clone(),
                        metrics={k: v.clone() for k, v in metrics.items()}))
    # the captured graph acts under the parameters the learner left: an eager actor holding them reproduces
    # the next replay's first step, one holding the parameters from before the last update does not
    h_before, reset_before, key_before = policy.hidden.clone(), policy.reset.clone(), policy.key.clone()
    obs0 = roll._obs_of(roll.state).clone()
    roll.replay()
    torch.cuda.synchronize()
    assert torch.equal(roll.obs[0], obs0)
    for theta, same in ((out[-1]["theta"], True), (before, False)):
        eager = networks.RecurrentTanhPolicy(p_model, types.SimpleNamespace(theta=theta.clone()), key_before,
                                             normalizer=norm)
        eager._buffers(B)
        eager.hidden.copy_(h_before); eager.reset.copy_(reset_before)
        action = torch.empty_like(roll.actions[0])
        eager.act_into(obs0, action)
        torch.cuda.synchronize()
        assert torch.equal(action, roll.actions[0]) == same
    return out


@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
def test_replay_learn_replay(masked):
    a = _loop("native", masked)  # both halves in the engine: every sum in a fixed order
    b = _loop("native", masked)
    for ra, rb in zip(a[:2], b[:2]):
        for x, y in zip(ra["acted"], rb["acted"]):
            assert torch.equal(x, y)
        assert torch.equal(ra["theta"].view(torch.int32), rb["theta"].view(torch.int32))
        assert torch.equal(ra["v_theta"].view(torch.int32), rb["v_theta"].view(torch.int32))
        assert all(torch.equal(ra["metrics"][k], rb["metrics"][k]) for k in ra["metrics"])
    # round 2 acted under round 1's update
    assert not torch.equal(a[0]["acted"][0], a[1]["acted"][0])
