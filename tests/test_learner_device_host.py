"""CPU: the learners' ``optimizer=`` and ``permutation=`` options on host tensors.

``optimizer="fused"`` (``FusedAdam``'s torch-op path, the restatement's bits) with ``permutation="torch"``:
one update of each learner through learner_ref.record_steps / check_update and their recurrent
counterparts, the problems, seeds and bounds of test_learner_host.py / test_recurrent_learner_host.py
unchanged (gradients within 4 x the float32 torch error + ulp32 of float64 autograd, every Adam step
within ulp32(theta) + 1e-6 lr of the float64 textbook Adam).

``permutation="threefry"``: the index slices the loss saw are slices of ``jumpy.random_permutation``
of the host restatement drawn from ``perm_key`` as it advances, once per epoch; ``key`` (the entropy
draws) takes the steps it always took."""
import numpy as np
import pytest
import torch

import learner_ref as ref
import recurrent_learner_ref as rref
import test_learner_host as ff
import test_recurrent_learner_host as rec_host
from po_brax_amd.training import networks


def _ff_update(seed, T, B, minibatches, epochs, tag, lr=3e-3, noise=0.3):
    from po_brax_amd.training import FusedAdam, PPOLearner
    rng = np.random.default_rng(seed)
    norm = ff.StubNormalizer(rng, ff.D)
    policy, value_fn = ff.stub_actors(seed, norm, norm)
    roll = ref.make_roll(rng, T, B, ff.D, ff.A, policy, norm, noise)
    learner = PPOLearner(policy, value_fn, learning_rate=lr, num_minibatches=minibatches, num_update_epochs=epochs,
                         key=ff._key(300 + seed), optimizer="fused", permutation="torch")
    assert isinstance(learner.optimizer, FusedAdam) and learner.perm_key is None
    rec = ref.record_steps(learner)
    metrics = learner.update(roll)
    return ref.check_update(learner, roll, rec, metrics, "live", f"{tag} seed {seed}")


def test_fused_adam_in_the_feed_forward_learner():
    """test_learner_host.test_update_with_clipping_live with optimizer="fused"."""
    out = ref.check_case([_ff_update(seed, 8, 32, 4, 2, "fused, live") for seed in range(4)], "fused, live")
    assert out["adam"] <= 1.0


def _recurrent_update(seed, T, B, minibatches, epochs, tag, lr=3e-3, noise=0.3):
    from po_brax_amd.training import FusedAdam, RecurrentPPOLearner
    rng = np.random.default_rng(seed)
    norm = ff.StubNormalizer(rng, rec_host.D)
    policy, value_fn = rec_host.stub_actors(seed, norm, norm)
    roll = rref.make_roll(rng, T, B, rec_host.D, rec_host.A, rec_host.H, policy, norm, noise)
    learner = RecurrentPPOLearner(policy, value_fn, learning_rate=lr, num_minibatches=minibatches,
                                  num_update_epochs=epochs, key=rec_host._key(300 + seed), backward="torch",
                                  optimizer="fused", permutation="torch")
    assert isinstance(learner.optimizer, FusedAdam)
    rec = ref.record_steps(learner)
    metrics = learner.update(roll)
    return rref.check_update(learner, roll, rec, metrics, f"{tag} seed {seed}")


def test_fused_adam_in_the_recurrent_learner():
    """test_recurrent_learner_host.test_update_with_a_shared_normaliser with optimizer="fused"."""
    out = ref.check_case([_recurrent_update(seed, 8, 32, 4, 2, "fused, recurrent") for seed in (0, 1, 2, 4)],
                         "fused, recurrent")
    assert out["adam"] <= 1.0


def test_defaults_are_torch():
    from po_brax_amd.training import PPOLearner
    policy, value_fn = ff.stub_actors(0, None, None)
    learner = PPOLearner(policy, value_fn, key=ff._key(1))
    assert isinstance(learner.optimizer, torch.optim.Adam) and learner.permutation == "torch" and learner.perm_key is None
    for kw in (dict(optimizer="adam"), dict(permutation="jax")):
        with pytest.raises(ValueError):
            PPOLearner(policy, value_fn, key=ff._key(1), **kw)


def _spy_on_loss(monkeypatch):
    """Records the ``idx`` every ``ppo_loss`` call of the learner module received."""
    from po_brax_amd.training import ppo
    seen, inner = [], ppo.ppo_loss

    def spy(*args, **kw):
        seen.append(kw["idx"].clone())
        return inner(*args, **kw)

    monkeypatch.setattr(ppo, "ppo_loss", spy)
    return seen


def _host_permutations(perm_key, n, epochs):
    """([permutation of each epoch], the key after them) from the host restatement alone."""
    from po_brax_amd import jumpy
    key, out = perm_key.clone(), []
    for _ in range(epochs):
        out.append(jumpy.random_permutation(key, n))
        key = networks._host_split(key)[0].to(torch.uint32)
    return out, key


@pytest.mark.parametrize("optimizer", ["torch", "fused"])
def test_threefry_permutation_in_the_feed_forward_learner(monkeypatch, optimizer):
    from po_brax_amd.training import PPOLearner
    seed, T, B, minibatches, epochs = 1, 8, 32, 4, 3
    rng = np.random.default_rng(seed)
    policy, value_fn = ff.stub_actors(seed, None, None)
    roll = ref.make_roll(rng, T, B, ff.D, ff.A, policy, None, 0.3)
    key = ff._key(300 + seed)
    learner = PPOLearner(policy, value_fn, num_minibatches=minibatches, num_update_epochs=epochs, key=key,
                         optimizer=optimizer, permutation="threefry")
    assert learner._generator is not None
    perm_key0 = networks._host_split(key, 3)[2].to(torch.uint32)
    assert learner.perm_key.dtype == torch.uint32 and torch.equal(learner.perm_key, perm_key0)
    key_after = key.clone()
    for _ in range(minibatches * epochs):
        key_after = networks._host_split(key_after)[0].to(torch.uint32)
    seen = _spy_on_loss(monkeypatch)
    before = [t.clone() for t in (policy.theta, value_fn.theta)]
    learner.update(roll)
    perms, perm_key_after = _host_permutations(perm_key0, T * B, epochs)
    M = T * B // minibatches
    assert len(seen) == minibatches * epochs
    for i, idx in enumerate(seen):
        e, m = divmod(i, minibatches)
        assert idx.dtype == torch.int32 and torch.equal(idx, perms[e][m * M:(m + 1) * M]), (e, m)
    assert not torch.equal(perms[0], perms[1]) and not torch.equal(perms[1], perms[2])
    assert torch.equal(learner.perm_key, perm_key_after)  # one advance an epoch
    assert torch.equal(learner.key, key_after)            # the entropy key's steps are unchanged
    assert all(not torch.equal(a, b) for a, b in zip(before, (policy.theta, value_fn.theta)))


def test_threefry_permutation_in_the_recurrent_learner(monkeypatch):
    from po_brax_amd.training import RecurrentPPOLearner
    seed, T, B, minibatches, epochs = 0, 5, 24, 3, 2
    rng = np.random.default_rng(seed)
    policy, value_fn = rec_host.stub_actors(seed, None, None)
    roll = rref.make_roll(rng, T, B, rec_host.D, rec_host.A, rec_host.H, policy, None, 0.3)
    key = rec_host._key(300 + seed)
    learner = RecurrentPPOLearner(policy, value_fn, num_minibatches=minibatches, num_update_epochs=epochs, key=key,
                                  backward="torch", optimizer="fused", permutation="threefry")
    perm_key0 = networks._host_split(key, 3)[2].to(torch.uint32)
    assert torch.equal(learner.perm_key, perm_key0)
    seen = _spy_on_loss(monkeypatch)
    learner.update(roll)
    perms, perm_key_after = _host_permutations(perm_key0, B, epochs)  # over ENVS
    M = B // minibatches
    row0 = (torch.arange(T, dtype=torch.int32) * B).reshape(T, 1)
    assert len(seen) == minibatches * epochs
    for i, rows in enumerate(seen):
        e, m = divmod(i, minibatches)
        want = (row0 + perms[e][m * M:(m + 1) * M].reshape(1, M)).reshape(T * M)  # trajectory row t B + idx[m]
        assert torch.equal(rows, want), (e, m)
    assert torch.equal(learner.perm_key, perm_key_after)
