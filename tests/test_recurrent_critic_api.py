"""No GPU: the argument checks of the recurrent critic's pieces -- ``RecurrentValueFunction``'s
constructor, the rollouts' ``critic=`` type check, ``RecurrentPPOLearner``'s ``backward`` default and its
``value_hidden0`` requirement, and ``pob_gru_sequence_forward``'s argument errors, which are reported
through ``pob_last_error`` before any HIP call."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from test_recurrent_critic_learner_host import A, D, H, _key, stub_actors

KEY = torch.tensor([0, 1], dtype=torch.uint32)


def test_recurrent_value_function_checks():
    from po_brax_amd.training import RecurrentValueFunction, make_model, make_recurrent_model
    from po_brax_amd.training.normalization import ObservationNormalizer
    wide = make_recurrent_model([], 6, [2], D)
    with pytest.raises(ValueError, match="last width must be 1, got 2"):
        RecurrentValueFunction(wide, wide.init(KEY))
    two = make_recurrent_model([4], 6, [3, 2], D)
    with pytest.raises(ValueError, match="last width must be 1"):
        RecurrentValueFunction(two, two.init(KEY))
    flat = make_model([8, 1], D)  # a feed-forward model: ValueFunction's, not this class's
    with pytest.raises(ValueError, match="make_recurrent_model"):
        RecurrentValueFunction(flat, flat.init(KEY))
    good = make_recurrent_model([], 6, [1], D)
    norm = ObservationNormalizer.__new__(ObservationNormalizer)  # its device state needs a GPU: the fields the check reads
    norm.obs_size, norm.table = D + 1, torch.zeros((3, D + 1))
    with pytest.raises(ValueError, match="width"):
        RecurrentValueFunction(good, good.init(KEY), normalizer=norm)
    with pytest.raises(TypeError, match="ObservationNormalizer"):
        RecurrentValueFunction(good, good.init(KEY), normalizer=object())
    with pytest.raises(ValueError, match="CUDA"):  # parameters on the host: no CPU fallback
        RecurrentValueFunction(good, good.init(KEY))
    params = good.init(KEY)
    params.theta = params.theta[:-1]
    with pytest.raises(ValueError):
        RecurrentValueFunction(good, params)


def test_exports():
    from po_brax_amd import _lib, training
    assert training.RecurrentValueFunction is training.gae.RecurrentValueFunction
    assert "pob_gru_sequence_forward" in _lib.EXPORTS and _lib.ABI_VERSION == 8 and _lib.lib.pob_abi_version() == 8


def test_actor_rollout_still_refuses_the_recurrent_critic():
    """The feed-forward ``ActorRollout``'s ``critic=`` check (``_critic_buffers`` as it calls it) takes a
    ``ValueFunction`` only; ``RecurrentActorRollout``'s takes both and nothing else."""
    from po_brax_amd import rollout
    _, critic = stub_actors(0, None)
    state = types.SimpleNamespace(aux={}, info={})
    with pytest.raises(TypeError, match="training.gae.ValueFunction$"):
        rollout._critic_buffers(types.SimpleNamespace(), critic, None, False, state, 4, 8, D, "cpu")
    with pytest.raises(TypeError, match="ValueFunction or RecurrentValueFunction"):
        rollout._critic_buffers(types.SimpleNamespace(), object(), None, False, state, 4, 8, D, "cpu", recurrent=True)


def test_learner_backward_default_follows_the_critic():
    from po_brax_amd.training import RecurrentPPOLearner
    from test_recurrent_learner_host import stub_actors as feed_forward_actors
    policy, value_fn = feed_forward_actors(0, None, None)
    assert RecurrentPPOLearner(policy, value_fn, key=_key(1)).backward == ("native", "torch")
    policy, critic = stub_actors(0, None)
    assert RecurrentPPOLearner(policy, critic, key=_key(1)).backward == ("native", "native")
    assert RecurrentPPOLearner(policy, critic, key=_key(1), backward="torch").backward == ("torch", "torch")
    assert RecurrentPPOLearner(policy, critic, key=_key(1), backward=("native", "torch")).backward == ("native", "torch")
    with pytest.raises(ValueError, match="backward"):
        RecurrentPPOLearner(policy, critic, key=_key(1), backward="hip")
    with pytest.raises(TypeError, match="value_fn"):
        RecurrentPPOLearner(policy, object(), key=_key(1))


def test_update_needs_value_hidden0():
    import recurrent_critic_ref as cref
    from po_brax_amd.training import RecurrentPPOLearner
    policy, critic = stub_actors(0, None)
    roll = cref.make_roll(np.random.default_rng(0), 3, 12, D, A, H, critic.hidden_size, policy, None, 0.3)
    del roll.value_hidden0  # the buffers of a rollout built with the feed-forward critic
    learner = RecurrentPPOLearner(policy, critic, num_minibatches=3, num_update_epochs=1, key=_key(1), backward="torch")
    before = [t.clone() for t in (policy.theta, critic.theta)]
    with pytest.raises(ValueError, match="value_hidden0"):
        learner.update(roll)
    assert torch.equal(before[0], policy.theta) and torch.equal(before[1], critic.theta)


def test_pob_gru_sequence_forward_rejects_bad_arguments_without_a_gpu():
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import GRUHandle
    lib = _lib.lib
    gru = GRUHandle([7], 5, [1], 1)
    a = np.zeros(64, np.float32)
    p = a.ctypes.data_as(C.c_void_p)  # never dereferenced: every call below is rejected before any HIP call
    ok = dict(g=gru.handle, S=3, M=4, B=4, obs=p, idx=None, h0=p, theta=p, y=p, step=3)

    def call(**kw):
        k = {**ok, **kw}
        return lib.pob_gru_sequence_forward(k["g"], k["S"], k["M"], k["B"], k["obs"], k["idx"], k["h0"], None, k["theta"],
                                            k["y"], None, None, k["step"], None, 0.0, None)

    for kw, word in ((dict(S=0), "step count"), (dict(S=-2), "step count"), (dict(step=0), "h_out_step"),
                     (dict(step=4), "h_out_step"), (dict(y=None), "NULL"), (dict(obs=None), "NULL"), (dict(h0=None), "NULL"),
                     (dict(theta=None), "NULL"), (dict(g=None), "NULL"), (dict(M=0), "M"), (dict(B=5), "without idx"),
                     (dict(M=2 ** 31, B=2 ** 31), "too many rows")):
        assert call(**kw) == _lib.POB_EINVAL, kw
        msg = lib.pob_last_error().decode()
        assert msg.startswith("gru") and word in msg, (kw, msg)
        with pytest.raises(ValueError, match="gru"):
            _lib.check(call(**kw))
