"""GPU: ``RecurrentActorRollout(..., critic=RecurrentValueFunction(...))`` on ant_heavenhell with
``obs_mask`` and ``masked=True``, B = 64, T = 4, two replays.

Episodes last 3 steps and the envs start at three phases (the engine's own ``steps`` buffer is set to
b mod 3 before the capture), so that within the two replays ``done`` falls inside a window, on a
window's last step -- the boundary reset of the next replay -- and not at all for the other envs at
that boundary, whose state is carried across it: all three are asserted from the recorded ``done``.

Bitwise: ``roll.values`` against a step-by-step chain of ``model.apply`` over the recorded rows that
starts from zeros before the first replay and runs through both; ``roll.value_hidden0``;
``critic.hidden`` and ``critic.reset``; ``roll.vs`` / ``roll.advantages`` against ``compute_gae``; the
actor-side buffers against a twin rollout with the feed-forward critic from the same keys.  The
normaliser is shared and updated by the graph, and the chain normalises with the table the replay
left: the critic's launch comes after the update."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, EPISODE = 64, 4, 3
NAME = "ant_heavenhell"


def _build(recurrent):
    from po_brax_amd import envs, jumpy
    from po_brax_amd import standard_observability_masks as masks
    from po_brax_amd.rollout import RecurrentActorRollout
    from po_brax_amd.training import RecurrentValueFunction, ValueFunction, networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    from test_gpu_parity import _keys
    env = envs.create(NAME, batch_size=B, episode_length=EPISODE, obs_mask=masks.po_env_mask(NAME, cfrc=False))
    state = env.reset(torch.from_numpy(_keys(B, 3)).cuda())
    state.info["steps"].copy_(torch.arange(B, device="cuda") % EPISODE)  # three phases: in place, the engine's buffer
    width = env.masked_observation_size
    norm = ObservationNormalizer(width)
    p_model = networks.make_recurrent_model([], 64, [2 * env.action_size], width)
    policy = networks.RecurrentTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6),
                                          normalizer=norm)
    if recurrent:
        v_model = networks.make_recurrent_model([], 64, [1], width)
        critic = RecurrentValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)), normalizer=norm)
    else:
        v_model = networks.make_model([64, 64, 1], width)
        critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)), normalizer=norm)
    roll = RecurrentActorRollout(env, state, policy, T, masked=True, update_normalizer=True, critic=critic)
    return roll, critic, v_model, norm


ACTOR_SIDE = ("obs", "final_obs", "actions", "raw", "logp", "hidden", "reward", "done", "truncation")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_values_carry_across_replays_and_the_actor_side_is_untouched():
    from po_brax_amd.training import compute_gae
    roll, critic, v_model, norm = _build(True)
    twin = _build(False)[0]
    assert roll.done.shape == (T, B) and roll.done.dtype == torch.float32 and roll.done.is_contiguous()
    assert roll.values.shape == (T + 1, B) and roll.value_hidden0.shape == (B, 64)
    assert not critic.hidden.any() and not critic.reset.any()  # both start as zeros
    hidden_ptr, reset_ptr = critic.hidden.data_ptr(), critic.reset.data_ptr()
    h = torch.zeros((B, 64), device="cuda")       # the chain's state, from zeros before the first replay
    boundary = torch.zeros(B, device="cuda")      # the reset of the next replay's row 0
    seen = dict(inside=False, last=False, carried=False)
    for replay in range(2):
        roll.replay()
        twin.replay()
        torch.cuda.synchronize()
        for name in ACTOR_SIDE:
            assert torch.equal(_bits(getattr(roll, name)), _bits(getattr(twin, name))), (replay, name)
        done = roll.done
        seen["inside"] |= bool(done[:T - 1].any())
        seen["last"] |= bool(done[T - 1].any())
        if replay == 1:
            seen["carried"] = bool((boundary == 0).any()) and bool((boundary != 0).any())
        # ---- the chain over this replay's rows: T trajectory rows, then final_obs without advancing the carry
        resets = [boundary] + [done[t] for t in range(T)]
        rows = [roll.obs[t] for t in range(T)] + [roll.final_obs]
        for t in range(T + 1):
            if t == 0:
                want_h0 = torch.where(resets[0].reshape(B, 1) != 0, torch.zeros_like(h), h)
                assert torch.equal(_bits(roll.value_hidden0), _bits(want_h0)), replay
            y, h_new = v_model.apply(critic.params, norm.apply(rows[t]), h, resets[t])
            assert torch.equal(_bits(roll.values[t]), _bits(y.reshape(B))), (replay, t)
            if t < T:
                h = h_new
        assert torch.equal(_bits(critic.hidden), _bits(h)), replay           # after the T trajectory rows
        assert torch.equal(_bits(critic.reset), _bits(done[T - 1])), replay
        assert critic.hidden.data_ptr() == hidden_ptr and critic.reset.data_ptr() == reset_ptr
        boundary = done[T - 1].clone()
        # ---- vs and advantages: the same pob_gae launch as with the feed-forward critic
        vs, adv = compute_gae(roll.truncation, done * (1.0 - roll.truncation), roll.reward, roll.values[:T].contiguous(),
                              roll.values[T].contiguous(), **roll.gae)
        assert torch.equal(_bits(roll.vs), _bits(vs)) and torch.equal(_bits(roll.advantages), _bits(adv)), replay
        assert not torch.equal(roll.values[:T], twin.values[:T])  # another network: the twin shares the actor side only
    assert seen == dict(inside=True, last=True, carried=True), seen


def test_memory_shows_in_the_values():
    """The same rows under another carried state give other values: the rows alone do not determine them."""
    roll = _build(True)[0]
    roll.replay()
    other, critic2, _, _ = _build(True)
    critic2.hidden.fill_(0.5)
    other.replay()
    torch.cuda.synchronize()
    assert torch.equal(roll.obs, other.obs) and torch.equal(roll.final_obs, other.final_obs)
    assert not torch.equal(roll.values, other.values)


def test_actor_rollout_refuses_the_recurrent_critic():
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import RecurrentValueFunction, networks
    from test_gpu_parity import _keys
    env = envs.create(NAME, batch_size=B)
    state = env.reset(torch.from_numpy(_keys(B, 3)).cuda())
    D = env.observation_size
    p_model = networks.make_models(2 * env.action_size, D)[0]
    policy = networks.NormalTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(0)), jumpy.random_prngkey(1))
    v_model = networks.make_recurrent_model([], 8, [1], D)
    critic = RecurrentValueFunction(v_model, v_model.init(jumpy.random_prngkey(2)))
    with pytest.raises(TypeError, match="ValueFunction"):
        ActorRollout(env, state, policy, 2, critic=critic)
