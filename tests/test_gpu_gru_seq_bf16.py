"""GPU: the bf16 recurrent window (``pob_gru_sequence_forward_bf16``, ``RecurrentValueFunction(kernel="bf16")``) against the
float64 statement of its definition: within TOL on random networks, exact on saturating small integers, the pack pass inside a
captured graph, and as the critic of a ``RecurrentActorRollout``."""
import pytest
import torch

from test_gru_seq_bf16_api import B_ALL, CLIP, NETS, TOL, VARIANTS, case, exact_case, metric, reference, rows_of

pytestmark = pytest.mark.gpu

GUARD = 64


def _guarded(shape):
    flat = torch.full((GUARD + int(torch.Size(shape).numel()) + GUARD,), 7.0, device="cuda")
    return flat, flat[GUARD:-GUARD].view(shape)


def _window(model, theta, obs, h0, reset, table, rows=None, step=None, alias=False):
    """One launch on device tensors: obs (S, B, D), the sequences ``rows`` (int32 idx; None: all B).  Returns y, h_first,
    h_out on the CPU after checking the guard elements around each; ``alias``: h_out is h0's own memory."""
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import gru_bf16_workspace
    S, B = obs.shape[0], obs.shape[1]
    M, H = B if rows is None else rows.shape[0], model.hidden_size
    ws = gru_bf16_workspace(model.gru, "cuda")
    bufs = [_guarded((S, M, model.post_sizes[-1])), _guarded((M, H)), _guarded((M, H))]
    h_in = h0.clone()
    h_out = h_in if alias else bufs[2][1]
    _lib.check(_lib.lib.pob_gru_sequence_forward_bf16(
        model.gru.handle, S, M, B, obs.data_ptr(), None if rows is None else rows.data_ptr(), h_in.data_ptr(), reset.data_ptr(),
        theta.data_ptr(), bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), h_out.data_ptr(), S if step is None else step,
        table.data_ptr(), CLIP, ws.data_ptr(), _lib.stream_handle(obs.device)))
    torch.cuda.synchronize()
    for flat, _ in bufs:
        assert bool((flat[:GUARD] == 7.0).all()) and bool((flat[-GUARD:] == 7.0).all())
    return bufs[0][1].cpu(), bufs[1][1].cpu(), h_out.cpu()


def _variant(tensors, M, use_idx):
    """The device arguments of a variant: the first M envs as the whole batch, or M rows of all B_ALL through idx."""
    obs, h0, reset = tensors
    if use_idx:
        return obs, h0, reset, rows_of(M, True).to(torch.int32).cuda()
    return obs[:, :M].contiguous(), h0[:M].contiguous(), reset[:, :M].contiguous(), None


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("net", range(len(NETS)))
def test_window_against_the_float64_definition(net, S):
    model, theta, obs, h0, reset, table = case(net, S)
    pre, H, post, _ = NETS[net]
    want_y, want_h = reference(pre, H, post, model.activation, theta, obs, h0, reset, table)
    first = torch.where(reset[0].reshape(-1, 1) != 0, torch.zeros_like(h0), h0)  # the f32 reset rule: no rounding touches it
    td, tb, dev = theta.cuda(), table.cuda(), (obs.cuda(), h0.cuda(), reset.cuda())
    for M, use_idx in VARIANTS:
        rows, step = rows_of(M, use_idx), (max(1, S - 1) if use_idx else S)
        args = _variant(dev, M, use_idx)
        y, h_first, h_out = _window(model, td, *args[:3], tb, args[3], step)
        ey, eh = metric(y, want_y[:, rows]), metric(h_out, want_h[step][rows])
        print(f"bf16 window {NETS[net]} S={S} M={M} idx={use_idx}: y {ey:.3e} h_out {eh:.3e}")
        assert ey <= TOL and eh <= TOL, (M, use_idx, ey, eh)
        assert torch.equal(h_first, first[rows]), (M, use_idx)
        again = _window(model, td, *args[:3], tb, args[3], step, alias=not use_idx)  # deterministic; h_out may be h0 without idx
        assert all(torch.equal(a, b) for a, b in zip((y, h_first, h_out), again)), (M, use_idx)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 200])
def test_window_layout_exact_integers(M):
    """Every value an integer that bf16 holds, every gate saturated: a wrong fragment index, pad, pitch or tail row shows."""
    model, theta, obs, h0, reset, table, (pre, H, post) = exact_case()
    want_y, want_h = reference(pre, H, post, 0, theta, obs, h0, reset, table)
    td, tb, dev = theta.cuda(), table.cuda(), (obs.cuda(), h0.cuda(), reset.cuda())
    for use_idx in (False, True):
        rows = rows_of(M, use_idx)
        args = _variant(dev, M, use_idx)
        y, _, h_out = _window(model, td, *args[:3], tb, args[3])
        assert torch.equal(y.double(), want_y[:, rows]) and torch.equal(h_out.double(), want_h[-1][rows]), use_idx


def test_pack_pass_is_in_a_captured_graph():
    """theta changed in place between replays: a hoisted pack pass would keep the old weights."""
    from po_brax_amd.training import RecurrentValueFunction
    from po_brax_amd.training.networks import RecurrentParams
    from po_brax_amd.training.normalization import ObservationNormalizer
    model, theta, obs, _, reset, _ = case(2, 3)
    pre, H, post, _ = NETS[2]
    params = RecurrentParams(theta.cuda(), pre, H, post)
    critic = RecurrentValueFunction(model, params, normalizer=ObservationNormalizer(pre[0]), kernel="bf16")
    od, rd = obs[:, :96].contiguous().cuda(), reset[:, :96].contiguous().cuda()
    y, hf = torch.empty((3, 96), device="cuda"), torch.empty((96, H), device="cuda")
    critic.values_sequence_into(od, rd, y, hf)  # allocates hidden and reset before the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        critic.values_sequence_into(od, rd, y, hf)
    for scale in (0.5, 3.0, 0.7):
        before, h_start = y.clone(), critic.hidden.clone()
        critic.theta.mul_(scale)
        g.replay()
        got, h_got = y.clone(), critic.hidden.clone()
        critic.hidden.copy_(h_start)
        critic.values_sequence_into(od, rd, y, hf)  # eagerly, from the same state
        torch.cuda.synchronize()
        assert torch.equal(got, y) and torch.equal(h_got, critic.hidden) and not torch.equal(got, before), scale


def _rollout(kernel):
    from po_brax_amd import envs, jumpy
    from po_brax_amd import standard_observability_masks as masks
    from po_brax_amd.rollout import RecurrentActorRollout
    from po_brax_amd.training import RecurrentValueFunction, networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    from test_gpu_parity import _keys
    name, B = "ant_heavenhell", 64
    env = envs.create(name, batch_size=B, episode_length=3, obs_mask=masks.po_env_mask(name, cfrc=False))
    state = env.reset(torch.from_numpy(_keys(B, 3)).cuda())
    state.info["steps"].copy_(torch.arange(B, device="cuda") % 3)  # three phases: done falls inside and between the windows
    width = env.masked_observation_size
    norm = ObservationNormalizer(width)
    p_model = networks.make_recurrent_model([], 64, [2 * env.action_size], width)
    policy = networks.RecurrentTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6), normalizer=norm)
    v_model = networks.make_recurrent_model([], 64, [1], width)
    critic = RecurrentValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)), normalizer=norm, kernel=kernel)
    return RecurrentActorRollout(env, state, policy, 3, masked=True, critic=critic), critic, v_model, norm


def test_rollout_critic_carries_its_state_across_replays():
    roll, critic, v_model, norm = _rollout("bf16")
    twin = _rollout("tile")[0]
    B, T = 64, 3
    h, boundary = torch.zeros((B, 64), device="cuda"), torch.zeros(B, device="cuda")
    for replay in range(2):
        roll.replay()
        twin.replay()
        torch.cuda.synchronize()
        for name in ("obs", "final_obs", "actions", "raw", "logp", "hidden", "reward", "done", "truncation"):
            assert torch.equal(getattr(roll, name), getattr(twin, name)), (replay, name)
        resets = torch.stack([boundary, *roll.done])
        rows = norm.apply(torch.cat([roll.obs, roll.final_obs[None]]))
        want = []
        for t in range(T + 1):  # the chain in torch ops; final_obs does not advance the carry
            y, h_new = v_model.apply_sequence(critic.params, rows[t:t + 1], h, resets[t:t + 1], kernel="bf16")
            want.append(y.reshape(B))
            h = h_new if t < T else h
        err, err_h = metric(roll.values.cpu(), torch.stack(want).double().cpu()), metric(critic.hidden.cpu(), h.double().cpu())
        print(f"bf16 rollout critic replay {replay}: values {err:.3e} hidden {err_h:.3e}")
        assert err <= TOL and err_h <= TOL, (replay, err, err_h)
        assert not torch.equal(roll.values, twin.values)
        boundary = roll.done[T - 1].clone()
    assert bool(torch.isfinite(roll.values).all()) and bool(roll.done.any())
