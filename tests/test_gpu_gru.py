"""GPU: the recurrent-actor kernels (csrc/pob_mlp.hip k_gru_forward / k_gru_policy_act) equal
their plain-C restatement (csrc/pob_mlp.h gru_forward_ref / gru_policy_ref, built for the host by
tests/host/gru_host.cpp) bit for bit -- forward, hidden state, reset, actor -- and
RecurrentActorRollout equals the same loop run eagerly."""
import numpy as np
import pytest
import torch

import pob_np
from test_gru_host import build_gru_host, random_gru, ref_forward, ref_policy

pytestmark = pytest.mark.gpu

BATCHES = (1, 31, 32, 33, 65, 2049)
PAD = 3          # sentinel rows behind every output
SENTINEL = -777.0
# (pre = [D, *pre widths], H, post)
NETS = [([6], 5, [4]),                 # odd concatenation: the pad
        ([19], 7, [6]),
        ([40], 33, [8]),               # a second output tile with a tail
        ([128], 128, [2]),             # both limits
        ([114, 32], 64, [32, 16])]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_gru_host(tmp_path_factory.mktemp("gru_host_gpu"))


def _handle(pre, H, post, act):
    from po_brax_amd.training.networks import GRUHandle
    return GRUHandle(pre, H, post, act)


def _sentinel(rows, width=None):
    shape = (rows + PAD,) if width is None else (rows + PAD, width)
    return torch.full(shape, SENTINEL, device="cuda")


def _forward(g, B, x, theta, reset, h):
    """One launch on the first B rows of sentinel-padded buffers; returns y, h_out, h_in_copy (B rows each)."""
    from po_brax_amd import _lib
    H, O = g.hidden, g.post_sizes[-1]
    h_io, y, hc = _sentinel(B, H), _sentinel(B, O), _sentinel(B, H)
    h_io[:B] = h[:B]
    _lib.check(_lib.lib.pob_gru_forward(g.handle, B, x.data_ptr(), theta.data_ptr(), None if reset is None else reset.data_ptr(),
                                        h_io.data_ptr(), y.data_ptr(), hc.data_ptr(), _lib.stream_handle(x.device)))
    torch.cuda.synchronize()
    for t in (h_io, y, hc):
        assert (t[B:] == SENTINEL).all()  # rows >= B untouched
    return y[:B].cpu(), h_io[:B].cpu(), hc[:B].cpu()


def _case(pre, H, post, rng, B):
    x, h, theta = random_gru(pre, H, post, rng, B)
    x[:, 1] = 1e-40  # a subnormal input column
    x[:, 2] = 0.0    # and an exactly-zero one
    h[:, 0] = -0.0
    h[:, 1] = -1e-41
    reset = np.zeros(B, np.float32)
    reset[::3] = 1.0
    return x, h, theta, reset


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("net", range(len(NETS)))
def test_forward_bit_exact(host, net, act):
    pre, H, post = NETS[net]
    rng = np.random.default_rng(2000 + 10 * net + act)
    x, h, theta, reset = _case(pre, H, post, rng, max(BATCHES))
    want = [torch.from_numpy(a) for a in ref_forward(host, pre, H, post, act, x, theta, reset, h)]  # rows are independent
    g = _handle(pre, H, post, act)
    xd, hd, td, rd = (torch.from_numpy(a).cuda() for a in (x, h, theta, reset))
    for B in BATCHES:
        got = _forward(g, B, xd[:B].contiguous(), td, rd[:B].contiguous(), hd)
        for name, a, b in zip(("y", "h_out", "h_in_copy"), got, want):
            assert torch.equal(a.view(torch.int32), b[:B].view(torch.int32)), (pre, H, post, act, B, name)
    # no reset array: every env keeps its h
    want0 = [torch.from_numpy(a) for a in ref_forward(host, pre, H, post, act, x[:65], theta, None, h[:65])]
    got0 = _forward(g, 65, xd[:65].contiguous(), td, None, hd)
    for a, b in zip(got0, want0):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_chained_steps_bit_exact(host):
    pre, H, post = NETS[4]
    B, act = 33, 1
    rng = np.random.default_rng(31)
    _, h, theta = random_gru(pre, H, post, rng, B)
    g = _handle(pre, H, post, act)
    td = torch.from_numpy(theta).cuda()
    hd = torch.from_numpy(h).cuda()
    for step in range(5):
        x = rng.uniform(-3, 3, (B, pre[0])).astype(np.float32)
        reset = ((np.arange(B) + step) % (step + 2) == 0).astype(np.float32)  # differs per step
        y, h_out, h_copy = ref_forward(host, pre, H, post, act, x, theta, reset, h)
        got = _forward(g, B, torch.from_numpy(x).cuda(), td, torch.from_numpy(reset).cuda(), hd)
        for name, a, b in zip(("y", "h_out", "h_in_copy"), got, (y, h_out, h_copy)):
            assert torch.equal(a, torch.from_numpy(b)), (step, name)
        h = h_out
        hd = got[1].cuda()  # the kernel's own h' fed back


POLICY = ([114], 64, [16])
A = 8


def _uniform_rows(key_np, total, first, B):
    sub = pob_np.split(key_np)[1]
    u = np.asarray(pob_np.uniform(sub, (total * A,), np.float32(-1), np.float32(1)), np.float32).reshape(total, A)
    return u[first:first + B]


def _act(g, obs, theta, key, total, first, reset, h, det=False, logp_fill=0.0):
    from po_brax_amd import _lib
    B, D = obs.shape
    H = g.hidden
    out = {"action": _sentinel(B, A), "logp": torch.full((B + PAD,), logp_fill, device="cuda"), "raw": _sentinel(B, A),
           "logits": _sentinel(B, 2 * A), "obs_copy": _sentinel(B, D), "h_in_copy": _sentinel(B, H)}
    h_io = _sentinel(B, H)
    h_io[:B] = h
    _lib.check(_lib.lib.pob_gru_policy_act(
        g.handle, B, total, first, obs.data_ptr(), theta.data_ptr(), key.data_ptr(), int(det), reset.data_ptr(),
        h_io.data_ptr(), *(out[k].data_ptr() for k in ("action", "logp", "raw", "logits", "obs_copy", "h_in_copy")),
        _lib.stream_handle(obs.device)))
    torch.cuda.synchronize()
    out["h_out"] = h_io
    for k, v in out.items():
        assert (v[B:] == (logp_fill if k == "logp" else SENTINEL)).all(), k
    return {k: v[:B].cpu() for k, v in out.items()}


@pytest.fixture(scope="module")
def actor_case(host):
    pre, H, post = POLICY
    rng = np.random.default_rng(78)
    x, h, theta, reset = _case(pre, H, post, rng, 4096)
    return x, h, theta, reset


def _same(got, want, keys):
    for k in keys:
        assert torch.equal(got[k], torch.from_numpy(want[k])), k


@pytest.mark.parametrize("B", [33, 2049])
def test_actor_bit_exact(host, actor_case, B):
    from po_brax_amd import jumpy
    pre, H, post = POLICY
    x, h, theta, reset = actor_case
    key_np = np.asarray(pob_np.prngkey(11), np.uint32)
    key = torch.from_numpy(key_np.copy()).cuda()
    g = _handle(pre, H, post, 1)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    got = _act(g, c(x[:B]), c(theta), key, B, 0, c(reset[:B]), c(h[:B]))
    want = ref_policy(host, pre, H, post, 1, x[:B], theta, reset[:B], h[:B], _uniform_rows(key_np, B, 0, B))
    _same(got, want, ("logits", "h_out", "h_in_copy", "raw", "action", "logp"))
    assert torch.equal(got["obs_copy"], torch.from_numpy(x[:B]))
    assert torch.equal(key.cpu(), jumpy.random_split(torch.from_numpy(key_np).cuda())[0].cpu())
    assert np.array_equal(key.cpu().numpy(), pob_np.split(key_np)[0])


def test_actor_shard_equals_slice_and_deterministic(host, actor_case):
    pre, H, post = POLICY
    x, h, theta, reset = actor_case
    key_np = np.asarray(pob_np.prngkey(12), np.uint32)
    g = _handle(pre, H, post, 1)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    td = c(theta)
    whole = _act(g, c(x), td, c(key_np.copy()), 4096, 0, c(reset), c(h))
    sl = slice(1000, 1097)
    shard = _act(g, c(x[sl]), td, c(key_np.copy()), 4096, 1000, c(reset[sl]), c(h[sl]))
    for k in whole:
        assert torch.equal(shard[k], whole[k][sl]), k
    want = ref_policy(host, pre, H, post, 1, x[sl], theta, reset[sl], h[sl], _uniform_rows(key_np, 4096, 1000, 97))
    _same(shard, want, ("action", "logp", "h_out", "h_in_copy"))
    # deterministic: tanh(loc), the key neither read nor advanced, logp untouched
    key = c(key_np.copy())
    det = _act(g, c(x[:97]), td, key, 97, 0, c(reset[:97]), c(h[:97]), det=True, logp_fill=-7.0)
    wd = ref_policy(host, pre, H, post, 1, x[:97], theta, reset[:97], h[:97], np.zeros((97, A), np.float32), deterministic=True)
    _same(det, wd, ("action", "raw", "logits", "h_out"))
    assert torch.equal(det["raw"], det["logits"][:, :A])
    assert (det["logp"] == -7.0).all() and np.array_equal(key.cpu().numpy(), key_np)


def test_apply_runs_the_kernel_and_matches_torch_path():
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_recurrent_model([32], 24, [32, 6], 19)
    p_cpu = model.init(torch.from_numpy(np.asarray(pob_np.prngkey(7), np.uint32)))
    p = model.init(jumpy.random_prngkey(7))
    assert p.theta.is_cuda and torch.equal(p.theta.cpu(), p_cpu.theta)  # the same draw with or without a GPU
    x = torch.rand((50, 19), device="cuda") * 2 - 1
    h = torch.rand((50, 24), device="cuda") * 2 - 1
    reset = (torch.arange(50, device="cuda") % 4 == 0).float()
    h0 = h.clone()
    y, h1 = model.apply(p, x, h, reset)
    assert torch.equal(h, h0) and y.shape == (50, 6) and h1.shape == (50, 24)  # a clone carries h'
    x.requires_grad_(True)
    y_t, h1_t = model.apply(p, x, h, reset)  # gradient required: torch ops
    assert y_t.requires_grad
    assert torch.allclose(y, y_t.detach(), atol=1e-5) and torch.allclose(h1, h1_t.detach(), atol=1e-5)


def _policy(env, obs_size, seed=5):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_recurrent_model([], 64, [2 * env.action_size], obs_size)
    params = model.init(jumpy.random_prngkey(seed))
    params.theta.mul_(3.0)  # livelier actions than the init's
    return networks.RecurrentTanhPolicy(model, params, jumpy.random_prngkey(seed + 1))


FIELDS = ("obs", "actions", "logp", "raw", "hidden", "reward", "done")


def _eager(env, s, policy, steps, obs_of):
    """policy(obs), step_, policy.reset <- done by hand; the trajectory as stacked tensors."""
    done_of = lambda st: st.aux["done"] if "done" in st.aux else st.done  # noqa: E731
    traj = {k: [] for k in FIELDS}
    for t in range(steps):
        obs = obs_of(s)
        traj["obs"].append(obs.clone())
        traj["hidden"].append(torch.where(policy.reset[:, None] != 0, torch.zeros_like(policy.hidden), policy.hidden))
        a = policy(obs)
        traj["actions"].append(a.clone()); traj["logp"].append(policy.logp.clone())
        traj["raw"].append(policy.raw.clone())
        s = env.step_(s, traj["actions"][-1])
        traj["reward"].append(s.reward.clone()); traj["done"].append(done_of(s).float().clone())
        policy.reset.copy_(traj["done"][-1])
    return s, {k: torch.stack(v) for k, v in traj.items()}


@pytest.mark.parametrize("name", ["ant_heavenhell", "ant_tag"])
def test_rollout_equals_eager(name):
    from po_brax_amd import envs
    from po_brax_amd.rollout import RecurrentActorRollout
    from test_gpu_parity import _keys
    B, T = 512, 6
    keys = torch.from_numpy(_keys(B, 3)).cuda()
    es = [envs.create(name, batch_size=B, episode_length=4) for _ in range(2)]
    ss = [e.reset(keys) for e in es]
    ps = [_policy(e, e.observation_size) for e in es]
    for p in ps:
        p._buffers(B)
    s, traj = _eager(es[0], ss[0], ps[0], 2 * T, lambda st: st.obs)
    assert traj["done"].any() and not traj["done"].all()  # autoresets fall inside
    # the state is zero exactly where the step before ended an episode (and at the very start)
    zero = (traj["hidden"] == 0).all(-1)
    assert zero[0].all() and torch.equal(zero[1:], traj["done"][:-1] != 0)
    ar = RecurrentActorRollout(es[1], ss[1], ps[1], T)
    for rep in range(2):
        sl = slice(rep * T, (rep + 1) * T)
        ar.replay()
        torch.cuda.synchronize()
        for k in FIELDS:
            assert torch.equal(getattr(ar, k), traj[k][sl]), (name, k, rep)
    assert torch.equal(ps[0].hidden, ps[1].hidden) and torch.equal(ps[0].reset, ps[1].reset)
    assert torch.equal(ps[0].key, ps[1].key)
    assert torch.equal(s.obs, ar.state.obs) and torch.equal(s.qp.pos, ar.state.qp.pos)


def test_rollout_masked_observation():
    from po_brax_amd import envs
    from po_brax_amd import standard_observability_masks as M
    from po_brax_amd.rollout import RecurrentActorRollout
    from test_gpu_parity import _keys
    name, B, T = "ant_heavenhell", 4096, 4
    idx = M.po_env_mask(name, cfrc=False)
    keys = torch.from_numpy(_keys(B, 3)).cuda()
    es = [envs.create(name, batch_size=B, episode_length=3, obs_mask=idx) for _ in range(2)]
    assert es[0].masked_observation_size == len(idx)
    ss = [e.reset(keys) for e in es]
    ps = [_policy(e, len(idx)) for e in es]
    for p in ps:
        p._buffers(B)
    s, traj = _eager(es[0], ss[0], ps[0], T, lambda st: st.info["obs_masked"])
    ar = RecurrentActorRollout(es[1], ss[1], ps[1], T, masked=True)
    ar.replay()
    torch.cuda.synchronize()
    assert ar.obs.shape == (T, B, len(idx))
    for k in FIELDS:
        assert torch.equal(getattr(ar, k), traj[k]), k
    assert torch.equal(ar.state.info["obs_masked"], s.obs[:, torch.as_tensor(idx, device="cuda")])
    # without a mask on the env, or with a policy of the full width, masked=True is refused
    plain = envs.create(name, batch_size=64)
    sp = plain.reset(torch.from_numpy(_keys(64, 3)).cuda())
    with pytest.raises(ValueError, match="obs_mask"):
        RecurrentActorRollout(plain, sp, _policy(plain, plain.observation_size), 2, masked=True)
    with pytest.raises(ValueError, match="the policy maps"):
        RecurrentActorRollout(es[1], ar.state, _policy(es[1], es[1].observation_size), 2, masked=True)
