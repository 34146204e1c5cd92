"""GPU: the policy-network kernels (csrc/pob_mlp.hip) equal their plain-C restatement
(csrc/pob_mlp.h, built for the host by tests/host/mlp_host.cpp) bit for bit -- forward and
tanh-normal actor -- and the rollouts built on them equal the same loop run eagerly."""
import numpy as np
import pytest
import torch

import pob_np
from test_mlp_host import NETS, build_host, random_net, ref_forward, ref_head

pytestmark = pytest.mark.gpu

BATCHES = (1, 31, 32, 33, 65, 2049)
ACT_NAME = {0: "relu", 1: "swish", 2: "tanh"}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("mlp_host_gpu"))


def _handle(sizes, act, act_final=False):
    from po_brax_amd.training.networks import MLPHandle
    return MLPHandle(sizes, act, act_final)


def _forward(h, x, theta):
    from po_brax_amd import _lib
    y = torch.full((x.shape[0], h.sizes[-1]), float("nan"), device="cuda")
    _lib.check(_lib.lib.pob_mlp_forward(h.handle, x.shape[0], x.data_ptr(), theta.data_ptr(), y.data_ptr(),
                                        _lib.stream_handle(x.device)))
    return y


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("net", range(len(NETS)))
def test_forward_bit_exact(host, net, act):
    sizes, act_final = NETS[net]
    rng = np.random.default_rng(1000 + 10 * net + act)
    x, theta = random_net(sizes, rng, max(BATCHES))
    x[:, 1] = 1e-40  # a subnormal input column
    x[:, 2] = 0.0    # and an exactly-zero one
    want = torch.from_numpy(ref_forward(host, sizes, act, act_final, x, theta))  # rows are independent: one reference
    h = _handle(sizes, act, act_final)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(theta).cuda()
    for B in BATCHES:
        got = _forward(h, xd[:B].contiguous(), td).cpu()
        assert torch.equal(got, want[:B]), (sizes, act, B, float((got - want[:B]).abs().max()))


def test_forward_layout_exact_integers():
    """Identity first layer, then W[i][j] = i + 100 j (asymmetric) on integer inputs: every sum
    is an exact small integer, so a row/column swap or a wrong k order shows."""
    n, m, B = 40, 37, 70
    W1 = np.arange(n)[:, None] + 100 * np.arange(m)[None, :]
    b1 = np.arange(m) - 5
    theta = np.concatenate([np.eye(n).ravel(), np.zeros(n), W1.ravel(), b1]).astype(np.float32)
    x = np.random.default_rng(0).integers(0, 8, (B, n))
    want = x @ W1 + b1
    assert np.abs(want).max() < 2 ** 24
    for act in (0,):  # relu keeps the non-negative integers
        got = _forward(_handle([n, n, m], act), torch.from_numpy(x.astype(np.float32)).cuda(), torch.from_numpy(theta).cuda())
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want)


def test_apply_runs_the_kernel_and_matches_torch_path():
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_model([32, 32, 6], 19)
    p_cpu = model.init(torch.from_numpy(np.asarray(pob_np.prngkey(7), np.uint32)))
    p = model.init(jumpy.random_prngkey(7))
    assert p.theta.is_cuda and torch.equal(p.theta.cpu(), p_cpu.theta)  # the same draw with or without a GPU
    x = torch.rand((3, 50, 19), device="cuda") * 2 - 1
    y = model.apply(p, x)
    assert y.shape == (3, 50, 6)
    x.requires_grad_(True)
    y_t = model.apply(p, x)  # gradient required: torch ops
    assert y_t.requires_grad and torch.allclose(y, y_t.detach(), atol=1e-5)
    with torch.no_grad():
        assert torch.equal(model.apply(p, x), y)


POLICY = [114, 32, 32, 32, 32, 16]
A = 8


def _uniform_rows(key_np, total, first, B):
    sub = pob_np.split(key_np)[1]
    u = np.asarray(pob_np.uniform(sub, (total * A,), np.float32(-1), np.float32(1)), np.float32).reshape(total, A)
    return u[first:first + B]


def _act(h, obs, theta, key, total, first, det=False, logp_fill=0.0):
    from po_brax_amd import _lib
    B, D = obs.shape
    out = {"action": torch.full((B, A), float("nan"), device="cuda"), "logp": torch.full((B,), logp_fill, device="cuda"),
           "raw": torch.full((B, A), float("nan"), device="cuda"), "logits": torch.full((B, 2 * A), float("nan"), device="cuda"),
           "obs_copy": torch.full((B, D), float("nan"), device="cuda")}
    _lib.check(_lib.lib.pob_policy_act(h.handle, B, total, first, obs.data_ptr(), theta.data_ptr(), key.data_ptr(), int(det),
                                       *(out[k].data_ptr() for k in ("action", "logp", "raw", "logits", "obs_copy")),
                                       _lib.stream_handle(obs.device)))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.fixture(scope="module")
def actor_case(host):
    rng = np.random.default_rng(77)
    x, theta = random_net(POLICY, rng, 4096)
    logits = ref_forward(host, POLICY, 1, False, x, theta)
    return x, theta, logits


@pytest.mark.parametrize("B", [33, 2049])
def test_actor_bit_exact(host, actor_case, B):
    from po_brax_amd import jumpy
    x, theta, logits = actor_case
    key_np = np.asarray(pob_np.prngkey(11), np.uint32)
    key = torch.from_numpy(key_np.copy()).cuda()
    h = _handle(POLICY, 1)
    got = _act(h, torch.from_numpy(x[:B]).cuda(), torch.from_numpy(theta).cuda(), key, B, 0)
    action, logp, raw = ref_head(host, logits[:B], _uniform_rows(key_np, B, 0, B))
    assert torch.equal(got["logits"], torch.from_numpy(logits[:B]))
    assert torch.equal(got["obs_copy"], torch.from_numpy(x[:B]))
    assert torch.equal(got["raw"], torch.from_numpy(raw)) and torch.equal(got["action"], torch.from_numpy(action))
    assert torch.equal(got["logp"], torch.from_numpy(logp))
    assert torch.equal(key.cpu(), jumpy.random_split(torch.from_numpy(key_np).cuda())[0].cpu())
    assert np.array_equal(key.cpu().numpy(), pob_np.split(key_np)[0])


def test_actor_shard_equals_slice_and_deterministic(host, actor_case):
    x, theta, logits = actor_case
    key_np = np.asarray(pob_np.prngkey(12), np.uint32)
    h = _handle(POLICY, 1)
    td = torch.from_numpy(theta).cuda()
    whole = _act(h, torch.from_numpy(x).cuda(), td, torch.from_numpy(key_np.copy()).cuda(), 4096, 0)
    shard = _act(h, torch.from_numpy(x[1000:1097]).cuda(), td, torch.from_numpy(key_np.copy()).cuda(), 4096, 1000)
    for k in whole:
        assert torch.equal(shard[k], whole[k][1000:1097]), k
    action, logp, raw = ref_head(host, logits[1000:1097], _uniform_rows(key_np, 4096, 1000, 97))
    assert torch.equal(shard["action"], torch.from_numpy(action)) and torch.equal(shard["logp"], torch.from_numpy(logp))
    # deterministic: tanh(loc), the key neither read nor advanced, logp untouched
    key = torch.from_numpy(key_np.copy()).cuda()
    det = _act(h, torch.from_numpy(x[:97]).cuda(), td, key, 97, 0, det=True, logp_fill=-7.0)
    a_det, _, raw_det = ref_head(host, logits[:97], np.zeros((97, A), np.float32), deterministic=True)
    assert torch.equal(det["action"], torch.from_numpy(a_det)) and torch.equal(det["raw"], torch.from_numpy(raw_det))
    assert torch.equal(det["raw"], torch.from_numpy(logits[:97, :A]))
    assert (det["logp"] == -7.0).all() and np.array_equal(key.cpu().numpy(), key_np)


def test_noise_statistics_and_logp():
    """2^20 draws: mean and variance of eps within 5 sigma (sigma_mean = 1 / sqrt N, sigma_var =
    sqrt(2 / N) for a unit normal), every sample finite; logp against torch's float64
    Normal(loc, scale).log_prob(raw) - log(1 - tanh^2), bounded by 4 x the error of the same
    expression in torch float32 + 1e-6, on rows with every |raw| <= 4."""
    B, D = 1 << 17, 6
    N = B * A
    rng = np.random.default_rng(3)
    sizes = [D, 2 * A]
    x, theta = random_net(sizes, rng, B)
    h = _handle(sizes, 1)
    key = torch.from_numpy(np.asarray(pob_np.prngkey(99), np.uint32)).cuda()
    got = _act(h, torch.from_numpy(x).cuda(), torch.from_numpy(theta).cuda(), key, B, 0)
    for k in ("action", "raw", "logp", "logits"):
        assert torch.isfinite(got[k]).all(), k
    logits, raw = got["logits"].double(), got["raw"].double()
    loc, scale = logits[:, :A], torch.nn.functional.softplus(logits[:, A:]) + 0.001
    eps = (raw - loc) / scale
    mean, var = float(eps.mean()), float(eps.var())
    print(f"eps: N = {N}  mean {mean:.3e} (bound {5 / np.sqrt(N):.3e})  var - 1 {var - 1:.3e} (bound {5 * np.sqrt(2 / N):.3e})")
    assert abs(mean) <= 5 / np.sqrt(N) and abs(var - 1) <= 5 * np.sqrt(2 / N)

    def logp_of(dtype):
        lo, sc, rw = loc.to(dtype), (torch.nn.functional.softplus(got["logits"][:, A:].to(dtype)) + 0.001), got["raw"].to(dtype)
        lp = torch.distributions.Normal(lo, sc).log_prob(rw) - torch.log(1 - torch.tanh(rw) ** 2)
        return lp.sum(-1)

    rows = (got["raw"].abs() <= 4).all(-1)
    assert int(rows.sum()) > B // 2
    exact = logp_of(torch.float64)[rows]
    e_torch = float((logp_of(torch.float32)[rows].double() - exact).abs().max())
    e_ours = float((got["logp"][rows].double() - exact).abs().max())
    print(f"logp: rows {int(rows.sum())}  ours {e_ours:.3e}  torch f32 {e_torch:.3e}")
    assert e_ours <= 4 * e_torch + 1e-6


def _policy(env, seed=5):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_models(2 * env.action_size, env.observation_size)[0]
    params = model.init(jumpy.random_prngkey(seed))
    params.theta.mul_(3.0)  # livelier actions than the init's
    return networks.NormalTanhPolicy(model, params, jumpy.random_prngkey(seed + 1))


@pytest.mark.parametrize("name", ["ant_heavenhell", "ant_tag"])
def test_rollouts_equal_eager(name):
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout, PolicyRollout
    from test_gpu_parity import _keys
    B, T = 512, 6
    keys = torch.from_numpy(_keys(B, 3)).cuda()
    es = [envs.create(name, batch_size=B, episode_length=4) for _ in range(3)]
    ss = [e.reset(keys) for e in es]
    ps = [_policy(e) for e in es]
    done_of = lambda s: s.aux["done"] if "done" in s.aux else s.done  # noqa: E731
    # PolicyRollout's warm-up calls the policy (twice) before the capture, which advances its
    # key: the eager loop and the ActorRollout start from the key it is left with
    k0 = ps[1].key.clone()
    pr = PolicyRollout(es[1], ss[1], ps[1], T)
    torch.cuda.synchronize()
    assert torch.equal(ps[1].key, jumpy.random_split(jumpy.random_split(k0)[0])[0])
    ps[0].key.copy_(ps[1].key); ps[2].key.copy_(ps[1].key)
    # eager: 2 T steps
    traj = {k: [] for k in ("obs", "actions", "logp", "raw", "reward", "done")}
    s = ss[0]
    for t in range(2 * T):
        traj["obs"].append(s.obs.clone())
        a = ps[0](s.obs)
        traj["actions"].append(a.clone()); traj["logp"].append(ps[0].logp.clone()); traj["raw"].append(ps[0].raw.clone())
        s = es[0].step_(s, traj["actions"][-1])
        traj["reward"].append(s.reward.clone()); traj["done"].append(done_of(s).float().clone())
    traj = {k: torch.stack(v) for k, v in traj.items()}
    assert traj["done"].any() and not traj["done"].all()  # autoresets fall inside
    ar = ActorRollout(es[2], ss[2], ps[2], T)
    for rep in range(2):
        sl = slice(rep * T, (rep + 1) * T)
        pr.replay(); ar.replay()
        torch.cuda.synchronize()
        for k in ("obs", "actions", "reward", "done"):
            assert torch.equal(getattr(pr, k), traj[k][sl]), (name, "PolicyRollout", k, rep)
            assert torch.equal(getattr(ar, k), traj[k][sl]), (name, "ActorRollout", k, rep)
        assert torch.equal(ar.logp, traj["logp"][sl]) and torch.equal(ar.raw, traj["raw"][sl])
    assert torch.equal(ss[0].obs, pr.state.obs) and torch.equal(ss[0].obs, ar.state.obs)
    assert torch.equal(ss[0].qp.pos, ar.state.qp.pos)
    # the parameters are read at replay time: an in-place edit changes the next replay's actions
    before = ar.actions.clone()
    obs0 = ar.state.obs.clone()
    ps[2].theta.mul_(0.5)
    ar.replay()
    torch.cuda.synchronize()
    assert torch.equal(ar.obs[0], obs0) and not torch.equal(ar.actions, before)
    ps[0].theta.mul_(0.5)
    assert torch.equal(ps[0](obs0), ar.actions[0])
