"""GPU: the bf16 forward (``kernel="bf16"``) against its float64 definition: exact on small integers, within TOL on random
networks; the pack pass inside a captured graph; the critic of an actor rollout."""
import numpy as np
import pytest
import torch

from test_mlp_bf16_api import TOL, metric, reference

pytestmark = pytest.mark.gpu

CRITIC = [114, 256, 256, 256, 256, 256, 1]
# odd `in`, tile + 1 widths and a last width of 1; a wave holding two tiles; one layer; eight layers
RANDOM_NETS = [[7, 33, 65, 1], [114, 160, 256, 256, 1], [256, 256], [40] * 9]


def _forward(sizes, act, x, theta, *norm):
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import MLPHandle, bf16_workspace
    h = MLPHandle(sizes, act, False)
    ws = bf16_workspace(h, "cuda")
    y = torch.full((x.shape[0], sizes[-1]), float("nan"), device="cuda")
    entry = _lib.lib.pob_mlp_forward_bf16_norm if norm else _lib.lib.pob_mlp_forward_bf16
    _lib.check(entry(h.handle, x.shape[0], x.data_ptr(), theta.data_ptr(), y.data_ptr(), *norm, ws.data_ptr(),
                     _lib.stream_handle(x.device)))
    return y.cpu()


@pytest.mark.parametrize("sizes", [[7, 33, 65, 1], [114, 256, 256, 1], [40] * 6])
def test_bf16_layout_exact_integers(sizes):
    """Every value an integer below 256, exact in bf16 and in f32 sums of any order: a wrong index, pad or tail shows."""
    rng = np.random.default_rng(len(sizes) * 1000 + sizes[1])
    parts = []
    for n_in, n_out in zip(sizes[:-1], sizes[1:]):
        W = np.zeros((n_in, n_out))
        for j in range(n_out):
            W[rng.integers(0, n_in, 2), j] = rng.choice([-1.0, 1.0], 2)
        parts += [W.ravel(), rng.integers(-2, 3, n_out)]
    theta = torch.from_numpy(np.concatenate(parts).astype(np.float32))
    x = torch.from_numpy(rng.integers(-3, 4, (161, sizes[0])).astype(np.float32))
    want = reference(sizes, 0, x, theta, hidden := [])
    assert all(bool((h == h.round()).all()) and float(h.abs().max()) <= 158 for h in hidden)
    xd, td = x.cuda(), theta.cuda()
    for B in (1, 63, 64, 65, 161):
        assert torch.equal(_forward(sizes, 0, xd[:B].contiguous(), td), want[:B].float()), B


@pytest.mark.parametrize("act", ["relu", "swish", "tanh"])
@pytest.mark.parametrize("net", range(len(RANDOM_NETS)))
def test_bf16_random_networks(net, act):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    sizes = RANDOM_NETS[net]
    model = networks.make_model(sizes[1:], sizes[0], activation=act)
    p = model.init(jumpy.random_prngkey(20 + net))
    x = torch.randn((161, sizes[0]), generator=torch.Generator().manual_seed(net))
    want = reference(sizes, model.activation, x, p.theta.cpu())  # rows are independent: one reference
    for B in (1, 65, 161):
        err = metric(model.apply(p, x[:B].cuda(), kernel="bf16").cpu(), want[:B])
        print(f"bf16 {sizes} {act} B={B}: {err:.3e}")
        assert err <= TOL, (sizes, act, B, err)


def test_bf16_norm():
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    rng = np.random.default_rng(7)
    model = networks.make_model(CRITIC[1:], 114)
    p = model.init(jumpy.random_prngkey(3))
    x = torch.randn((65, 114), generator=torch.Generator().manual_seed(9))
    table = torch.from_numpy(np.stack([rng.uniform(-1, 1, 114), rng.uniform(0.2, 3, 114), np.ones(114)]).astype(np.float32))
    xn = torch.clamp((x - table[0]) * table[1], -2.5, 2.5)  # pob_obsnorm_apply: one f32 subtract, one f32 multiply, the clamp
    td = table.cuda()
    err = metric(_forward(CRITIC, model.activation, x.cuda(), p.theta, td.data_ptr(), 2.5),
                 reference(CRITIC, model.activation, xn, p.theta.cpu()))
    print(f"bf16 norm: {err:.3e}")
    assert err <= TOL, err


def test_bf16_critic_in_a_captured_graph_and_through_the_rollout():
    """theta changed in place between replays (a hoisted pack pass would keep the old weights); then an ActorRollout's critic."""
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import ValueFunction, networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    from test_gpu_parity import _keys
    B, T = 96, 3
    env = envs.create("ant_tag", batch_size=B, episode_length=4)
    norm = ObservationNormalizer(env.observation_size)
    pm, vm = networks.make_models(2 * env.action_size, env.observation_size)
    critic = ValueFunction(vm, vm.init(jumpy.random_prngkey(9)), normalizer=norm, kernel="bf16")
    rows, y = torch.rand((B, env.observation_size), device="cuda") * 2 - 1, torch.empty((B,), device="cuda")
    critic.values_into(rows, y)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        critic.values_into(rows, y)
    for scale in (0.5, 3.0):
        before = y.clone()
        critic.theta.mul_(scale)
        g.replay()
        assert torch.equal(y, critic(rows)) and not torch.equal(y, before), scale
    policy = networks.NormalTanhPolicy(pm, pm.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6), normalizer=norm)
    roll = ActorRollout(env, env.reset(torch.from_numpy(_keys(B, 3)).cuda()), policy, T, critic=critic)
    for rep in range(2):
        roll.replay()
        torch.cuda.synchronize()
        assert torch.equal(roll.values, critic(torch.cat([roll.obs, roll.final_obs[None]]))), rep
    assert bool(torch.isfinite(roll.values).all()) and bool(roll.values.any())
