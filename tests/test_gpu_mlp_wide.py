"""GPU: the wide forward (pob_mlp_forward_wide / _norm, ``kernel="resident"``) equals the plain-C restatement and the
one-wave kernel bit for bit, sees theta in place from a captured graph, and serves an actor rollout's critic pass."""
import numpy as np
import pytest
import torch

from test_mlp_host import NETS, build_host, random_net, ref_forward

pytestmark = pytest.mark.gpu

# beside NETS: odd `in`, tile + 1 widths and a last width of 1; a wave holding two tiles; one layer; eight layers
WIDE_NETS = NETS + [([7, 33, 65, 1], False), ([114, 160, 256, 256, 1], False), ([256, 256], False), ([40] * 9, False)]
CRITIC = [114, 256, 256, 256, 256, 256, 1]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("mlp_host_wide"))


def _forward(entry, sizes, act, act_final, x, theta, *norm):
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import MLPHandle
    h = MLPHandle(sizes, act, act_final)
    y = torch.full((x.shape[0], sizes[-1]), float("nan"), device="cuda")
    _lib.check(getattr(_lib.lib, entry)(h.handle, x.shape[0], x.data_ptr(), theta.data_ptr(), y.data_ptr(), *norm,
                                        _lib.stream_handle(x.device)))
    return y.cpu()


def _rows(k, extra):
    from po_brax_amd._lib import MLP_WIDE_ROWS
    return k * MLP_WIDE_ROWS + extra


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("net", range(len(WIDE_NETS)))
def test_wide_forward_bit_exact(host, net, act):
    sizes, act_final = WIDE_NETS[net]
    batches = (1, 31, _rows(1, -1), _rows(1, 0), _rows(1, 1), _rows(2, 33))
    x, theta = random_net(sizes, np.random.default_rng(2000 + 10 * net + act), max(batches))
    want = torch.from_numpy(ref_forward(host, sizes, act, act_final, x, theta))  # rows are independent: one reference
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(theta).cuda()
    for B in batches:
        got = _forward("pob_mlp_forward_wide", sizes, act, act_final, xd[:B].contiguous(), td)
        assert torch.equal(got, want[:B]), (sizes, act, B, float((got - want[:B]).abs().max()))


def test_wide_forward_layout_exact_integers():
    """test_forward_layout_exact_integers' network over 3 R + 5 rows: a misplaced row or feature is a wrong integer."""
    n, m, B = 40, 37, _rows(3, 5)
    W1 = np.arange(n)[:, None] + 100 * np.arange(m)[None, :]
    b1 = np.arange(m) - 5
    theta = np.concatenate([np.eye(n).ravel(), np.zeros(n), W1.ravel(), b1]).astype(np.float32)
    x = np.random.default_rng(0).integers(0, 8, (B, n))
    got = _forward("pob_mlp_forward_wide", [n, n, m], 0, False, torch.from_numpy(x.astype(np.float32)).cuda(),
                   torch.from_numpy(theta).cuda())
    assert np.array_equal(got.numpy().astype(np.int64), x @ W1 + b1)


@pytest.mark.parametrize("B", [(1, 1), (0, 2049)])
def test_wide_norm_equals_tile_norm(B):
    rng = np.random.default_rng(7)
    x, theta = random_net(CRITIC, rng, _rows(*B))
    table = torch.from_numpy(np.stack([rng.uniform(-1, 1, 114), rng.uniform(0.2, 3, 114), np.ones(114)]).astype(np.float32)).cuda()
    args = (CRITIC, 1, False, torch.from_numpy(x).cuda(), torch.from_numpy(theta).cuda(), table.data_ptr(), 2.5)
    assert torch.equal(_forward("pob_mlp_forward_wide_norm", *args), _forward("pob_mlp_forward_norm", *args))


def test_resident_graph_sees_theta_in_place():
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_model([256, 256, 1], 114)
    p = model.init(jumpy.random_prngkey(3))
    x = torch.rand((200, 114), device="cuda") * 2 - 1
    model.apply(p, x, kernel="resident")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = model.apply(p, x, kernel="resident")
    for scale in (1.0, 0.5, 3.0):  # replay, change theta in place, replay: every replay equals the eager one-wave forward
        p.theta.mul_(scale)
        g.replay()
        assert torch.equal(y, model.apply(p, x, kernel="tile"))


def test_resident_critic_through_the_rollout():
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import ValueFunction, networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    from test_gpu_parity import _keys
    B, T, rolls = 96, 3, []
    keys = torch.from_numpy(_keys(B, 3)).cuda()
    for kernel in ("resident", "tile"):
        env = envs.create("ant_tag", batch_size=B, episode_length=4)
        norm = ObservationNormalizer(env.observation_size)
        pm, vm = networks.make_models(2 * env.action_size, env.observation_size)
        policy = networks.NormalTanhPolicy(pm, pm.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6), normalizer=norm)
        critic = ValueFunction(vm, vm.init(jumpy.random_prngkey(9)), normalizer=norm, kernel=kernel)
        rolls.append(ActorRollout(env, env.reset(keys), policy, T, update_normalizer=True, critic=critic))
    for rep in range(2):
        for r in rolls:
            r.replay()
        torch.cuda.synchronize()
        for k in ("values", "vs", "advantages"):
            assert torch.equal(getattr(rolls[0], k), getattr(rolls[1], k)), (k, rep)
    assert bool(torch.isfinite(rolls[0].values).all()) and bool(rolls[0].values.any())
