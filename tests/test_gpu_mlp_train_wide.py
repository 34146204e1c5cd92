"""GPU: the wide training pass (pob_mlp_forward_train_wide / pob_mlp_backward_wide, ``kernel="resident"``) equals the
plain-C restatement (mlp_forward_train_ref / mlp_backward_ref of csrc/pob_mlp.h) bit for bit, and the one-wave
kernels through ``apply_native`` and ``PPOLearner``."""
import types

import numpy as np
import pytest
import torch

from test_gpu_mlp_bwd import B_ROLL, N_MINI, T_ROLL, Buffers, _bits, _cuda, _same_bits
from test_mlp_bwd_host import RELU, SWISH, TANH, host, integer_problem, make_problem, ref_train_and_back  # noqa: F401 (host: a fixture)

pytestmark = pytest.mark.gpu

# every wave assignment: one tile, two tiles (a wave per pair), two tiles a wave, five tiles, a single layer, depth
NETS = {"single": [3, 1], "odd": [27, 33, 16], "wide": [40, 256, 255, 1], "five": [114, 160, 256, 256, 1],
        "layer": [256, 256], "deep": [40] * 9}
CRITIC = [114, 256, 256, 256, 256, 256, 1]


class WideBuffers(Buffers):
    """``Buffers`` (NaN-filled saved, workspace and outputs) run through the two wide entry points."""
    def run(self):
        from po_brax_amd import _lib
        from po_brax_amd._lib import check, lib, ptr
        st, saved = _lib.stream_handle(self.x.device), ptr(self.saved) if self.saved.numel() else None
        check(lib.pob_mlp_forward_train_wide(self.mlp.handle, self.M, ptr(self.x), ptr(self.theta), ptr(self.y), saved, st))
        check(lib.pob_mlp_backward_wide(self.mlp.handle, self.M, ptr(self.x), ptr(self.theta), saved, ptr(self.dy),
                                        ptr(self.dtheta), ptr(self.dx), ptr(self.workspace), st))


ROWS = [1, 63, 64, 65, 129, 1025]  # the tail on either side of one block, three blocks, a second weights chunk
CASES = [(n, M, 0, True) for n in NETS for M in ROWS] + [("odd", 65, 1, True), ("single", 65, 0, False), ("five", 65, 0, False)]


@pytest.mark.parametrize("net,M,fin,want_dx", CASES)
def test_wide_kernels_equal_restatement(host, net, M, fin, want_dx):
    """y, saved, dtheta and dx (the last two CASES: NULL dx) against the restatement, bit for bit."""
    for act in (RELU, SWISH, TANH):
        x, theta, dy = make_problem(np.random.default_rng(100 * M + act), NETS[net], M)
        b = WideBuffers(NETS[net], act, fin, M, want_dx)
        b.load(x, theta, dy)
        b.run()
        b.check(ref_train_and_back(host, NETS[net], act, fin, x, theta, dy, want_dx), (net, M, act))


def test_integer_layout():
    x, theta, dy, want_y, want_dtheta, want_dx = integer_problem(np.random.default_rng(35), 35, 37, 70)
    b = WideBuffers([35, 37], SWISH, 0, 70)
    b.load(x, theta, dy)
    b.run()
    torch.cuda.synchronize()
    for got, want in ((b.y, want_y), (b.dtheta, want_dtheta), (b.dx, want_dx)):
        _same_bits(got, want, "integer layout")


def _critic_problem(seed, M=65):
    """The critic's network with leaf tensors for theta, x and dy, and one forward + backward of them."""
    from po_brax_amd.training import make_model
    model = make_model(CRITIC[1:], CRITIC[0])
    x, theta, dy = (_cuda(a) for a in make_problem(np.random.default_rng(seed), CRITIC, M))
    theta.requires_grad_(True)
    x.requires_grad_(True)

    def run(kernel):
        theta.grad = x.grad = None
        y = model.apply_native(types.SimpleNamespace(theta=theta), x, kernel=kernel)
        y.backward(dy)
        return y.detach(), theta.grad, x.grad

    return run, (theta, x, dy)


def test_apply_native_resident_equals_tile_eager_and_in_one_graph():
    run, leaves = _critic_problem(22)
    for g, w in zip(run("resident"), run("tile")):  # also loads the modules before the capture
        assert g is not w and torch.equal(_bits(g), _bits(w))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run("resident")
    for rep in range(3):
        x, theta, dy = make_problem(np.random.default_rng(30 + rep), CRITIC, 65)
        with torch.no_grad():  # in place: the graph reads the same addresses
            for leaf, new in zip(leaves, (theta, x, dy)):
                leaf.copy_(_cuda(new))
        graph.replay()
        got = [t.clone() for t in out]
        for g, w in zip(got, run("tile")):
            assert torch.equal(_bits(g), _bits(w)), rep


def _two_rounds(backward):
    """Both theta vectors after two rounds of replay(); update(roll) on ant_heavenhell from fixed keys."""
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import PPOLearner, ValueFunction, networks
    from test_gpu_parity import _keys
    env = envs.create("ant_heavenhell", batch_size=B_ROLL, episode_length=3)
    state = env.reset(torch.from_numpy(_keys(B_ROLL, 3)).cuda())
    p_model, v_model = networks.make_models(2 * env.action_size, env.observation_size)
    policy = networks.NormalTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6))
    critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)))
    roll = ActorRollout(env, state, policy, T_ROLL, critic=critic)
    learner = PPOLearner(policy, critic, learning_rate=1e-2, num_minibatches=N_MINI, num_update_epochs=1,
                         key=jumpy.random_prngkey(7), backward=backward)
    for _ in range(2):
        roll.replay()
        learner.update(roll)
    return policy.theta.clone(), critic.theta.clone()


def test_learner_resident_equals_native():
    want, got = _two_rounds("native"), _two_rounds(("native", "resident"))
    for g, w in zip(got, want):
        assert bool(torch.isfinite(g).all()) and torch.equal(_bits(g), _bits(w))
    assert not torch.equal(_bits(got[1]), _bits(_two_rounds(("native", "torch"))[1]))  # the value half did run natively
