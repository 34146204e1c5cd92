"""GPU: the row-indexed training pass (``apply_native(idx=, normalizer=)``: pob_mlp_*_rows, DESIGN.md "Row-indexed
training pass") against the existing pass on the materialised rows ``norm.apply(x[idx])``, bit for bit, and against
float64 torch ops within the bound of tests/test_gpu_mlp_bwd.py; the learners' ``rows="in_place"``; one captured graph."""
import types

import numpy as np
import pytest
import torch

from test_mlp_bwd_host import SWISH, check_against_float64, make_problem, within_bound

pytestmark = pytest.mark.gpu

NETS = {"small": [5, 7, 6, 2], "critic": [114, 256, 1]}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _problem(sizes, M, N, with_idx, with_norm, seed):
    """x (N, D), theta, dy on the device; idx holding row 0, row N - 1 and a duplicate where M allows (None: every
    row, M = N); a loaded normaliser or None."""
    from po_brax_amd.training.normalization import ObservationNormalizer
    rng = np.random.default_rng(seed)
    x, theta, dy = make_problem(rng, sizes, max(N, M))
    idx = norm = None
    if with_idx:
        idx = rng.permutation(N)[np.arange(M) % N].astype(np.int32)
        idx[[0, M // 2, -1]] = 0, N - 1, N - 1
        idx = torch.from_numpy(idx).cuda()
    if with_norm:
        norm = ObservationNormalizer(sizes[0])
        table = np.stack([rng.standard_normal(sizes[0]), rng.uniform(0.5, 4.0, sizes[0]), np.ones(sizes[0])])
        norm.load_state_dict({"table": torch.from_numpy(table.astype(np.float32)),
                              "count": torch.tensor([1000.0], dtype=torch.float64), "clip": 2.5})
    rows = M if with_idx else N
    return torch.from_numpy(x[:N]).cuda(), torch.from_numpy(theta).cuda(), torch.from_numpy(dy[:rows]).cuda(), idx, norm


@pytest.mark.parametrize("N_of", ["M", "3M+1"])
@pytest.mark.parametrize("M", [1, 31, 33, 65, 129])
@pytest.mark.parametrize("with_idx", [False, True], ids=["all", "idx"])
@pytest.mark.parametrize("with_norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("kernel", ["tile", "resident"])
def test_rows_pass_equals_the_pass_on_materialised_rows(kernel, net, with_norm, with_idx, M, N_of):
    from po_brax_amd.training import make_model
    sizes = NETS[net]
    N = M if N_of == "M" else 3 * M + 1
    x, theta, dy, idx, norm = _problem(sizes, M, N, with_idx, with_norm, 1000 * M + N)
    model = make_model(sizes[1:], sizes[0])
    rows = x if idx is None else x.index_select(0, idx)
    rows = rows if norm is None else norm.apply(rows)
    got, want = (theta.clone().requires_grad_(True) for _ in range(2))
    y = model.apply_native(types.SimpleNamespace(theta=got), x, kernel=kernel, idx=idx, normalizer=norm)
    y.backward(dy)
    y_want = model.apply_native(types.SimpleNamespace(theta=want), rows, kernel=kernel)  # the existing pass
    y_want.backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(y_want)) and torch.equal(_bits(got.grad), _bits(want.grad))
    # float64 torch ops of the same function: the bound of test_gpu_mlp_bwd.py (test_mlp_bwd_host.within_bound)
    r, th = rows.cpu().numpy(), theta.cpu().numpy()
    check_against_float64(sizes, SWISH, 0, r, th, dy.cpu().numpy(), got.grad.cpu().numpy(), None, "rows")
    y32, y64 = (model.apply(types.SimpleNamespace(theta=torch.from_numpy(th).to(t)), torch.from_numpy(r).to(t)).numpy()
                for t in (torch.float32, torch.float64))
    within_bound(y.detach().cpu().numpy(), y32, y64, "rows y")


def _learner_thetas(rows):
    """Both theta vectors before and after one update at T B = 4 x 64, 2 minibatches, 1 epoch."""
    from po_brax_amd import jumpy
    from po_brax_amd.training import PPOLearner
    from test_gpu_learner import real_rollout
    roll, policy, critic = real_rollout(0, update_normalizer=False, loaded=True)
    learner = PPOLearner(policy, critic, learning_rate=1e-2, num_minibatches=2, num_update_epochs=1,
                         key=jumpy.random_prngkey(7), backward=("native", "resident"), rows=rows)
    roll.replay()
    before = policy.theta.clone(), critic.theta.clone()
    learner.update(roll)
    torch.cuda.synchronize()
    return before, (policy.theta.clone(), critic.theta.clone())


def test_learner_in_place_equals_the_gather_route():
    (b0, want), (b1, got) = _learner_thetas("gather"), _learner_thetas("in_place")
    for k in range(2):
        assert torch.equal(_bits(b0[k]), _bits(b1[k])) and not torch.equal(_bits(got[k]), _bits(b1[k]))
        assert torch.equal(_bits(got[k]), _bits(want[k]))


def test_captured_graph_sees_theta_and_idx_in_place():
    from po_brax_amd.training import make_model
    sizes, M, N = NETS["critic"], 96, 289
    x, theta, dy, idx, norm = _problem(sizes, M, N, True, True, 5)
    model = make_model(sizes[1:], sizes[0])
    theta.requires_grad_(True)

    def run(**kw):
        theta.grad = None
        y = model.apply_native(types.SimpleNamespace(theta=theta), x, kernel="resident", **kw)
        y.backward(dy)
        return y.detach(), theta.grad

    run(idx=idx, normalizer=norm)  # loads the modules before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(idx=idx, normalizer=norm)
    for rep in range(2):
        _, new_theta, _, new_idx, _ = _problem(sizes, M, N, True, True, 50 + rep)
        with torch.no_grad():  # in place: the graph reads the same addresses
            theta.copy_(new_theta)
            idx.copy_(new_idx)
        graph.replay()
        got = [t.clone() for t in out]
        for g, w in zip(got, run(idx=idx, normalizer=norm)):
            assert torch.equal(_bits(g), _bits(w)), rep
