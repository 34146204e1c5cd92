"""GPU: k_gru_seq_infer (``pob_gru_sequence_forward``) against the host restatement
(gru_sequence_forward_ref), against chained ``pob_gru_forward_norm`` launches on the device, and
against the chained host step and the training forward's ``y`` -- all bitwise, with the aliasing and
guard-row checks of test_gru_seq_infer_host.py (its ``check_window``).

Shapes: S in {1, 3, 21} and M in {1, 31, 33, 70} (one row, both sides of the 32-row tile, three tiles)
for the critic's networks; per shape four variants that together take every level of idx (none / a
permutation with a repeated env), the normaliser (off / on) and the reset rows (none / a tenth / a NaN
entry / a -0.0 entry).  The pool template is chosen by rows = I + 2 H + P0 + P1 (thresholds 96, 160,
248, 408, 616, 896): the networks below land in every template, and three fill theirs to the last row.
One case each of ``pob_gru_sequence_forward_train`` and ``pob_gru_sequence_backward`` at out width 1, of
which the critic is the first user."""
import numpy as np
import pytest
import torch

from test_gru_bwd_host import SWISH, build_gru_bwd_host, problem as bwd_problem, same_bits
from test_gru_seq_infer_host import CANARY, GUARD, NETS as HOST_NETS, build_seq_infer_host, check_window, host_runner, problem

pytestmark = pytest.mark.gpu

NETS = dict(HOST_NETS, **{"114-gru64-1": ([114], 64, [1])})  # pool rows 18, 159, 213; 243
# (net, pool rows, template): every template, and the ones filled to their last row
TEMPLATE_NETS = {
    "5-gru45-1": (([5], 45, [1]), 96, 96),
    "31-gru64-1": (([31], 64, [1]), 160, 160),
    "32-gru64-1": (([32], 64, [1]), 161, 248),
    "119-gru64-1": (([119], 64, [1]), 248, 248),
    "200-gru56-1": (([200], 56, [1]), 313, 408),
    "250-100-gru100-1": (([250, 100], 100, [1]), 550, 616),
    "256-128-gru128-256-1": (([256, 128], 128, [256, 1]), 641, 896),
}
VARIANTS = [(False, False, "none"), (True, True, "tenth"), (False, True, "nan"), (True, False, "negzero")]


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gru_seq_infer_gpu")
    return build_seq_infer_host(d), build_gru_bwd_host(d)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pool_rows(net):
    """I + 2 H + P0 + P1 by gru_tile_forward's walk (gru_plan of csrc/pob_mlp.hip)."""
    pre, H, post = net
    w, pp = [0, 0], 0
    if len(pre) > 1:
        w[0], pp = pre[0], 1
    for l in range(len(pre) - 1):
        if l != len(pre) - 2:
            w[pp] = max(w[pp], pre[l + 1])
        pp ^= 1
    for width in post:
        w[pp] = max(w[pp], width)
        pp ^= 1
    return pre[-1] + 2 * H + w[0] + w[1]


def device_runner():
    """``host_runner``'s contract on the kernel: every output with GUARD canary rows behind it."""
    from po_brax_amd import _lib
    from po_brax_amd._lib import check, lib, ptr
    from po_brax_amd.training.networks import GRUHandle
    handles = {}

    def run(pb, h_out_step, alias=False):
        pre, H, post = pb["net"]
        S, M, B = pb["S"], pb["M"], pb["B"]
        key = (tuple(pre), H, tuple(post), pb["act"])
        gru = handles.setdefault(key, GRUHandle(pre, H, post, pb["act"]))
        y = torch.full((S * M * post[-1] + GUARD,), float(CANARY), device="cuda")
        h_first, h_out = (torch.full((M + GUARD, H), float(CANARY), device="cuda") for _ in range(2))
        h0 = _cuda(pb["h0"])
        obs, idx, reset, theta, norm = (_cuda(pb[k]) for k in ("obs", "idx", "reset", "theta", "norm"))
        check(lib.pob_gru_sequence_forward(gru.handle, S, M, B, ptr(obs), ptr(idx), ptr(h0), ptr(reset), ptr(theta), ptr(y),
                                           ptr(h_first), ptr(h0 if alias else h_out), h_out_step, ptr(norm), pb["clip"],
                                           _lib.stream_handle(obs.device)))
        torch.cuda.synchronize()
        out = h0 if alias else h_out
        return dict(y=y.cpu().numpy(), h_first=h_first.cpu().numpy(), h_out=out.cpu().numpy(), h0_after=h0.cpu().numpy())

    run.handles = handles
    return run


def device_chain(run, pb):
    """y (S, M, out) and the last state of S chained ``pob_gru_forward_norm`` launches on the gathered rows."""
    from po_brax_amd import _lib
    from po_brax_amd._lib import check, lib, ptr
    pre, H, post = pb["net"]
    S, M = pb["S"], pb["M"]
    gru = run.handles[(tuple(pre), H, tuple(post), pb["act"])]
    sel = torch.arange(M, device="cuda") if pb["idx"] is None else _cuda(pb["idx"]).long()
    obs, theta, norm = _cuda(pb["obs"]), _cuda(pb["theta"]), _cuda(pb["norm"])
    reset = _cuda(pb["reset"])
    h = _cuda(pb["h0"])[sel].contiguous()
    y = torch.empty((S, M, post[-1]), device="cuda")
    for s in range(S):
        x = obs[s, sel].contiguous()
        rs = None if reset is None else reset[s, sel].contiguous()
        check(lib.pob_gru_forward_norm(gru.handle, M, ptr(x), ptr(theta), ptr(rs), ptr(h), ptr(y[s]), None, ptr(norm),
                                       pb["clip"], _lib.stream_handle(x.device)))
    torch.cuda.synchronize()
    return y.cpu().numpy(), h.cpu().numpy()


def _check(libs, run, pb):
    lib, bwd = libs
    outs = check_window(run, bwd, pb)  # the host chain, the training forward's y, aliasing, guard rows
    S, M = pb["S"], pb["M"]
    n_y = S * M * pb["net"][2][-1]
    want = host_runner(lib)(pb, S)      # the specification
    for k in ("y", "h_first", "h_out"):
        assert same_bits(outs[S][k], want[k]), f"{k} against gru_sequence_forward_ref"
    y_d, h_d = device_chain(run, pb)    # chained launches of the existing step kernel
    assert same_bits(outs[S]["y"][:n_y], y_d.reshape(-1)) and same_bits(outs[S]["h_out"][:M], h_d)


@pytest.mark.parametrize("M", [1, 31, 33, 70])
@pytest.mark.parametrize("S", [1, 3, 21])
@pytest.mark.parametrize("name", list(NETS))
def test_kernel_is_the_restatement_and_the_chain(libs, name, S, M):
    run = device_runner()
    for v, (use_idx, use_norm, kind) in enumerate(VARIANTS):
        _check(libs, run, problem(100 * S + M + 7 * v, NETS[name], S, M, use_idx, use_norm, kind))


@pytest.mark.parametrize("name", list(TEMPLATE_NETS))
def test_every_pool_template(libs, name):
    """Networks on both sides of every template threshold, three of them filling the pool to its last
    row: S = 3, M = 33 (a full tile and a one-row tail), idx, a normaliser and resets."""
    net, rows, template = TEMPLATE_NETS[name]
    assert pool_rows(net) == rows and rows <= template
    assert min(t for t in (96, 160, 248, 408, 616, 896) if rows <= t) == template
    _check(libs, device_runner(), problem(11, net, 3, 33, True, True, "tenth"))


def test_critic_networks_pool_rows():
    assert [pool_rows(n) for n in NETS.values()] == [18, 159, 213, 243]


def test_argument_errors_leave_the_outputs_alone():
    """A refused call writes nothing (the checks come before any HIP call)."""
    from po_brax_amd._lib import POB_EINVAL, lib, ptr
    from po_brax_amd.training.networks import GRUHandle
    gru = GRUHandle([7], 5, [1], SWISH)
    obs, h0, theta = torch.zeros((2, 4, 7), device="cuda"), torch.zeros((4, 5), device="cuda"), torch.zeros(
        gru.param_count, device="cuda")
    y = torch.full((2, 4), float(CANARY), device="cuda")
    for S, step, yy in ((0, 1, y), (2, 0, y), (2, 3, y), (2, 1, None)):
        assert lib.pob_gru_sequence_forward(gru.handle, S, 4, 4, ptr(obs), None, ptr(h0), None, ptr(theta), ptr(yy), None,
                                            None, step, None, 0.0, None) == POB_EINVAL
    torch.cuda.synchronize()
    assert bool((y == float(CANARY)).all())


def test_training_kernels_at_out_width_one(libs):
    """``pob_gru_sequence_forward_train`` and ``pob_gru_sequence_backward`` at 30 -> GRU 64 -> 1, T = 3,
    M = 33, against their restatements (the ``Seq`` harness of test_gpu_gru_bwd.py): y, h_last, saved,
    dtheta, dh0 and the delta arrays in integer views."""
    from test_gpu_gru_bwd import Seq
    _, bwd = libs
    net, T, M = HOST_NETS["30-gru64-1"], 3, 33
    rng = np.random.default_rng(31)
    pr = bwd_problem(rng, net, T, M)
    dh_last = (rng.standard_normal((M, net[1])) / M).astype(np.float32)
    s = Seq(net, SWISH, T, M, M)
    s.load(pr, None, pr["reset"], dh_last)
    s.run()
    s.check(bwd, SWISH, pr, "out width 1", None, pr["reset"], dh_last)
