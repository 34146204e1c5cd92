"""GPU: the recurrent training forward and truncated-BPTT backward kernels
(pob_gru_sequence_forward_train / pob_gru_sequence_backward) against the plain-C restatement
(gru_sequence_forward_train_ref / gru_sequence_backward_ref of csrc/pob_mlp.h, built for the host by
tests/host/gru_bwd_host.cpp), in integer views: y, h_last, what the forward saved, dtheta, dh0, the
delta arrays; ``apply_sequence_native`` on top of them, and the window of a real
``RecurrentActorRollout`` replay."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gru_bwd_host import (NETS as HOST_NETS, RELU, SWISH, TANH, build_gru_bwd_host, layout, param_count, problem,
                               ref_backward, ref_forward)

pytestmark = pytest.mark.gpu

NETS = dict(HOST_NETS, **{"128-gru128-16": ([128], 128, [16])})
SHAPES = [(1, 1), (2, 31), (5, 32), (5, 33), (3, 65), (33, 32), (2, 1025)]  # (33, 32) crosses a 1024-row chunk
SENTINEL = 12345.5


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_gru_bwd_host(tmp_path_factory.mktemp("gru_bwd_host"))


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(got, want, what):
    want = _cuda(np.ascontiguousarray(want, np.float32)).reshape(got.shape)
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())


def _guarded(n, tail=64):
    """(the first n floats, the whole buffer): ``tail`` sentinel floats lie behind the array."""
    buf = torch.full((n + tail,), SENTINEL, device="cuda")
    return buf[:n], buf


class Seq:
    """The device buffers of one forward_train + backward of a network over a (T, M) window of B envs."""

    def __init__(self, net, act, T, M, B, h_last=True, dh0=True):
        from po_brax_amd._lib import check, lib
        from po_brax_amd.training.networks import GRUHandle
        pre, H, post = net
        self.gru, self.dims, self.net = GRUHandle(pre, H, post, act), (T, M, B), net
        n = C.c_longlong()
        check(lib.pob_gru_sequence_saved_bytes(self.gru.handle, T, M, C.byref(n)))
        self.saved, self._saved = _guarded(n.value // 4)
        check(lib.pob_gru_sequence_backward_workspace_bytes(self.gru.handle, T, M, C.byref(n)))
        self.workspace = torch.full((n.value // 8 + 8,), float("nan"), dtype=torch.float64, device="cuda")
        self.workspace[-8:] = SENTINEL
        P = param_count(net)
        assert P == self.gru.param_count
        self.obs = torch.zeros((T, B, pre[0]), device="cuda")
        self.h0 = torch.zeros((B, H), device="cuda")
        self.theta = torch.zeros(P, device="cuda")
        self.dy = torch.zeros((T, M, post[-1]), device="cuda")
        self.y, self._y = _guarded(T * M * post[-1])
        self.h_last, self._h_last = _guarded(M * H) if h_last else (None, None)
        self.dtheta, self._dtheta = _guarded(P)
        self.dh0, self._dh0 = _guarded(M * H) if dh0 else (None, None)
        self.idx = self.reset = self.dh_last = self.table = None
        self.clip = 0.0

    def load(self, pr, idx=None, reset=None, dh_last=None, table=None, clip=0.0):
        self.obs.copy_(_cuda(pr["obs"])); self.h0.copy_(_cuda(pr["h0"])); self.theta.copy_(_cuda(pr["theta"]))
        self.dy.copy_(_cuda(pr["dy"]))
        self.idx = None if idx is None else _cuda(np.asarray(idx, np.int32))
        self.reset, self.dh_last, self.table, self.clip = _cuda(reset), _cuda(dh_last), _cuda(table), clip

    def run(self):
        from po_brax_amd import _lib
        from po_brax_amd._lib import check, lib, ptr
        T, M, B = self.dims
        st = _lib.stream_handle(self.obs.device)
        check(lib.pob_gru_sequence_forward_train(self.gru.handle, T, M, B, ptr(self.obs), ptr(self.idx), ptr(self.h0),
                                                 ptr(self.reset), ptr(self.theta), ptr(self.y), ptr(self.h_last),
                                                 ptr(self.saved), ptr(self.table), self.clip, st))
        check(lib.pob_gru_sequence_backward(self.gru.handle, T, M, B, ptr(self.idx), ptr(self.reset), ptr(self.theta),
                                            ptr(self.saved), ptr(self.dy), ptr(self.dh_last), ptr(self.dtheta), ptr(self.dh0),
                                            ptr(self.workspace), st))

    def check(self, host, act, pr, what, idx=None, reset=None, dh_last=None, table=None, clip=0.0):
        T, M, B = self.dims
        y, h_last, saved = ref_forward(host, self.net, act, pr["obs"], pr["h0"], pr["theta"], idx, reset, table, clip)
        want = ref_backward(host, self.net, act, T, M, B, pr["theta"], saved, pr["dy"], idx, reset, dh_last)
        torch.cuda.synchronize()
        _same_bits(self.y, y, (what, "y"))
        _same_bits(self.saved, saved, (what, "saved"))
        _same_bits(self.dtheta, want["dtheta"], (what, "dtheta"))
        if self.h_last is not None:
            _same_bits(self.h_last, h_last, (what, "h_last"))
        if self.dh0 is not None:
            _same_bits(self.dh0, want["dh0"], (what, "dh0"))
        n_delta = want["delta"].size
        _same_bits(self.workspace.view(torch.float32)[:n_delta], want["delta"], (what, "delta"))
        for name in ("_y", "_saved", "_dtheta", "_h_last", "_dh0"):  # the rows behind every output
            buf = getattr(self, name)
            assert buf is None or bool((buf[-64:] == SENTINEL).all()), (what, name)
        assert bool((self.workspace[-8:] == SENTINEL).all()), (what, "workspace")
        return dict(y=y, h_last=h_last, saved=saved, **want)


def _third(T, B):
    r = np.zeros(T * B, np.float32)
    r[::3] = 1.0
    return r.reshape(T, B)


@pytest.mark.parametrize("T,M", SHAPES)
@pytest.mark.parametrize("net", list(NETS))
def test_kernels_equal_restatement(host, net, T, M):
    """Resets on every third entry, dh_last given, every output asked for; relu, swish and tanh."""
    for act in (RELU, SWISH, TANH):
        rng = np.random.default_rng(1000 * T + M + act)
        pr = problem(rng, NETS[net], T, M)
        reset = _third(T, M)
        dh_last = (rng.standard_normal((M, NETS[net][1])) / M).astype(np.float32)
        s = Seq(NETS[net], act, T, M, M)
        s.load(pr, None, reset, dh_last)
        s.run()
        s.check(host, act, pr, (net, T, M, act), None, reset, dh_last)


@pytest.mark.parametrize("net", ["7-gru5-4", "114-32-gru33-16-8", "114-gru64-16"])
def test_gather_normaliser_and_special_resets(host, net):
    """idx a permutation of a strict subset (B > M), a normaliser table with a live clamp, a NaN reset
    (counts) and a -0.0 reset (does not)."""
    T, M, B = 4, 37, 50
    rng = np.random.default_rng(21)
    pr = problem(rng, NETS[net], T, M, B)
    D = NETS[net][0][0]
    idx = rng.permutation(B)[:M].astype(np.int32)
    table = np.stack([0.5 * rng.standard_normal(D), rng.uniform(0.5, 2.0, D), np.ones(D)]).astype(np.float32)
    reset = pr["reset"].copy()
    reset[1, idx[0]], reset[2, idx[1]] = np.nan, -0.0
    reset[:, idx[2]] = -0.0
    for act in (RELU, SWISH, TANH):
        s = Seq(NETS[net], act, T, M, B)
        s.load(pr, idx, reset, None, table, 2.0)
        s.run()
        s.check(host, act, pr, (net, act), idx, reset, None, table, 2.0)


@pytest.mark.parametrize("net", ["7-gru5-4", "114-32-gru33-16-8"])
def test_null_optionals(host, net):
    """reset = NULL, idx = NULL, no table, and NULL h_last / dh_last / dh0."""
    T, M = 3, 65
    pr = problem(np.random.default_rng(22), NETS[net], T, M)
    s = Seq(NETS[net], SWISH, T, M, M, h_last=False, dh0=False)
    s.load(pr)
    s.run()
    s.check(host, SWISH, pr, (net, "null"))


def test_subnormal_and_zero_observation_columns(host):
    net, T, M = NETS["114-32-gru33-16-8"], 3, 40
    pr = problem(np.random.default_rng(23), net, T, M)
    pr["obs"][:, :, 1] = (pr["obs"][:, :, 1] * np.float32(1e-39)).astype(np.float32)
    pr["obs"][:, :, 2] = 0.0
    assert (np.abs(pr["obs"][:, :, 1]) < 1.2e-38).all() and (pr["obs"][:, :, 1] != 0).any()
    for act in (RELU, SWISH, TANH):
        s = Seq(net, act, T, M, M)
        s.load(pr, None, pr["reset"])
        s.run()
        want = s.check(host, act, pr, ("subnormal", act), None, pr["reset"])
        assert not want["dtheta"][2 * 32:3 * 32].view(np.uint32).any()  # the zero column's row of the first layer


def test_bad_arguments():
    from po_brax_amd._lib import check, lib, ptr
    s = Seq(NETS["7-gru5-4"], SWISH, 2, 3, 3)
    g, n = s.gru.handle, C.c_longlong()
    fwd = lambda T=2, M=3, B=3, obs=s.obs, idx=None, h0=s.h0, theta=s.theta, y=s.y, saved=s.saved, gru=g: check(  # noqa: E731
        lib.pob_gru_sequence_forward_train(gru, T, M, B, ptr(obs), ptr(idx), ptr(h0), None, ptr(theta), ptr(y), None,
                                           ptr(saved), None, 0.0, None))
    bwd = lambda T=2, M=3, B=3, theta=s.theta, saved=s.saved, dy=s.dy, dtheta=s.dtheta, ws=s.workspace, gru=g: check(  # noqa: E731
        lib.pob_gru_sequence_backward(gru, T, M, B, None, None, ptr(theta), ptr(saved), ptr(dy), None, ptr(dtheta), None,
                                      ptr(ws), None))
    for call, kw, msg in ((fwd, dict(T=0), "T must be positive"), (fwd, dict(M=0), "M must be positive"),
                          (fwd, dict(B=4), "without idx M must equal B"), (fwd, dict(obs=None), "NULL argument"),
                          (fwd, dict(h0=None), "NULL argument"), (fwd, dict(saved=None), "NULL argument"),
                          (fwd, dict(gru=None), "gru is NULL"), (fwd, dict(M=2 ** 29, B=2 ** 29), "too many rows"),
                          (bwd, dict(T=-1), "T must be positive"), (bwd, dict(dy=None), "NULL argument"),
                          (bwd, dict(ws=None), "NULL argument"), (bwd, dict(dtheta=None), "NULL argument"),
                          (bwd, dict(B=2), "without idx M must equal B"), (bwd, dict(T=2 ** 20, M=2 ** 10, B=2 ** 10), "too many rows")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    for query in (lib.pob_gru_sequence_saved_bytes, lib.pob_gru_sequence_backward_workspace_bytes):
        with pytest.raises(ValueError, match="T must be positive"):
            check(query(g, 0, 3, C.byref(n)))
        with pytest.raises(ValueError, match="bytes is NULL"):
            check(query(g, 2, 3, None))
    torch.cuda.synchronize()


def test_one_graph_replayed_after_in_place_changes(host):
    """Forward and backward captured into ONE graph; theta, obs and dy then change in place."""
    net, T, M = NETS["114-32-gru33-16-8"], 3, 70
    rng = np.random.default_rng(24)
    pr = problem(rng, net, T, M)
    s = Seq(net, TANH, T, M, M)
    s.load(pr, None, pr["reset"])
    s.run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.run()
    pr2 = problem(rng, net, T, M)
    pr2["reset"] = pr["reset"]
    s.obs.copy_(_cuda(pr2["obs"])); s.theta.copy_(_cuda(pr2["theta"])); s.dy.copy_(_cuda(pr2["dy"]))
    s.h0.copy_(_cuda(pr2["h0"]))
    s.dtheta.fill_(float("nan"))
    graph.replay()
    s.check(host, TANH, pr2, "graph replay", None, pr["reset"])


@pytest.mark.parametrize("with_idx", [False, True])
def test_apply_sequence_native_is_the_c_calls(host, with_idx):
    import types
    from po_brax_amd.training import networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    pre, H, post = net = NETS["114-32-gru33-16-8"]
    T, B = 4, 45
    M = 33 if with_idx else B
    rng = np.random.default_rng(25)
    pr = problem(rng, net, T, M, B)
    idx = rng.permutation(B)[:M].astype(np.int32) if with_idx else None
    norm = ObservationNormalizer(pre[0], clip=2.0)
    table = np.stack([0.5 * rng.standard_normal(pre[0]), rng.uniform(0.5, 2.0, pre[0]), np.ones(pre[0])]).astype(np.float32)
    norm.load_state_dict({"table": torch.from_numpy(table), "count": torch.tensor([9.0], dtype=torch.float64), "clip": 2.0})
    model = networks.make_recurrent_model(pre[1:], H, post, pre[0], "swish")
    theta = _cuda(pr["theta"]).requires_grad_(True)
    h0 = _cuda(pr["h0"]).requires_grad_(True)
    dh_last = (rng.standard_normal((M, H)) / M).astype(np.float32)
    y, h_last = model.apply_sequence_native(types.SimpleNamespace(theta=theta), _cuda(pr["obs"]), h0, _cuda(pr["reset"]),
                                            _cuda(idx), norm)
    ((y * _cuda(pr["dy"])).sum() + (h_last * _cuda(dh_last)).sum()).backward()
    yr, hr, saved = ref_forward(host, net, SWISH, pr["obs"], pr["h0"], pr["theta"], idx, pr["reset"], table, 2.0)
    want = ref_backward(host, net, SWISH, T, M, B, pr["theta"], saved, pr["dy"], idx, pr["reset"], dh_last)
    torch.cuda.synchronize()
    _same_bits(y, yr, "y"); _same_bits(h_last, hr, "h_last"); _same_bits(theta.grad, want["dtheta"], "theta.grad")
    dh0 = np.zeros((B, H), np.float32)
    dh0[idx if with_idx else np.arange(B)] = want["dh0"]
    _same_bits(h0.grad, dh0, "h0.grad")
    # no gradient needed: the torch ops, the same values to rounding
    with torch.no_grad():
        y2, _ = model.apply_sequence_native(types.SimpleNamespace(theta=theta), _cuda(pr["obs"]), h0, _cuda(pr["reset"]),
                                            _cuda(idx), norm)
    torch.testing.assert_close(y2, y.detach(), rtol=1e-4, atol=1e-5)
    # theta.grad alone: dh0 is not asked of the kernel
    th2 = _cuda(pr["theta"]).requires_grad_(True)
    y3, _ = model.apply_sequence_native(types.SimpleNamespace(theta=th2), _cuda(pr["obs"]), _cuda(pr["h0"]),
                                        _cuda(pr["reset"]), _cuda(idx), norm)
    (y3 * _cuda(pr["dy"])).sum().backward()
    want3 = ref_backward(host, net, SWISH, T, M, B, pr["theta"], saved, pr["dy"], idx, pr["reset"], None)
    _same_bits(th2.grad, want3["dtheta"], "theta.grad without dh_last")


def test_window_of_a_real_replay(host):
    """After one replay on ant_heavenhell (B = 64, T = 8, the normaliser loaded and not updated) with
    theta unchanged: the native sequence forward over all envs from roll.hidden[0] with reset[t] =
    done[t - 1] reproduces roll.hidden[t] for every t and the logits of an eager act_into, bit for bit."""
    from po_brax_amd import _lib, envs, jumpy
    from po_brax_amd._lib import check, lib, ptr
    from po_brax_amd.rollout import RecurrentActorRollout
    from po_brax_amd.training import networks
    from test_gpu_learner import _loaded_normalizer
    from test_gpu_parity import _keys
    B, T, H = 64, 8, 64
    env = envs.create("ant_heavenhell", batch_size=B, episode_length=3)
    state = env.reset(torch.from_numpy(_keys(B, 3)).cuda())
    D, A = env.observation_size, env.action_size
    norm = _loaded_normalizer(np.random.default_rng(5), D, 5.0, mean_sd=0.2, lo=0.5, hi=2.0)
    model = networks.make_recurrent_model([], H, [2 * A], D)
    params = model.init(jumpy.random_prngkey(5))
    params.theta.mul_(3.0)
    policy = networks.RecurrentTanhPolicy(model, params, jumpy.random_prngkey(6), normalizer=norm)
    roll = RecurrentActorRollout(env, state, policy, T)
    roll.replay()
    torch.cuda.synchronize()
    assert bool(roll.done[:-1].any()) and not bool(roll.done.all())  # resets fall inside the window
    reset = torch.cat([torch.zeros_like(roll.done[:1]), roll.done[:-1]]).contiguous()
    n = C.c_longlong()
    check(lib.pob_gru_sequence_saved_bytes(model.gru.handle, T, B, C.byref(n)))
    saved = torch.empty(n.value // 4, device="cuda")
    y, h_last = torch.empty((T, B, 2 * A), device="cuda"), torch.empty((B, H), device="cuda")
    h0 = roll.hidden[0].contiguous()
    check(lib.pob_gru_sequence_forward_train(model.gru.handle, T, B, B, ptr(roll.obs), None, ptr(h0), ptr(reset),
                                             ptr(policy.theta), ptr(y), ptr(h_last), ptr(saved), ptr(norm.table), norm.clip,
                                             _lib.stream_handle(y.device)))
    torch.cuda.synchronize()
    lay = layout(host, ([D], H, [2 * A]), T * B)
    hin = saved[lay["hin"]:lay["hin"] + T * B * H].reshape(T, B, H)
    assert torch.equal(_bits(hin), _bits(roll.hidden))
    assert torch.equal(_bits(h_last), _bits(policy.hidden))
    eager = networks.RecurrentTanhPolicy(model, params, jumpy.random_prngkey(7), deterministic=True, normalizer=norm)
    eager._buffers(B)
    action, logits = torch.empty((B, A), device="cuda"), torch.empty((B, 2 * A), device="cuda")
    for t in range(T):
        eager.hidden.copy_(roll.hidden[t])
        eager.reset.zero_()
        eager.act_into(roll.obs[t].contiguous(), action, logits=logits)
        torch.cuda.synchronize()
        assert torch.equal(_bits(logits), _bits(y[t])), t
