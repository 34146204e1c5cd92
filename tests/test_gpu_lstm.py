"""GPU: the LSTM kernels (csrc/pob_lstm.hip k_lstm_forward / k_lstm_policy_act, reached through
make_recurrent_model(..., cell="lstm")) against the definition in float64 torch ops on the CPU:
addmm layers and torch.nn.LSTMCell through the mapping of DESIGN.md "LSTM cell".

Tolerance (the rule of test_gru_host.py): the kernel's max abs error against float64 is at most 4 x
the error of the same network in float32 torch ops on the CPU against float64, + 1e-7.  The float32
error is taken once per network over the case's 65 rows (rows are independent; B = 1 and 33 run its
first rows), never from the kernel.  Each figure is printed before it is asserted."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ACT = {0: torch.relu, 1: torch.nn.functional.silu, 2: torch.tanh}
# (pre = [D, *pre widths], H, post, activation)
NETS = [([7], 5, [4], 0),            # odd concatenation: the pad step, one partial tile
        ([30], 64, [16], 1),         # two output tiles, gate columns at stride 4 H crossing tiles
        ([114, 40], 33, [16], 2),    # a pre-MLP, a tail tile, odd H
        ([128], 128, [2], 1)]        # the limit I + H = 256
BMAX, STEPS, PAD, SENTINEL = 65, 3, 2, -777.0


def _ref(net, theta, x, s, reset, dtype):
    pre, H, post, act = net
    th, v, off, I = theta.to(dtype), x.to(dtype), 0, net[0][-1]

    def take(i, o):
        nonlocal off
        off += i * o + o
        return th[off - i * o - o:off - o].view(i, o), th[off - o:off]

    with torch.no_grad():
        for i, o in zip(pre[:-1], pre[1:]):
            W, b = take(i, o)
            v = ACT[act](torch.addmm(b, v, W))
        W, b = take(I + H, 4 * H)
        cell = torch.nn.LSTMCell(I, H, dtype=dtype)
        cell.weight_ih.copy_(W[:I].T); cell.weight_hh.copy_(W[I:].T); cell.bias_ih.copy_(b); cell.bias_hh.zero_()
        s = torch.where(reset[:, None] != 0, 0.0, s.to(dtype))
        h, c = cell(v, (s[:, :H], s[:, H:]))
        v = h
        for n, (i, o) in enumerate(zip([H] + post[:-1], post)):
            W, b = take(i, o)
            v = torch.addmm(b, v, W)
            v = ACT[act](v) if n != len(post) - 1 else v
    return v, torch.cat([h, c], 1)


@pytest.fixture(scope="module", params=range(len(NETS)))
def case(request):
    """One network: model, device theta, inputs of STEPS steps, and per step the float64 chain (y, state)
    with the float32 chain's error against it."""
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    net = NETS[request.param]
    pre, H, post, act = net
    model = networks.make_recurrent_model(pre[1:], H, post, pre[0], activation=("relu", "swish", "tanh")[act], cell="lstm")
    gen = torch.Generator().manual_seed(100 + request.param)
    u = lambda shape, lim: (torch.rand(shape, generator=gen) * 2 - 1) * lim  # noqa: E731
    params = model.init(jumpy.random_prngkey(request.param).cpu())
    for leaf in params.values():  # lively weights and non-zero biases, written into theta's views
        leaf["kernel"].copy_(u(leaf["kernel"].shape, (3.0 / leaf["kernel"].shape[0]) ** 0.5))
        leaf["bias"].copy_(u(leaf["bias"].shape, 0.5))
    xs = [u((BMAX, pre[0]), 3.0) for _ in range(STEPS)]
    s0 = torch.cat([u((BMAX, H), 1.0), u((BMAX, H), 2.0)], 1)
    resets = [((torch.arange(BMAX) + t) % 3 == 0).float() for t in range(STEPS)]  # every third row, moving
    want, tol, s64, s32 = [], [], s0.double(), s0
    for t in range(STEPS):
        y64, s64 = _ref(net, params.theta, xs[t], s64, resets[t], torch.float64)
        y32, s32 = _ref(net, params.theta, xs[t], s32, resets[t], torch.float32)
        want.append((y64, s64))
        tol.append(tuple(4.0 * float((a - b).abs().max()) + 1e-7 for a, b in ((y32, y64), (s32[:, :H], s64[:, :H]),
                                                                            (s32[:, H:], s64[:, H:]))))
    return dict(net=net, model=model, params=params.to("cuda"), xs=xs, s0=s0, resets=resets, want=want, tol=tol)


def _forward(case, B, x, s, reset, norm=None, clip=0.0):
    """One k_lstm_forward launch on the first B rows of sentinel-padded buffers."""
    from po_brax_amd import _lib
    H, O = case["net"][1], case["net"][2][-1]
    bufs = [torch.full((B + PAD, w), SENTINEL, device="cuda") for w in (2 * H, O, 2 * H)]
    h_io, y, s_copy = bufs
    h_io[:B] = s[:B]
    tail = () if norm is None else (norm.data_ptr(), clip)
    fn = _lib.lib.pob_gru_forward if norm is None else _lib.lib.pob_gru_forward_norm
    _lib.check(fn(case["model"].gru.handle, B, x[:B].contiguous().data_ptr(), case["params"].theta.data_ptr(),
                  None if reset is None else reset[:B].contiguous().data_ptr(), h_io.data_ptr(), y.data_ptr(),
                  s_copy.data_ptr(), *tail, _lib.stream_handle("cuda")))
    torch.cuda.synchronize()
    for t in bufs:
        assert (t[B:] == SENTINEL).all()  # the rows behind every output are untouched
    return y[:B], h_io[:B], s_copy[:B]


def _within(case, t, B, y, s, what):
    H = case["net"][1]
    y64, s64 = case["want"][t]
    for name, got, ref, tol in (("y", y, y64, case["tol"][t][0]), ("h'", s[:, :H], s64[:, :H], case["tol"][t][1]),
                                ("c'", s[:, H:], s64[:, H:], case["tol"][t][2])):
        err = float((got.double().cpu() - ref[:B]).abs().max())
        print(f"{case['net']} B {B} step {t} {what} {name}: kernel {err:.3e} bound {tol:.3e}")
        assert err <= tol, (case["net"], B, t, what, name)


@pytest.mark.parametrize("B", [1, 33, BMAX])
def test_forward_chain_reset_and_sentinels(case, B):
    xs, resets = [x.cuda() for x in case["xs"]], [r.cuda() for r in case["resets"]]
    s = case["s0"].cuda()
    for t in range(STEPS):  # the kernel's own state fed back, as h_io carries it
        s_in = s
        y, s, s_copy = _forward(case, B, xs[t], s_in, resets[t])
        _within(case, t, B, y, s, "forward")
        assert torch.equal(s_copy, torch.where(resets[t][:B, None] != 0, 0.0, s_in[:B]))
        assert not torch.signbit(s_copy[resets[t][:B] != 0]).any()  # +0 in all 2 H columns
        y0, z0, _ = _forward(case, B, xs[t], torch.zeros_like(s_in), None)
        rows = resets[t][:B] != 0
        assert torch.equal(y[rows], y0[rows]) and torch.equal(s[rows], z0[rows])  # reset = a zero state, bit for bit


@pytest.mark.parametrize("B", [1, 33, BMAX])
def test_deterministic_actor_and_normaliser(case, B):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    model, params, (pre, H, post, _) = case["model"], case["params"], case["net"]
    A = post[-1] // 2
    x, s_in, reset = (t.cuda()[:B].contiguous() for t in (case["xs"][0], case["s0"], case["resets"][0]))
    ya, sa = model.apply(params, x, s_in, reset)
    policy = networks.RecurrentTanhPolicy(model, params, jumpy.random_prngkey(3), deterministic=True)
    policy._buffers(B)
    policy.hidden.copy_(s_in)
    out = {k: torch.full((B + PAD, w), SENTINEL, device="cuda") for k, w in (("action", A), ("logits", 2 * A), ("s", 2 * H))}
    policy.act_into(x, out["action"][:B], None, None, out["logits"][:B], None, out["s"][:B], reset)
    torch.cuda.synchronize()
    assert all((v[B:] == SENTINEL).all() for v in out.values())
    assert torch.equal(out["logits"][:B], ya) and torch.equal(policy.hidden, sa)
    assert torch.equal(out["s"][:B], torch.where(reset[:, None] != 0, 0.0, s_in))
    want = torch.tanh(case["want"][0][0][:B, :A])  # tanh is 1-Lipschitz: the logits' bound serves
    err = float((out["action"][:B].double().cpu() - want).abs().max())
    print(f"{case['net']} B {B} tanh(mean): kernel {err:.3e} bound {case['tol'][0][0]:.3e}")
    assert err <= case["tol"][0][0]
    # the normaliser folded into the tile load: the same bits as apply on rows normalised in torch; the state is not normalised
    gen = torch.Generator().manual_seed(7)
    norm = ObservationNormalizer(pre[0], clip=2.0)
    norm.table[0].copy_(torch.rand(pre[0], generator=gen) - 0.5)
    norm.table[1].copy_(torch.rand(pre[0], generator=gen) + 0.5)
    xn = torch.clamp((x - norm.table[0]) * norm.table[1], -2.0, 2.0)
    yn, sn, _ = _forward(case, B, x, s_in, reset, norm.table, 2.0)
    ya, sa = model.apply(params, xn, s_in, reset)
    assert torch.equal(yn, ya) and torch.equal(sn, sa) and not torch.equal(xn, x)


def test_rollout_equals_eager():
    from po_brax_amd import envs, jumpy
    from po_brax_amd import standard_observability_masks as masks
    from po_brax_amd.rollout import RecurrentActorRollout
    from po_brax_amd.training import networks
    from test_gpu_parity import _keys
    name, B, T, H = "ant_heavenhell", 64, 4, 64
    idx = masks.po_env_mask(name, cfrc=False)
    assert len(idx) == 30
    keys = torch.from_numpy(_keys(B, 3)).cuda()
    es = [envs.create(name, batch_size=B, episode_length=3, obs_mask=idx) for _ in range(2)]
    ss = [e.reset(keys) for e in es]
    model = networks.make_recurrent_model([], H, [16], 30, cell="lstm")
    params = model.init(jumpy.random_prngkey(5))
    params.theta.mul_(3.0)  # livelier actions than the init's
    ps = [networks.RecurrentTanhPolicy(model, params, jumpy.random_prngkey(6)) for _ in range(2)]
    roll = RecurrentActorRollout(es[1], ss[1], ps[1], T, masked=True)
    assert roll.hidden.shape == (T, B, 2 * H)
    f = dict(dtype=torch.float32, device="cuda")
    s, done_before = ss[0], torch.zeros(B, **f)
    for rep in range(2):
        roll.replay()
        torch.cuda.synchronize()
        for t in range(T):
            obs = s.info["obs_masked"].clone()
            action, logp, raw = torch.empty((B, 8), **f), torch.empty(B, **f), torch.empty((B, 8), **f)
            hidden = torch.empty((B, 2 * H), **f)
            ps[0].act_into(obs, action, logp, raw, None, None, hidden, done_before)
            s = es[0].step_(s, action)
            for k, v in (("obs", obs), ("raw", raw), ("logp", logp), ("hidden", hidden)):
                assert torch.equal(getattr(roll, k)[t], v), (k, rep, t)
            if rep or t:  # all 2 H columns zero exactly after a done (the very first state is zero everywhere)
                assert torch.equal((hidden == 0).all(-1), done_before != 0)
            done_before = (s.aux["done"] if "done" in s.aux else s.done).float().clone()
            assert torch.equal(roll.done[t], done_before)
    assert torch.equal(ps[0].hidden, ps[1].hidden) and torch.equal(ps[0].key, ps[1].key) and bool(roll.done.any())
