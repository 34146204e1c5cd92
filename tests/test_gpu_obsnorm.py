"""GPU: the running observation normaliser.  k_obsnorm_accumulate / k_obsnorm_update equal the
restatement (csrc/pob_mlp.h obsnorm_accumulate_ref / obsnorm_update_ref, built for the host by
tests/host/obsnorm_host.cpp) with integer-view equality; the ``_norm`` twins of the four forward
entry points equal pob_obsnorm_apply followed by the network's restatement; ``norm = NULL``
gives the plain entry points' results; the actor rollouts with ``update_normalizer=True`` equal
the same loop run eagerly."""
import ctypes as C

import numpy as np
import pytest
import torch

import pob_np
from test_gru_host import build_gru_host, random_gru
from test_gru_host import ref_forward as gru_ref_forward
from test_gru_host import ref_policy as gru_ref_policy
from test_mlp_host import build_host as build_mlp_host
from test_mlp_host import random_net, ref_head
from test_mlp_host import ref_forward as mlp_ref_forward
from test_obsnorm_host import (brax_update, build_obsnorm_host, columns, fresh_table, ref_apply, ref_update,
                               within_bound)

pytestmark = pytest.mark.gpu

PAD = 5  # sentinel elements behind every buffer the kernels write
SENT64, SENT32 = -777.0, -555.0


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("obsnorm_host_gpu")
    return {"norm": build_obsnorm_host(d), "mlp": build_mlp_host(d), "gru": build_gru_host(d)}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), what


class DeviceNorm:
    """count, table, sums and the workspace in sentinel-padded device buffers, driven through the C ABI."""

    def __init__(self, D, n_max, R=1):
        from po_brax_amd import _lib
        self.lib, self.D, self.R = _lib, D, R
        need = C.c_longlong()
        _lib.check(_lib.lib.pob_obsnorm_workspace_bytes(n_max, D, C.byref(need)))
        assert need.value == ((n_max + 1023) // 1024) * 2 * D * 8
        self.n_ws = need.value // 8
        self.count = torch.tensor([0.0] + [SENT64] * PAD, dtype=torch.float64, device="cuda")
        self.table = torch.full((3 * D + PAD,), SENT32, device="cuda")
        self.table[:3 * D] = _cuda(fresh_table(D)).reshape(-1)
        self.sums = torch.full((R * 2 * D + PAD,), SENT64, dtype=torch.float64, device="cuda")
        self.ws = torch.full((self.n_ws + PAD,), SENT64, dtype=torch.float64, device="cuda")

    def accumulate(self, x, r=0):
        L = self.lib
        L.check(L.lib.pob_obsnorm_accumulate(x.data_ptr(), x.shape[0], self.D, self.table.data_ptr(), self.ws.data_ptr(),
                                             self.sums.data_ptr() + r * 2 * self.D * 8, L.stream_handle(x.device)))

    def update(self, n_new):
        L = self.lib
        L.check(L.lib.pob_obsnorm_update(self.count.data_ptr(), self.table.data_ptr(), self.D, self.sums.data_ptr(), self.R,
                                         n_new, L.stream_handle(self.table.device)))

    def check_sentinels(self):
        torch.cuda.synchronize()
        assert (self.count[1:] == SENT64).all() and (self.table[3 * self.D:] == SENT32).all()
        assert (self.sums[self.R * 2 * self.D:] == SENT64).all() and (self.ws[self.n_ws:] == SENT64).all()


@pytest.mark.parametrize("D", [1, 30, 65, 114, 256])
def test_accumulate_update_bit_exact(hosts, D):
    host = hosts["norm"]
    for N in (1, 31, 1023, 1024, 1025, 2055):
        rng = np.random.default_rng(100 * D + N)
        dev = DeviceNorm(D, N)
        count, table = 0.0, fresh_table(D)
        for step in range(3):
            x, _ = columns(rng, N, D)
            x[0, 0] = -0.0
            count, table, sums = ref_update(host, count, table, [x])
            dev.accumulate(_cuda(x))
            dev.update(N)
            dev.check_sentinels()
            _same_bits(dev.sums[:2 * D].reshape(1, 2, D), sums, ("sums", D, N, step))
            _same_bits(dev.table[:3 * D].reshape(3, D), table, ("table", D, N, step))
            _same_bits(dev.count[:1], np.array([count]), ("count", D, N, step))


def test_two_shards_bit_exact_and_close_to_float64(hosts):
    host = hosts["norm"]
    N, D = 2055, 114
    rng = np.random.default_rng(9)
    dev = DeviceNorm(D, N, R=2)
    count, table = 0.0, fresh_table(D)
    s64 = (0, np.zeros(D, np.float64), np.ones(D, np.float64))
    s32 = (0, np.zeros(D, np.float32), np.ones(D, np.float32))
    for step in range(3):
        x, kind = columns(rng, N, D)
        halves = [x[:N // 2], x[N // 2:]]
        count, table, sums = ref_update(host, count, table, halves)
        for r, h in enumerate(halves):
            dev.accumulate(_cuda(h), r)
        dev.update(N)
        dev.check_sentinels()
        _same_bits(dev.sums[:4 * D].reshape(2, 2, D), sums, ("sums", step))
        _same_bits(dev.table[:3 * D].reshape(3, D), table, ("table", step))
        _same_bits(dev.count[:1], np.array([count]), ("count", step))
        s64, s32 = brax_update(s64, x, np.float64), brax_update(s32, x, np.float32)
    within_bound(dev.table[:3 * D].reshape(3, D).cpu().numpy(), s64, s32, kind, f"GPU R 2 D {D} N {N}")


def test_argument_errors():
    from po_brax_amd import _lib
    L = _lib.lib
    need = C.c_longlong()
    t = torch.zeros(64, device="cuda")
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    p, q = t.data_ptr(), d.data_ptr()
    for rc in (L.pob_obsnorm_workspace_bytes(10, 0, C.byref(need)), L.pob_obsnorm_workspace_bytes(10, 257, C.byref(need)),
               L.pob_obsnorm_workspace_bytes(0, 4, C.byref(need)),
               L.pob_obsnorm_accumulate(p, 0, 4, p, q, q, None), L.pob_obsnorm_accumulate(p, 4, 257, p, q, q, None),
               L.pob_obsnorm_accumulate(p, 4, 4, None, q, q, None), L.pob_obsnorm_accumulate(p, 4, 4, p, None, q, None),
               L.pob_obsnorm_accumulate(p, 4, 4, p, q, None, None),
               L.pob_obsnorm_update(q, p, 4, q, 0, 4, None), L.pob_obsnorm_update(q, p, 0, q, 1, 4, None),
               L.pob_obsnorm_update(q, None, 4, q, 1, 4, None), L.pob_obsnorm_update(q, p, 4, None, 1, 4, None)):
        assert rc == _lib.POB_EINVAL
        assert b"obsnorm" in L.pob_last_error()
    with pytest.raises(ValueError, match="1 .. 256"):
        _lib.check(L.pob_obsnorm_workspace_bytes(10, 300, C.byref(need)))


# ---------------------------------------------------------------------------- the _norm twins
BATCHES = (1, 33, 65)
A = 8


def norm_case(rng, B, D):
    """Inputs out to +-20, means in +-3, scales in [0.05, 20] (log-uniform): the clamp fires on some
    elements and not on others."""
    x = rng.uniform(-20, 20, (B, D)).astype(np.float32)
    table = fresh_table(D)
    table[0] = rng.uniform(-3, 3, D)
    table[1] = np.exp(rng.uniform(np.log(0.05), np.log(20.0), D))
    table[2] = np.nan  # never read by the forward kernels
    return x, table


def _uniform_rows(key_np, total, first, B):
    sub = pob_np.split(key_np)[1]
    u = np.asarray(pob_np.uniform(sub, (total * A,), np.float32(-1), np.float32(1)), np.float32).reshape(total, A)
    return u[first:first + B]


def _same_with_nan(got, want, what):
    """Integer-view equality where the restatement is a number, NaN where it is NaN (IEEE 754
    leaves a propagated NaN's sign and payload to the implementation)."""
    got = got.detach().cpu()
    want = torch.from_numpy(np.ascontiguousarray(want))
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), what


def _mlp_out(B, D, O, fill=float("nan")):
    return {"action": torch.full((B, A), fill, device="cuda"), "logp": torch.full((B,), fill, device="cuda"),
            "raw": torch.full((B, A), fill, device="cuda"), "logits": torch.full((B, O), fill, device="cuda"),
            "obs_copy": torch.full((B, D), fill, device="cuda")}


def _mlp_act(h, obs, theta, key, norm, clip, plain=False):
    from po_brax_amd import _lib
    B, D = obs.shape
    out = _mlp_out(B, D, 2 * A)
    args = (h.handle, B, B, 0, obs.data_ptr(), theta.data_ptr(), key.data_ptr(), 0,
            *(out[k].data_ptr() for k in ("action", "logp", "raw", "logits", "obs_copy")))
    if plain:
        _lib.check(_lib.lib.pob_policy_act(*args, _lib.stream_handle(obs.device)))
    else:
        _lib.check(_lib.lib.pob_policy_act_norm(*args, None if norm is None else norm.data_ptr(), clip,
                                                _lib.stream_handle(obs.device)))
    torch.cuda.synchronize()
    return out


def _mlp_forward(h, x, theta, norm, clip, plain=False):
    from po_brax_amd import _lib
    y = torch.full((x.shape[0], h.sizes[-1]), float("nan"), device="cuda")
    if plain:
        _lib.check(_lib.lib.pob_mlp_forward(h.handle, x.shape[0], x.data_ptr(), theta.data_ptr(), y.data_ptr(),
                                            _lib.stream_handle(x.device)))
    else:
        _lib.check(_lib.lib.pob_mlp_forward_norm(h.handle, x.shape[0], x.data_ptr(), theta.data_ptr(), y.data_ptr(),
                                                 None if norm is None else norm.data_ptr(), clip,
                                                 _lib.stream_handle(x.device)))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("sizes", [[27, 33, 16], [114, 32, 32, 32, 32, 16]])
def test_mlp_twins_bit_exact(hosts, sizes):
    from po_brax_amd.training.networks import MLPHandle
    rng = np.random.default_rng(sum(sizes))
    Bmax, D = max(BATCHES), sizes[0]
    _, theta = random_net(sizes, rng, 1)
    x, table = norm_case(rng, Bmax, D)
    x[2 % Bmax, 3] = np.nan  # one NaN element (row 2 exists from B = 33 on)
    h = MLPHandle(sizes, 1, False)
    td, nd = _cuda(theta), _cuda(table)
    key_np = np.asarray(pob_np.prngkey(21), np.uint32)
    for clip in (5.0, 0.0):
        xn = ref_apply(hosts["norm"], x, table, clip)
        fired = np.abs(xn) == clip
        assert clip == 0.0 or (fired.any() and not fired[~np.isnan(xn)].all())
        want_y = mlp_ref_forward(hosts["mlp"], sizes, 1, False, xn, theta)
        for B in BATCHES:
            xd = _cuda(x[:B])
            _same_with_nan(_mlp_forward(h, xd, td, nd, clip), want_y[:B], ("forward", sizes, B, clip))
            got = _mlp_act(h, xd, td, _cuda(key_np.copy()), nd, clip)
            action, logp, raw = ref_head(hosts["mlp"], want_y[:B], _uniform_rows(key_np, B, 0, B))
            for k, w in (("logits", want_y[:B]), ("action", action), ("logp", logp), ("raw", raw)):
                _same_with_nan(got[k], w, (k, sizes, B, clip))
            _same_with_nan(got["obs_copy"], x[:B], ("obs_copy keeps the raw rows", B))
    # norm = NULL: the twin is the plain entry point, every output, integer view (finite inputs)
    x[2 % Bmax, 3] = 0.5
    for B in BATCHES:
        xd = _cuda(x[:B])
        assert torch.equal(_bits(_mlp_forward(h, xd, td, None, 5.0)), _bits(_mlp_forward(h, xd, td, None, 0.0, plain=True)))
        a = _mlp_act(h, xd, td, _cuda(key_np.copy()), None, 5.0)
        b = _mlp_act(h, xd, td, _cuda(key_np.copy()), None, 0.0, plain=True)
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (k, B)


GRU_NETS = [([30], 64, [16]), ([114, 32], 64, [32, 16])]


def _gru_call(g, obs, theta, key, reset, h, norm, clip, plain=False, actor=True):
    from po_brax_amd import _lib
    B, D = obs.shape
    H, O = g.hidden, g.post_sizes[-1]
    out = _mlp_out(B, D, O)
    out["h_in_copy"] = torch.full((B, H), float("nan"), device="cuda")
    out["h_out"] = h.clone()
    tail = () if plain else (None if norm is None else norm.data_ptr(), clip)
    st = _lib.stream_handle(obs.device)
    if actor:
        fn = _lib.lib.pob_gru_policy_act if plain else _lib.lib.pob_gru_policy_act_norm
        _lib.check(fn(g.handle, B, B, 0, obs.data_ptr(), theta.data_ptr(), key.data_ptr(), 0, reset.data_ptr(),
                      out["h_out"].data_ptr(), *(out[k].data_ptr() for k in ("action", "logp", "raw", "logits", "obs_copy",
                                                                             "h_in_copy")), *tail, st))
    else:
        fn = _lib.lib.pob_gru_forward if plain else _lib.lib.pob_gru_forward_norm
        _lib.check(fn(g.handle, B, obs.data_ptr(), theta.data_ptr(), reset.data_ptr(), out["h_out"].data_ptr(),
                      out["logits"].data_ptr(), out["h_in_copy"].data_ptr(), *tail, st))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("net", range(len(GRU_NETS)))
def test_gru_twins_bit_exact(hosts, net):
    from po_brax_amd.training.networks import GRUHandle
    pre, H, post = GRU_NETS[net]
    rng = np.random.default_rng(300 + net)
    Bmax, D = max(BATCHES), pre[0]
    _, h, theta = random_gru(pre, H, post, rng, Bmax)
    x, table = norm_case(rng, Bmax, D)
    x[2 % Bmax, 3] = np.nan
    h = (h * 30.0).astype(np.float32)  # a hidden state the table would change (and the clamp cut) if it were normalised
    reset = np.zeros(Bmax, np.float32)
    reset[::3] = 1.0
    g = GRUHandle(pre, H, post, 1)
    td, nd = _cuda(theta), _cuda(table)
    key_np = np.asarray(pob_np.prngkey(22), np.uint32)
    h0 = h.copy()
    h0[reset != 0] = 0.0
    for clip in (5.0, 0.0):
        xn = ref_apply(hosts["norm"], x, table, clip)
        for B in BATCHES:
            want = gru_ref_policy(hosts["gru"], pre, H, post, 1, xn[:B], theta, reset[:B], h[:B], _uniform_rows(key_np, B, 0, B))
            assert np.array_equal(want["h_in_copy"].view(np.uint32), h0[:B].view(np.uint32))  # raw h, reset rows +0
            xd, hd, rd = _cuda(x[:B]), _cuda(h[:B]), _cuda(reset[:B])
            got = _gru_call(g, xd, td, _cuda(key_np.copy()), rd, hd, nd, clip)
            for k in ("logits", "h_out", "h_in_copy", "action", "logp", "raw"):
                _same_with_nan(got[k], want[k], (k, pre, B, clip))
            _same_with_nan(got["obs_copy"], x[:B], ("obs_copy keeps the raw rows", B))
            fw = _gru_call(g, xd, td, None, rd, hd, nd, clip, actor=False)
            y, h_out, h_copy = gru_ref_forward(hosts["gru"], pre, H, post, 1, xn[:B], theta, reset[:B], h[:B])
            for k, w in (("logits", y), ("h_out", h_out), ("h_in_copy", h_copy)):
                _same_with_nan(fw[k], w, ("forward", k, pre, B, clip))
    x[2 % Bmax, 3] = 0.5
    for B in BATCHES:
        xd, hd, rd = _cuda(x[:B]), _cuda(h[:B]), _cuda(reset[:B])
        for actor in (True, False):
            key = lambda: _cuda(key_np.copy()) if actor else None  # noqa: E731
            a = _gru_call(g, xd, td, key(), rd, hd, None, 5.0, actor=actor)
            b = _gru_call(g, xd, td, key(), rd, hd, None, 0.0, plain=True, actor=actor)
            for k in (a if actor else ("logits", "h_out", "h_in_copy")):
                assert torch.equal(_bits(a[k]), _bits(b[k])), (k, B, actor)


@pytest.mark.parametrize("clip", [5.0, 0.0])
def test_apply_in_torch_ops_equals_the_staged_values(clip):
    """An identity-weight one-layer network returns what the tile load staged: fmaf(1, t, +0)
    behind fmaf(0, finite, +0) terms is t itself (-0 comes out as +0, equal under torch.equal)."""
    from po_brax_amd.training import networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    D, B = 65, 97
    rng = np.random.default_rng(4)
    x, table = norm_case(rng, B, D)
    norm = ObservationNormalizer(D, clip=clip)
    norm.table.copy_(_cuda(np.nan_to_num(table, nan=1.0)))
    theta = torch.cat([torch.eye(D).reshape(-1), torch.zeros(D)]).cuda()
    h = networks.MLPHandle([D, D], 1, False)
    xd = _cuda(x)
    staged = _mlp_forward(h, xd, theta, norm.table, norm.clip)
    applied = norm.apply(xd)
    assert torch.equal(applied, staged)
    assert clip == 0.0 or ((applied.abs() == clip).any() and (applied.abs() < clip).any())
    # the fresh table is the identity (up to the clamp)
    fresh = ObservationNormalizer(D, clip=0.0)
    assert torch.equal(_mlp_forward(h, xd, theta, fresh.table, 0.0), xd)
    sd = norm.state_dict()
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.table, norm.table) and fresh.clip == clip and torch.equal(fresh.count, norm.count)


def test_python_update_matches_the_abi_and_brax_spelling(hosts):
    from po_brax_amd.training.normalization import create_observation_normalizer
    D, T, B = 30, 3, 700
    rng = np.random.default_rng(12)
    x, _ = columns(rng, T * B, D)
    data, update_fn, apply_fn = create_observation_normalizer(D)
    assert update_fn(data, _cuda(x).reshape(T, B, D)) is data  # any leading dims
    count, table, _ = ref_update(hosts["norm"], 0.0, fresh_table(D), [x])
    _same_bits(data.table, table, "table")
    assert float(data.count) == count == T * B
    assert torch.equal(data.mean, data.table[0]) and torch.equal(data.scale, data.table[1]) and torch.equal(data.m2, data.table[2])
    assert torch.equal(apply_fn(data, _cuda(x)), _cuda(ref_apply(hosts["norm"], x, table, 5.0)))
    none, upd, app = create_observation_normalizer(D, normalize_observations=False)
    assert none is None and upd(none, _cuda(x)) is None and app(none, xd := _cuda(x)) is xd
    off = create_observation_normalizer(D, apply_clipping=False)[0]
    assert off.clip == 0.0


# ---------------------------------------------------------------------------- rollouts
B_ROLL, T_ROLL = 64, 5


def _ff_policy(env, D, kw, seed=5):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_models(2 * env.action_size, D)[0]
    params = model.init(jumpy.random_prngkey(seed))
    params.theta.mul_(3.0)
    return networks.NormalTanhPolicy(model, params, jumpy.random_prngkey(seed + 1), **kw)


def _rec_policy(env, D, kw, seed=5):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_recurrent_model([], 64, [2 * env.action_size], D)
    params = model.init(jumpy.random_prngkey(seed))
    params.theta.mul_(3.0)
    return networks.RecurrentTanhPolicy(model, params, jumpy.random_prngkey(seed + 1), **kw)


def _setup(name, recurrent, n):
    """n twin (env, state, obs_of, D) of B_ROLL envs: HH with the feed-forward actor on the full
    observation, TAG with the recurrent actor on the masked columns."""
    from po_brax_amd import envs
    from po_brax_amd import standard_observability_masks as M
    from test_gpu_parity import _keys
    keys = torch.from_numpy(_keys(B_ROLL, 3)).cuda()
    idx = M.po_env_mask(name, cfrc=False) if recurrent else None
    es = [envs.create(name, batch_size=B_ROLL, episode_length=4, obs_mask=idx) for _ in range(n)]
    ss = [e.reset(keys) for e in es]
    D = len(idx) if recurrent else es[0].observation_size
    obs_of = (lambda st: st.info["obs_masked"]) if recurrent else (lambda st: st.obs)
    return es, ss, obs_of, D


def _make(recurrent, env, state, D, normalizer, update):
    from po_brax_amd.rollout import ActorRollout, RecurrentActorRollout
    kw = {} if normalizer is False else {"normalizer": normalizer}
    if recurrent:
        p = _rec_policy(env, D, kw)
        return p, RecurrentActorRollout(env, state, p, T_ROLL, masked=True, **update)
    p = _ff_policy(env, D, kw)
    return p, ActorRollout(env, state, p, T_ROLL, **update)


FIELDS = ("obs", "actions", "logp", "raw", "reward", "done")


def _eager(recurrent, env, s, policy, obs_of):
    """T_ROLL steps of act_into with the table, step_; the trajectory as stacked tensors."""
    done_of = lambda st: st.aux["done"] if "done" in st.aux else st.done  # noqa: E731
    traj = {k: [] for k in FIELDS + ("hidden",)}
    for t in range(T_ROLL):
        obs = obs_of(s)
        traj["obs"].append(obs.clone())
        if recurrent:
            traj["hidden"].append(torch.where(policy.reset[:, None] != 0, torch.zeros_like(policy.hidden), policy.hidden))
        else:
            traj["hidden"].append(torch.zeros(1, device="cuda"))
        a = policy(obs)
        traj["actions"].append(a.clone()); traj["logp"].append(policy.logp.clone()); traj["raw"].append(policy.raw.clone())
        s = env.step_(s, traj["actions"][-1])
        traj["reward"].append(s.reward.clone()); traj["done"].append(done_of(s).float().clone())
        if recurrent:
            policy.reset.copy_(traj["done"][-1])
    return s, {k: torch.stack(v) for k, v in traj.items()}


@pytest.mark.parametrize("name,recurrent", [("ant_heavenhell", False), ("ant_tag", True)])
def test_rollout_with_update_equals_eager_and_reads_the_table_at_replay(name, recurrent):
    from po_brax_amd.training.normalization import ObservationNormalizer
    es, ss, obs_of, D = _setup(name, recurrent, 3)
    norms = [ObservationNormalizer(D) for _ in range(3)]
    p_eager = (_rec_policy if recurrent else _ff_policy)(es[0], D, {"normalizer": norms[0]})
    if recurrent:
        p_eager._buffers(B_ROLL)
    p_graph, roll = _make(recurrent, es[1], ss[1], D, norms[1], {"update_normalizer": True})
    p_twin, twin = _make(recurrent, es[2], ss[2], D, norms[2], {})  # its normaliser is never updated
    s = ss[0]
    for rep in range(2):
        s, traj = _eager(recurrent, es[0], s, p_eager, obs_of)
        norms[0].update(traj["obs"])
        roll.replay(); twin.replay()
        torch.cuda.synchronize()
        for k in FIELDS + (("hidden",) if recurrent else ()):
            assert torch.equal(getattr(roll, k), traj[k]), (name, k, rep)
        assert torch.equal(_bits(norms[1].table), _bits(norms[0].table)) and torch.equal(norms[1].count, norms[0].count)
        assert float(norms[1].count) == (rep + 1) * T_ROLL * B_ROLL
        if rep == 0:  # both started from the identity table
            assert torch.equal(twin.raw, roll.raw)
    # the second replay ran under the table the first one left: not the twin's actions
    assert not torch.equal(twin.raw, roll.raw)
    assert float(norms[2].count) == 0.0 and torch.equal(norms[2].table, _cuda(fresh_table(D)))
    assert not torch.equal(norms[1].table, norms[2].table)


@pytest.mark.parametrize("name,recurrent", [("ant_heavenhell", False), ("ant_tag", True)])
def test_rollout_construction_guards_and_defaults(name, recurrent):
    from po_brax_amd.training.normalization import ObservationNormalizer
    es, ss, obs_of, D = _setup(name, recurrent, 4)
    with pytest.raises(ValueError, match="normalizer"):
        _make(recurrent, es[3], ss[3], D, False, {"update_normalizer": True})
    with pytest.raises(ValueError, match="width"):
        _make(recurrent, es[3], ss[3], D, ObservationNormalizer(D + 1), {})
    _, parent = _make(recurrent, es[0], ss[0], D, False, {})                              # the parent's spelling
    _, default = _make(recurrent, es[1], ss[1], D, None, {"update_normalizer": False})  # the new arguments' defaults
    _, ident = _make(recurrent, es[2], ss[2], D, ObservationNormalizer(D, clip=0.0), {})  # the identity table
    for rep in range(2):
        for r in (parent, default, ident):
            r.replay()
        torch.cuda.synchronize()
        for k in FIELDS + (("hidden",) if recurrent else ()):
            assert torch.equal(getattr(default, k), getattr(parent, k)), (name, k, rep)
            assert torch.equal(getattr(ident, k), getattr(parent, k)), (name, "identity table", k, rep)
