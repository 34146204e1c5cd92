"""GPU: k_gae against its restatement (gae_ref of po-brax_amd/csrc/pob_mlp.h: torch.equal, no
tolerance), and the critic pass of the actor rollouts (truncation, final_obs, values, vs,
advantages) against the eager loop and the standalone entry points."""
import numpy as np
import pytest
import torch

from test_gae_host import build_gae_host, ref_gae, trajectory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_gae_host(tmp_path_factory.mktemp("gae_host_gpu"))


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what):
    want = want if isinstance(want, torch.Tensor) else _cuda(want)
    assert torch.equal(_bits(got), _bits(want)), what


def _pob_gae(trunc, second, done_input, reward, scale, values, boot, lam, disc, want_vs=True, want_adv=True):
    """One pob_gae launch on device copies; outputs pre-filled with NaN."""
    from po_brax_amd import _lib
    t = [_cuda(a) for a in (trunc, second, reward, values, boot)]
    T, B = values.shape
    vs = torch.full((T, B), float("nan"), device="cuda") if want_vs else None
    adv = torch.full((T, B), float("nan"), device="cuda") if want_adv else None
    _lib.check(_lib.lib.pob_gae(T, B, _lib.ptr(t[0]), _lib.ptr(t[1]), done_input, _lib.ptr(t[2]), scale, _lib.ptr(t[3]),
                                _lib.ptr(t[4]), lam, disc, _lib.ptr(vs), _lib.ptr(adv), _lib.stream_handle()))
    torch.cuda.synchronize()
    return vs, adv


def _chunk(host):
    return int(host.gae_ref_chunk())


def test_chunk_constant(host):
    """The T values below straddle POB_GAE_CHUNK (the restatement's header is the kernel's)."""
    import re
    from test_gae_host import CSRC
    with open(f"{CSRC}/pob_mlp.h") as f:
        assert int(re.search(r"#define POB_GAE_CHUNK (\d+)", f.read()).group(1)) == _chunk(host) >= 4


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 1000])
def test_kernel_equals_restatement(host, B):
    ch = _chunk(host)
    for T in (1, 2, ch - 1, ch, ch + 1, 2 * ch + 3):
        d = trajectory(np.random.default_rng(1000 * B + T), T, B)
        for done_input, second in ((0, d["term"]), (1, d["done"])):
            want = ref_gae(host, d["trunc"], second, done_input, d["reward"], 0.3, d["values"], d["boot"], 0.95, 0.99)
            got = _pob_gae(d["trunc"], second, done_input, d["reward"], 0.3, d["values"], d["boot"], 0.95, 0.99)
            _same_bits(got[0], want[0], ("vs", B, T, done_input))
            _same_bits(got[1], want[1], ("advantages", B, T, done_input))


@pytest.mark.parametrize("lam,disc", [(1.0, 1.0), (0.0, 0.99), (0.95, 0.0)])
def test_kernel_equals_restatement_other_coefficients(host, lam, disc):
    T, B = 2 * _chunk(host) + 3, 257
    d = trajectory(np.random.default_rng(7), T, B)
    want = ref_gae(host, d["trunc"], d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], lam, disc)
    got = _pob_gae(d["trunc"], d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], lam, disc)
    _same_bits(got[0], want[0], "vs")
    _same_bits(got[1], want[1], "advantages")


def test_nan_reward_stays_in_its_env(host):
    T, B = 2 * _chunk(host) + 3, 257
    d = trajectory(np.random.default_rng(8), T, B)
    clean = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    d["reward"][T - 3, 100] = np.nan
    want = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    got = _pob_gae(d["trunc"], d["term"], 0, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    _same_bits(got[0], want[0], "vs")
    _same_bits(got[1], want[1], "advantages")
    others = torch.arange(B, device="cuda") != 100
    _same_bits(got[0][:, others], clean[0][:, np.arange(B) != 100], "other envs")
    assert bool(torch.isnan(got[1][T - 3, 100])) and bool(torch.isnan(got[0][T - 3, 100]))


def test_subnormal_values(host):
    T, B = _chunk(host) + 1, 65
    d = trajectory(np.random.default_rng(9), T, B)
    for k in ("reward", "values", "boot"):
        d[k] = (d[k] * np.float32(1e-40)).astype(np.float32)
    assert (np.abs(d["values"][d["values"] != 0]) < 1.2e-38).all() and (d["values"] != 0).any()
    want = ref_gae(host, d["trunc"], d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    assert (want[0] != 0).any()
    got = _pob_gae(d["trunc"], d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    _same_bits(got[0], want[0], "vs")
    _same_bits(got[1], want[1], "advantages")


def test_null_truncation_and_null_outputs(host):
    T, B = 2 * _chunk(host) + 3, 65
    d = trajectory(np.random.default_rng(10), T, B)
    want = ref_gae(host, None, d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    got = _pob_gae(None, d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    _same_bits(got[0], want[0], "vs, no truncation")
    _same_bits(got[1], want[1], "advantages, no truncation")
    zeros = _pob_gae(np.zeros_like(d["done"]), d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    _same_bits(zeros[0], want[0], "vs, zeros")
    _same_bits(zeros[1], want[1], "advantages, zeros")
    want = ref_gae(host, d["trunc"], d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    only_vs = _pob_gae(d["trunc"], d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99, want_adv=False)
    only_adv = _pob_gae(d["trunc"], d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99, want_vs=False)
    _same_bits(only_vs[0], want[0], "vs alone")
    _same_bits(only_adv[1], want[1], "advantages alone")


def test_compute_gae_takes_the_kernel_and_is_capturable(host):
    from po_brax_amd.training import compute_gae
    T, B = 2 * _chunk(host) + 3, 257
    d = trajectory(np.random.default_rng(11), T, B)
    ins = [_cuda(d[k]) for k in ("trunc", "term", "reward", "values", "boot")]
    vs, adv = compute_gae(*ins, reward_scaling=0.3)
    want = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], 0.3, d["values"], d["boot"], 0.95, 0.99)
    _same_bits(vs, want[0], "vs")
    _same_bits(adv, want[1], "advantages")
    assert not vs.requires_grad and not adv.requires_grad
    # inputs that require a gradient take the torch spelling; still no graph on the outputs
    v = ins[3].clone().requires_grad_(True)
    vs_t, adv_t = compute_gae(ins[0], ins[1], ins[2], v, ins[4], reward_scaling=0.3)
    assert not vs_t.requires_grad and not adv_t.requires_grad
    torch.testing.assert_close(vs_t, vs, rtol=1e-5, atol=1e-3)
    # captured with out=, replayed after the inputs changed in place
    out = (torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = compute_gae(*ins, reward_scaling=0.3, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(out[0], want[0], "vs, replay 1")
    e = trajectory(np.random.default_rng(12), T, B)
    for t, k in zip(ins, ("trunc", "term", "reward", "values", "boot")):
        t.copy_(_cuda(e[k]))
    graph.replay()
    torch.cuda.synchronize()
    want = ref_gae(host, e["trunc"], e["term"], 0, e["reward"], 0.3, e["values"], e["boot"], 0.95, 0.99)
    _same_bits(out[0], want[0], "vs, replay 2")
    _same_bits(out[1], want[1], "advantages, replay 2")


# ---------------------------------------------------------------------------- rollouts
B_ROLL = 64
FIELDS = ("obs", "actions", "raw", "logp", "reward", "done")
GAE = dict(lambda_=0.9, discount=0.97, reward_scaling=0.5)


def _envs(name, n, mask):
    from po_brax_amd import envs
    from po_brax_amd import standard_observability_masks as M
    from test_gpu_parity import _keys
    keys = torch.from_numpy(_keys(B_ROLL, 3)).cuda()
    idx = M.po_env_mask(name, cfrc=False) if mask else None
    es = [envs.create(name, batch_size=B_ROLL, episode_length=3, obs_mask=idx) for _ in range(n)]
    return es, [e.reset(keys) for e in es], (len(idx) if mask else es[0].observation_size)


def _critic(D, normalizer, seed=9):
    from po_brax_amd import jumpy
    from po_brax_amd.training import ValueFunction, networks
    model = networks.make_models(16, D)[1]
    params = model.init(jumpy.random_prngkey(seed))
    return ValueFunction(model, params, normalizer=normalizer)


def _ff_policy(env, D, normalizer, seed=5):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_models(2 * env.action_size, D)[0]
    params = model.init(jumpy.random_prngkey(seed))
    params.theta.mul_(3.0)
    return networks.NormalTanhPolicy(model, params, jumpy.random_prngkey(seed + 1), normalizer=normalizer)


def _rec_policy(env, D, normalizer, seed=5):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_recurrent_model([], 64, [2 * env.action_size], D)
    params = model.init(jumpy.random_prngkey(seed))
    params.theta.mul_(3.0)
    return networks.RecurrentTanhPolicy(model, params, jumpy.random_prngkey(seed + 1), normalizer=normalizer)


def _standalone_values(critic, rows):
    """pob_mlp_forward_norm over (N, D) rows under the critic's table as it stands now."""
    from po_brax_amd import _lib
    rows = rows.contiguous()
    out = torch.full((rows.shape[0],), float("nan"), device="cuda")
    n = critic.normalizer
    _lib.check(_lib.lib.pob_mlp_forward_norm(critic.model.mlp.handle, rows.shape[0], _lib.ptr(rows), _lib.ptr(critic.theta),
                                             _lib.ptr(out), _lib.ptr(n.table), n.clip, _lib.stream_handle()))
    torch.cuda.synchronize()
    return out


def _check_critic_outputs(host, roll, critic, T, D, what):
    from po_brax_amd.training import compute_gae
    rows = torch.cat([roll.obs, roll.final_obs[None]]).reshape((T + 1) * B_ROLL, D)
    _same_bits(roll.values.reshape(-1), _standalone_values(critic, rows), (what, "values"))
    term = roll.done * (1.0 - roll.truncation)
    vs, adv = compute_gae(roll.truncation, term, roll.reward, roll.values[:T].contiguous(), roll.values[T].contiguous(),
                          **GAE)
    _same_bits(roll.vs, vs, (what, "vs against compute_gae"))
    _same_bits(roll.advantages, adv, (what, "advantages against compute_gae"))
    n = lambda t: t.cpu().numpy()  # noqa: E731
    want = ref_gae(host, n(roll.truncation), n(roll.done), 1, n(roll.reward), GAE["reward_scaling"], n(roll.values[:T]),
                   n(roll.values[T]), GAE["lambda_"], GAE["discount"])
    _same_bits(roll.vs, want[0], (what, "vs against gae_ref"))
    _same_bits(roll.advantages, want[1], (what, "advantages against gae_ref"))
    assert bool(torch.isfinite(roll.vs).all()) and bool(torch.isfinite(roll.advantages).all())


def test_actor_rollout_with_critic(host):
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training.normalization import ObservationNormalizer
    T = 7
    es, ss, D = _envs("ant_heavenhell", 3, False)
    norms = [ObservationNormalizer(D) for _ in range(3)]
    p_plain = _ff_policy(es[0], D, norms[0])
    plain = ActorRollout(es[0], ss[0], p_plain, T, update_normalizer=True)
    p_crit = _ff_policy(es[1], D, norms[1])
    critic = _critic(D, norms[1])
    roll = ActorRollout(es[1], ss[1], p_crit, T, update_normalizer=True, critic=critic, gae=GAE)
    p_eager = _ff_policy(es[2], D, norms[2])
    s = ss[2]
    assert roll.obs.shape == (T, B_ROLL, D) and roll.obs.is_contiguous() and roll.final_obs.shape == (B_ROLL, D)
    assert roll.values.shape == (T + 1, B_ROLL) and roll.vs.shape == roll.advantages.shape == (T, B_ROLL)
    for rep in range(2):
        trunc, rows = [], []
        for t in range(T):  # the eager loop from the same state and key
            a = torch.empty((B_ROLL, es[2].action_size), device="cuda")
            rows.append(s.obs.clone())
            p_eager.act_into(s.obs, a)
            s = es[2].step_(s, a)
            trunc.append(s.aux["truncation"].clone())
        norms[2].update(torch.stack(rows))  # the next replay acts under the updated table
        plain.replay()
        roll.replay()
        torch.cuda.synchronize()
        for k in FIELDS:
            assert torch.equal(_bits(getattr(roll, k)), _bits(getattr(plain, k))), (k, rep)
        assert torch.equal(norms[1].table, norms[0].table)
        assert torch.equal(roll.truncation, torch.stack(trunc)), rep
        _same_bits(roll.final_obs, s.obs, ("final_obs", rep))
        assert {float(v) for v in roll.truncation.unique()} == {0.0, 1.0}
        # truncations fall inside the unroll: not at its ends only
        assert bool(roll.truncation[1:T - 1].any()) and bool((roll.truncation * roll.done == roll.truncation).all())
        assert torch.equal(norms[1].table, norms[2].table) and float(norms[1].count) == (rep + 1) * T * B_ROLL
        _check_critic_outputs(host, roll, critic, T, D, ("actor", rep))  # under the table AFTER the replay's update
    # the critic's parameters are read at replay time
    critic.theta.mul_(1.5)
    before = roll.values.clone()
    roll.replay()
    torch.cuda.synchronize()
    assert not torch.equal(roll.values, before)
    _check_critic_outputs(host, roll, critic, T, D, ("actor", "theta changed"))


def test_recurrent_rollout_with_critic_on_masked_columns(host):
    from po_brax_amd.rollout import RecurrentActorRollout
    from po_brax_amd.training.normalization import ObservationNormalizer
    T = 5
    es, ss, D = _envs("ant_tag", 2, True)
    norms = [ObservationNormalizer(D) for _ in range(2)]
    plain = RecurrentActorRollout(es[0], ss[0], _rec_policy(es[0], D, norms[0]), T, masked=True, update_normalizer=True)
    critic = _critic(D, norms[1])
    roll = RecurrentActorRollout(es[1], ss[1], _rec_policy(es[1], D, norms[1]), T, masked=True, update_normalizer=True,
                                 critic=critic, gae=GAE)
    assert roll.obs.shape == (T, B_ROLL, D) and D < es[1].observation_size
    for rep in range(2):
        plain.replay()
        roll.replay()
        torch.cuda.synchronize()
        for k in FIELDS + ("hidden",):
            assert torch.equal(_bits(getattr(roll, k)), _bits(getattr(plain, k))), (k, rep)
        _same_bits(roll.final_obs, roll.state.info["obs_masked"], ("final_obs", rep))
        assert bool(roll.truncation.any()) and not bool(roll.truncation.all())
        _check_critic_outputs(host, roll, critic, T, D, ("recurrent", rep))


def test_defaults_unchanged_and_guards():
    from po_brax_amd.rollout import ActorRollout
    T = 4
    es, ss, D = _envs("ant_heavenhell", 4, False)
    roll = ActorRollout(es[0], ss[0], _ff_policy(es[0], D, None), T)
    assert not hasattr(roll, "final_obs") and not hasattr(roll, "truncation") and not hasattr(roll, "values")
    assert roll.obs.shape == (T, B_ROLL, D) and roll.obs.untyped_storage().nbytes() == T * B_ROLL * D * 4
    # record_truncation alone: the rows, no critic buffers
    rec = ActorRollout(es[1], ss[1], _ff_policy(es[1], D, None), T, record_truncation=True)
    roll.replay()
    rec.replay()
    torch.cuda.synchronize()
    for k in FIELDS:
        assert torch.equal(_bits(getattr(rec, k)), _bits(getattr(roll, k))), k
    assert rec.truncation.shape == (T, B_ROLL) and bool(rec.truncation[2].any()) and not bool(rec.truncation[:2].any())
    assert bool((rec.truncation * rec.done == rec.truncation).all())
    assert not hasattr(rec, "final_obs") and rec.obs.untyped_storage().nbytes() == T * B_ROLL * D * 4
    with pytest.raises(ValueError, match="width"):
        ActorRollout(es[2], ss[2], _ff_policy(es[2], D, None), T, critic=_critic(D + 1, None))
    with pytest.raises(TypeError, match="ValueFunction"):
        ActorRollout(es[2], ss[2], _ff_policy(es[2], D, None), T, critic=object())
    with pytest.raises(ValueError, match="gae="):
        ActorRollout(es[2], ss[2], _ff_policy(es[2], D, None), T, critic=_critic(D, None), gae={"gamma": 0.9})


def test_env_without_a_time_limit_records_zeros():
    from po_brax_amd import envs
    from po_brax_amd.rollout import ActorRollout
    from test_gpu_parity import _keys
    T = 3
    env = envs.create("ant_heavenhell", batch_size=B_ROLL, episode_length=None)
    state = env.reset(torch.from_numpy(_keys(B_ROLL, 3)).cuda())
    D = env.observation_size
    roll = ActorRollout(env, state, _ff_policy(env, D, None), T, critic=_critic(D, None))
    roll.replay()
    torch.cuda.synchronize()
    assert roll.truncation.shape == (T, B_ROLL) and not bool(roll.truncation.any())
    assert bool(torch.isfinite(roll.values).all()) and bool(torch.isfinite(roll.advantages).all())
