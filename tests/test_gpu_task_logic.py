"""GPU: the kernels' task logic against what the reference's own code returned
(tests/golden/task_logic_*.npz; tests/task_cases.py holds the rule: bit for bit, every env).

The random-action rollouts of the other parity tests almost never reach the task branches
(no heaven, hell, tag, visible target or all-collected ``done`` in 307 200
env-steps per kind), so the arranged cases are the only ones that run the kernels' code for
them.  Each kind's 64 reset cases and 97 one-step cases (a ragged last wave at every lane width)
run on the default launch (sixteen lanes per env at this batch), on the eight-lane kernel
(POB_HEXA_MAX_B=0) and on the four-lane kernel (POB_HEXA_MAX_B=0 POB_OCTET_MAX_B=0), as
tests/test_gpu_headline_parity.py switches them, and the three kinds together through
``create_mixed``; the autoreset wrappers run against the reference's wrapper records.  This file
reads the fixtures only, never the reference tree."""
import numpy as np
import pytest
import torch

import task_cases as TC
from test_gpu_parity import _np

pytestmark = pytest.mark.gpu
LAUNCHES = {"default": {}, "eight_lane": {"POB_HEXA_MAX_B": "0"},
            "four_lane": {"POB_HEXA_MAX_B": "0", "POB_OCTET_MAX_B": "0"}}
_FIX = {}


def _envs():
    from po_brax_amd import envs
    return envs


def _fix(kind):
    if kind not in _FIX:
        _FIX[kind] = TC.load(kind)
    return _FIX[kind]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _set_keys(s, keys):
    s.aux["rng"].view(torch.int32).copy_(_dev(np.ascontiguousarray(keys, np.uint32).view(np.int32)))


def _arrange(kind, s, fix, pre="step"):
    """tests/task_cases.py arrange() on the kernels' own reset"""
    with torch.no_grad():
        pos = s.qp.pos.clone()
        pos[:, :9] += _dev(fix[f"{pre}_off"])[:, None, :]
        pos[:, list(TC.FROZEN[kind])] = _dev(fix[f"{pre}_frozen"])
        s.qp.pos.copy_(pos)
        _set_keys(s, fix[f"{pre}_rng"])


def _outputs(kind, s):
    out = dict(obs=_np(s.obs), reward=_np(s.reward), done=_np(s.done),
               frozen=_np(s.qp.pos)[:, list(TC.FROZEN[kind])], rng=_np(s.aux["rng"]).astype(np.uint32))
    assert tuple(s.metrics) == TC.METRICS[kind]
    out.update({m: _np(s.metrics[m]).astype(np.float32) for m in TC.METRICS[kind]})
    return out


def _launch(monkeypatch, launch):
    for k, v in LAUNCHES[launch].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_reset_matches_reference(monkeypatch, launch, kind):
    _launch(monkeypatch, launch)
    fix = _fix(kind)
    env = _envs().create(kind, batch_size=TC.N_RESET, auto_reset=False)
    s = env.reset(_dev(TC.keys(fix["reset_seed"], TC.N_RESET)))
    TC.compare_reset(kind, dict(pos=_np(s.qp.pos), obs=_np(s.obs), rng=_np(s.info["rng"]).astype(np.uint32)), fix,
                     f"{kind} {launch} reset")
    assert tuple(s.metrics) == TC.RESET_METRICS[kind]
    assert not _np(s.reward).any() and not _np(s.done).any() and not any(_np(v).any() for v in s.metrics.values())


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_step_matches_reference(monkeypatch, launch, kind):
    _launch(monkeypatch, launch)
    fix = _fix(kind)
    env = _envs().create(kind, batch_size=TC.B_STEP, auto_reset=False)
    s = env.reset(_dev(TC.keys(fix["step_seed"], TC.B_STEP)))
    _arrange(kind, s, fix)
    s2 = env.step(s, _dev(fix["step_act"]))
    TC.compare_step(kind, _outputs(kind, s2), fix, f"{kind} {launch} step")


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_last_sensor_slot_matches_reference(monkeypatch, launch):
    """AntGather with ten apples and six bombs (17 envs): a bomb's reading in the last sensor
    slot, kept or zeroed by the -1 wrap of a later object without a bin"""
    _launch(monkeypatch, launch)
    fix = _fix(TC.GA)
    env = _envs().create(TC.GA, batch_size=TC.B_ALT, auto_reset=False, **TC.ALT_PARAMS)
    s = env.reset(_dev(TC.keys(fix["alt_seed"], TC.B_ALT)))
    _arrange(TC.GA, s, fix, "alt")
    s2 = env.step(s, _dev(fix["alt_act"]))
    TC.compare_step(TC.GA, _outputs(TC.GA, s2), fix, f"ant_gather ten apples {launch}", "alt")


def test_mixed_step_matches_reference():
    """the three kinds' arranged cases in one pob_step_mixed launch"""
    mixed = _envs().create_mixed(TC.KINDS, auto_reset=False)
    states = []
    for kind, e in zip(TC.KINDS, mixed.envs):
        s = e.reset(_dev(TC.keys(_fix(kind)["step_seed"], TC.B_STEP)))
        _arrange(kind, s, _fix(kind))
        states.append(s)
    outs = mixed.step(states, [_dev(_fix(kind)["step_act"]) for kind in TC.KINDS])
    for kind, s2 in zip(TC.KINDS, outs):
        TC.compare_step(kind, _outputs(kind, s2), _fix(kind), f"{kind} mixed step")


# ------------------------------------------------------------------------- the wrappers
def _wrap_row(s):
    return dict(pos=_np(s.qp.pos), rot=_np(s.qp.rot), vel=_np(s.qp.vel), ang=_np(s.qp.ang), obs=_np(s.obs),
                reward=_np(s.reward), done=_np(s.done), steps=_np(s.info["steps"]),
                rng=_np(s.aux["rng"]).astype(np.uint32))


def _wrapped(cls, **kw):
    envs = _envs()
    return cls(envs.create(TC.WRAP_KIND, batch_size=TC.WRAP_B, auto_reset=False, episode_length=TC.WRAP_L), **kw)


def test_naive_autoreset_matches_reference():
    fix = _fix(TC.WRAP_KIND)
    keys, steps0, acts = TC.wrap_inputs(fix)
    env = _wrapped(_envs().wrappers.RandomizedAutoResetWrapperNaive)
    s = env.reset(_dev(keys))
    s.info["steps"].copy_(_dev(steps0))
    for t, act in enumerate(acts):
        s = env.step(s, _dev(act))
        TC.compare_wrap("naive", t, _wrap_row(s), fix, "naive")
        TC.same(_np(s.done), fix["naive_inner_done"][t], f"naive step {t}: inner done")


def test_cached_autoreset_matches_reference():
    fix = _fix(TC.WRAP_KIND)
    keys, steps0, acts = TC.wrap_inputs(fix)
    env = _wrapped(_envs().wrappers.RandomizedAutoResetWrapperCached, n_steps_between_updates=TC.WRAP_N)
    s = env.reset(_dev(keys))
    s.info["steps"].copy_(_dev(steps0))
    for t, act in enumerate(acts):
        s = env.step(s, _dev(act))
        TC.compare_wrap("cached", t, _wrap_row(s), fix, "cached")
        TC.same(_np(s.info["first_obs"]), fix["cached_first_obs"][t], f"cached step {t}: first_obs")
        TC.same(_np(s.info["first_qp"].pos), fix["cached_first_pos"][t], f"cached step {t}: first_qp.pos")


def test_gym_autoreset_matches_reference():
    fix = _fix(TC.WRAP_KIND)
    _, steps0, acts = TC.wrap_inputs(fix)
    g = _envs().create_gym_env(TC.WRAP_KIND, batch_size=TC.WRAP_B, seed=TC.GYM_SEED, episode_length=TC.WRAP_L)
    g.reset()
    g._state.info["steps"].copy_(_dev(steps0))
    for t, act in enumerate(acts):
        obs, reward, done, _ = g.step(_dev(act))
        row = _wrap_row(g._state)
        TC.same(_np(obs), row["obs"], f"gym step {t}: returned obs")
        row.update(reward=_np(reward), done=_np(done))
        TC.compare_wrap("gym", t, row, fix, "gym")
        TC.same(_np(done), fix["gym_inner_done"][t], f"gym step {t}: inner done")
        TC.same(_np(g._key).astype(np.uint32), fix["gym_key"][t], f"gym step {t}: gym key")
