"""GPU: the wall-contact overflow paths of the sixteen- and eight-lane step kernels, bit-exact
against the oracle on every field.

k_step_hex keeps a wave's wall contacts of a collide substep in an LDS pool of HPOOL_N = 64
entries (pob_hexa.h); past it the lanes with contacts walk their contact faces again in the
position pass and in the velocity pass.  k_step_oct does the same for HH (OPOOL_N = 64) and keeps
OMAXC = 4 contacts per lane for TAG and GA, a lane with more re-walking from its stored segments
(pob_octet.h).  Neither kernel leaves a mark to read, so every test asserts from the oracle's
contact record of the very states the kernel stepped (tests/wall_arrange.py: roles, the two bounds
per wave, the per-lane counts) that the launch held the waves and lanes it is there for, and a
test whose states miss a condition fails.  The step-0 conditions are asserted before the kernel
steps; tests/test_wall_arrange_host.py asserts the same on the CPU.

One setup: B = 261 (sixteen lanes: 65 waves and a one-env tail; eight lanes: 32 waves and five
envs) or 257, the arrangement of wall_arrange.roles_for placed on the reset state, T = 4 steps of
one-step parity with the oracle restarted from the GPU's state, episode_length 1 000; before step 2
the heavy envs are placed again by the same rule (left alone they drift off the corner: on the
oracle's own rollout the sixteen-lane HH launch holds no wave that overflows for certain in steps
1 to 3).  Kernel selection as elsewhere in the suite: the default is sixteen lanes at these
batches, POB_HEXA_MAX_B=0 eight."""
import time

import numpy as np
import pytest
import torch

import orc
import wall_arrange as WA
from test_gpu_parity import compare_states
from test_gpu_variants import _assert_fp16_step, _state_np32

pytestmark = pytest.mark.gpu
HH, GA, TAG = "ant_heavenhell", "ant_gather", "ant_tag"


def _teleport(s, off):
    """the 9 ant bodies moved by off, one rounding to the storage type (wall_arrange.place)"""
    pos = s.qp.pos.float()
    pos[:, :9, :2] += torch.from_numpy(off).cuda()[:, None, :]
    s.qp.pos.copy_(pos.to(s.qp.pos.dtype))


def _run(monkeypatch, name, B, W, qp_dtype=torch.float32, poke=None, check0=None, check_later=None):
    """the shared setup; check0(rec, roles, rec_unpoked) asserts the step-0 conditions before the
    kernel steps, check_later(waves that overflow for certain, per step) after the last step"""
    from po_brax_amd import envs
    t0 = time.time()
    if W == 8:
        monkeypatch.setenv("POB_HEXA_MAX_B", "0")
    npdt = np.float16 if qp_dtype == torch.float16 else np.float32
    env = envs.create(name, batch_size=B, episode_length=1000, qp_dtype=qp_dtype)
    s = env.reset(torch.from_numpy(WA.keys(B)).cuda())
    acts, roles = WA.actions(B), WA.roles_for(B)
    o = orc.OracleEnv(name)
    heavy = roles == WA.HEAVY
    rec_unpoked = None
    with torch.no_grad():
        off = WA.arrange(name, _state_np32(s), acts[0], roles, npdt)
        _teleport(s, off)
        if poke is not None:
            rec_unpoked = WA.record(o, _state_np32(s), acts[0])[1]
            s.qp.vel[poke, 0, 0] = 1e25
            heavy[poke] = False  # (not placed again: its state is not finite)
    recs = []
    for t, act in enumerate(acts):
        if t == 2:
            with torch.no_grad():
                off = WA.arrange(name, _state_np32(s), act, roles, npdt, only=heavy)
                _teleport(s, off)
        so, rec = WA.record(o, _state_np32(s), act)
        recs.append(rec)
        print(f"{name} B={B} W={W} step {t}: {WA.pool_conditions(rec, W, roles)} lanes {WA.lane_conditions(rec)}")
        if t == 0 and check0 is not None:
            check0(rec, roles, rec_unpoked)
        s = env.step(s, torch.from_numpy(act).cuda())
        if qp_dtype == torch.float16:
            _assert_fp16_step(s, so, f"{name} B={B} W={W} fp16 step {t}")
        else:
            compare_states(s, so, f"{name} B={B} W={W} step {t}")
    n_ovf = [int(WA.wave_kinds(r, W)[0].sum()) for r in recs]
    print(f"{name} B={B} W={W}: waves that overflow for certain per step {n_ovf}; {time.time() - t0:.2f} s")
    if check_later is not None:
        check_later(n_ovf)


def _pool0(W):
    def check(rec, roles, _):
        WA.assert_pool(WA.pool_conditions(rec, W, roles), W)
    return check


def _hh_later(n_ovf):
    assert max(n_ovf[1:]) >= 1, n_ovf


@pytest.mark.parametrize("name", [HH, TAG, GA])
def test_sixteen_lane_pool(monkeypatch, name):
    """step 0: >= 2 waves that overflow for certain, >= 8 with contacts that for certain never do,
    a clear wave, and an overflowing wave-substep with contact-free bodies beside bodies with
    contacts (the povf && nct > 0 split); HH: a wave that overflows for certain after step 0 too"""
    _run(monkeypatch, name, 261, 4, check0=_pool0(4), check_later=_hh_later if name == HH else None)


def test_eight_lane_pool(monkeypatch):
    """step 0: >= 2 waves that overflow for certain, one of them five heavy envs and three idle
    ones (the re-walk with whole envs idle), waves that for certain do not, a clear wave"""
    _run(monkeypatch, HH, 261, 8, check0=_pool0(8), check_later=_hh_later)


@pytest.mark.parametrize("name", [TAG, GA])
def test_eight_lane_store(monkeypatch, name):
    """lanes with exactly OMAXC contacts (kept in the store), with more (re-walk), with none, and
    the three in one wave-substep"""
    def check(rec, roles, _):
        WA.assert_lanes(WA.lane_conditions(rec))
    _run(monkeypatch, name, 261, 8, check0=check)


@pytest.mark.parametrize("W,B", [(4, 261), (8, 257)])
def test_ragged_tail(monkeypatch, W, B):
    """env B - 1 heavy and the only live env of its wave: the lanes past the batch replay it, so by
    the padded model the wave overflows for certain (W copies of 17 or more contacts)"""
    def check(rec, roles, _):
        assert B % W == 1 and roles[B - 1] == WA.HEAVY
        assert WA.tail_overflows(rec, W) is True, WA.wave_bounds(rec, W)
    _run(monkeypatch, HH, B, W, check0=check)


@pytest.mark.parametrize("W,gacc", [(4, "1"), (4, "0"), (8, "1"), (8, "0")])
def test_guard_rerun_with_contacts(monkeypatch, W, gacc):
    """env 1 of wave 0 (all heavy: it overflows for certain before the poke) with its torso at
    1e25 m/s: under GuardAcc the wave reruns its substeps under the branch guards, pool overflow
    and re-walks included; parity on every field (NaN and inf too) in that env and its neighbours.
    With the poked env gone the eight-lane wave still overflows for certain (seven heavy envs); the
    sixteen-lane wave's three others pass 64 only in the kernel's own count, the upper bound
    (wall_arrange's docstring), which is what this case asserts for it."""
    monkeypatch.setenv("POB_HEX_GACC" if W == 4 else "POB_OCT_GACC", gacc)

    def check(rec, roles, rec_unpoked):
        k = WA.guard_conditions(rec_unpoked, rec, W, 1)
        print(k)
        assert k["lower_before"] > WA.POOL_N, k
        assert (k["lower"] if W == 8 else k["upper"]) > WA.POOL_N, k
    _run(monkeypatch, HH, 261, W, poke=1, check0=check)


@pytest.mark.parametrize("W", [4, 8])
def test_pools_fp16_storage(monkeypatch, W):
    """binary16 qp storage: placed on the decoded fp16 state, the conditions from the record of
    that state, the oracle's step rounded to binary16 equal to the kernel's bit for bit"""
    _run(monkeypatch, HH, 261, W, qp_dtype=torch.float16, check0=_pool0(W), check_later=_hh_later)
