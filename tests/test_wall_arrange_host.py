"""CPU: the arranged wall states of tests/test_gpu_lane_pools.py hold what those tests are there
for.  The oracle's reset equals the kernels' reset bit for bit (tests/test_gpu_parity.py), so the
state every GPU case steps first is known here: each case's arrangement (tests/wall_arrange.py) is
built from the oracle's reset and its step-0 conditions asserted from the oracle's contact record;
the later steps are the oracle's own rollout with the heavy envs placed again before step 2, as
the GPU tests do."""
import numpy as np
import pytest

import orc
import wall_arrange as WA

HH, GA, TAG = "ant_heavenhell", "ant_gather", "ant_tag"
_cache = {}


def _case(name, B, dtype=np.float32):
    """(placed state, roles, actions, step-0 record), one arrangement per (kind, B, storage)"""
    k = (name, B, np.dtype(dtype).name)
    if k not in _cache:
        acts, roles = WA.actions(B), WA.roles_for(B)
        s, off = WA.arrange_from_keys(name, WA.keys(B), acts[0], roles, dtype)
        st = WA.place(s, off, dtype)
        _cache[k] = (st, roles, acts, WA.record(orc.OracleEnv(name), st, acts[0])[1])
    return _cache[k]


@pytest.mark.parametrize("name", [HH, TAG, GA])
def test_roles_hold(name):
    _, roles, _, rec = _case(name, 261)
    c0 = rec[:, 0].sum(-1)
    assert (c0[roles == WA.HEAVY] >= 17).all(), c0[roles == WA.HEAVY]
    assert rec[roles == WA.CLEAR].sum() == 0
    light = rec[roles == WA.LIGHT].sum(-1)
    assert (light[:, 0] >= 1).all() and light.max() <= 3, light


@pytest.mark.parametrize("name,dtype", [(HH, np.float32), (TAG, np.float32), (GA, np.float32), (HH, np.float16)])
def test_sixteen_lane_pool_conditions(name, dtype):
    _, roles, _, rec = _case(name, 261, dtype)
    k = WA.pool_conditions(rec, 4, roles)
    print(name, np.dtype(dtype).name, k)
    WA.assert_pool(k, 4)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_eight_lane_pool_conditions(dtype):
    _, roles, _, rec = _case(HH, 261, dtype)
    k = WA.pool_conditions(rec, 8, roles)
    print(np.dtype(dtype).name, k)
    WA.assert_pool(k, 8)


@pytest.mark.parametrize("name", [TAG, GA])
def test_eight_lane_store_conditions(name):
    k = WA.lane_conditions(_case(name, 261)[3])
    print(name, k)
    WA.assert_lanes(k)


@pytest.mark.parametrize("W,B", [(4, 261), (8, 257)])
def test_ragged_tail_conditions(W, B):
    """env B - 1 heavy and alone in its wave: replayed W times over it overflows for certain"""
    _, roles, _, rec = _case(HH, B)
    assert B % W == 1 and roles[B - 1] == WA.HEAVY
    lower, upper = WA.wave_bounds(rec, W)
    print(W, B, "tail lower", lower[-1], "upper", upper[-1])
    assert WA.tail_overflows(rec, W) is True


@pytest.mark.parametrize("W", [4, 8])
def test_guard_rerun_conditions(W):
    """env 1 (wave 0, all heavy) poked: before the poke the wave overflows for certain; with it the
    eight-lane wave still does (seven heavy envs), the sixteen-lane wave's three other envs reach
    the pool's size only in the kernel's own count (the upper bound; wall_arrange's docstring)"""
    st, roles, acts, rec0 = _case(HH, 261)
    st = {k: v.copy() for k, v in st.items()}
    WA.poke(st, 1)
    rec = WA.record(orc.OracleEnv(HH), st, acts[0])[1]
    k = WA.guard_conditions(rec0, rec, W, 1)
    print(W, k)
    assert k["lower_before"] > WA.POOL_N, k
    assert (k["lower"] if W == 8 else k["upper"]) > WA.POOL_N, k


@pytest.mark.parametrize("name", [HH, TAG, GA])
def test_later_steps(name):
    """the oracle's own rollout: waves that overflow for certain per step; HH keeps one after step 0
    on both kernels once the heavy envs are placed again before step 2"""
    st, roles, acts, _ = _case(name, 261)
    o = orc.OracleEnv(name)
    n = {4: [], 8: []}
    for t, act in enumerate(acts):
        if t == 2:
            st = WA.place(st, WA.arrange(name, st, act, roles, only=roles == WA.HEAVY))
        st, rec = WA.record(o, st, act)
        for W in n:
            n[W].append(int(WA.wave_kinds(rec, W)[0].sum()))
    print(name, n)
    if name == HH:
        assert max(n[4][1:]) >= 1 and max(n[8][1:]) >= 1, n
