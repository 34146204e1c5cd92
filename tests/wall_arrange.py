"""Arranged wall states for the sixteen- and eight-lane step kernels' contact pools and per-lane
stores, chosen and judged on the C oracle alone (oracle/orc.py and numpy; no GPU, no product code).

The kernels keep a wave's wall contacts of a collide substep in a pool of 64 entries (pob_hexa.h
HPOOL_N, pob_octet.h OPOOL_N for HH) or, on the eight-lane kernel for TAG and GA, in a per-lane
store of OMAXC = 4 contacts; past either the lanes walk their contact faces again.  Random wall
states put more than 64 contacts, each body counted once, into one wave at no useful rate (the
worst random env holds 18 in a substep), so no test on them can say that a pool overflowed, and none reaches
the eight-lane kernel's two paths at all (the mutation table).  This module
teleports ants by role:

  heavy     the best point of a seeded candidate set within 0.6 of a wall corner (CORNERS), judged
            by the env's wall contacts in the first collide substep;
  clear     a point at least 3 m from every wall: no contact;
  ordinary  three of four onto the walls (tests/test_gpu_torso_once.py _teleport_offsets);
  light     a point where the env holds one to three contacts in every collide substep it has any,
            and at least one in the first.

The oracle's contact record (orc_contacts_record) gives the wall contacts c[env, substep, body]
(body 0 the torso, 2 k + 1 Aux k + 1, 2 k + 2 lower leg k).  A wave is W consecutive envs (W = 4
on sixteen lanes, 8 on eight); both kernels let the lanes past the batch of the last wave replay
env B - 1 (k_step_hex / k_step_oct: ``bl = act_lane ? b : B - 1``), so the model pads a ragged
tail with copies of env B - 1.  Two bounds per wave and substep:

  lower  sum of c over the wave's envs and bodies, each body once.  lower > 64: the pool
         overflowed however the kernel counts its body replicas.
  upper  4 x torso + 2 x Aux + lower legs.  upper <= 64: it did not.

Which one the kernels count: the UPPER one, exactly.  Every lane hands mesh_wave_walk the item mask
of its own body (sixteen lanes: one body per lane, the torso on four lanes, an Aux body on two;
eight lanes: slots torso + Aux k on A_k, Aux k + lower leg k on B_k), the walk evaluates every
lane's items, and the sinks' store() adds the ballot of every winner lane's hit to npool -- the
replicas' contacts are stored once per replica.  The tests' conditions still use the two bounds
only, so they hold for either count.

The eight-lane per-lane store counts per lane: lane A_k torso + Aux k, lane B_k Aux k + lower leg k
(lane_counts)."""
import numpy as np

import orc

NSUB = 5          # collide substeps per step
POOL_N = 64       # HPOOL_N, OPOOL_N
OMAXC = 4         # the eight-lane kernel's per-lane store
FLAGS = orc.F_EPISODE | orc.F_AUTORESET
HEAVY, CLEAR, ORDINARY, LIGHT = 0, 1, 2, 3
N_CAND = 384      # heavy candidates per env
N_LIGHT_CAND = 96
# a wall corner per kind with room for an ant on both faces (scanned on the oracle over all box
# corners with 64 candidates each; these gave the most contacts in the first collide substep)
CORNERS = {"ant_heavenhell": (-2.43, -0.39), "ant_tag": (5.33, -5.34), "ant_gather": (7.25, -7.0)}
_REPL = np.array([4, 2, 1, 2, 1, 2, 1, 2, 1])  # lanes holding body i (both kernels)


def wall_distance(xy, walls):
    """distance (xy) of each point to the nearest wall box; walls: orc.OracleEnv.walls() rows"""
    xy = np.asarray(xy, np.float64)
    d = np.full(len(xy), np.inf)
    for cx, cy, c, s, hx, hy in np.asarray(walls, np.float64):
        dx, dy = xy[:, 0] - cx, xy[:, 1] - cy
        lx, ly = dx * c + dy * s, -dx * s + dy * c
        d = np.minimum(d, np.hypot(np.maximum(np.abs(lx) - hx, 0), np.maximum(np.abs(ly) - hy, 0)))
    return d


def arena_box(walls):
    lo, hi = np.full(2, np.inf), np.full(2, -np.inf)
    for cx, cy, c, s, hx, hy in np.asarray(walls, np.float64):
        ex, ey = abs(c) * hx + abs(s) * hy, abs(s) * hx + abs(c) * hy
        lo = np.minimum(lo, [cx - ex, cy - ey]); hi = np.maximum(hi, [cx + ex, cy + ey])
    return lo, hi


def roles_for(B):
    """envs 0..12 heavy, 13..23 clear, 24..31 light, env B - 1 heavy, the rest ordinary: with W = 4
    waves 0, 1, 2 all heavy, wave 3 one heavy + three clear, 4 and 5 clear, 6 and 7 light; with
    W = 8 wave 0 all heavy, wave 1 five heavy + three clear, wave 2 clear, wave 3 light.  Env B - 1
    is the only live env of its wave when B = 1 (mod W)."""
    r = np.full(B, ORDINARY)
    r[0:13] = HEAVY; r[13:24] = CLEAR; r[24:32] = LIGHT; r[B - 1] = HEAVY
    return r


def place(state, off, dtype=np.float32):
    """the state with the 9 ant bodies of every env moved by off (B, 2), in the storage type's
    rounding (as ``qp.pos[:, :9, :2] += off`` on a tensor of that type), decoded to float32"""
    out = {k: v.copy() for k, v in state.items()}
    p = out["pos"]
    p[:, :9, :2] = (p[:, :9, :2] + np.asarray(off, np.float32)[:, None, :]).astype(dtype).astype(np.float32)
    return out


def record(oenv, state, act, L=1000):
    """(next state, wall contacts (B, NSUB, 9)) of one oracle step from state"""
    return oenv.step_recorded(state, act, NSUB, flags=FLAGS, episode_length=L)


def _probe(oenv, state, act, i, pts, dtype, L):
    """env i teleported to each of pts: the record (len(pts), NSUB, 9)"""
    n = len(pts)
    rep = {k: np.ascontiguousarray(np.repeat(v[i:i + 1], n, 0)) for k, v in state.items()}
    off = np.asarray(pts, np.float32) - rep["pos"][:, 0, :2]
    return record(oenv, place(rep, off, dtype), np.ascontiguousarray(np.repeat(act[i:i + 1], n, 0)), L)[1]


def heavy_candidates(name, seed=3):
    rng = np.random.default_rng(seed)
    r, a = 0.6 * np.sqrt(rng.uniform(0, 1, N_CAND)), rng.uniform(0, 2 * np.pi, N_CAND)
    return (np.array(CORNERS[name]) + np.stack([r * np.cos(a), r * np.sin(a)], 1)).astype(np.float32)


def arrange(name, state, act, roles, dtype=np.float32, seed=3, L=1000, only=None):
    """xy teleport offsets (B, 2) float32 for the envs' roles, from a state (oracle layout, float32;
    binary16 storage: the decoded state and dtype=np.float16) and the first action.  ``only``: a
    bool mask of the envs to place (the others get a zero offset)."""
    oenv = orc.OracleEnv(name)
    walls = oenv.walls()
    B = len(roles)
    rng = np.random.default_rng(seed)
    lo, hi = arena_box(walls)
    xy0 = state["pos"][:, 0, :2]
    xy = xy0.copy()
    todo = np.ones(B, bool) if only is None else np.asarray(only, bool)
    # ordinary: three of four within 1.0 of a wall, the rest anywhere in the arena's box
    cand = rng.uniform(lo, hi, (16 * B, 2))
    near = cand[wall_distance(cand, walls) < 1.0]
    assert len(near) >= 3 * B // 4
    ordn = np.concatenate([near[: 3 * B // 4], cand[: B - 3 * B // 4]]).astype(np.float32)[rng.permutation(B)]
    # clear: at least 3 m from every wall (inside or outside the arena)
    cc = rng.uniform(lo - 5.0, hi + 5.0, (64 * B, 2))
    cc = cc[wall_distance(cc, walls) >= 3.25].astype(np.float32)
    assert len(cc) >= B
    hc = heavy_candidates(name, seed)
    lc = rng.uniform(lo, hi, (64 * N_LIGHT_CAND, 2))
    dl = wall_distance(lc, walls)
    lc = lc[(dl > 0.25) & (dl < 0.9)][:N_LIGHT_CAND].astype(np.float32)
    assert len(lc) == N_LIGHT_CAND
    for i in range(B):
        if not todo[i]:
            continue
        if roles[i] == ORDINARY:
            xy[i] = ordn[i]
        elif roles[i] == CLEAR:
            xy[i] = cc[i]
        elif roles[i] == HEAVY:
            c = _probe(oenv, state, act, i, hc, dtype, L)[:, 0].sum(-1)
            xy[i] = hc[int(np.argmax(c))]                      # (the first of the best)
        else:
            c = _probe(oenv, state, act, i, lc, dtype, L).sum(-1)   # (candidate, substep)
            ok = (c[:, 0] >= 1) & (c.max(1) <= 3)
            assert ok.any(), (name, i, "no light point among the candidates")
            xy[i] = lc[int(np.argmax(ok))]
    off = (xy - xy0).astype(np.float32)
    off[~todo] = 0.0
    return off


KEY_SEED, ACT_SEED, T = 5, 13, 4


def keys(B, seed=KEY_SEED):
    import pob_np as P
    return P.split(P.prngkey(seed), B + 1)[1:]


def actions(B, seed=ACT_SEED, steps=T):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, (B, 8)).astype(np.float32) for _ in range(steps)]


def reset_state(name, keys, dtype=np.float32):
    """the oracle's reset (the kernels' reset bit for bit; binary16 storage: rounded qp, decoded)"""
    s = orc.OracleEnv(name).reset(keys, first=True)
    if dtype != np.float32:
        for k in ("pos", "rot", "vel", "ang", "first_pos", "first_rot", "first_vel", "first_ang"):
            s[k] = s[k].astype(dtype).astype(np.float32)
    return s


def arrange_from_keys(name, keys, act, roles, dtype=np.float32, seed=3):
    """arrange() from the reset of keys: (the reset state, the offsets)"""
    s = reset_state(name, keys, dtype)
    return s, arrange(name, s, act, roles, dtype, seed)


def poke(state, env):
    """a torso at 1e25 m/s (tests/test_gpu_headline_parity.py
    test_out_of_range_inputs_take_exact_fallbacks): the wave's GuardAcc pass reruns"""
    state["vel"][env, 0, 0] = 1e25


def guard_conditions(rec_before, rec, W, env):
    """the wave of the poked env: lower bound before the poke (rec_before: the same state and
    action without it), both bounds with it"""
    w = env // W
    lb, _ = wave_bounds(rec_before, W)
    lo, up = wave_bounds(rec, W)
    return dict(lower_before=int(lb[w].max()), lower=int(lo[w].max()), upper=int(up[w].max()))


# ------------------------------------------------------------------ the bounds and the conditions
def _pad(rec, W):
    """(B, NSUB, 9) -> (waves, W, NSUB, 9): the lanes past the batch replay env B - 1"""
    B = rec.shape[0]
    n = -(-B // W) * W
    return np.concatenate([rec, np.repeat(rec[-1:], n - B, 0)]).reshape(n // W, W, *rec.shape[1:])


def wave_bounds(rec, W):
    """(lower, upper), each (waves, NSUB): every body once; 4 x torso + 2 x Aux + lower legs"""
    w = _pad(rec, W)
    return w.sum((1, 3)), (w * _REPL).sum((1, 3))


def lane_counts(rec):
    """the eight-lane kernel's contacts per lane (B, NSUB, 8): lanes 0..3 A_k = torso + Aux k,
    lanes 4..7 B_k = Aux k + lower leg k"""
    torso, aux, leg = rec[..., :1], rec[..., 1::2], rec[..., 2::2]
    return np.concatenate([torso + aux, aux + leg], -1)


def wave_kinds(rec, W):
    """per wave: overflows for certain in some substep; holds contacts and for certain never
    overflows; holds none"""
    lower, upper = wave_bounds(rec, W)
    return (lower > POOL_N).any(1), (lower.sum(1) > 0) & (upper <= POOL_N).all(1), lower.sum(1) == 0


def pool_conditions(rec, W, roles=None):
    """the counts behind the pool tests' conditions (see assert_pool)"""
    lower, upper = wave_bounds(rec, W)
    ovf, calm, clear = wave_kinds(rec, W)
    w = _pad(rec, W)                                            # (waves, W, NSUB, 9)
    # an overflowing wave-substep with bodies of both kinds: contacts, none (povf && nct > 0 splits)
    o = lower > POOL_N                                          # (waves, NSUB)
    body = w.transpose(0, 2, 1, 3).reshape(w.shape[0], NSUB, -1)  # (waves, NSUB, W * 9)
    split = o & (body == 0).any(-1) & (body > 0).any(-1)
    out = dict(overflow=int(ovf.sum()), calm=int(calm.sum()), clear=int(clear.sum()), split=int(split.sum()),
               lower_max=int(lower.max()), upper_max=int(upper.max()),
               unsure=int((~ovf & ~calm & ~clear).sum()))
    if roles is not None and W == 8:
        r = np.concatenate([roles, np.repeat(roles[-1:], -len(roles) % W)]).reshape(-1, W)
        envc = w.sum((2, 3))                                    # (waves, W): an env's contacts of the step
        five_three = ((r == HEAVY).sum(1) == 5) & ((r == CLEAR).sum(1) == 3) & ovf & \
            ((envc == 0) == (r == CLEAR)).all(1)                # the clear envs idle, the heavy ones not
        out["five_heavy_three_idle"] = int(five_three.sum())
    return out


def assert_pool(k, W, want_split=True):
    """sixteen lanes: >= 2 waves overflow for certain, >= 8 hold contacts and for certain never
    overflow, >= 1 clear, an overflowing wave-substep with contact-free bodies beside others;
    eight lanes: >= 2 overflow, one of them five heavy envs and three idle ones, >= 1 calm, >= 1 clear"""
    assert k["overflow"] >= 2, k
    assert k["clear"] >= 1, k
    if W == 4:
        assert k["calm"] >= 8, k
        assert not want_split or k["split"] >= 1, k
    else:
        assert k["calm"] >= 1, k
        assert k["five_heavy_three_idle"] >= 1, k


def lane_conditions(rec):
    """the eight-lane per-lane store: lanes (env-substeps x 8) with exactly OMAXC contacts (kept),
    more (re-walk), none; waves holding all three in one substep"""
    lc = _pad(lane_counts(rec), 8)                              # (waves, 8, NSUB, 8)
    l = lc.transpose(0, 2, 1, 3).reshape(lc.shape[0], NSUB, 64)
    at, over, none = l == OMAXC, l > OMAXC, l == 0
    return dict(at=int(at.sum()), over=int(over.sum()), none=int(none.sum()), lane_max=int(l.max()),
                together=int((at.any(-1) & over.any(-1) & none.any(-1)).sum()))


def assert_lanes(k):
    assert k["at"] > 0 and k["over"] > 0 and k["none"] > 0 and k["together"] > 0, k


def tail_overflows(rec, W):
    """the last wave (env B - 1 and its replays): True overflows for certain, False for certain
    does not, None undecided by the bounds"""
    lower, upper = wave_bounds(rec, W)
    if (lower[-1] > POOL_N).any():
        return True
    return False if (upper[-1] <= POOL_N).all() else None
