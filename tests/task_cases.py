"""The arranged task-logic cases of tests/golden/task_logic_*.npz: how a fixture's inputs are
rebuilt, the comparison rule, and the events a fixture must hold.

The fixtures record what the reference's own env code (po_brax/envs/ant_heavenhell.py,
ant_gather.py, ant_tag.py, utils.py, wrappers.py) returned when run on the numpy stand-in of
oracle/ref_standin.py (tests/golden/make_task_logic_fixture.py).  Inputs are not stored as states:
a fixture holds the seed of the reset keys and the edits applied to that reset (xyz offsets of the
nine ant bodies, positions of the frozen bodies, per-env keys, initial episode counters) and the
actions; ``arrange`` applies them to the reset of whoever is under test -- the C oracle's or the
kernels', which are bit-equal (tests/test_gpu_parity.py test_reset_parity).

Comparison rule: bit for bit (``numpy.testing.assert_array_equal``, as in the rest of the suite),
every array, every env, no tolerance, no case left out -- the walls' rotation included, as the
float32 cos / sin of the reference's angle (tests/test_task_logic_host.py).

Members of a fixture (one per kind; prefix ``reset_`` 64 reset cases, ``step_`` 97 one-step cases):

  reset_seed                  keys = split(PRNGKey(seed), 65)[1:]
  reset_pos, reset_obs, reset_rng     the reference's reset: all body positions, obs, the kept key
  step_seed                   the base state is the reset of split(PRNGKey(seed), 98)[1:]
  step_off (97, 3)            added to pos[:, :9] (float32)
  step_frozen (97, F, 3)      pos[:, FROZEN[kind]] before the step
  step_rng (97, 2)            info['rng'] before the step
  step_act (97, 8), step_role (97,)   the action; the arrangement's role (see the maker)
  step_obs, step_reward, step_done, step_metric_<name>, step_frozen_after, step_rng_after
                              what the reference's step returned
  step_choice (TAG)           the adversary's randint draw
  walls (n, 7)                the reference's wall boxes: cx, cy, rotation z (degrees), hx, hy, hz, body z
  grid, waiting_area (GA)     possible_grid_positions, waiting_area
  alt_* (GA)                  B_ALT step cases as step_* with n_apples = 10, n_bombs = 6 (ALT_PARAMS): the only
                              way to a reading in the last sensor slot, which the default counts rule out
  naive_*, cached_*, gym_* (TAG)   the wrapper records (WRAP_B envs, WRAP_T steps, episode length WRAP_L)
"""
import os

import numpy as np

import orc
import pob_np as P

HERE = os.path.dirname(os.path.abspath(__file__))
HH, GA, TAG = "ant_heavenhell", "ant_gather", "ant_tag"
KINDS = (HH, GA, TAG)
SHORT = {HH: "heavenhell", GA: "gather", TAG: "tag"}
N_RESET, B_STEP = 64, 97
FROZEN = {HH: (10, 11, 12), TAG: (10,), GA: tuple(range(11, 27))}  # HH: priest, heaven, hell
METRICS = {HH: ("heavens", "hells", "hits"), GA: ("apples", "bombs", "objects"), TAG: ("hits",)}
SLOT = {HH: dict(heavens="m0", hells="m1", hits="m2"), GA: dict(apples="m0", bombs="m1", objects="m2"),
        TAG: dict(hits="m0")}
RESET_METRICS = {HH: ("heavens", "hells"), GA: ("apples", "bombs", "objects"), TAG: ("hits",)}
RADIUS = {HH: 2.0, "tag": 1.5, "visible": 3.0, "catch": 1.0, "sensor": 6.0, "cage": 4.5}
WRAP_KIND, WRAP_B, WRAP_T, WRAP_L, WRAP_N, WRAP_SEED, GYM_SEED = TAG, 13, 6, 3, 3, 11, 3
MIN_CASES = 4
B_ALT, ALT_PARAMS = 17, dict(n_apples=10, n_bombs=6)
# GA roles (the arrangement of an env's sixteen objects)
(GA_APPLE, GA_BOMB, GA_BOTH, GA_APPLE_EXACT, GA_BOMB_EXACT, GA_NEAR, GA_ALL, GA_TWO_IN_BIN, GA_SENSOR_EXACT,
 GA_SPAN, GA_OVERLAP, GA_SCATTER) = range(12)


def path(kind):
    return os.path.join(HERE, "golden", f"task_logic_{SHORT[kind]}.npz")


def load(kind, file=None):
    with np.load(file or path(kind), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def keys(seed, n):
    return P.split(P.prngkey(int(seed)), n + 1)[1:]


def arrange(kind, state, fix, pre="step"):
    """the step cases' input: ``state`` (oracle layout, the reset of keys(step_seed, 97)) with the
    fixture's edits applied"""
    s = {k: v.copy() for k, v in state.items()}
    s["pos"][:, :9] = s["pos"][:, :9] + fix[f"{pre}_off"][:, None, :]
    s["pos"][:, list(FROZEN[kind])] = fix[f"{pre}_frozen"]
    s["rng"] = np.ascontiguousarray(fix[f"{pre}_rng"])
    return s


def dist32(a, b):
    """float32 sqrt(dx * dx + dy * dy), the form every radius test of the task code takes"""
    d = np.asarray(a, np.float32) - np.asarray(b, np.float32)
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)


def compare_step(kind, got, fix, what, pre="step"):
    """``got``: obs, reward, done, the frozen bodies' positions, rng and the metrics by name, after
    one step of the arranged state"""
    same(got["obs"], fix[f"{pre}_obs"], f"{what}: obs")
    same(got["reward"], fix[f"{pre}_reward"], f"{what}: reward")
    same(np.asarray(got["done"], np.float32), fix[f"{pre}_done"], f"{what}: done")
    same(got["frozen"], fix[f"{pre}_frozen_after"], f"{what}: frozen bodies")
    same(got["rng"], fix[f"{pre}_rng_after"], f"{what}: rng")
    for m in METRICS[kind]:
        same(np.asarray(got[m], np.float32), fix[f"{pre}_metric_{m}"], f"{what}: metric {m}")


def compare_reset(kind, got, fix, what):
    same(got["pos"], fix["reset_pos"], f"{what}: pos")
    same(got["obs"], fix["reset_obs"], f"{what}: obs")
    same(got["rng"], fix["reset_rng"], f"{what}: rng")


def oracle_step_outputs(kind, s):
    out = dict(obs=s["obs"], reward=s["reward"], done=s["done"], frozen=s["pos"][:, list(FROZEN[kind])], rng=s["rng"])
    out.update({m: s[SLOT[kind][m]] for m in METRICS[kind]})
    return out


# ------------------------------------------------------------------------------ events
def _near(d, r, w=0.05):
    return (d < r) & (d > r - w), (d > r) & (d < r + w)


def _ga_view(obs, F1, n_apples):
    """where AntGather's sensor sees each object, worked out in float64 from the reference's outputs
    alone (the observation's torso position and quaternion, the returned object positions; an
    object caught in the step is at the waiting area there and counts as out of range): the
    float32 distance, the bearing relative to the torso's heading, and the slot of its reading
    (-1: no bin).  Only the event counts use this, never a comparison."""
    a, q = obs[:, :2], obs[:, 3:7].astype(np.float64)
    ori = np.arctan2(2 * (q[:, 1] * q[:, 2] + q[:, 0] * q[:, 3]), 1 - 2 * (q[:, 2] ** 2 + q[:, 3] ** 2))
    p = F1[:, :, :2].astype(np.float64)
    ang = np.arctan2(p[..., 0], p[..., 1]) - ori[:, None]
    d = dist32(a[:, None, :], F1[:, :, :2])
    b = np.floor((ang + np.pi / 2) / (np.pi / 10)).astype(int)
    shift = np.where(np.arange(F1.shape[1]) >= n_apples, n_apples, 0)
    seen = (np.abs(ang) <= np.pi / 2) & (d <= np.float32(RADIUS["sensor"]))
    return d, ang, b + shift, np.where(seen, b + shift, -1)


def _ga_sensor_events(obs, F1, n_apples=8):
    """per env, from _ga_view and the readings: two apples seen in one slot; an object at exactly
    the sensor range whose zero intensity replaced an earlier object's reading in its slot
    (clobber), or one within 0.05 of the range, either side, beside which a reading survives
    (kept); a seen object within 0.15 rad inside the half span with a reading, one as far outside
    it with none; a bomb and an apple seen in one slot"""
    rd = obs[:, -20:]
    d, ang, raw, slot = _ga_view(obs, F1, n_apples)
    B, n = d.shape
    out = {k: np.zeros(B, bool) for k in ("two_in_bin", "sensor_clobber", "sensor_kept", "span_in", "span_out",
                                          "overlap")}
    half, R = np.pi / 2, np.float32(RADIUS["sensor"])
    for i in range(B):
        for k2 in range(n):
            edge = abs(ang[i, k2]) - half
            if slot[i, k2] >= 0 and -0.15 < edge <= 0 and rd[i, slot[i, k2]] != 0:
                out["span_in"][i] = True
            if d[i, k2] <= R and 0 < edge < 0.15 and not rd[i].any():
                out["span_out"][i] = True
            for k1 in range(k2):
                if slot[i, k1] < 0 or raw[i, k1] != raw[i, k2] or abs(ang[i, k2]) > half:
                    continue
                s_ = slot[i, k1]
                if slot[i, k2] >= 0 and k2 < n_apples:
                    out["two_in_bin"][i] |= rd[i, s_] != 0 and d[i, k2] < R
                if slot[i, k2] >= 0 and k1 < n_apples <= k2:
                    out["overlap"][i] |= rd[i, s_] != 0
                if (k1 < n_apples) == (k2 < n_apples) and d[i, k1] < R - 0.05:
                    if d[i, k2] == R:
                        out["sensor_clobber"][i] |= rd[i, s_] == 0
                    elif abs(float(d[i, k2]) - float(R)) < 0.05:
                        out["sensor_kept"][i] |= rd[i, s_] != 0
    return out, slot


def events(kind, fix):
    """bool masks (97,) by event name, from what the reference returned: observation, reward, done,
    metrics, the frozen bodies' positions, the adversary's draw.  The arranged input positions
    enter where an event is by definition about the state before the step: whether the TAG target
    moved, and the distance at which a GA object was caught (it is at the waiting area afterwards)."""
    obs, r, done = fix["step_obs"], fix["step_reward"], fix["step_done"]
    a, z = obs[:, :2], obs[:, 2]
    F0, F1 = fix["step_frozen"], fix["step_frozen_after"]
    high = z > 1.0
    ev = dict(high=high, not_high=~high)
    if kind == HH:
        dirn = obs[:, -1]
        ev.update(heaven=r == 1, no_heaven=r != 1, hell=r == -1, no_hell=r != -1, priest_left=dirn == -1,
                  priest_right=dirn == 1, priest_out=dirn == 0, dead_only=r == -2, dead_heaven=high & (r == 1),
                  dead_no_heaven=high & (r != 1), done=done == 1, not_done=done == 0)
        for j, name in enumerate(("priest", "heaven", "hell")):
            d = dist32(F1[:, j, :2], a)
            ev[f"{name}_exact"] = d == np.float32(RADIUS[HH])
            ev[f"{name}_near_in"], ev[f"{name}_near_out"] = _near(d, RADIUS[HH])
    elif kind == TAG:
        hits, ch = fix["step_metric_hits"], fix["step_choice"]
        d1 = dist32(a, F1[:, 0, :2])
        moved = (F1[:, 0, :2] != F0[:, 0, :2]).any(1)
        ev.update(tagged=hits == 1, not_tagged=hits == 0, tagged_dead=(hits == 1) & high, tagged_alive=(hits == 1) & ~high,
                  dead_only=r == -1, alive_untagged=(r == 0) & (done == 0),
                  visible=(obs[:, -2:] != 0).any(1), not_visible=(obs[:, -2:] == 0).all(1),
                  refused=(ch != 3) & ~moved, accepted=moved, tag_exact=d1 == np.float32(RADIUS["tag"]),
                  visible_exact=d1 == np.float32(RADIUS["visible"]),
                  cage_exact=moved & (np.abs(F1[:, 0, :2]) == np.float32(RADIUS["cage"])).any(1),
                  z_one=(F1[:, 0, 2] == 1.0) & (F0[:, 0, 2] == 0.5))
        ev["tag_near_in"], ev["tag_near_out"] = _near(d1, RADIUS["tag"])
        ev["visible_near_in"], ev["visible_near_out"] = _near(d1, RADIUS["visible"])
        for k in range(4):
            ev[f"choice_{k}"] = ch == k
    else:
        ap, bo = fix["step_metric_apples"], fix["step_metric_bombs"]
        d0 = dist32(a[:, None, :], F0[:, :, :2])
        caught = (ap + bo) > 0
        ev.update(apple=ap > 0, no_apple=ap == 0, bomb=bo > 0, no_bomb=bo == 0, both=(ap > 0) & (bo > 0),
                  apple_reward=r == 1, bomb_reward=r == -1, dead_only=(r == -10) & ~caught, catch_dead=caught & high & (r == -10),
                  catch_alive=caught & ~high, all_collected=(done == 1) & ~high, not_all=(done == 0),
                  catch_exact=(d0 == np.float32(RADIUS["catch"])).any(1),
                  sensor_exact=(d0 == np.float32(RADIUS["sensor"])).any(1),
                  moved_to_waiting=(F1 == fix["waiting_area"]).all(2).any(1) & caught)
        ci, co = _near(d0, RADIUS["catch"])
        ev["catch_near_in"], ev["catch_near_out"] = ci.any(1), co.any(1)
        si, so = _near(d0, RADIUS["sensor"])
        ev["sensor_near_in"], ev["sensor_near_out"] = si.any(1), so.any(1)
        ev.update(_ga_sensor_events(obs, F1)[0])
    return ev


def assert_events(kind, fix):
    """every listed event and its opposite at least MIN_CASES times; returns the counts"""
    ev = events(kind, fix)
    n = {k: int(v.sum()) for k, v in ev.items()}
    short = {k: c for k, c in n.items() if c < MIN_CASES}
    assert not short, (kind, "events with fewer than", MIN_CASES, "cases", short, n)
    if kind == TAG:
        assert n["z_one"] == B_STEP, n  # the target's z is 1.0 after every step, whatever it was
    if kind == GA:
        # n_apples = 8 shifts the bombs' bins by 8, not by n_bins = 10: no reading can land in the
        # last slot (19), and the -1 wrap only ever writes a zero there.  With ten apples it can:
        # a bomb in bin 9 reads into slot 19, and an object without a bin (-1) written after it
        # zeroes the reading
        assert not fix["step_obs"][:, -1].any()
        last = fix["alt_obs"][:, -1]
        slot = _ga_sensor_events(fix["alt_obs"], fix["alt_frozen_after"], ALT_PARAMS["n_apples"])[1]
        in_last = (slot == 19).any(1)  # a bomb seen in bin 9, by the reference's returned positions
        assert in_last.all(), in_last
        alt = dict(last_slot_live=int((last != 0).sum()), last_slot_zeroed=int(((last == 0) & in_last).sum()))
        assert min(alt.values()) >= MIN_CASES, alt
        n.update(alt)
        assert len(fix["grid"]) == 156 and fix["waiting_area"].tolist() == [18.0, 18.0, 12.0]
    return n


# ------------------------------------------------------- the wrappers on the oracle's own steps
def wrap_inputs(fix):
    rng = np.random.default_rng(int(fix["wrap_act_seed"]))
    acts = [rng.uniform(-1, 1, (WRAP_B, 8)).astype(np.float32) for _ in range(WRAP_T)]
    return keys(WRAP_SEED, WRAP_B), fix["wrap_steps0"], acts


WRAP_FIELDS = ("pos", "rot", "vel", "ang", "obs", "reward", "done", "steps", "rng")


def oracle_naive(o, keys_, steps0, acts):
    """RandomizedAutoResetWrapperNaive on the oracle (the emulation tests/test_gpu_parity.py uses)"""
    s = o.reset(keys_)
    s["steps"] = steps0.copy()
    for act in acts:
        s["steps"] = np.where(s["done"] != 0, 0, s["steps"]).astype(np.float32)
        s = o.step(s, act, flags=orc.F_EPISODE, episode_length=WRAP_L)
        inner = s["done"].copy()
        d = s["done"] != 0
        if d.any():
            fresh = o.reset(np.ascontiguousarray(s["rng"][d]))
            for k in ("pos", "rot", "vel", "ang", "obs"):
                s[k][d] = fresh[k]
        yield s, inner


def oracle_cached(o, keys_, steps0, acts):
    """RandomizedAutoResetWrapperCached(n = WRAP_N) on the oracle (tests/test_gpu_wrappers.py)"""
    s = o.reset(keys_, first=True)
    s["steps"] = steps0.copy()
    for t, act in enumerate(acts):
        if (t + 1) % WRAP_N == 0:
            ks = np.stack([P.split(k, 2) for k in s["rng"]])
            fresh = o.reset(np.ascontiguousarray(ks[:, 1]))
            for f in ("pos", "rot", "vel", "ang", "obs"):
                s["first_" + f] = fresh[f].copy()
            s["rng"] = np.ascontiguousarray(ks[:, 0])
        s = o.step(s, act, flags=orc.F_EPISODE | orc.F_AUTORESET, episode_length=WRAP_L)
        yield s, None


def oracle_gym(o, steps0, acts):
    """AutoresetVmapGymWrapper on the oracle: orc.gym_autoreset after every step"""
    ks = P.split(P.prngkey(GYM_SEED), WRAP_B + 1)
    s, gkey = o.reset(np.ascontiguousarray(ks[1:])), ks[0].copy()
    s["steps"] = steps0.copy()
    for act in acts:
        s = o.step(s, act, flags=orc.F_EPISODE, episode_length=WRAP_L)
        inner = s["done"].copy()
        o.gym_autoreset(s, gkey)
        yield s, inner, gkey.copy()


def compare_wrap(prefix, t, got, fix, what, fields=WRAP_FIELDS):
    for f in fields:
        same(np.asarray(got[f], fix[f"{prefix}_{f}"].dtype), fix[f"{prefix}_{f}"][t], f"{what} step {t}: {f}")
