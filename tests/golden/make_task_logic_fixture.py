"""Regenerate tests/golden/task_logic_{heavenhell,gather,tag}.npz: what the reference's own task
code returns for arranged states.

Needs the reference checkout (argument or $PO_BRAX_REFERENCE); it is imported from there, unchanged,
on the numpy stand-in of oracle/ref_standin.py -- no jax, no brax.  The files written hold arrays
and names only (tests/task_cases.py lists the members).  Run after a deliberate change to the
physics restatement (the arranged placements are chosen on the oracle's post-physics torso):

    python tests/golden/make_task_logic_fixture.py /path/to/po-brax [--out DIR]

Reset cases: 64 keys per kind.  Step cases: 97 envs per kind, one step each from the reset of 97
keys with edits.  The placements are chosen by candidate search on the C oracle alone (its physics
gives the torso after the step, which no frozen body influences; pob_np gives the adversary's draw
of a key), never on the reference's outputs; the events are then counted from the reference's
outputs (tests/task_cases.py assert_events: at least 4 cases of each event and of its opposite).
Thresholds are met three ways: well inside and outside, within 0.05 on either side, and exactly
(a float32 distance equal to the radius, found by stepping a coordinate through neighbouring
floats), which is what tells ``<=`` from ``<``.

Not reachable, so not arranged: a torso below 0.2 after a step (the ground contact's position
pass runs last and keeps the torso, a sphere of radius 0.25, at z >= 0.25: 0 of 1 394 lift x fall
speed candidates), and a reading in AntGather's last sensor slot (task_cases).
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import orc  # noqa: E402
import pob_np as P  # noqa: E402
import ref_standin as RS  # noqa: E402
import task_cases as TC  # noqa: E402

HH, GA, TAG = TC.HH, TC.GA, TC.TAG
RESET_SEED = {HH: 101, GA: 102, TAG: 103}
STEP_SEED = {HH: 201, GA: 202, TAG: 203}
F32 = np.float32
HIGH_DZ = 0.7  # lifts the torso past 1.0 for the step (it falls 0.013 in 0.05 s)


# ------------------------------------------------------------------- placement helpers
def exact_point(a, r, u):
    """a float32 point p near a + r u with dist32(p, a) == r exactly, or None: both coordinates
    stepped through up to 8 neighbouring floats"""
    a = np.asarray(a, F32)
    p0 = (a + F32(r) * np.asarray(u, F32)).astype(F32)
    xs, ys = [p0[0]], [p0[1]]
    for _ in range(8):
        xs = [np.nextafter(xs[0], F32(-np.inf))] + xs + [np.nextafter(xs[-1], F32(np.inf))]
        ys = [np.nextafter(ys[0], F32(-np.inf))] + ys + [np.nextafter(ys[-1], F32(np.inf))]
    order = sorted(range(17), key=lambda k: abs(k - 8))
    for i in order:
        for j in order:
            p = np.array([xs[i], ys[j]], F32)
            if TC.dist32(p, a) == F32(r):
                return p
    return None


def on_ray(a, d, phi):
    """the point p with atan2(p.x, p.y) = phi (the sensor's bearing of an absolute position) at
    distance d from a"""
    u = np.array([np.sin(phi), np.cos(phi)])
    au = float(np.dot(a, u))
    rho = au + np.sqrt(au * au - float(np.dot(a, a)) + d * d)
    return (rho * u).astype(F32)


def polar(a, d, th):
    return (np.asarray(a, np.float64) + d * np.array([np.cos(th), np.sin(th)])).astype(F32)


AXES = ((1, 0), (-1, 0), (0, 1), (0, -1))


def by_mode(rng, a, r, mode):
    """a point at a distance from a chosen by mode: far, in, out, near_in, near_out, exact"""
    th = rng.uniform(0, 2 * np.pi)
    if mode == "exact":
        for k in rng.permutation(4):
            p = exact_point(a, r, AXES[k])
            if p is not None:
                return p
        mode = "near_in"
    d = {"far": r + 3 + rng.uniform(0, 3), "in": r - rng.uniform(0.3, 0.9 * r if r < 1.6 else 1.5),
         "out": r + rng.uniform(0.3, 1.5), "near_in": r - rng.uniform(1e-4, 0.03),
         "near_out": r + rng.uniform(1e-4, 0.03)}[mode]
    return polar(a, d, th)


MODES = ("far", "in", "out", "near_in", "near_out", "exact")


def post_physics(kind, base, off, act):
    """the oracle's torso (xy, rot) after the step of base moved by off: the frozen bodies play no
    part in the physics, so it holds for every placement of them"""
    s = {k: v.copy() for k, v in base.items()}
    s["pos"][:, :9] = s["pos"][:, :9] + off[:, None, :]
    out = orc.OracleEnv(kind).step(s, act)
    return out["pos"][:, 0, :2].copy(), out["rot"][:, 0].copy()


def draw_key(rng, want):
    """a key whose adversary draw (split(key)[1] -> randint(0, 4)) is ``want`` (None: any)"""
    while True:
        key = rng.integers(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
        if want is None or P.randint(P.split(key)[1], 0, 4) == want:
            return key


# ------------------------------------------------------------------------ arrangements
def arrange_hh(base, act, rng):
    B = TC.B_STEP
    off = np.zeros((B, 3), F32)
    off[:, :2] = rng.uniform(-0.3, 0.3, (B, 2))
    off[np.arange(B) % 5 == 0, 2] = HIGH_DZ
    a, _ = post_physics(HH, base, off, act)
    frozen = np.ones((B, 3, 3), F32)  # priest, heaven, hell; z = 1 as the reference places them
    for i in range(B):
        modes = (MODES[(i // 2 + 1) % 6], MODES[i % 6], MODES[(i // 6) % 6])
        for j in range(3):
            frozen[i, j, :2] = by_mode(rng, a[i], TC.RADIUS[HH], modes[j])
    return off, frozen, TC.keys(STEP_SEED[HH] + 1000, B), np.arange(B) % 6


def arrange_tag(base, act, rng):
    B = TC.B_STEP
    off = np.zeros((B, 3), F32)
    role = np.arange(B) % 12
    want_xy = rng.uniform(-3.0, 3.0, (B, 2))
    sgn = rng.choice([-1.0, 1.0], B)
    axis = rng.integers(0, 2, B)
    for i in range(B):
        if role[i] in (7, 8):  # next to a cage side, the ant further inside on the same line
            want_xy[i, axis[i]] = sgn[i] * (4.0 - rng.uniform(1.0, 2.5))
    off[:, :2] = (want_xy - base["pos"][:, 0, :2]).astype(F32)
    off[np.arange(B) % 8 < 2, 2] = HIGH_DZ
    a, _ = post_physics(TAG, base, off, act)
    frozen = np.full((B, 1, 3), 0.5, F32)
    keys = np.zeros((B, 2), np.uint32)
    tr, vr = TC.RADIUS["tag"], TC.RADIUS["visible"]
    for i in range(B):
        want = None
        if role[i] == 0:
            p = polar(a[i], rng.uniform(0.3, 0.9), rng.uniform(0, 2 * np.pi))
        elif role[i] in (1, 2, 3, 4):  # the target stays (draw 3): its distance is the arranged one
            want = 3
            r = tr if role[i] < 3 else vr
            p = by_mode(rng, a[i], r, "exact" if role[i] in (1, 3) else ("near_in", "near_out")[(i // 12) % 2])
        elif role[i] == 5:
            p = polar(a[i], rng.uniform(2.1, 2.4), rng.uniform(0, 2 * np.pi))
        elif role[i] == 6:
            p = polar(a[i], rng.uniform(3.7, 4.5), rng.uniform(0, 2 * np.pi))
        elif role[i] in (7, 8):
            # 7: at 4.0 on the ant's line, running away (draw 2) lands on 4.5 exactly: not > 4.5,
            # accepted; 8: at 4.3 the same move leaves the cage and is refused
            want = 2
            p = a[i].copy()
            p[axis[i]] = F32(sgn[i] * (4.0 if role[i] == 7 else 4.3))
        elif role[i] == 9:
            p = np.array([sgn[i] * 4.3, rng.choice([-1.0, 1.0]) * 4.3], F32)  # a corner: most moves refused
            want = int(rng.integers(0, 3))
        elif role[i] == 10:
            want = int(rng.integers(0, 2))  # a sideways move
            p = polar(a[i], rng.uniform(1.3, 1.6), rng.uniform(0, 2 * np.pi))
        else:
            want = 2  # within the tag radius before the move, outside after it
            p = polar(a[i], rng.uniform(1.1, 1.4), rng.uniform(0, 2 * np.pi))
        if role[i] not in (7, 8, 9):
            p = np.clip(p, -4.4, 4.4).astype(F32) if role[i] not in (1, 2, 3, 4) else p
        frozen[i, 0, :2] = p
        keys[i] = draw_key(rng, want)
    return off, frozen, keys, role


def arrange_ga(base, act, rng):
    B = TC.B_STEP
    off = np.zeros((B, 3), F32)
    off[:, :2] = rng.uniform(-0.2, 0.2, (B, 2))
    off[np.arange(B) % 8 < 2, 2] = HIGH_DZ
    a, rot = post_physics(GA, base, off, act)
    q = rot.astype(np.float64)
    ori = np.arctan2(2 * (q[:, 1] * q[:, 2] + q[:, 0] * q[:, 3]), 1 - 2 * (q[:, 2] ** 2 + q[:, 3] ** 2))
    role = np.arange(B) % 12
    cr, sr = TC.RADIUS["catch"], TC.RADIUS["sensor"]
    waiting = np.array([18.0, 18.0, 12.0], F32)
    frozen = np.zeros((B, 16, 3), F32)
    for i in range(B):
        f = frozen[i]
        f[:8, 2] = 1.0  # apples higher, as the reset leaves them
        # parked: behind the ant (outside the span) and beyond the sensor range
        f[:, 0] = rng.uniform(-9, 9, 16)
        f[:, 1] = rng.uniform(-9.5, -7.5, 16)
        ka, kb = int(rng.integers(0, 8)), int(8 + rng.integers(0, 8))
        th = rng.uniform(0, 2 * np.pi)
        r = role[i]
        if r == TC.GA_APPLE:
            f[ka, :2] = polar(a[i], rng.uniform(0.2, 0.8), th)
        elif r == TC.GA_BOMB:
            f[kb, :2] = polar(a[i], rng.uniform(0.2, 0.8), th)
        elif r == TC.GA_BOTH:
            f[ka, :2] = polar(a[i], rng.uniform(0.2, 0.8), th)
            f[kb, :2] = polar(a[i], rng.uniform(0.2, 0.8), th + 2.0)
            if i % 24 >= 12:  # two apples in one step: the metric counts, the reward does not
                f[(ka + 1) % 8, :2] = polar(a[i], rng.uniform(0.2, 0.8), th + 4.0)
        elif r == TC.GA_APPLE_EXACT:
            f[ka, :2] = by_mode(rng, a[i], cr, "exact")
        elif r == TC.GA_BOMB_EXACT:
            f[kb, :2] = by_mode(rng, a[i], cr, "exact")
        elif r == TC.GA_NEAR:
            f[ka, :2] = by_mode(rng, a[i], cr, ("near_in", "near_out")[(i // 12) % 2])
            f[kb, :2] = by_mode(rng, a[i], cr, ("near_out", "near_in")[(i // 24) % 2])
        elif r == TC.GA_ALL:
            f[:] = waiting
            v = (i // 12) % 4
            if v == 0:    # the last free apple is caught in this step
                f[ka] = (*polar(a[i], 0.5, th), 1.0)
            elif v == 1:  # the last free bomb
                f[kb] = (*polar(a[i], 0.5, th), 0.0)
            elif v == 3:  # one object left free and out of reach: not done
                f[kb] = (*polar(a[i], 3.0, th), 0.0)
        elif r == TC.GA_TWO_IN_BIN:
            k1, k2 = sorted(rng.choice(8, 2, replace=False))
            phi = ori[i] + rng.uniform(-1.2, 1.2)
            d1, d2 = (3.0, 4.5) if (i // 12) % 2 else (4.5, 3.0)  # the later index wins, nearer or not
            f[k1, :2], f[k2, :2] = on_ray(a[i], d1, phi), on_ray(a[i], d2, phi)
            # and a bomb just inside or just outside the sensor range, on another bearing
            f[kb, :2] = on_ray(a[i], sr + (0.02 if (i // 12) % 2 else -0.02), phi + 0.5 * (1 if phi < ori[i] else -1))
        elif r == TC.GA_SENSOR_EXACT:
            # an apple at 3 m and, with a later index and the same bearing's bin, one at the sensor
            # range: exactly (in range: it writes its zero intensity over the first), or just
            # inside, or just outside (its -1 bin writes the last slot instead)
            k1, k2 = sorted(rng.choice(8, 2, replace=False))
            u = np.array([np.sin(0.75), np.cos(0.75)])
            f[k1, :2] = (a[i] + 3.0 * u).astype(F32)
            v = (i // 12) % 4
            p = exact_point(a[i], sr, u) if v < 2 else None
            if p is None:
                p = (a[i] + (sr + (0.02 if v == 3 else -0.02 if v == 2 else 0.01)) * u).astype(F32)
            f[k2, :2] = p
        elif r == TC.GA_SPAN:
            side = 1 if (i // 12) % 2 else -1
            delta = (0.02, 0.1, -0.02, -0.1)[(i // 24) % 4]  # inside the half span, or outside it
            k = ka if (i // 12) % 4 < 2 else kb
            f[k, :2] = on_ray(a[i], 3.0, ori[i] + side * (np.pi / 2 - delta))
        elif r == TC.GA_OVERLAP:
            # an apple in bin 8 or 9 and a bomb in bin 0 or 1: the bombs' bins are shifted by
            # n_apples = 8, so both land in slot 8 or 9 and the bomb, written later, wins
            b = int(rng.integers(0, 2))
            f[ka, :2] = on_ray(a[i], 2.0, ori[i] - np.pi / 2 + (8.5 + b) * np.pi / 10)
            f[kb, :2] = on_ray(a[i], 4.0, ori[i] - np.pi / 2 + (0.5 + b) * np.pi / 10)
        else:
            f[:, :2] = rng.uniform(-6, 6, (16, 2))
    return off, frozen, TC.keys(STEP_SEED[GA] + 1000, B), role


ARRANGE = {HH: arrange_hh, GA: arrange_ga, TAG: arrange_tag}
ALT_SEED = 302


def build_ga_alt(ref):
    """AntGather with ten apples and six bombs: a bomb in bin 9 reads into the last slot (19).
    role 0: every other object has a bin of its own, the reading stays; 1: the bomb is the last
    object and the others have none (their -1 writes come first), it stays; 2: a later bomb has
    none, its -1 write zeroes the reading; 3: only earlier objects have none, it stays"""
    B = TC.B_ALT
    env = ref.ant_gather.AntGatherEnv(**TC.ALT_PARAMS)
    keys = TC.keys(ALT_SEED, B)
    base = orc.OracleEnv(GA).reset(keys)
    rng = np.random.default_rng(ALT_SEED)
    act = rng.uniform(-1, 1, (B, 8)).astype(F32)
    off = np.zeros((B, 3), F32)
    a, rot = post_physics(GA, base, off, act)
    q = rot.astype(np.float64)
    ori = np.arctan2(2 * (q[:, 1] * q[:, 2] + q[:, 0] * q[:, 3]), 1 - 2 * (q[:, 2] ** 2 + q[:, 3] ** 2))
    role = np.arange(B) % 4
    frozen = np.zeros((B, 16, 3), F32)
    ray = lambda i, d, b: on_ray(a[i], d, ori[i] - np.pi / 2 + (b + 0.5) * np.pi / 10)  # noqa: E731
    for i in range(B):
        f = frozen[i]
        f[:10, 2] = 1.0
        f[:, 0], f[:, 1] = rng.uniform(-9, 9, 16), rng.uniform(-9.5, -7.5, 16)  # parked: no bin
        kb = 15 if role[i] == 1 else int(10 + rng.integers(0, 5))
        seen = range(16) if role[i] == 0 else (range(kb + 1, 16) if role[i] == 3 else ())
        for k in seen:
            f[k, :2] = ray(i, rng.uniform(2.0, 5.0), k % 8)
        f[kb, :2] = ray(i, 3.0, 9)
    fix = dict(alt_seed=np.int64(ALT_SEED), alt_off=off, alt_frozen=frozen, alt_rng=TC.keys(ALT_SEED + 1000, B),
               alt_act=act, alt_role=role.astype(np.int8))
    fix.update(reference_step(env, GA, TC.arrange(GA, base, fix, "alt"), act, keys, "alt"))
    return fix


# ------------------------------------------------------------- running the reference
def make_env(ref, kind):
    cls = {HH: ref.ant_heavenhell.AntHeavenHellEnv, GA: ref.ant_gather.AntGatherEnv, TAG: ref.ant_tag.AntTagEnv}
    return cls[kind]()


def f32(x, what):
    x = np.asarray(x)
    assert x.dtype == np.float32, (what, x.dtype)
    return x


def reference_reset(env, kind):
    out = dict(pos=[], obs=[], rng=[])
    for key in TC.keys(RESET_SEED[kind], TC.N_RESET):
        st = env.reset(key.copy())
        out["pos"].append(f32(st.qp.pos, "pos")); out["obs"].append(f32(st.obs, "obs"))
        out["rng"].append(np.asarray(st.info["rng"], np.uint32))
        assert float(st.reward) == 0 and float(st.done) == 0
        assert tuple(st.metrics) == TC.RESET_METRICS[kind] and not any(float(v) for v in st.metrics.values())
    return {f"reset_{k}": np.stack(v) for k, v in out.items()}


def reference_step(env, kind, state, act, keys, pre="step"):
    """the reference's step of every arranged env: its reset State for the pytree, the arranged
    qp and key put in"""
    fr = list(TC.FROZEN[kind])
    rec = {k: [] for k in ("obs", "reward", "done", "frozen_after", "rng_after", "choice")}
    mets = {m: [] for m in TC.METRICS[kind]}
    for b in range(len(keys)):
        st = env.reset(keys[b].copy())
        st = st.replace(qp=RS.QP(state["pos"][b], state["rot"][b], state["vel"][b], state["ang"][b]))
        st.info["rng"] = state["rng"][b].copy()
        n0 = len(RS.RANDINT_LOG)
        out = env.step(st, act[b])
        rec["obs"].append(f32(out.obs, "obs")); rec["reward"].append(f32(out.reward, "reward"))
        rec["done"].append(np.float32(out.done))
        rec["frozen_after"].append(f32(out.qp.pos, "pos")[fr]); rec["rng_after"].append(np.asarray(out.info["rng"], np.uint32))
        rec["choice"].append(RS.RANDINT_LOG[n0] if len(RS.RANDINT_LOG) > n0 else -1)
        assert len(RS.RANDINT_LOG) - n0 == (1 if kind == TAG else 0)
        for m in mets:
            mets[m].append(np.float32(out.metrics[m]))
        # the physics is the oracle's, whatever the frozen bodies: the torso is where the search saw it
        assert set(out.metrics) == set(TC.METRICS[kind]), set(out.metrics)
    res = {f"{pre}_{k}": np.stack(v) for k, v in rec.items()}
    res[f"{pre}_choice"] = res[f"{pre}_choice"].astype(np.int8)
    if kind != TAG:
        del res[f"{pre}_choice"]
    res.update({f"{pre}_metric_{m}": np.array(v, np.float32) for m, v in mets.items()})
    return res


def reference_walls(env):
    arena = [b for b in env.sys.config.bodies if b.name == "Arena"][0]
    z = [q.pos.z for d in env.sys.config.defaults for q in d.qps if q.name == "Arena"][0]
    rows = [[c.position.x, c.position.y, c.rotation.z, c.box.halfsize.x, c.box.halfsize.y, c.box.halfsize.z, z]
            for c in arena.colliders]
    return np.array(rows, np.float32)


# ----------------------------------------------------------------------- the wrappers
def _grab(st, extra=None):
    d = dict(pos=st.qp.pos, rot=st.qp.rot, vel=st.qp.vel, ang=st.qp.ang, obs=st.obs, reward=st.reward,
             done=np.asarray(st.done, np.float32), steps=st.info["steps"], rng=np.asarray(st.info["rng"], np.uint32))
    d.update(extra or {})
    return {k: np.array(v) for k, v in d.items()}


def reference_wrappers(ref):
    W = ref.wrappers
    kind = TC.WRAP_KIND
    steps0 = (np.arange(TC.WRAP_B) % 3).astype(np.float32)
    fix = dict(wrap_act_seed=np.int64(17), wrap_steps0=steps0)
    keys, _, acts = TC.wrap_inputs(fix)
    runs = {}
    # RandomizedAutoResetWrapperNaive
    inner = RS.OracleBatchEnv(kind, TC.WRAP_L)
    env = W.RandomizedAutoResetWrapperNaive(inner)
    st = env.reset(keys)
    st.info["steps"] = steps0.copy()
    rows = []
    for act in acts:
        st = env.step(st, act)
        rows.append(_grab(st, dict(inner_done=inner.inner_done[-1])))
    runs["naive"] = rows
    # RandomizedAutoResetWrapperCached, refreshed every third step
    inner = RS.OracleBatchEnv(kind, TC.WRAP_L)
    env = W.RandomizedAutoResetWrapperCached(inner, n_steps_between_updates=TC.WRAP_N)
    st = env.reset(keys)
    st.info["steps"] = steps0.copy()
    rows = []
    for act in acts:
        st = env.step(st, act)
        rows.append(_grab(st, dict(inner_done=inner.inner_done[-1], first_obs=st.info["first_obs"],
                                   first_pos=st.info["first_qp"].pos)))
    runs["cached"] = rows
    # AutoresetVmapGymWrapper
    inner = RS.OracleBatchEnv(kind, TC.WRAP_L)
    g = W.AutoresetVmapGymWrapper(inner, TC.WRAP_B, seed=TC.GYM_SEED)
    obs = g.reset()
    g._state.info["steps"] = steps0.copy()
    rows = []
    for act in acts:
        obs, reward, done, _info = g.step(act)
        row = _grab(g._state, dict(inner_done=inner.inner_done[-1], key=np.asarray(g._key, np.uint32)))
        row.update(obs=np.array(obs), reward=np.array(reward), done=np.asarray(done, np.float32))
        rows.append(row)
    runs["gym"] = rows
    for name, rows in runs.items():
        for k in rows[0]:
            fix[f"{name}_{k}"] = np.stack([r[k] for r in rows])
        d = fix[f"{name}_inner_done"]
        assert (d != 0).any(1).sum() >= 3 and (d == 0).any(1).all(), (name, d)  # some done, some not, per step
    return fix


# -------------------------------------------------------------------------------- main
def write_npz(path, arrays):
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) if np.ndim(v) else np.asarray(v)
                                 for k, v in sorted(arrays.items())})


def build_kind(ref, kind):
    env = make_env(ref, kind)
    fix = dict(reset_seed=np.int64(RESET_SEED[kind]), step_seed=np.int64(STEP_SEED[kind]))
    fix.update(reference_reset(env, kind))
    base = orc.OracleEnv(kind).reset(TC.keys(STEP_SEED[kind], TC.B_STEP))
    rng = np.random.default_rng(STEP_SEED[kind])
    act = rng.uniform(-1, 1, (TC.B_STEP, 8)).astype(F32)
    off, frozen, keys, role = ARRANGE[kind](base, act, rng)
    fix.update(step_off=off.astype(F32), step_frozen=frozen.astype(F32), step_rng=np.ascontiguousarray(keys, np.uint32),
               step_act=act, step_role=np.asarray(role, np.int8))
    state = TC.arrange(kind, base, fix)
    fix.update(reference_step(env, kind, state, act, TC.keys(STEP_SEED[kind], TC.B_STEP)))
    fix["walls"] = reference_walls(env)
    if kind == GA:
        fix["grid"] = f32(env.possible_grid_positions, "grid")
        fix["waiting_area"] = f32(env.waiting_area, "waiting_area")
        fix.update(build_ga_alt(ref))
    if kind == TC.WRAP_KIND:
        fix.update(reference_wrappers(ref))
    if kind == GA:
        # the sensor bins pass through arctan2 and quat_mul, which the stand-in takes from the
        # oracle: with numpy's arctan2 and an unfused product every observation must be the same,
        # so that no recorded case hangs on whose rounding it is
        RS.MATH = "numpy"
        try:
            other = dict(reference_reset(env, kind))
            other.update(reference_step(env, kind, state, act, TC.keys(STEP_SEED[kind], TC.B_STEP)))
            other.update({k: v for k, v in build_ga_alt(ref).items() if k == "alt_obs"})
        finally:
            RS.MATH = "oracle"
        for k in ("reset_obs", "step_obs", "alt_obs"):
            assert np.array_equal(other[k], fix[k]), (k, "depends on the rounding of arctan2 / quat_mul")
    counts = TC.assert_events(kind, fix)
    return fix, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", nargs="?", default=os.environ.get("PO_BRAX_REFERENCE"))
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, "po_brax")):
        sys.exit("the reference checkout is needed (argument or $PO_BRAX_REFERENCE)")
    ref = RS.load(args.reference)
    for kind in TC.KINDS:
        fix, counts = build_kind(ref, kind)
        out = os.path.join(args.out, os.path.basename(TC.path(kind)))
        write_npz(out, fix)
        print(f"{kind}: {os.path.getsize(out)} bytes; events {counts}")


if __name__ == "__main__":
    main()
