"""NumPy stand-in for the modules the reference's env files import -- TEST INFRASTRUCTURE ONLY.

The reference's task code (``po_brax/envs/ant_heavenhell.py``, ``ant_gather.py``, ``ant_tag.py``,
``utils.py``, ``wrappers.py``, ``more_jp.py``) is plain Python over ``brax.jumpy``.  With this module
installed in ``sys.modules`` those files import and run unchanged, without jax, brax, protobuf
or gym, so that tests/golden/make_task_logic_fixture.py can record what the reference's OWN code
returns for arranged states.  Nothing here is the reference's text, and nothing of the reference is
copied: ``load()`` imports its files from a tree given by path, and only where that tree exists.

What the stand-in decides, and what it therefore does NOT pin:

* arithmetic is numpy float32 / int32 (jnp's defaults with x64 off); python scalars are weak, as
  in jax (numpy >= 2 promotion);
* index scatter (``index_update``, ``.at[].set``) follows numpy, which is what the oracle assumes
  of XLA: among equal indices the last writer wins and ``-1`` wraps to the last slot; an index
  past the end is dropped, as jax's ``.at[].set`` does (AntGather's bin 10 of an object at exactly
  +half_span, with ten apples);
* ``jp.norm`` is ``sqrt(sum(x * x))`` in float32 without contraction;
* the random functions are oracle/pob_np.py's (threefry split / uniform / randint / choice "as
  recalled"): pinned is which key feeds which draw, not the generators;
* ``arctan2`` and ``brax.math.quat_mul`` are the C oracle's (orc.math_check): XLA's own roundings
  are not available, pinned is what is fed to them and what is done with the result.  ``MATH =
  "numpy"`` switches both to numpy's arctan2 and an unfused product; the maker records nothing
  unless every AntGather observation comes out the same under either;
* ``brax.System`` is the C oracle: ``default_angle`` / ``default_qp`` / ``info`` / ``step`` (the
  physics alone, orc_physics_only: the ant bodies as the oracle leaves them, the frozen bodies
  where they were, the unclipped contact terms) / ``joints[0].angle_vel``.  Body names, indices and
  ``num_bodies`` come from the config the reference's own ``extend_ant_cfg`` builds;
* ``_in_jit()`` is true and ``_which_np`` returns the jnp side, so more_jp.py takes its jitted
  branches (threefry, ``lax.while_loop``), never ``default_rng``;
* ``random_split`` of a batch of keys (B, 2) splits every key and returns (num, B, 2): the only
  shape under which RandomizedAutoResetWrapperCached's ``rng, rng1 = split(info['rng'], 2)`` runs
  on a batched env (jax.vmap of split); brax's own VectorGymWrapper is restated as far as
  AutoresetVmapGymWrapper needs it (``seed``, ``reset``) [ext].
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types
import typing

import numpy as np

import orc
import pob_np as P

HERE = os.path.dirname(os.path.abspath(__file__))
F32, I32 = np.float32, np.int32
RANDINT_LOG = []  # every jax.random.randint draw, in call order (the TAG adversary's choices)


# ------------------------------------------------------------------------------ arrays
class Arr(np.ndarray):
    """ndarray with jnp's functional update property ``.at``."""

    @property
    def at(self):
        return _At(self)


class _At:
    def __init__(self, x, idx=None):
        self.x, self.idx = x, idx

    def __getitem__(self, idx):
        return _At(self.x, idx)

    def add(self, y):
        out = np.array(self.x)
        np.add.at(out, self.idx, y)
        return out.view(Arr)

    def set(self, y, mode=None):
        out = np.array(self.x)
        out[self.idx] = y
        return out.view(Arr)


def _a(x, dtype=None):
    """jnp.asarray with x64 off: 64-bit floats and ints become 32-bit."""
    x = np.asarray(x, dtype)
    if dtype is None:
        if x.dtype == np.float64:
            x = x.astype(F32)
        elif x.dtype == np.int64:
            x = x.astype(I32)
    return x.view(Arr) if x.ndim else x[()]


MATH = "oracle"  # "numpy": numpy's arctan2 and an unfused quaternion product instead of the oracle's
                 # (the maker asserts that no recorded case depends on the choice)


def _arctan2(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, F32), np.asarray(x, F32))
    if MATH == "numpy":
        return _a(np.arctan2(y, x))
    out = orc.math_check(0, np.ascontiguousarray(y.ravel()), np.ascontiguousarray(x.ravel()))
    return _a(out.reshape(y.shape))


def _norm(x, axis=None):
    x = np.asarray(x)
    return _a(np.sqrt(np.sum(x * x, axis=axis)))


def _where(condition, x=None, y=None):
    return _a(np.where(condition, x, y))


def _index_update(x, idx, y):
    out = np.array(x)
    if isinstance(idx, np.ndarray) and idx.dtype.kind == "i" and idx.ndim == 1 and np.ndim(y) == 1:
        ok = (idx >= -len(out)) & (idx < len(out))  # jax drops a scatter index past the end
        idx, y = idx[ok], np.asarray(y)[ok]
    out[idx] = y
    return out.view(Arr)


def _split(key, num=2):
    key = np.asarray(key, np.uint32)
    if key.ndim == 2:  # a batch of keys: every key split, the split axis first
        return np.stack([P.split(k, num) for k in key], 1)
    return P.split(key, num)


def _uniform(key, shape=(), low=0.0, high=1.0):
    return _a(P.uniform(np.asarray(key, np.uint32), tuple(shape), low, high))


def _tree_map(fn, *trees):
    t = trees[0]
    if isinstance(t, QP):
        return QP(*[fn(*[getattr(x, f) for x in trees]) for f in QP.FIELDS])
    if isinstance(t, dict):
        return {k: _tree_map(fn, *[x[k] for x in trees]) for k in t}
    return fn(*trees)


def _numpy_like(name, extra):
    """a module whose creation functions give 32-bit arrays and whose other names are numpy's"""
    m = types.ModuleType(name)

    def wrap(f):
        return lambda *a, **k: _a(f(*a, **k))

    for n in ("array", "asarray", "zeros", "ones", "zeros_like", "ones_like", "arange", "stack", "concatenate",
              "multiply", "abs", "sign", "clip", "reshape", "arccos", "dot", "logical_and", "logical_or", "sqrt",
              "sum", "maximum", "minimum", "atleast_1d", "atleast_2d", "atleast_3d", "nanmean", "amax", "amin"):
        setattr(m, n, wrap(getattr(np, n)))
    m.meshgrid = lambda *xi, **k: [_a(g) for g in np.meshgrid(*xi, **k)]
    m.arctan2, m.where = _arctan2, _where
    m.float32, m.int32, m.pi, m.inf, m.nan, m.ndarray = F32, I32, np.pi, np.inf, np.nan, np.ndarray
    for k, v in extra.items():
        setattr(m, k, v)
    return m


# ------------------------------------------------------------------ protobuf messages
_REPEATED = ("bodies", "colliders", "defaults", "qps", "collide_include", "joints", "actuators")


class Msg:
    """autovivifying protobuf message: unknown fields are sub-messages, the repeated ones lists"""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = Repeated() if name in _REPEATED else Msg()
        object.__setattr__(self, name, v)
        return v


class Repeated(list):
    def add(self, **kw):
        m = Msg(**kw)
        self.append(m)
        return m


ANT_CONFIG_TEXT = "<the ant's system config>"  # brax.envs.ant._SYSTEM_CONFIG: read by Parse only


def _parse(text, msg):
    """text_format.Parse of the ant's config: the ant's bodies and the Ground, in the order of the
    Config export of the reference's notebook (tests/golden/ant_tag_notebook_trajectory.json,
    pinned by tests/test_export.py)."""
    assert text is ANT_CONFIG_TEXT
    path = os.path.join(HERE, "..", "tests", "golden", "ant_tag_notebook_trajectory.json")
    with open(path) as f:
        bodies = json.load(f)["config"]["bodies"]
    names = [b["name"] for b in bodies]
    for b in bodies[:names.index("Ground") + 1]:
        msg.bodies.add(name=b["name"], mass=b["mass"])
    return msg


# ----------------------------------------------------------------------- brax objects
class QP:
    FIELDS = ("pos", "rot", "vel", "ang")

    def __init__(self, pos, rot, vel, ang):
        self.pos, self.rot, self.vel, self.ang = (_a(x, F32) for x in (pos, rot, vel, ang))

    def replace(self, **kw):
        return QP(*[kw.get(f, getattr(self, f)) for f in self.FIELDS])


class State:
    FIELDS = ("qp", "obs", "reward", "done", "metrics", "info")

    def __init__(self, qp, obs, reward, done, metrics=None, info=None):
        self.qp, self.obs, self.reward, self.done = qp, obs, reward, done
        self.metrics = {} if metrics is None else metrics
        self.info = {} if info is None else info

    def replace(self, **kw):
        return State(*[kw.get(f, getattr(self, f)) for f in self.FIELDS])


class Env:
    @property
    def unwrapped(self):
        return self

    @property
    def observation_size(self):
        return self.unwrapped._observation_size

    @property
    def action_size(self):
        return 8


class Wrapper(Env):
    def __init__(self, env):
        self.env = env

    def reset(self, rng):
        return self.env.reset(rng)

    def step(self, state, action):
        return self.env.step(state, action)

    @property
    def unwrapped(self):
        return self.env.unwrapped

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.env, name)


class _Joint:
    def __init__(self, system):
        self._sys = system

    def angle_vel(self, qp):
        a, v = self._sys.oracle.joint_angle_vel(qp.pos, qp.rot, qp.vel, qp.ang)
        return (_a(a),), (_a(v),)


class System:
    """brax.System over the C oracle (see the module docstring)."""

    def __init__(self, config):
        self.config = config
        names = [b.name for b in config.bodies]
        self.body = types.SimpleNamespace(index={n: i for i, n in enumerate(names)})
        self.num_bodies = len(names)
        kind = "ant_heavenhell" if "Priest" in names else ("ant_gather" if "Bomb_1" in names else "ant_tag")
        self.oracle = orc.OracleEnv(kind)
        assert self.oracle.N == self.num_bodies, (kind, self.oracle.N, names)
        self.num_joint_dof = 8
        self.joints = [_Joint(self)]
        config.dt, config.substeps = 0.05, 10

    def default_angle(self):
        return _a(P.default_angle())

    def default_qp(self, joint_angle=None, joint_velocity=None):
        qpos = self.default_angle() if joint_angle is None else joint_angle
        qvel = np.zeros(8, F32) if joint_velocity is None else joint_velocity
        return QP(*self.oracle.default_qp(qpos, qvel))

    @staticmethod
    def _info(cv, ca):
        return types.SimpleNamespace(contact=types.SimpleNamespace(vel=_a(cv), ang=_a(ca)))

    def info(self, qp):
        return self._info(*self.oracle.contact_info(qp.pos, qp.rot, qp.vel, qp.ang))

    def step(self, qp, act):
        q, (cv, ca) = self.oracle.physics_only(qp.pos, qp.rot, qp.vel, qp.ang, act)
        return QP(*q), self._info(cv, ca)


class OracleBatchEnv(Env):
    """A batched env for the reference's wrappers to wrap: ``reset`` and ``step`` are the C
    oracle's, with brax's EpisodeWrapper folded in (F_EPISODE: info['steps'], info['truncation'],
    done at ``episode_length``).  ``inner_done`` keeps ``done`` as every inner step returned it."""

    def __init__(self, kind, episode_length):
        self.oracle = orc.OracleEnv(kind)
        self.episode_length = int(episode_length)
        self._observation_size = self.oracle.D
        self.sys = types.SimpleNamespace(config=types.SimpleNamespace(dt=0.05, substeps=10))
        self.inner_done = []

    @staticmethod
    def _state(s):
        return State(QP(s["pos"], s["rot"], s["vel"], s["ang"]), _a(s["obs"]), _a(s["reward"]), _a(s["done"]),
                     {k: _a(s[k]) for k in ("m0", "m1", "m2")},
                     {"rng": s["rng"].copy(), "steps": _a(s["steps"]), "truncation": _a(s["truncation"])})

    def reset(self, rng):
        return self._state(self.oracle.reset(np.asarray(rng, np.uint32)))

    def step(self, state, action):
        c = lambda x, t=F32: np.array(x, t, order="C")  # noqa: E731
        s = dict(pos=c(state.qp.pos), rot=c(state.qp.rot), vel=c(state.qp.vel), ang=c(state.qp.ang),
                 obs=c(state.obs), reward=c(state.reward), done=c(state.done), steps=c(state.info["steps"]),
                 truncation=c(state.info["truncation"]), rng=c(state.info["rng"], np.uint32),
                 **{k: c(state.metrics[k]) for k in ("m0", "m1", "m2")})
        out = self.oracle.step(s, np.asarray(action, F32), flags=orc.F_EPISODE, episode_length=self.episode_length)
        self.inner_done.append(out["done"].copy())
        new = self._state(out)
        state.metrics.update(new.metrics)
        state.info.update(new.info)
        return state.replace(qp=new.qp, obs=new.obs, reward=new.reward, done=new.done)


def _quat_mul(u, v):
    if MATH == "numpy":
        u, v = np.asarray(u, F32), np.asarray(v, F32)
        return _a(np.array([u[0] * v[0] - u[1] * v[1] - u[2] * v[2] - u[3] * v[3],
                            u[0] * v[1] + u[1] * v[0] + u[2] * v[3] - u[3] * v[2],
                            u[0] * v[2] - u[1] * v[3] + u[2] * v[0] + u[3] * v[1],
                            u[0] * v[3] + u[1] * v[2] - u[2] * v[1] + u[3] * v[0]], F32))
    u, v = (np.ascontiguousarray(np.asarray(x, F32).reshape(1, 4)) for x in (u, v))
    return _a(orc.math_check(2, u, v)[0])


def _quat_inv(q):
    return _a(np.asarray(q, F32) * np.array([1, -1, -1, -1], F32))


class VectorGymWrapper:
    """brax's VectorGymWrapper as far as AutoresetVmapGymWrapper builds on it [ext]"""

    def seed(self, seed=0):
        self._key = P.prngkey(seed)

    def reset(self):
        self._state, obs, self._key = self._reset(self._key)
        return obs

    def step(self, action):
        self._state, obs, reward, done, info = self._step(self._state, action)
        return obs, reward, done, info


def _randint(key, shape=(), minval=0, maxval=1):
    assert tuple(shape) == ()
    v = P.randint(np.asarray(key, np.uint32), int(minval), int(maxval))
    RANDINT_LOG.append(v)
    return I32(v)


def _choice(key, a, shape=(), replace=True, p=None, axis=0):
    assert not replace and p is None and axis == 0 and len(shape) == 1
    return _a(P.choice_noreplace(np.asarray(key, np.uint32), np.asarray(a), int(shape[0])))


def _while_loop(cond_fun, body_fun, init_val):
    val = init_val
    while cond_fun(val):
        val = body_fun(val)
    return val


def _fori_loop(lower, upper, body_fun, init_val):
    val = init_val
    for i in range(lower, upper):
        val = body_fun(i, val)
    return val


def _mod(name, **kw):
    m = types.ModuleType(name)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def modules() -> dict:
    """the stand-in modules by import name"""
    jnp = _numpy_like("jax.numpy", {})
    jp = _numpy_like("brax.jumpy", dict(
        norm=_norm, index_update=_index_update, random_split=_split, random_uniform=_uniform,
        random_prngkey=P.prngkey, tree_map=_tree_map, onp=np, jnp=jnp,
        _in_jit=lambda: True, _which_np=lambda *a: jnp,
        X=typing.TypeVar("X"), Optional=typing.Optional, Tuple=typing.Tuple, Callable=typing.Callable,
        Any=typing.Any))
    jrandom = _mod("jax.random", randint=_randint, choice=_choice, split=_split, PRNGKey=P.prngkey)
    lax = _mod("jax.lax", while_loop=_while_loop, fori_loop=_fori_loop,
               cond=lambda pred, t, f, *ops: t(*ops) if pred else f(*ops))
    jax = _mod("jax", numpy=jnp, lax=lax, random=jrandom, tree_map=_tree_map,
               jit=lambda fn, **kw: fn, block_until_ready=lambda x: x)
    bmath = _mod("brax.math", quat_mul=_quat_mul, quat_inv=_quat_inv)
    pmath = _mod("brax.physics.math", quat_mul=_quat_mul, quat_inv=_quat_inv)
    pb2 = _mod("brax.physics.config_pb2", Body=Msg, Config=Msg)
    physics = _mod("brax.physics", math=pmath, config_pb2=pb2)
    benv = _mod("brax.envs.env", Env=Env, State=State, Wrapper=Wrapper)
    bant = _mod("brax.envs.ant", _SYSTEM_CONFIG=ANT_CONFIG_TEXT)
    bwrap = _mod("brax.envs.wrappers", VmapWrapper=Wrapper, VectorWrapper=Wrapper, AutoResetWrapper=Wrapper,
                 EpisodeWrapper=Wrapper, VectorGymWrapper=VectorGymWrapper, GymWrapper=VectorGymWrapper)
    benvs = _mod("brax.envs", env=benv, ant=bant, wrappers=bwrap)
    brax = _mod("brax", jumpy=jp, math=bmath, physics=physics, envs=benvs, Config=Msg, System=System, QP=QP,
                Info=types.SimpleNamespace)
    tf = _mod("google.protobuf.text_format", Parse=_parse)
    pbuf = _mod("google.protobuf", text_format=tf)
    google = _mod("google", protobuf=pbuf)
    box = lambda low, high, dtype=None: types.SimpleNamespace(low=low, high=high, dtype=dtype)  # noqa: E731
    spaces = _mod("gym.spaces", Box=box)
    vutils = _mod("gym.vector.utils", batch_space=lambda space, n: (space, n))
    vector = _mod("gym.vector", utils=vutils, VectorEnv=object)
    gym = _mod("gym", spaces=spaces, vector=vector, Wrapper=object, Env=object)
    out = {m.__name__: m for m in (jnp, jp, jrandom, lax, jax, bmath, pmath, pb2, physics, benv, bant, bwrap,
                                   benvs, brax, tf, pbuf, google, spaces, vutils, vector, gym)}
    for name in ("brax", "brax.physics", "brax.envs", "google", "google.protobuf", "gym", "gym.vector", "jax"):
        out[name].__path__ = []
    return out


def load(ref_root: str) -> types.SimpleNamespace:
    """Install the stand-ins and import the reference's env modules from ``ref_root`` without its
    ``envs/__init__.py`` (which pulls in all of brax).  No bytecode is written: the tree may be
    read-only.  Returns the imported modules by short name."""
    sys.dont_write_bytecode = True
    sys.modules.update(modules())
    root = os.path.join(ref_root, "po_brax")
    for name, path in (("po_brax", root), ("po_brax.envs", os.path.join(root, "envs"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    names = ("more_jp", "envs.utils", "envs.ant_heavenhell", "envs.ant_gather", "envs.ant_tag", "envs.wrappers")
    return types.SimpleNamespace(**{n.split(".")[-1]: importlib.import_module("po_brax." + n) for n in names})
