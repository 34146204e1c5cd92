"""Multi-step rollouts replayed from a HIP graph.

``env.step_`` issues one fused kernel per env-step from Python (ctypes argument marshalling,
a launch per step).  For a fixed-shape loop -- the same State buffers stepped in place with
actions taken from a device array -- the launches can be captured once into a hipGraph
(``torch.cuda.CUDAGraph``: the kernels go to torch's current stream, which is the capture
stream inside ``torch.cuda.graph``) and replayed with one call, so consecutive step kernels
run back to back with no host work in between.  This is the MI355X replacement for the
reference's ``jax.jit`` / ``lax.scan`` of the step function over time: everything executed
is the same kernels on the same data, nothing is skipped.

    roll = GraphRollout(env, state, actions)   # actions: (T, B, 8) device tensor
    roll.replay()                              # T env-steps, in place on ``state``

``state`` must be stepped in place (its buffers are the graph's buffers); refill
``actions`` between replays to feed new actions (``roll.actions`` is the captured array).
Works for ``create(...)`` chains and ``MixedEnv`` (one launch per step either way); the gym
wrappers keep their eager path.
"""
from __future__ import annotations

import contextlib
import gc
from typing import Sequence

import torch


def _release_deferred():
    """Outside a capture: free the tables of envs destroyed (possibly by a GC pass inside the
    capture) since the last env creation (include/pob.h pob_release_deferred)."""
    from . import _lib
    _lib.release_deferred()


@contextlib.contextmanager
def no_gc():
    """Keep the cyclic garbage collector off for the span of a hipGraph capture: a collection
    there runs arbitrary finalisers, and any HIP runtime call one makes that is illegal during
    a global-mode capture (hipFree, a synchronisation) invalidates the capture.  (The engine's
    own handles are already safe -- no env <-> System cycle, and pob_env_destroy defers its
    frees -- this guards the caller's objects too.)"""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _slice_state(state, lo: int, hi: int, B: int):
    """The State of envs [lo, hi): every per-env tensor (first dim B, batch-major, so the
    slice is a contiguous view) sliced, the same object -> the same view (the engine tells
    its public tensors from caller replacements by identity, envs/env.py _bufs_of)."""
    from .envs.env import QP, State
    memo = {}

    def sl(x):
        if isinstance(x, torch.Tensor):
            if x.dim() >= 1 and x.shape[0] == B:
                if id(x) not in memo:
                    memo[id(x)] = x[lo:hi]
                return memo[id(x)]
            return x
        if isinstance(x, QP):
            return QP(sl(x.pos), sl(x.rot), sl(x.vel), sl(x.ang))
        if isinstance(x, dict):
            return {k: sl(v) for k, v in x.items()}
        return x

    return State(sl(state.qp), sl(state.obs), sl(state.reward), sl(state.done), sl(state.metrics),
                 sl(state.info), sl(state.aux))


class GraphRollout:
    def __init__(self, env, state, actions: torch.Tensor, warmup: bool = False, groups: int = 1):
        """Capture ``actions.shape[0]`` in-place steps of ``env`` on ``state``.

        Capture does not execute the kernels; ``warmup=True`` first runs one eager step on a
        side stream (needed only when the env has never been stepped in this process, so
        that lazily initialised state is set up outside the capture).

        ``groups = G > 1`` (single-kind envs): the batch is split into G contiguous env groups
        whose step chains are captured on G streams -- the groups are independent, so group
        g's step t + 1 may start while group g' still finishes step t, filling the SIMDs a
        launch's last waves leave idle.  Every env still takes exactly the same steps with
        the same kernels and actions (results bit-identical to ``groups = 1``)."""
        if actions.dim() != 3:
            raise ValueError("actions must be (T, B, A)")
        self.env, self.state, self.actions = env, state, actions
        self.steps = int(actions.shape[0])
        dev = actions.device
        B = int(actions.shape[1])
        groups = max(1, min(int(groups), B))
        if groups > 1 and isinstance(state, (list, tuple)):
            raise ValueError("groups > 1 needs a single-kind env")
        if warmup:
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                self.state = self.env.step_(self.state, self.actions[0])
            torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        if groups == 1:
            with no_gc(), torch.cuda.graph(self.graph):
                for t in range(self.steps):
                    # follow the returned State: its public typed outputs (TAG done, GA
                    # counts) are the buffers the captured kernels write
                    self.state = self.env.step_(self.state, self.actions[t])
            _release_deferred()
            return
        bounds = [(B * g // groups, B * (g + 1) // groups) for g in range(groups)]
        # the typed step outputs (TAG bool done, GA int32 counts) live in the whole batch's
        # buffers, so that the groups write slices of them
        u = env.unwrapped
        u._typed_outputs(self.state.aux, B, "steps" in self.state.info)
        parts = [_slice_state(self.state, lo, hi, B) for lo, hi in bounds]
        streams = [None] + [torch.cuda.Stream(dev) for _ in range(groups - 1)]
        with no_gc(), torch.cuda.graph(self.graph):
            cap = torch.cuda.current_stream(dev)
            for st in streams[1:]:
                st.wait_stream(cap)  # fork from the capture stream
            for t in range(self.steps):
                for g, (lo, hi) in enumerate(bounds):
                    with torch.cuda.stream(streams[g] or cap):
                        parts[g] = self.env.step_(parts[g], self.actions[t, lo:hi])
            for st in streams[1:]:
                cap.wait_stream(st)  # join
        self.parts = parts
        _release_deferred()
        # the whole batch's State after a step (public fields in the reference's dtypes)
        self.state = u._state_of(u._bufs_of(self.state), True, False)

    def replay(self):
        """Run the captured steps (stream-ordered on torch's current stream)."""
        self.graph.replay()
        return self.state


def graph_rollout(env, state, actions: Sequence[torch.Tensor] | torch.Tensor) -> GraphRollout:
    """Convenience: capture a rollout of ``actions`` (T, B, A) and return it (not run)."""
    if not isinstance(actions, torch.Tensor):
        actions = torch.stack(list(actions))
    return GraphRollout(env, state, actions)


class GymGraphRollout:
    """``T`` steps of a gym vector env (``create_gym_env``: ``AutoresetVmapGymWrapper``,
    wrappers.py:240-262) captured into one hipGraph: per step the fused step kernel (which
    also ORs the device any-done word) and the masked gym reset kernel (which reads that word,
    re-samples the done envs from ``split(gym_key, B + 1)`` and advances the key only if
    something was done).  The decision ``if done.any()`` lives on the device, so the whole
    loop is capture-safe; nothing is skipped -- the same kernels run on the same buffers as
    ``gym.step`` called T times.

    The wrapper's host-side bookkeeping (the alternating any-done words and gym-key buffers)
    is advanced by the capture itself, so ``T`` must be even: after T steps it is back where
    it started, and every replay continues from the device state the last one left.
    ``actions`` (T, B, A) is read at replay time (refill it between replays).  Sharded
    (``create_gym_env(shard=...)``) under an RCCL process group, each step's 4-byte any-done
    all-reduce is captured with the kernels (RCCL collectives are stream-ordered and
    capturable: bit-equal to the eager steps through a one-rank communicator,
    ``scripts/gym_capture_check.py``, profiles/r7w); a gloo group's host-side collective
    cannot be captured, so that case is refused."""

    def __init__(self, gym, actions: torch.Tensor):
        from .envs.wrappers import AutoresetVmapGymWrapper, EvalGymWrapper
        if actions.dim() != 3 or actions.shape[0] % 2:
            raise ValueError("actions must be (T, B, A) with T even")
        # Only the bare device-side gym is capture-safe.  A wrapper with host-side per-step
        # bookkeeping (EvalGymWrapper's queue count / growth; it forwards _shard / _state to the
        # inner gym) would not advance on replay -- its queue would overrun its fixed capacity --
        # and may sync the host inside the capture, so it is refused by type.
        if isinstance(gym, EvalGymWrapper):
            raise NotImplementedError("GymGraphRollout cannot capture an EvalGymWrapper (host-side episode "
                                      "queues); capture the inner gym and step the eval wrapper eagerly")
        if not isinstance(gym, AutoresetVmapGymWrapper):
            raise NotImplementedError(f"GymGraphRollout captures create_gym_env's AutoresetVmapGymWrapper, "
                                      f"not {type(gym).__name__}")
        sh = getattr(gym, "_shard", None)
        if sh is not None:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_backend(sh.group) != "nccl":
                raise NotImplementedError("a sharded gym step captures its any-done all-reduce over RCCL "
                                          "(backend nccl) only; over gloo it steps eagerly")
        if gym._state is None:
            raise ValueError("reset() the gym before capturing its steps")
        self.gym, self.actions = gym, actions
        self.steps = int(actions.shape[0])
        dev = actions.device
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with no_gc(), torch.cuda.graph(self.graph):
            for t in range(self.steps):
                gym.step(self.actions[t])
        # the buffers the captured kernels read and write (T even: the key pair is back in order)
        self._captured = (gym._state, gym._key, gym._key2)
        _release_deferred()

    def replay(self):
        """Run the captured gym steps; returns (obs, reward, done, metrics) of the last."""
        st, k, k2 = self._captured
        g = self.gym
        if g._state is not st or g._key is not k or g._key2 is not k2:
            raise RuntimeError("the gym was reset or stepped outside the captured graph since capture; "
                               "rebuild the GymGraphRollout")
        self.graph.replay()
        return st.obs, st.reward, st.done, st.metrics


class PolicyRollout:
    """``T`` env-steps with the policy in the loop, replayed from ONE hipGraph: per step
    ``action = policy(obs)`` (any torch ops -- an MLP on hipBLASLt, sampling with a device
    generator -- static shapes, no host sync) then the fused step kernel, and the trajectory
    written to device buffers.  This is the MI355X counterpart of the reference's training-side
    ``jax.lax.scan`` over (policy, ``env.step``): one replay runs the whole unroll with no
    per-step host work.

        roll = PolicyRollout(env, state, policy, steps=T)
        roll.replay()        # T steps, in place on ``state``
        roll.obs[t]          # (B, D) observation the policy acted on at step t
        roll.actions[t], roll.reward[t], roll.done[t]   # its action, then the step's reward / done

    ``done`` is float32 (the engine's done; AntTag's public bool done is ``done != 0``).  The
    capture is preceded by ``warmup`` eager policy calls on a side stream (library handles and
    workspaces must exist before a capture); they do not step the env."""

    def __init__(self, env, state, policy, steps: int, warmup: int = 2):
        if steps <= 0:
            raise ValueError("steps must be positive")
        self.env, self.state, self.policy, self.steps = env, state, policy, int(steps)
        obs = state.obs
        dev = obs.device
        B, D = int(obs.shape[0]), int(obs.shape[1])
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, int(warmup))):
                a = policy(obs)
        torch.cuda.current_stream(dev).wait_stream(side)
        if not (isinstance(a, torch.Tensor) and a.shape == (B, env.action_size) and a.is_cuda):
            raise ValueError(f"policy must map obs (B, D) to a (B, {env.action_size}) device tensor")
        T = self.steps
        self.obs = torch.empty((T, B, D), dtype=obs.dtype, device=dev)
        self.actions = torch.empty((T, B, env.action_size), dtype=torch.float32, device=dev)
        self.reward = torch.empty((T, B), dtype=torch.float32, device=dev)
        self.done = torch.empty((T, B), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with no_gc(), torch.cuda.graph(self.graph):
            for t in range(T):
                self.obs[t].copy_(self.state.obs)
                self.actions[t].copy_(policy(self.state.obs))
                self.state = env.step_(self.state, self.actions[t])
                self.reward[t].copy_(self.state.reward)
                self.done[t].copy_(self.state.aux["done"] if "done" in self.state.aux else self.state.done)

    def replay(self):
        """Run the captured unroll (stream-ordered on torch's current stream)."""
        self.graph.replay()
        return self.state


class ActorRollout:
    """The native unroll of a ``training.networks.NormalTanhPolicy``: ``T`` env-steps captured
    into ONE hipGraph, per step one ``pob_policy_act`` launch (forward, tanh-normal head, and
    the observation rows written out again) straight into the (T, B, ...) trajectory buffers,
    the one-thread key advance, the fused step kernel, and the reward / done copies.  Equal,
    bit for bit, to ``PolicyRollout`` with the same policy, without its per-step observation
    and action copies.

        roll = ActorRollout(env, state, policy, steps=T)
        roll.replay()
        roll.obs[t], roll.actions[t], roll.logp[t], roll.raw[t]   # what the policy saw and did
        roll.reward[t], roll.done[t]                              # the step's outcome

    The parameters are read at replay time: ``policy.theta`` updated in place between replays
    changes the next replay's actions.  Single-kind ``create(...)`` chains only.

    A policy with a ``normalizer`` acts on the normalised observation (``roll.obs`` keeps the raw
    rows).  ``update_normalizer=True`` appends the statistics update over ``roll.obs`` (T B rows)
    as the graph's last nodes: a replay acts under the table it started with and leaves the
    updated one for the next (brax PPO's order), with no host work in between.

    ``critic=training.gae.ValueFunction(...)`` appends the critic pass (DESIGN.md "Critic pass and
    GAE"): the observation buffer gains a row ``T`` (``roll.final_obs``, the last state's
    observation; ``roll.obs`` stays the (T, B, D) view), every step records ``roll.truncation[t]``,
    and after the normaliser update the graph ends with one value launch over all (T + 1) B rows
    into ``roll.values`` (T + 1, B) and one ``pob_gae`` launch into ``roll.vs`` and
    ``roll.advantages`` (T, B), bootstrapped from ``values[T]``; ``gae=dict(lambda_=, discount=,
    reward_scaling=)`` over ``compute_gae``'s defaults.  ``record_truncation=True`` records
    ``roll.truncation`` without a critic."""

    def __init__(self, env, state, policy, steps: int, update_normalizer: bool = False, critic=None, gae=None,
                 record_truncation: bool = False):
        from .training.networks import NormalTanhPolicy
        if steps <= 0:
            raise ValueError("steps must be positive")
        if not isinstance(policy, NormalTanhPolicy):
            raise TypeError("policy must be a training.networks.NormalTanhPolicy")
        if isinstance(state, (list, tuple)):
            raise NotImplementedError("ActorRollout unrolls a single-kind create(...) env, not a MixedEnv")
        obs = state.obs
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2):
            raise ValueError("state.obs must be a float32 (B, D) device tensor")
        B, D = int(obs.shape[0]), int(obs.shape[1])
        A = env.action_size
        if policy.action_size != A or policy.obs_size != D:
            raise ValueError(f"the policy maps {policy.obs_size} -> {policy.action_size}, the env {D} -> {A}")
        self.env, self.state, self.policy, self.steps = env, state, policy, int(steps)
        dev, T = obs.device, self.steps
        self.update_normalizer = _normalizer_to_update(policy, update_normalizer, T * B)
        self.obs = _critic_buffers(self, critic, gae, record_truncation, state, T, B, D, dev)
        self.actions = torch.empty((T, B, A), dtype=torch.float32, device=dev)
        self.raw = torch.empty((T, B, A), dtype=torch.float32, device=dev)
        self.logp = torch.zeros((T, B), dtype=torch.float32, device=dev)
        self.reward = torch.empty((T, B), dtype=torch.float32, device=dev)
        self.done = torch.empty((T, B), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with no_gc(), torch.cuda.graph(self.graph):
            for t in range(T):
                policy.act_into(self.state.obs, self.actions[t], self.logp[t], self.raw[t], None, self.obs[t])
                self.state = env.step_(self.state, self.actions[t])
                self.reward[t].copy_(self.state.reward)
                self.done[t].copy_(self.state.aux["done"] if "done" in self.state.aux else self.state.done)
                _record_truncation(self, t)
            if self.critic is not None:
                self.final_obs.copy_(self.state.obs)
            if self.update_normalizer:
                policy.normalizer.update(self.obs)
            _critic_pass(self)
        _release_deferred()

    def replay(self):
        """Run the captured unroll (stream-ordered on torch's current stream)."""
        self.graph.replay()
        return self.state


def _normalizer_to_update(policy, update_normalizer: bool, n_rows: int) -> bool:
    """The ``update_normalizer=`` guard of the actor rollouts; sizes the update's workspace
    before the capture."""
    if not update_normalizer:
        return False
    if getattr(policy, "normalizer", None) is None:
        raise ValueError("update_normalizer=True needs a policy constructed with normalizer=...")
    policy.normalizer.reserve(n_rows)
    return True


def _critic_buffers(roll, critic, gae, record_truncation: bool, state, T: int, B: int, D: int, dev,
                    recurrent: bool = False) -> torch.Tensor:
    """The ``critic=``, ``gae=``, ``record_truncation=`` arguments of the actor rollouts: checks
    them, allocates what they add to the trajectory and returns the (T, B, D) observation rows --
    with a critic the first T of a (T + 1, B, D) buffer whose last is ``roll.final_obs``.
    ``recurrent``: the rollout takes a ``RecurrentValueFunction`` too; it then gains the critic's
    (T + 1, B) reset rows (``roll._reset_rows``: row 0 the critic's, rows 1 .. T the trajectory's
    ``done``) and ``roll.value_hidden0``."""
    f = dict(dtype=torch.float32, device=dev)
    roll.critic = critic
    if critic is None and gae is not None:
        raise ValueError("gae= needs critic=")
    if critic is not None:
        from .training.gae import RecurrentValueFunction, ValueFunction, gae_options
        if recurrent:
            if not isinstance(critic, (ValueFunction, RecurrentValueFunction)):
                raise TypeError("critic must be a training.gae.ValueFunction or RecurrentValueFunction")
        elif not isinstance(critic, ValueFunction):
            raise TypeError("critic must be a training.gae.ValueFunction")
        if critic.obs_size != D:
            raise ValueError(f"the critic is for observations of width {critic.obs_size}, the rollout records {D}")
        if critic.theta.device != dev:
            raise ValueError(f"the critic is on {critic.theta.device}, the rollout on {dev}")
        if (T + 1) * B >= 2 ** 31:
            raise ValueError("the critic pass takes fewer than 2^31 observation rows")
        roll.gae = gae_options(gae)
    if critic is not None or record_truncation:
        roll._truncation_source = "truncation" in state.aux
        # an env without a time limit never truncates: zeros, set once
        roll.truncation = (torch.empty if roll._truncation_source else torch.zeros)((T, B), **f)
    if critic is None:
        return torch.empty((T, B, D), **f)
    roll._obs_buffer = torch.empty((T + 1, B, D), **f)
    roll.final_obs = roll._obs_buffer[T]
    roll.values = torch.empty((T + 1, B), **f)
    roll.vs = torch.empty((T, B), **f)
    roll.advantages = torch.empty((T, B), **f)
    if recurrent and isinstance(critic, RecurrentValueFunction):
        critic._buffers(B)  # hidden and reset exist before the capture
        roll._reset_rows = torch.empty((T + 1, B), **f)
        roll.value_hidden0 = torch.empty((B, critic.hidden_size), **f)
    return roll._obs_buffer[:T]


def _record_truncation(roll, t: int) -> None:
    """Step t's truncation row, from the engine's float32 buffer of the state just stepped."""
    if getattr(roll, "_truncation_source", False):
        roll.truncation[t].copy_(roll.state.aux["truncation"])


def _critic_pass(roll) -> None:
    """The graph's last nodes with a critic: the values of all (T + 1) B recorded rows in one
    launch, then ``pob_gae`` on the trajectory's ``done`` (done_input = 1)."""
    if roll.critic is None:
        return
    from . import _lib
    T, B = roll.steps, int(roll.values.shape[1])
    if getattr(roll, "_reset_rows", None) is not None:
        # The recurrent critic: the rows in time order in ONE launch, from the state the last replay's
        # T trajectory rows left (final_obs is the next replay's obs[0]: it must not advance the carry).
        critic = roll.critic
        roll._reset_rows[0].copy_(critic.reset)
        critic.values_sequence_into(roll._obs_buffer, roll._reset_rows, roll.values, roll.value_hidden0, carry_step=T)
        critic.reset.copy_(roll.done[T - 1])
    else:
        roll.critic.values_into(roll._obs_buffer.view((T + 1) * B, -1), roll.values.view(-1))
    o = roll.gae
    _lib.check(_lib.lib.pob_gae(T, B, _lib.ptr(roll.truncation), _lib.ptr(roll.done), 1, _lib.ptr(roll.reward),
                                o["reward_scaling"], _lib.ptr(roll.values), _lib.ptr(roll.values[T]), o["lambda_"],
                                o["discount"], _lib.ptr(roll.vs), _lib.ptr(roll.advantages),
                                _lib.stream_handle(roll.values.device)))


class RecurrentActorRollout:
    """``ActorRollout`` for a ``training.networks.RecurrentTanhPolicy``: ``T`` env-steps in ONE
    hipGraph, per step one ``pob_gru_policy_act`` launch (pre-MLP, GRU cell, post-MLP, head),
    the key advance, the fused step kernel and the reward / done copies.  The hidden state
    lives in ``policy.hidden`` and is carried in place; the kernel zeroes it where the last
    step ended an episode: at step t its ``reset`` input is ``done[t - 1]``, the trajectory
    row already on the device, and at t = 0 it is ``policy.reset``, into which the graph's last
    node copies ``done[T - 1]`` -- so state and episode boundaries carry across replays with
    no host work.

        roll = RecurrentActorRollout(env, state, policy, steps=T)
        roll.replay()
        roll.hidden[t]     # (B, H) the post-reset state step t started from (BPTT restarts here)
        roll.obs[t], roll.actions[t], roll.logp[t], roll.raw[t], roll.reward[t], roll.done[t]

    ``masked=True`` acts on ``state.info["obs_masked"]`` (the ``obs_mask=`` columns the step
    kernel writes) instead of ``state.obs``; ``roll.obs`` then holds those columns.
    Single-kind ``create(...)`` chains only.  ``update_normalizer=True``: as ``ActorRollout``
    (with ``masked=True`` the policy's normaliser is one over the masked columns).  ``critic=``,
    ``gae=``, ``record_truncation=``: as ``ActorRollout``; the critic is of the recorded observation's
    width (the masked columns' with ``masked=True``), a feed-forward ``ValueFunction`` or a
    ``training.gae.RecurrentValueFunction`` (DESIGN.md "Recurrent critic").  The recurrent one sees the
    (T + 1) B rows in time order, in ONE ``pob_gru_sequence_forward`` launch where the feed-forward
    launch sits: ``roll.values[t]`` is its value of ``obs[t]`` given everything it saw since the episode
    began, across replays (its reset rows are ``[critic.reset, done[0], .., done[T - 1]]``);
    ``roll.value_hidden0`` (B, H) is the post-reset state row 0 started from (the learner's BPTT restarts
    there); ``critic.hidden`` is left as the state after the T trajectory rows -- ``final_obs`` is the
    next replay's ``obs[0]`` and does not advance it -- and ``critic.reset`` as ``done[T - 1]``."""

    def __init__(self, env, state, policy, steps: int, masked: bool = False, update_normalizer: bool = False,
                 critic=None, gae=None, record_truncation: bool = False):
        from .training.networks import RecurrentTanhPolicy
        if steps <= 0:
            raise ValueError("steps must be positive")
        if not isinstance(policy, RecurrentTanhPolicy):
            raise TypeError("policy must be a training.networks.RecurrentTanhPolicy")
        if isinstance(state, (list, tuple)):
            raise NotImplementedError("RecurrentActorRollout unrolls a single-kind create(...) env, not a MixedEnv")
        if masked and "obs_masked" not in state.info:
            raise ValueError("masked=True needs an env created with obs_mask=...")
        self.masked = bool(masked)
        obs = self._obs_of(state)
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2):
            raise ValueError("the observation must be a float32 (B, D) device tensor")
        B, D = int(obs.shape[0]), int(obs.shape[1])
        A, H = env.action_size, policy.hidden_size
        if policy.action_size != A or policy.obs_size != D:
            raise ValueError(f"the policy maps {policy.obs_size} -> {policy.action_size}, the env {D} -> {A}")
        self.env, self.state, self.policy, self.steps = env, state, policy, int(steps)
        dev, T = obs.device, self.steps
        policy._buffers(B)  # hidden and reset exist before the capture
        self.update_normalizer = _normalizer_to_update(policy, update_normalizer, T * B)
        self.obs = _critic_buffers(self, critic, gae, record_truncation, state, T, B, D, dev, recurrent=True)
        self.actions = torch.empty((T, B, A), dtype=torch.float32, device=dev)
        self.raw = torch.empty((T, B, A), dtype=torch.float32, device=dev)
        self.logp = torch.zeros((T, B), dtype=torch.float32, device=dev)
        self.hidden = torch.empty((T, B, H), dtype=torch.float32, device=dev)
        self.reward = torch.empty((T, B), dtype=torch.float32, device=dev)
        # under a recurrent critic done is rows 1 .. T of its reset rows: no copy of the trajectory's done
        rows = getattr(self, "_reset_rows", None)
        self.done = torch.empty((T, B), dtype=torch.float32, device=dev) if rows is None else rows[1:]
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with no_gc(), torch.cuda.graph(self.graph):
            for t in range(T):
                policy.act_into(self._obs_of(self.state), self.actions[t], self.logp[t], self.raw[t], None, self.obs[t],
                                self.hidden[t], policy.reset if t == 0 else self.done[t - 1])
                self.state = env.step_(self.state, self.actions[t])
                self.reward[t].copy_(self.state.reward)
                self.done[t].copy_(self.state.aux["done"] if "done" in self.state.aux else self.state.done)
                _record_truncation(self, t)
            policy.reset.copy_(self.done[T - 1])
            if self.critic is not None:
                self.final_obs.copy_(self._obs_of(self.state))
            if self.update_normalizer:
                policy.normalizer.update(self.obs)
            _critic_pass(self)
        _release_deferred()

    def _obs_of(self, state):
        return state.info["obs_masked"] if self.masked else state.obs

    def replay(self):
        """Run the captured unroll (stream-ordered on torch's current stream)."""
        self.graph.replay()
        return self.state
