"""The critic's side of a PPO unroll: generalised advantage estimation and the value network's
forward (brax v1 ``training/ppo.py``: ``compute_gae`` and the value ``apply`` of its loss, [ext]).

``compute_gae`` is brax's function with brax's argument and return order.  Contiguous float32
CUDA tensors take ONE ``pob_gae`` launch (one lane per env, t descending; ``gae_ref`` of
csrc/pob_mlp.h bit for bit); anything else takes the same formula in torch ops.  Neither output
carries a graph (brax stops the gradient on both).

``ValueFunction`` wraps a ``make_model`` network of last width 1 for the actor rollouts' critic
pass: ``values_into`` is one ``pob_mlp_forward_norm`` launch over (N, D) observation rows.
Formula, operation order and what is pinned: DESIGN.md "Critic pass and GAE".

``RecurrentValueFunction`` is the critic with a memory (DESIGN.md "Recurrent critic"): a
``make_recurrent_model`` network of last width 1 and its carried GRU state; ``values_sequence_into``
is one ``pob_gru_sequence_forward`` launch over (S, B, D) trajectory rows in time order.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import check, lib, ptr
from . import normalization as _normalization
from .networks import FeedForwardModel, Params, RecurrentModel, RecurrentParams


def _gae_torch(truncation, termination, rewards, values, bootstrap_value, lambda_, discount, reward_scaling, vs, adv):
    """The operation order of ``gae_ref`` in torch ops (products and sums rounded separately)."""
    T = values.shape[0]
    acc = torch.zeros_like(bootstrap_value)
    v_next = vs_next = bootstrap_value
    for t in range(T - 1, -1, -1):
        m = 1.0 - truncation[t]
        g = discount * (1.0 - termination[t])
        r = rewards[t] * reward_scaling
        v = values[t]
        delta = (r + g * v_next - v) * m
        adv[t] = (r + g * vs_next - v) * m
        acc = delta + ((g * m) * lambda_) * acc
        vs_next = acc + v
        vs[t] = vs_next
        v_next = v
    return vs, adv


def compute_gae(truncation: torch.Tensor, termination: torch.Tensor, rewards: torch.Tensor, values: torch.Tensor,
                bootstrap_value: torch.Tensor, lambda_: float = 0.95, discount: float = 0.99,
                reward_scaling: float = 1.0, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """brax's ``compute_gae``: ``(vs, advantages)``, both (T, B), from ``truncation``,
    ``termination``, ``rewards``, ``values`` (T, B) and ``bootstrap_value`` (B,), the value of the
    observation after the last step.  ``termination = done * (1 - truncation)`` in brax's data;
    ``rewards`` are multiplied by ``reward_scaling`` first.  ``out=(vs, advantages)`` writes into
    caller buffers (no allocation: capturable); the outputs must not overlap the inputs."""
    named = (("truncation", truncation), ("termination", termination), ("rewards", rewards), ("values", values),
             ("bootstrap_value", bootstrap_value))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    for name, t in named:
        if not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype}")
        if t.dtype != values.dtype or t.device != values.device:
            raise TypeError(f"{name} is {t.dtype} on {t.device}, values {values.dtype} on {values.device}")
    if values.dim() != 2 or values.shape[0] < 1 or values.shape[1] < 1:
        raise ValueError("values must be (T, B) with T >= 1 and B >= 1")
    T, B = int(values.shape[0]), int(values.shape[1])
    for name, t in named[:3]:
        if tuple(t.shape) != (T, B):
            raise ValueError(f"{name} must be ({T}, {B}) like values, got {tuple(t.shape)}")
    if tuple(bootstrap_value.shape) != (B,):
        raise ValueError(f"bootstrap_value must be ({B},), got {tuple(bootstrap_value.shape)}")
    ins = [t for _, t in named]
    if out is None:
        vs, adv = torch.empty_like(values, memory_format=torch.contiguous_format), torch.empty_like(
            values, memory_format=torch.contiguous_format)
    else:
        vs, adv = out
        for name, t in (("out[0]", vs), ("out[1]", adv)):
            if not (isinstance(t, torch.Tensor) and tuple(t.shape) == (T, B) and t.dtype == values.dtype
                    and t.device == values.device and t.is_contiguous() and not t.requires_grad):
                raise ValueError(f"{name} must be a contiguous {values.dtype} tensor ({T}, {B}) on {values.device}")
    fused = (values.is_cuda and values.dtype == torch.float32 and all(t.is_contiguous() for t in ins)
             and not any(t.requires_grad for t in ins))
    if fused:
        check(lib.pob_gae(T, B, ptr(truncation), ptr(termination), 0, ptr(rewards), float(reward_scaling),
                          ptr(values), ptr(bootstrap_value), float(lambda_), float(discount), ptr(vs), ptr(adv),
                          _lib.stream_handle(values.device)))
        return vs, adv
    with torch.no_grad():
        d = [t.detach() for t in ins]
        return _gae_torch(d[0], d[1], d[2], d[3], d[4], float(lambda_), float(discount), float(reward_scaling), vs, adv)


GAE_DEFAULTS = {"lambda_": 0.95, "discount": 0.99, "reward_scaling": 1.0}


def gae_options(gae: Optional[dict]) -> dict:
    """The actor rollouts' ``gae=`` argument over the defaults of ``compute_gae``."""
    opts = dict(GAE_DEFAULTS)
    if gae is not None:
        unknown = sorted(set(gae) - set(opts))
        if unknown:
            raise ValueError(f"gae= takes {sorted(opts)}, got {unknown}")
        opts.update({k: float(v) for k, v in gae.items()})
    return opts


class ValueFunction:
    """The critic of an actor rollout: a ``make_model`` network whose last width is 1 (the value
    half of ``make_models``).  ``values_into(obs_rows, out)`` is ONE ``pob_mlp_forward_norm``
    launch over (N, D) rows into an (N,) buffer: no allocation, no host sync, capture-safe.
    ``params.theta`` is read in place at launch time, so an optimiser step between replays is seen
    by a captured graph; so is the table of ``normalizer`` (a
    ``normalization.ObservationNormalizer`` of width ``obs_size``; the policy's, usually)."""

    def __init__(self, model: FeedForwardModel, params: Params, normalizer=None):
        if model.mlp is None or model.layer_sizes is None:
            raise ValueError("model must come from make_model")
        if model.layer_sizes[-1] != 1:
            raise ValueError(f"the value network's last width must be 1, got {model.layer_sizes[-1]}")
        theta = params.theta
        self.obs_size = model.layer_sizes[0]
        self.normalizer = _normalization.attach(normalizer, self.obs_size, theta.device)
        if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous()):
            raise ValueError("params.theta must be a contiguous float32 CUDA tensor (params.to('cuda'))")
        if theta.numel() != model.mlp.param_count:
            raise ValueError(f"theta has {theta.numel()} elements, the network {model.mlp.param_count}")
        self.model, self.params, self.theta = model, params, theta

    def values_into(self, obs_rows: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """``out`` (N,) <- the value of every row of ``obs_rows`` (N, D); both contiguous float32
        tensors on the parameters' device."""
        dev = self.theta.device
        if not (obs_rows.is_cuda and obs_rows.dtype == torch.float32 and obs_rows.dim() == 2
                and obs_rows.shape[1] == self.obs_size and obs_rows.is_contiguous() and obs_rows.device == dev):
            raise ValueError(f"obs_rows must be a contiguous float32 tensor (N, {self.obs_size}) on {dev}")
        N = int(obs_rows.shape[0])
        if not 1 <= N < 2 ** 31:
            raise ValueError("obs_rows must have 1 .. 2^31 - 1 rows")
        if not (tuple(out.shape) == (N,) and out.dtype == torch.float32 and out.is_contiguous() and out.device == dev):
            raise ValueError(f"out must be a contiguous float32 tensor ({N},) on {dev}")
        norm = self.normalizer
        check(lib.pob_mlp_forward_norm(self.model.mlp.handle, N, ptr(obs_rows), ptr(self.theta), ptr(out),
                                       None if norm is None else ptr(norm.table), 0.0 if norm is None else norm.clip,
                                       _lib.stream_handle(dev)))
        return out

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        """The values of ``obs`` (..., D) as a new (...) tensor."""
        rows = obs.detach().reshape(-1, self.obs_size).contiguous()
        out = torch.empty((rows.shape[0],), dtype=torch.float32, device=rows.device)
        return self.values_into(rows, out).reshape(obs.shape[:-1])


class RecurrentValueFunction:
    """The critic of a ``RecurrentActorRollout`` that remembers: a ``make_recurrent_model`` network whose
    last post-MLP width is 1.  It owns ``hidden`` (B, H), the GRU state carried from call to call, and
    ``reset`` (B,): where it is non-zero the env's next window starts from h = 0.  Both are allocated at
    first use and start as zeros (``RecurrentTanhPolicy``'s rule); after that no allocation and no host
    sync: capture-safe.  ``params.theta`` and the table of ``normalizer`` are read at launch time, as
    ``ValueFunction``'s."""

    def __init__(self, model: RecurrentModel, params: RecurrentParams, normalizer=None):
        if getattr(model, "gru", None) is None or getattr(model, "post_sizes", None) is None:
            raise ValueError("model must come from make_recurrent_model")
        if model.post_sizes[-1] != 1:
            raise ValueError(f"the value network's last width must be 1, got {model.post_sizes[-1]}")
        theta = params.theta
        self.obs_size, self.hidden_size = model.pre_sizes[0], model.hidden_size
        self.normalizer = _normalization.attach(normalizer, self.obs_size, theta.device)
        if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous()):
            raise ValueError("params.theta must be a contiguous float32 CUDA tensor (params.to('cuda'))")
        if theta.numel() != model.gru.param_count:
            raise ValueError(f"theta has {theta.numel()} elements, the network {model.gru.param_count}")
        self.model, self.params, self.theta = model, params, theta
        self.hidden = self.reset = None

    def _buffers(self, B: int):
        if self.hidden is None or self.hidden.shape[0] != B:
            dev = self.theta.device
            self.hidden = torch.zeros((B, self.hidden_size), dtype=torch.float32, device=dev)
            self.reset = torch.zeros((B,), dtype=torch.float32, device=dev)

    def values_sequence_into(self, obs: torch.Tensor, reset: torch.Tensor, values: torch.Tensor,
                             h_first: Optional[torch.Tensor] = None, carry_step: Optional[int] = None) -> torch.Tensor:
        """``values`` (S, B) <- the value of every row of ``obs`` (S, B, D) in time order, env b starting
        from ``self.hidden[b]`` and from h = 0 at every step s with ``reset[s][b] != 0`` (reset (S, B)):
        ONE ``pob_gru_sequence_forward`` launch.  ``h_first`` (B, H) receives the state row 0 started from,
        after ``reset[0]``; ``self.hidden`` is overwritten in place with the state after ``carry_step``
        steps (1 .. S; None: S).  All contiguous float32 tensors on the parameters' device."""
        dev, D, H = self.theta.device, self.obs_size, self.hidden_size

        def ok(t, shape):
            return (isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == torch.float32
                    and t.is_contiguous() and t.device == dev)

        if not (isinstance(obs, torch.Tensor) and obs.dim() == 3 and obs.shape[0] >= 1 and obs.shape[1] >= 1
                and ok(obs, (obs.shape[0], obs.shape[1], D))):
            raise ValueError(f"obs must be a contiguous float32 tensor (S, B, {D}) on {dev}")
        S, B = int(obs.shape[0]), int(obs.shape[1])
        for name, t, shape in (("reset", reset, (S, B)), ("values", values, (S, B)), ("h_first", h_first, (B, H))):
            if not (ok(t, shape) or (name == "h_first" and t is None)):
                raise ValueError(f"{name} must be a contiguous float32 tensor {shape} on {dev}")
        step = S if carry_step is None else int(carry_step)
        if not 1 <= step <= S:
            raise ValueError(f"carry_step must be in 1 .. {S}, got {carry_step}")
        self._buffers(B)
        norm = self.normalizer
        check(lib.pob_gru_sequence_forward(self.model.gru.handle, S, B, B, ptr(obs), None, ptr(self.hidden), ptr(reset),
                                           ptr(self.theta), ptr(values), ptr(h_first), ptr(self.hidden), step,
                                           None if norm is None else ptr(norm.table), 0.0 if norm is None else norm.clip,
                                           _lib.stream_handle(dev)))
        return values
