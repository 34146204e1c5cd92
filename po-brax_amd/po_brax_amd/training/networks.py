"""Policy / value networks (po_brax/training/networks.py: MLP, make_model, make_models).

The reference builds flax MLPs for the learner.  Here a model is a pair ``(init, apply)`` over
ONE flat float32 parameter vector ``theta`` (W_0, b_0, W_1, b_1, ..; W_i row-major (in, out),
flax ``Dense.kernel``'s layout), of which the ``{"hidden_i": {"kernel", "bias"}}`` mapping holds
views.  ``apply`` runs the fused HIP kernel (``pob_mlp_forward``: every layer in one launch on
the f32 matrix cores) when ``x`` is a CUDA float32 tensor and no gradient is required, and the
same network in plain torch ops otherwise (autograd for the learner, and the CPU).
``model.apply_native`` is ``apply`` whose backward pass runs in the engine too
(``pob_mlp_forward_train`` / ``pob_mlp_backward``: DESIGN.md "MLP backward").
``NormalTanhPolicy`` is the actor: forward + brax's tanh-normal head in one launch
(``pob_policy_act``), capture-safe, so it drops into ``rollout.PolicyRollout`` and is what
``rollout.ActorRollout`` unrolls.  Formulas, layouts and what is pinned: DESIGN.md "Policy
networks".

``make_recurrent_model`` / ``RecurrentTanhPolicy`` are the recurrent counterparts (pre-MLP ->
GRU cell -> post-MLP, ``pob_gru_forward`` / ``pob_gru_policy_act``, the hidden state carried on
the device), unrolled by ``rollout.RecurrentActorRollout``: DESIGN.md "Recurrent actor".
``model.apply_sequence`` runs a window of T steps in torch ops and ``model.apply_sequence_native`` in
the engine, forward and truncated-BPTT backward (``pob_gru_sequence_forward_train`` /
``pob_gru_sequence_backward``): DESIGN.md "Recurrent backward".

Both policies take ``normalizer=`` (``normalization.ObservationNormalizer``): the running
observation normaliser applied inside the actor kernel's tile load (``pob_*_policy_act_norm``):
DESIGN.md "Observation normaliser".
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Any, Callable, Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import check, lib, ptr
from . import normalization as _normalization

ACTIVATIONS = {"relu": 0, "swish": 1, "silu": 1, "tanh": 2}
_TORCH_ACT = {0: torch.relu, 1: torch.nn.functional.silu, 2: torch.tanh}
MAX_LAYERS, MAX_WIDTH = 8, 256


def _activation_id(activation) -> int:
    if isinstance(activation, str):
        name = activation
    else:
        name = getattr(activation, "__name__", str(activation))
    if name not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}, got {activation!r}")
    return ACTIVATIONS[name]


class MLPHandle:
    """A ``pob_mlp`` (shape and activation only: host memory, no HIP call to make or free)."""

    def __init__(self, sizes: Sequence[int], activation: int, activate_final: bool = False):
        self.sizes = [int(s) for s in sizes]
        arr = (C.c_int * len(self.sizes))(*self.sizes)
        h = C.c_void_p()
        check(lib.pob_mlp_create(len(self.sizes) - 1, arr, int(activation), int(bool(activate_final)), C.byref(h)))
        self._h = h
        n = C.c_longlong()
        check(lib.pob_mlp_param_count(h, C.byref(n)))
        self.param_count = int(n.value)

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.pob_mlp_destroy(h)


class Params(dict):
    """``{"hidden_i": {"kernel": (in, out), "bias": (out,)}}`` whose tensors are views into the
    flat ``theta`` (an in-place update of either is seen by the other, and by a captured graph)."""

    def __init__(self, theta: torch.Tensor, sizes: Sequence[int]):
        super().__init__()
        self.theta, self.sizes = theta, list(sizes)
        off = 0
        for i, (n_in, n_out) in enumerate(zip(sizes[:-1], sizes[1:])):
            kernel = theta[off:off + n_in * n_out].view(n_in, n_out)
            off += n_in * n_out
            self[f"hidden_{i}"] = {"kernel": kernel, "bias": theta[off:off + n_out]}
            off += n_out
        if off != theta.numel():
            raise ValueError(f"theta has {theta.numel()} elements, the network {off}")

    def to(self, device) -> "Params":
        return Params(self.theta.detach().to(device).contiguous(), self.sizes)


# ---- jax.random threefry2x32 on the host (the same scheme as the device's, csrc/pob_math.h),
# so that init() gives the same parameters from the same key with or without a GPU
_M32 = 0xFFFFFFFF


def _threefry(k0: int, k1: int, x0: torch.Tensor, x1: torch.Tensor):
    ks = (k0, k1, k0 ^ k1 ^ 0x1BD11BDA)
    rot = ((13, 15, 26, 6), (17, 29, 16, 24))
    a, b = (x0 + ks[0]) & _M32, (x1 + ks[1]) & _M32
    for i in range(5):
        for r in rot[i % 2]:
            a = (a + b) & _M32
            b = ((b << r) | (b >> (32 - r))) & _M32
            b = b ^ a
        a = (a + ks[(i + 1) % 3]) & _M32
        b = (b + ks[(i + 2) % 3] + i + 1) & _M32
    return a, b


def _host_bits(key, n: int) -> torch.Tensor:
    """threefry_2x32(key, iota(n)) as int64 values below 2^32 (odd n padded with a zero count)."""
    k0, k1 = int(key[0]), int(key[1])
    h = (n + 1) // 2
    x = torch.arange(2 * h, dtype=torch.int64)
    x[n:] = 0
    a, b = _threefry(k0, k1, x[:h], x[h:])
    return torch.cat([a, b])[:n]


def _host_split(key, num: int = 2) -> torch.Tensor:
    return _host_bits(key, 2 * num).reshape(num, 2)


def _host_uniform(key, n: int, lo: float, hi: float) -> torch.Tensor:
    bits = _host_bits(key, n)
    f = (((bits >> 9) | 0x3F800000).to(torch.int32).view(torch.float32)) - 1.0
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    v = f * (hi_t - lo_t) + lo_t
    return torch.maximum(v, lo_t)


def _key_words(key) -> torch.Tensor:
    key = torch.as_tensor(key)
    if key.dtype != torch.uint32 or key.numel() != 2:
        raise TypeError("key must be a torch.uint32 tensor of 2 words (jumpy.random_prngkey)")
    return key.reshape(2)


@dataclasses.dataclass
class FeedForwardModel:
    init: Any
    apply: Any
    layer_sizes: Optional[Tuple[int, ...]] = None  # (obs_size, *layer_sizes)
    activation: Optional[int] = None               # 0 relu, 1 swish, 2 tanh
    mlp: Optional[MLPHandle] = None
    apply_native: Any = None                       # apply whose backward pass is the engine's too


def _forward_torch(sizes, act: int, theta_or_params, x: torch.Tensor) -> torch.Tensor:
    theta = getattr(theta_or_params, "theta", None)
    h, off = x, 0
    n = len(sizes) - 1
    for i, (n_in, n_out) in enumerate(zip(sizes[:-1], sizes[1:])):
        if theta is not None:  # slice at call time: a view made before requires_grad_() is not tracked
            W = theta[off:off + n_in * n_out].view(n_in, n_out)
            off += n_in * n_out
            b = theta[off:off + n_out]
            off += n_out
        else:
            W, b = theta_or_params[f"hidden_{i}"]["kernel"], theta_or_params[f"hidden_{i}"]["bias"]
        h = torch.addmm(b, h.reshape(-1, n_in), W).reshape(*h.shape[:-1], n_out)
        if i != n - 1:
            h = _TORCH_ACT[act](h)
    return h


def make_model(layer_sizes: Sequence[int], obs_size: int, activation: Any = "swish",
               spectral_norm: bool = False) -> FeedForwardModel:
    """An MLP ``obs_size -> layer_sizes[0] -> .. -> layer_sizes[-1]`` with ``activation`` after
    every layer but the last.  ``model.init(key)`` returns ``Params`` (on the key's device):
    kernels lecun-uniform U(-sqrt(3 / in), sqrt(3 / in)) drawn through the jumpy uniform, one
    ``key, sub = split(key)`` per layer; biases zero.  ``model.apply(params, x)``: x (..., obs_size)
    -> (..., layer_sizes[-1])."""
    if spectral_norm:
        raise NotImplementedError("spectral_norm: brax's SNDense is not part of this engine (DESIGN.md "
                                  "\"Policy networks\")")
    sizes = (int(obs_size),) + tuple(int(s) for s in layer_sizes)
    act = _activation_id(activation)
    mlp = MLPHandle(sizes, act, False)  # ValueError for widths outside 1 .. 256 or more than 8 layers

    def init(key) -> Params:
        key = _key_words(key)
        dev = key.device
        parts = []
        for n_in, n_out in zip(sizes[:-1], sizes[1:]):
            lim = math.sqrt(3.0 / n_in)
            if dev.type == "cuda":
                from .. import jumpy
                key, sub = jumpy.random_split(key)
                w = jumpy.random_uniform(sub, (n_in * n_out,), -lim, lim)
            else:
                key, sub = _host_split(key)
                w = _host_uniform(sub, n_in * n_out, -lim, lim)
            parts += [w, torch.zeros(n_out, dtype=torch.float32, device=dev)]
        return Params(torch.cat(parts).contiguous(), sizes)

    def apply(params, x: torch.Tensor) -> torch.Tensor:
        theta = getattr(params, "theta", None)
        need_grad = torch.is_grad_enabled() and (x.requires_grad or (
            theta.requires_grad if theta is not None else any(t.requires_grad for p in params.values() for t in p.values())))
        fused = (theta is not None and x.is_cuda and x.dtype == torch.float32 and theta.is_cuda
                 and theta.dtype == torch.float32 and theta.is_contiguous() and not need_grad)
        if not fused:
            return _forward_torch(sizes, act, params, x)
        if theta.numel() != mlp.param_count:
            raise ValueError(f"theta has {theta.numel()} elements, the network {mlp.param_count}")
        if x.shape[-1] != sizes[0]:
            raise ValueError(f"x must be (..., {sizes[0]})")
        x2 = x.detach().reshape(-1, sizes[0]).contiguous()
        y = torch.empty((x2.shape[0], sizes[-1]), dtype=torch.float32, device=x.device)
        if x2.shape[0]:
            check(lib.pob_mlp_forward(mlp.handle, x2.shape[0], ptr(x2), ptr(theta.detach()), ptr(y),
                                      _lib.stream_handle(x.device)))
        return y.reshape(*x.shape[:-1], sizes[-1])

    class _NativeMLP(torch.autograd.Function):
        """theta (contiguous float32 CUDA), x2 (M, sizes[0]) contiguous float32 CUDA, M >= 1."""

        @staticmethod
        def forward(ctx, theta, x2):
            M, dev = int(x2.shape[0]), x2.device
            need = C.c_longlong()
            check(lib.pob_mlp_saved_bytes(mlp.handle, M, C.byref(need)))
            saved = torch.empty(need.value // 4, dtype=torch.float32, device=dev)
            y = torch.empty((M, sizes[-1]), dtype=torch.float32, device=dev)
            check(lib.pob_mlp_forward_train(mlp.handle, M, ptr(x2), ptr(theta), ptr(y), ptr(saved),
                                            _lib.stream_handle(dev)))
            ctx.save_for_backward(theta, x2, saved)
            return y

        @staticmethod
        @torch.autograd.function.once_differentiable  # the kernels are invisible to autograd: no double backward
        def backward(ctx, dy):
            theta, x2, saved = ctx.saved_tensors
            M, dev = int(x2.shape[0]), x2.device
            dy = dy.contiguous()
            need = C.c_longlong()
            check(lib.pob_mlp_backward_workspace_bytes(mlp.handle, M, C.byref(need)))
            workspace = torch.empty(need.value // 8, dtype=torch.float64, device=dev)
            dtheta = torch.empty_like(theta)
            dx = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
            check(lib.pob_mlp_backward(mlp.handle, M, ptr(x2), ptr(theta), ptr(saved), ptr(dy), ptr(dtheta), ptr(dx),
                                       ptr(workspace), _lib.stream_handle(dev)))
            return (dtheta if ctx.needs_input_grad[0] else None), dx

    def apply_native(params, x: torch.Tensor) -> torch.Tensor:
        """``apply`` whose backward pass runs in the engine as well: for a ``Params`` (or a namespace
        with ``.theta``) whose ``theta`` is a contiguous float32 CUDA tensor and a float32 CUDA ``x``,
        the forward is ``pob_mlp_forward_train`` (``apply``'s fused bits, the pre-activations kept)
        and the backward ``pob_mlp_backward`` (``theta.grad``, and ``x.grad`` only when ``x`` requires
        it).  Anything else (the CPU, other dtypes, the dict-of-views form) takes the torch ops under
        autograd; when no gradient is needed this is ``apply``."""
        theta = getattr(params, "theta", None)
        need_grad = torch.is_grad_enabled() and (x.requires_grad or (
            theta.requires_grad if theta is not None else any(t.requires_grad for p in params.values() for t in p.values())))
        if not need_grad:
            return apply(params, x)
        native = (theta is not None and x.is_cuda and x.dtype == torch.float32 and theta.is_cuda
                  and theta.dtype == torch.float32 and theta.is_contiguous() and x.numel() > 0)
        if not native:
            return _forward_torch(sizes, act, params, x)
        if theta.numel() != mlp.param_count:
            raise ValueError(f"theta has {theta.numel()} elements, the network {mlp.param_count}")
        if x.shape[-1] != sizes[0]:
            raise ValueError(f"x must be (..., {sizes[0]})")
        y = _NativeMLP.apply(theta, x.reshape(-1, sizes[0]).contiguous())
        return y.reshape(*x.shape[:-1], sizes[-1])

    return FeedForwardModel(init=init, apply=apply, layer_sizes=sizes, activation=act, mlp=mlp,
                            apply_native=apply_native)


def make_models(policy_params_size: int, obs_size: int) -> Tuple[FeedForwardModel, FeedForwardModel]:
    """The reference's PPO pair: policy [32] * 4 + [policy_params_size], value [256] * 5 + [1]."""
    return (make_model([32, 32, 32, 32, policy_params_size], obs_size),
            make_model([256, 256, 256, 256, 256, 1], obs_size))


# ---- the recurrent actor (DESIGN.md "Recurrent actor"): pre-MLP -> GRU cell -> post-MLP
MAX_HIDDEN, MAX_PRE, MAX_POST = 128, 3, 4


class GRUHandle:
    """A ``pob_gru`` (shape and activation only: host memory, no HIP call to make or free)."""

    def __init__(self, pre_sizes: Sequence[int], hidden: int, post_sizes: Sequence[int], activation: int):
        self.pre_sizes = [int(s) for s in pre_sizes]  # [obs width, *pre-MLP widths]
        self.post_sizes = [int(s) for s in post_sizes]
        self.hidden = int(hidden)
        if not self.pre_sizes:
            raise ValueError("gru: pre_sizes must start with the observation width")
        pre = (C.c_int * len(self.pre_sizes))(*self.pre_sizes)
        post = (C.c_int * max(1, len(self.post_sizes)))(*self.post_sizes)
        h = C.c_void_p()
        check(lib.pob_gru_create(len(self.pre_sizes) - 1, pre, self.hidden, len(self.post_sizes), post, int(activation),
                                 C.byref(h)))
        self._h = h
        n = C.c_longlong()
        check(lib.pob_gru_param_count(h, C.byref(n)))
        self.param_count = int(n.value)

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.pob_gru_destroy(h)


def _gru_layout(pre_sizes, hidden, post_sizes):
    """``[(path, n_in, n_out)]`` of the weight matrices in ``theta`` order (each followed by its
    bias of n_out entries); path = ("pre_i",), ("gru", "rz" | "xn" | "hn") or ("post_i",)."""
    I, H = pre_sizes[-1], hidden
    out = [((f"pre_{i}",), a, b) for i, (a, b) in enumerate(zip(pre_sizes[:-1], pre_sizes[1:]))]
    out += [(("gru", "rz"), I + H, 2 * H), (("gru", "xn"), I, H), (("gru", "hn"), H, H)]
    widths = [H] + list(post_sizes)
    out += [((f"post_{i}",), a, b) for i, (a, b) in enumerate(zip(widths[:-1], widths[1:]))]
    return out


class RecurrentParams(dict):
    """``{"pre_i": {kernel, bias}, "gru": {"rz" | "xn" | "hn": {kernel, bias}}, "post_i": {kernel,
    bias}}`` whose tensors are views into the flat ``theta``."""

    def __init__(self, theta: torch.Tensor, pre_sizes, hidden, post_sizes):
        super().__init__()
        self.theta = theta
        self.pre_sizes, self.hidden, self.post_sizes = list(pre_sizes), int(hidden), list(post_sizes)
        off = 0
        for path, n_in, n_out in _gru_layout(self.pre_sizes, self.hidden, self.post_sizes):
            kernel = theta[off:off + n_in * n_out].view(n_in, n_out)
            off += n_in * n_out
            leaf = {"kernel": kernel, "bias": theta[off:off + n_out]}
            off += n_out
            if len(path) == 1:
                self[path[0]] = leaf
            else:
                self.setdefault(path[0], {})[path[1]] = leaf
        if off != theta.numel():
            raise ValueError(f"theta has {theta.numel()} elements, the network {off}")

    def to(self, device) -> "RecurrentParams":
        return RecurrentParams(self.theta.detach().to(device).contiguous(), self.pre_sizes, self.hidden, self.post_sizes)


@dataclasses.dataclass
class RecurrentModel:
    init: Any
    apply: Any
    initial_state: Any
    pre_sizes: Optional[Tuple[int, ...]] = None   # (obs_size, *pre_sizes)
    hidden_size: Optional[int] = None
    post_sizes: Optional[Tuple[int, ...]] = None
    activation: Optional[int] = None
    gru: Optional[GRUHandle] = None
    apply_sequence: Any = None          # a window of T steps in torch ops (autograd, any dtype and device)
    apply_sequence_native: Any = None   # the same window in the engine, forward and backward


def _recurrent_torch(pre, H, post, act, theta, x, h, reset):
    """The recurrent network in torch ops on 2-D x (B, D), h (B, H)."""
    fn, off = _TORCH_ACT[act], 0

    def dense(v, n_in, n_out):
        nonlocal off
        W = theta[off:off + n_in * n_out].view(n_in, n_out)
        off += n_in * n_out
        b = theta[off:off + n_out]
        off += n_out
        return torch.addmm(b, v, W)

    for n_in, n_out in zip(pre[:-1], pre[1:]):
        x = fn(dense(x, n_in, n_out))
    I = pre[-1]
    if reset is not None:
        h = torch.where(reset.reshape(-1, 1) != 0, torch.zeros_like(h), h)
    rz = torch.sigmoid(dense(torch.cat([x, h], dim=-1), I + H, 2 * H))
    r, z = rz[:, :H], rz[:, H:]
    cx = dense(x, I, H)
    ch = dense(h, H, H)
    n = torch.tanh(cx + r * ch)
    h_new = n + z * (h - n)
    y, widths = h_new, [H] + list(post)
    for i, (n_in, n_out) in enumerate(zip(widths[:-1], widths[1:])):
        y = dense(y, n_in, n_out)
        if i != len(post) - 1:
            y = fn(y)
    return y, h_new


def make_recurrent_model(pre_sizes: Sequence[int], hidden_size: int, post_sizes: Sequence[int], obs_size: int,
                         activation: Any = "swish") -> RecurrentModel:
    """``obs_size -> pre_sizes (activation after every layer) -> GRU cell (hidden_size) ->
    post_sizes (activation after all but the last)``.  ``model.init(key)`` returns
    ``RecurrentParams``: one ``key, sub = split(key)`` per weight matrix in ``theta`` order (the
    pre-MLP's, W_rz, W_xn, W_hn, the post-MLP's), each lecun-uniform on its ``in``, biases zero.
    ``model.apply(params, x, h, reset=None) -> (y, h_new)``: x (B, obs_size), h (B, hidden_size),
    reset (B,) (non-zero: the env starts from h = 0).  ``model.initial_state(B, device)``: zeros."""
    pre = (int(obs_size),) + tuple(int(s) for s in pre_sizes)
    post = tuple(int(s) for s in post_sizes)
    H = int(hidden_size)
    act = _activation_id(activation)
    gru = GRUHandle(pre, H, post, act)  # ValueError names the limit that is exceeded
    layout = _gru_layout(pre, H, post)

    def init(key) -> RecurrentParams:
        key = _key_words(key)
        dev = key.device
        parts = []
        for _, n_in, n_out in layout:
            lim = math.sqrt(3.0 / n_in)
            if dev.type == "cuda":
                from .. import jumpy
                key, sub = jumpy.random_split(key)
                w = jumpy.random_uniform(sub, (n_in * n_out,), -lim, lim)
            else:
                key, sub = _host_split(key)
                w = _host_uniform(sub, n_in * n_out, -lim, lim)
            parts += [w, torch.zeros(n_out, dtype=torch.float32, device=dev)]
        return RecurrentParams(torch.cat(parts).contiguous(), pre, H, post)

    def initial_state(B: int, device=None) -> torch.Tensor:
        return torch.zeros((int(B), H), dtype=torch.float32, device=device)

    def apply(params, x: torch.Tensor, h: torch.Tensor, reset: Optional[torch.Tensor] = None):
        theta = params.theta
        if theta.numel() != gru.param_count:
            raise ValueError(f"theta has {theta.numel()} elements, the network {gru.param_count}")
        if x.dim() != 2 or x.shape[1] != pre[0] or tuple(h.shape) != (x.shape[0], H):
            raise ValueError(f"x must be (B, {pre[0]}) and h (B, {H})")
        if reset is not None and tuple(reset.shape) != (x.shape[0],):
            raise ValueError("reset must be (B,)")
        need_grad = torch.is_grad_enabled() and (x.requires_grad or h.requires_grad or theta.requires_grad)
        fused = (x.is_cuda and x.dtype == torch.float32 and theta.is_cuda and theta.dtype == torch.float32
                 and theta.is_contiguous() and h.is_cuda and h.dtype == torch.float32 and not need_grad)
        if not fused:
            return _recurrent_torch(pre, H, post, act, theta, x, h, reset)
        x2 = x.detach().contiguous()
        h_new = h.detach().clone(memory_format=torch.contiguous_format)
        rs = None if reset is None else reset.detach().to(torch.float32).contiguous()
        y = torch.empty((x2.shape[0], post[-1]), dtype=torch.float32, device=x.device)
        if x2.shape[0]:
            check(lib.pob_gru_forward(gru.handle, x2.shape[0], ptr(x2), ptr(theta.detach()), ptr(rs), ptr(h_new), ptr(y),
                                      None, _lib.stream_handle(x.device)))
        return y, h_new

    def _check_theta(theta):
        if theta.numel() != gru.param_count:
            raise ValueError(f"theta has {theta.numel()} elements, the network {gru.param_count}")

    def apply_sequence(params, x: torch.Tensor, h0: torch.Tensor, reset: Optional[torch.Tensor] = None):
        """A window of T steps in torch ops: x (T, M, obs_size), h0 (M, hidden_size), reset (T, M)
        (non-zero: sequence m starts step t from h = 0) -> ``(y (T, M, post_sizes[-1]), h_last)``.
        Any dtype and device; differentiable by autograd in ``theta``, ``x`` and ``h0``."""
        theta = params.theta
        _check_theta(theta)
        if x.dim() != 3 or x.shape[2] != pre[0] or x.shape[0] < 1:
            raise ValueError(f"x must be (T, M, {pre[0]}) with T >= 1")
        T, M = int(x.shape[0]), int(x.shape[1])
        if tuple(h0.shape) != (M, H):
            raise ValueError(f"h0 must be ({M}, {H})")
        if reset is not None and tuple(reset.shape) != (T, M):
            raise ValueError(f"reset must be ({T}, {M})")
        h, ys = h0, []
        for t in range(T):
            y, h = _recurrent_torch(pre, H, post, act, theta, x[t], h, None if reset is None else reset[t])
            ys.append(y)
        return torch.stack(ys), h

    class _NativeSequence(torch.autograd.Function):
        """theta, obs (T, B, D), h0 (B, H) contiguous float32 CUDA; reset (T, B) float32 or None;
        idx (M,) int32 or None; table (3, D) or None."""

        @staticmethod
        def forward(ctx, theta, obs, h0, reset, idx, table, clip):
            T, B, dev = int(obs.shape[0]), int(obs.shape[1]), obs.device
            M = B if idx is None else int(idx.shape[0])
            need = C.c_longlong()
            check(lib.pob_gru_sequence_saved_bytes(gru.handle, T, M, C.byref(need)))
            saved = torch.empty(need.value // 4, dtype=torch.float32, device=dev)
            y = torch.empty((T, M, post[-1]), dtype=torch.float32, device=dev)
            h_last = torch.empty((M, H), dtype=torch.float32, device=dev)
            check(lib.pob_gru_sequence_forward_train(gru.handle, T, M, B, ptr(obs), ptr(idx), ptr(h0), ptr(reset), ptr(theta),
                                                     ptr(y), ptr(h_last), ptr(saved), ptr(table), float(clip),
                                                     _lib.stream_handle(dev)))
            ctx.save_for_backward(theta, saved, reset, idx)
            ctx.dims = (T, M, B)
            return y, h_last

        @staticmethod
        @torch.autograd.function.once_differentiable  # the kernels are invisible to autograd: no double backward
        def backward(ctx, dy, dh_last):
            theta, saved, reset, idx = ctx.saved_tensors
            T, M, B = ctx.dims
            dev = theta.device
            need = C.c_longlong()
            check(lib.pob_gru_sequence_backward_workspace_bytes(gru.handle, T, M, C.byref(need)))
            workspace = torch.empty(need.value // 8, dtype=torch.float64, device=dev)
            dtheta = torch.empty_like(theta)
            dh0_m = torch.empty((M, H), dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
            dy = dy.contiguous()
            dh_last = None if dh_last is None else dh_last.contiguous()
            check(lib.pob_gru_sequence_backward(gru.handle, T, M, B, ptr(idx), ptr(reset), ptr(theta), ptr(saved), ptr(dy),
                                                ptr(dh_last), ptr(dtheta), ptr(dh0_m), ptr(workspace),
                                                _lib.stream_handle(dev)))
            dh0 = dh0_m
            if dh0_m is not None and idx is not None:  # h0 is (B, H): the sequences' rows, zeros elsewhere
                dh0 = torch.zeros((B, H), dtype=torch.float32, device=dev).index_add_(0, idx.long(), dh0_m)
            return (dtheta if ctx.needs_input_grad[0] else None), None, dh0, None, None, None, None

    def apply_sequence_native(params, obs: torch.Tensor, h0: torch.Tensor, reset: Optional[torch.Tensor] = None,
                              idx: Optional[torch.Tensor] = None, normalizer=None):
        """``apply_sequence`` over trajectory arrays read in place, forward and backward in the engine
        (``pob_gru_sequence_forward_train`` / ``pob_gru_sequence_backward``: DESIGN.md "Recurrent
        backward"): obs (T, B, obs_size), h0 (B, hidden_size), reset (T, B); sequence m is env
        ``idx[m]`` (int32 (M,); None: every env, M = B); ``normalizer`` (an ``ObservationNormalizer``)
        is applied to the observation rows -> ``(y (T, M, out), h_last (M, hidden_size))``.  Contiguous
        float32 CUDA tensors take the kernels when a gradient is needed: ``theta.grad`` always,
        ``h0.grad`` only when ``h0`` requires it, never a gradient to ``obs``; differentiable once.
        Anything else (the CPU, other dtypes, no gradient needed) is ``apply_sequence`` on the
        gathered, normalised rows."""
        theta = getattr(params, "theta", None)
        for name, t in (("params.theta", theta), ("obs", obs), ("h0", h0)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor")
            if not t.is_floating_point():
                raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype}")
        _check_theta(theta)
        if obs.dim() != 3 or obs.shape[2] != pre[0] or obs.shape[0] < 1 or obs.shape[1] < 1:
            raise ValueError(f"obs must be (T, B, {pre[0]}) with T >= 1 and B >= 1")
        T, B = int(obs.shape[0]), int(obs.shape[1])
        if tuple(h0.shape) != (B, H):
            raise ValueError(f"h0 must be ({B}, {H})")
        if h0.dtype != obs.dtype or h0.device != obs.device:
            raise TypeError(f"h0 is {h0.dtype} on {h0.device}, obs {obs.dtype} on {obs.device}")
        if theta.dtype != obs.dtype or theta.device != obs.device:
            raise TypeError(f"params.theta is {theta.dtype} on {theta.device}, obs {obs.dtype} on {obs.device}")
        if reset is not None:
            if not isinstance(reset, torch.Tensor):
                raise TypeError("reset must be a torch.Tensor")
            if tuple(reset.shape) != (T, B):
                raise ValueError(f"reset must be ({T}, {B})")
            if reset.device != obs.device:
                raise TypeError(f"reset is on {reset.device}, obs on {obs.device}")
        if idx is not None:
            if not (isinstance(idx, torch.Tensor) and idx.dtype == torch.int32 and idx.dim() == 1 and idx.shape[0] >= 1):
                raise ValueError("idx must be an int32 tensor (M,) with M >= 1")
            if idx.device != obs.device:
                raise TypeError(f"idx is on {idx.device}, obs on {obs.device}")
        if normalizer is not None and not callable(getattr(normalizer, "apply", None)):
            raise TypeError("normalizer must be a normalization.ObservationNormalizer (or have its apply)")
        table = getattr(normalizer, "table", None)  # the kernels read the table; anything else only has apply
        if table is not None and tuple(table.shape) != (3, pre[0]):
            raise ValueError(f"normalizer.table must be (3, {pre[0]}), got {tuple(table.shape)}")
        need_grad = torch.is_grad_enabled() and (theta.requires_grad or h0.requires_grad)
        native = (need_grad and not obs.requires_grad
                  and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (theta, obs, h0))
                  and (idx is None or idx.is_contiguous())
                  and (normalizer is None or (table is not None and table.is_cuda and table.dtype == torch.float32
                                              and table.is_contiguous())))
        if native:
            rs = None if reset is None else reset.detach().to(torch.float32).contiguous()
            return _NativeSequence.apply(theta, obs.detach(), h0, rs, idx, table,
                                         0.0 if normalizer is None else normalizer.clip)
        x, h, rs = obs, h0, reset
        if idx is not None:
            j = idx.long()
            x, h = obs.index_select(1, j), h0.index_select(0, j)
            rs = None if reset is None else reset.index_select(1, j)
        if normalizer is not None:
            x = normalizer.apply(x.reshape(-1, pre[0])).reshape(x.shape)
        return apply_sequence(params, x, h, rs)

    return RecurrentModel(init=init, apply=apply, initial_state=initial_state, pre_sizes=pre, hidden_size=H,
                          post_sizes=post, activation=act, gru=gru, apply_sequence=apply_sequence,
                          apply_sequence_native=apply_sequence_native)


class RecurrentTanhPolicy:
    """The recurrent counterpart of ``NormalTanhPolicy``: ``policy(obs) -> action`` is ONE
    ``pob_gru_policy_act`` launch (pre-MLP, GRU cell, post-MLP, tanh-normal head) plus the one-
    thread key advance.  The policy owns ``hidden`` (B, H), carried in place from call to call,
    and ``reset`` (B,): where it is non-zero the env starts the next call from h = 0 (write the
    env's ``done`` into it).  Both are allocated at first use and start as zeros; after that no
    allocation, no host sync: capture-safe.  ``normalizer`` (a ``normalization.ObservationNormalizer``
    of the observation's width -- the masked columns' when the policy acts on those): the network
    sees the normalised observation (``pob_gru_policy_act_norm``, its table read at launch time);
    ``obs_copy`` keeps the raw rows and the hidden state is never normalised."""

    def __init__(self, model: RecurrentModel, params: RecurrentParams, key, total: Optional[int] = None, first: int = 0,
                 deterministic: bool = False, normalizer=None):
        if model.gru is None:
            raise ValueError("model must come from make_recurrent_model")
        if model.post_sizes[-1] % 2:
            raise ValueError("the policy network's last width must be even (loc and scale halves)")
        theta = params.theta
        if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous()):
            raise ValueError("params.theta must be a contiguous float32 CUDA tensor (params.to('cuda'))")
        if theta.numel() != model.gru.param_count:
            raise ValueError(f"theta has {theta.numel()} elements, the network {model.gru.param_count}")
        self.model, self.params, self.theta = model, params, theta
        self.obs_size, self.action_size = model.pre_sizes[0], model.post_sizes[-1] // 2
        self.hidden_size = model.hidden_size
        self.normalizer = _normalization.attach(normalizer, self.obs_size, theta.device)
        self.key = _key_words(key).to(theta.device).clone()
        self.total, self.first = (None if total is None else int(total)), int(first)
        self.deterministic = bool(deterministic)
        self.action = self.logp = self.raw = self.hidden = self.reset = None

    def _buffers(self, B: int):
        if self.hidden is None or self.hidden.shape[0] != B:
            dev = self.theta.device
            self.action = torch.zeros((B, self.action_size), dtype=torch.float32, device=dev)
            self.raw = torch.zeros((B, self.action_size), dtype=torch.float32, device=dev)
            self.logp = torch.zeros((B,), dtype=torch.float32, device=dev)
            self.hidden = torch.zeros((B, self.hidden_size), dtype=torch.float32, device=dev)
            self.reset = torch.zeros((B,), dtype=torch.float32, device=dev)

    def act_into(self, obs: torch.Tensor, action: torch.Tensor, logp=None, raw=None, logits=None, obs_copy=None,
                 hidden_in=None, reset=None):
        """One launch on caller buffers (contiguous float32 device tensors; None = skip).
        ``hidden_in`` (B, H) receives the state the step started from, after the reset;
        ``reset`` (B,) replaces ``self.reset`` for this call."""
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] == self.obs_size
                and obs.is_contiguous()):
            raise ValueError(f"obs must be a contiguous float32 CUDA tensor (B, {self.obs_size})")
        B, A, H = int(obs.shape[0]), self.action_size, self.hidden_size
        self._buffers(B)
        reset = self.reset if reset is None else reset
        for t, shape in ((action, (B, A)), (logp, (B,)), (raw, (B, A)), (logits, (B, 2 * A)), (obs_copy, (B, self.obs_size)),
                         (hidden_in, (B, H)), (reset, (B,))):
            if t is not None and not (tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_contiguous()
                                      and t.device == obs.device):
                raise ValueError(f"buffer must be a contiguous float32 tensor {shape} on {obs.device}")
        total = B if self.total is None else self.total
        args = (self.model.gru.handle, B, total, self.first, ptr(obs), ptr(self.theta), ptr(self.key),
                int(self.deterministic), ptr(reset), ptr(self.hidden), ptr(action), ptr(logp), ptr(raw), ptr(logits),
                ptr(obs_copy), ptr(hidden_in))
        if self.normalizer is None:
            check(lib.pob_gru_policy_act(*args, _lib.stream_handle(obs.device)))
        else:
            check(lib.pob_gru_policy_act_norm(*args, ptr(self.normalizer.table), self.normalizer.clip,
                                              _lib.stream_handle(obs.device)))
        return action

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        self._buffers(int(obs.shape[0]))
        return self.act_into(obs, self.action, self.logp, self.raw)


class NormalTanhPolicy:
    """``policy(obs) -> action`` (B, A) on the device: the model's forward and brax's tanh-normal
    head (loc, s = split(logits); scale = softplus(s) + 0.001; action = tanh(loc + scale eps)) in
    ONE ``pob_policy_act`` launch, plus the one-thread key advance.  No allocation, no host sync
    after the first call at a batch size: capture-safe.  ``.logp`` (B,) and ``.raw`` (B, A) hold
    the last call's log-probability and pre-tanh action; ``deterministic = True`` gives
    ``tanh(loc)`` and leaves the key and ``.logp`` alone.  The noise of env ``b`` is row
    ``first + b`` of a draw for ``total`` envs, so a shard's actions equal the slice of the
    whole batch's.  ``normalizer`` (a ``normalization.ObservationNormalizer`` of width ``obs_size``):
    the network sees ``normalizer.apply(obs)``, computed in the tile load (``pob_policy_act_norm``,
    the table read at launch time: an update between replays changes the next replay's actions);
    ``obs_copy`` keeps the raw rows."""

    def __init__(self, model: FeedForwardModel, params: Params, key, total: Optional[int] = None, first: int = 0,
                 deterministic: bool = False, normalizer=None):
        if model.mlp is None or model.layer_sizes is None:
            raise ValueError("model must come from make_model")
        if model.layer_sizes[-1] % 2:
            raise ValueError("the policy network's last width must be even (loc and scale halves)")
        theta = params.theta
        if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous()):
            raise ValueError("params.theta must be a contiguous float32 CUDA tensor (params.to('cuda'))")
        if theta.numel() != model.mlp.param_count:
            raise ValueError(f"theta has {theta.numel()} elements, the network {model.mlp.param_count}")
        self.model, self.params, self.theta = model, params, theta
        self.obs_size, self.action_size = model.layer_sizes[0], model.layer_sizes[-1] // 2
        self.normalizer = _normalization.attach(normalizer, self.obs_size, theta.device)
        self.key = _key_words(key).to(theta.device).clone()
        self.total, self.first = (None if total is None else int(total)), int(first)
        self.deterministic = bool(deterministic)
        self.action = self.logp = self.raw = None

    def _buffers(self, B: int):
        if self.action is None or self.action.shape[0] != B:
            dev = self.theta.device
            self.action = torch.zeros((B, self.action_size), dtype=torch.float32, device=dev)
            self.raw = torch.zeros((B, self.action_size), dtype=torch.float32, device=dev)
            self.logp = torch.zeros((B,), dtype=torch.float32, device=dev)

    def act_into(self, obs: torch.Tensor, action: torch.Tensor, logp=None, raw=None, logits=None, obs_copy=None):
        """One launch on caller buffers (contiguous float32 device tensors; None = skip)."""
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] == self.obs_size
                and obs.is_contiguous()):
            raise ValueError(f"obs must be a contiguous float32 CUDA tensor (B, {self.obs_size})")
        B, A = int(obs.shape[0]), self.action_size
        for t, shape in ((action, (B, A)), (logp, (B,)), (raw, (B, A)), (logits, (B, 2 * A)), (obs_copy, (B, self.obs_size))):
            if t is not None and not (tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_contiguous()
                                      and t.device == obs.device):
                raise ValueError(f"output buffer must be a contiguous float32 tensor {shape} on {obs.device}")
        total = B if self.total is None else self.total
        args = (self.model.mlp.handle, B, total, self.first, ptr(obs), ptr(self.theta), ptr(self.key),
                int(self.deterministic), ptr(action), ptr(logp), ptr(raw), ptr(logits), ptr(obs_copy))
        if self.normalizer is None:
            check(lib.pob_policy_act(*args, _lib.stream_handle(obs.device)))
        else:
            check(lib.pob_policy_act_norm(*args, ptr(self.normalizer.table), self.normalizer.clip,
                                          _lib.stream_handle(obs.device)))
        return action

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        self._buffers(int(obs.shape[0]))
        return self.act_into(obs, self.action, self.logp, self.raw)
