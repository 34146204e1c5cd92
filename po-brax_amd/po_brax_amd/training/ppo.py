"""The learner's side of PPO: the loss on the tanh-normal head with its gradient to the logits and
the values, and the smallest learner that drives it (brax v1 ``training/ppo.py``:
``compute_ppo_loss`` and the minibatch loop of ``train``, as recalled, [ext]).

``ppo_loss`` is differentiable in ``logits`` and ``values`` through one ``torch.autograd.Function``
whose forward computes the four scalars AND both gradients: contiguous float32 CUDA tensors take
``pob_ppo_loss`` (``k_ppo_loss`` and its two small reduction launches; ``ppo_loss_ref`` of
csrc/pob_mlp.h bit for bit); anything else takes the same operation order in torch ops -- float32
with the header's scalar functions spelled out (fmaf through a round-to-odd float64 sum), so CPU
float32 tensors give ``ppo_loss_ref``'s bits, other dtypes with torch's own ``exp`` / ``log`` /
``erfinv`` and the constants to their precision.  The matrix work of the backward pass stays with
torch autograd over the networks' torch-op ``apply``, unless ``PPOLearner(backward=...)`` asks for
``model.apply_native`` (DESIGN.md "MLP backward").  Formula, operation order and what is pinned:
DESIGN.md "PPO loss".

``PPOLearner.update(roll)`` runs the epochs and minibatches over the buffers an
``ActorRollout(..., critic=...)`` replay left on the device and takes Adam steps on both parameter
vectors in place, so the captured rollout graph acts under the new parameters at its next replay.
Two deviations from brax: the advantages and value targets are the replay's and are not recomputed
per minibatch (``compute_gae`` exists for a learner that wants that), and the permutation is
torch's, not jax's, unless ``permutation="threefry"`` asks for ``jumpy.random_permutation``;
``optimizer="fused"`` steps both parameter vectors with one launch and no host step count.

``RecurrentPPOLearner`` is the same loop for a ``RecurrentTanhPolicy`` over a
``RecurrentActorRollout(..., critic=...)``: minibatches of envs, each the whole recorded window,
through ``model.apply_sequence`` / ``apply_sequence_native`` (DESIGN.md "Recurrent backward").
"""
from __future__ import annotations

import ctypes as C
import math
import types
from typing import Dict, Optional, Tuple

import torch

from .. import _lib
from .._lib import check, lib, ptr
from . import networks as _networks
from .gae import RecurrentValueFunction, ValueFunction

MAX_ACTION_SIZE = 128  # POB_PPO_MAX_A
CHUNK = 1024           # POB_PPO_CHUNK
_U_MIN = -float.fromhex("0x1.fffffep-1")


# ---------------------------------------------------------------------------- float32, bit for bit
# The scalar functions of csrc/pob_mlp.h on float32 tensors.  Every + and * is one torch op (one
# rounding); fmaf is the exact product in float64, a float64 sum rounded to odd, then one rounding
# to float32 (correct for every float32 result, subnormal ones too).
def _c(v: float, like: torch.Tensor) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32, device=like.device)


def _fma(a, b, c):
    ref = next(t for t in (a, b, c) if isinstance(t, torch.Tensor))
    a, b, c = (t if isinstance(t, torch.Tensor) else _c(t, ref) for t in (a, b, c))
    p = a.double() * b.double()
    c = c.double()
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    s = s.contiguous()
    odd = (s.view(torch.int64) & 1) != 0
    toward = torch.where(err > 0, float("inf"), -float("inf")).to(torch.float64)
    s = torch.where((err != 0) & ~odd & torch.isfinite(s), torch.nextafter(s, toward), s)
    return s.float()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _expf(x):
    x = torch.where(x < -104.0, _c(-104.0, x), x)
    x = torch.where(x > 89.0, _c(89.0, x), x)
    t = _fma(x, 1.44269504, 12582912.0)
    fn = t - 12582912.0
    n = _bits(t) - 0x4B400000
    r = _fma(fn, -0.693145751953125, x)
    r = _fma(fn, -1.42860677e-6, r)
    p = _c(1.98412698e-4, x)
    for k in (1.38888889e-3, 8.33333333e-3, 4.16666667e-2, 1.66666667e-1, 0.5, 1.0, 1.0):
        p = _fma(p, r, k)
    n1 = n >> 1
    n2 = n - n1
    s1 = ((n1 + 127) << 23).view(torch.float32)
    s2 = ((n2 + 127) << 23).view(torch.float32)
    return (p * s1) * s2


def _rcp(x):
    return 1.0 / x


def _logf(x):
    sub = x < 2.0 ** -126
    xs = torch.where(sub, x * 2.0 ** 25, x)
    ix = _bits(xs) + (0x3F800000 - 0x3F3504F3)
    k = (ix >> 23) - 127 - torch.where(sub, 25, 0).to(torch.int32)
    ix = (ix & 0x007FFFFF) + 0x3F3504F3
    f = ix.view(torch.float32) - 1.0
    s = f * _rcp(2.0 + f)
    z = s * s
    w = z * z
    t1 = w * _fma(w, 0.24279078841, 0.40000972152)
    t2 = z * _fma(w, 0.28498786688, 0.66666662693)
    R = t2 + t1
    hfsq = (0.5 * f) * f
    dk = k.to(torch.float32)
    r = _fma(s, hfsq + R, dk * _c(9.0580006145e-06, x))
    r = ((r - hfsq) + f) + dk * _c(6.9313812256e-01, x)
    r = torch.where(x == 0.0, _c(-float("inf"), x), r)
    r = torch.where(x < 0.0, _c(float("nan"), x), r)
    r = torch.where(x == float("inf"), x, r)
    return torch.where(x != x, x, r)


def _tanhf(x):
    a = torch.where(x < 0.0, -x, x)
    z = x * x
    p = _c(-5.70498872745e-3, x)
    for k in (2.06390887954e-2, -5.37397155531e-2, 1.33314422036e-1, -3.33332819422e-1):
        p = _fma(p, z, k)
    small = _fma(p * z, x, x)
    e = _expf(2.0 * torch.where(a > 10.0, _c(10.0, x), a))
    big = 1.0 - 2.0 * _rcp(e + 1.0)
    big = torch.where(x < 0.0, -big, big)
    r = torch.where(a < 0.625, small, big)
    return torch.where(x != x, x, r)


def _log1p_unit(t):
    u = 1.0 + t
    c = t - (u - 1.0)
    return _fma(c, _rcp(u), _logf(u))


def _softplusf(x):
    a = torch.where(x < 0.0, -x, x)
    m = torch.where(x > 0.0, x, _c(0.0, x))
    r = m + _log1p_unit(_expf(-a))
    return torch.where(x != x, x, r)


def _sigmoidf(x):
    return _rcp(1.0 + _expf(-x))


def _erfinvf(x):
    w = -_logf((1.0 - x) * (1.0 + x))
    wc = w - 2.5
    p = _c(2.81022636e-08, x)
    for k in (3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087, -0.00125372503, -0.00417768164,
              0.246640727, 1.50140941):
        p = _fma(p, wc, k)
    wt = torch.sqrt(torch.where(w < 5.0, _c(5.0, x), w)) - 3.0
    q = _c(-0.000200214257, x)
    for k in (0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773, -0.0076224613, 0.00943887047, 1.00167406,
              2.83297682):
        q = _fma(q, wt, k)
    return torch.where(w < 5.0, p, q) * x


class _F32:
    """The header's functions (float32 tensors)."""
    fma, exp, log, tanh, softplus, sigmoid, erfinv = map(staticmethod, (_fma, _expf, _logf, _tanhf, _softplusf, _sigmoidf,
                                                                        _erfinvf))


class _Native:
    """torch's own functions (every other dtype); the operation order around them is the same."""
    fma = staticmethod(lambda a, b, c: a * b + c)
    exp, log, tanh, sigmoid, erfinv = map(staticmethod, (torch.exp, torch.log, torch.tanh, torch.sigmoid, torch.erfinv))
    softplus = staticmethod(lambda x: torch.logaddexp(x, torch.zeros_like(x)))


def _chunk_sums(terms: torch.Tensor) -> torch.Tensor:
    """(3,) float64 sums of terms (3, M) in the order of ``ppo_loss_ref``: chunks of 1024 rows, rows
    ascending from +0.0, chunk partials ascending from +0.0 (``cumsum`` walks in order on the CPU;
    on a device tensor the order inside a chunk is torch's)."""
    M = terms.shape[1]
    n_chunks = (M + CHUNK - 1) // CHUNK
    t = torch.zeros((3, n_chunks * CHUNK), dtype=torch.float64, device=terms.device)
    t[:, :M] = terms
    zero = torch.zeros((3, n_chunks, 1), dtype=torch.float64, device=terms.device)
    partials = torch.cat([zero, t.reshape(3, n_chunks, CHUNK)], dim=2).cumsum(dim=2)[:, :, -1]
    return torch.cat([zero[:, 0], partials], dim=1).cumsum(dim=1)[:, -1]


def _ppo_torch(logits, values, raw, old_logp, advantages, vs, u, idx, entropy_cost: float, ppo_epsilon: float):
    """``ppo_loss_ref`` in torch ops: (losses (4,), dlogits (M, 2 A), dvalues (M,))."""
    dt = logits.dtype
    f32 = dt == torch.float32
    ops = _F32 if f32 else _Native
    M, A = int(logits.shape[0]), int(logits.shape[1]) // 2
    k = lambda v: torch.tensor(v, dtype=dt, device=logits.device)  # noqa: E731
    loc, p = logits[:, :A], logits[:, A:]
    if idx is not None:
        j = idx.long()
        raw, old_logp, advantages, vs = raw[j], old_logp[j], advantages[j], vs[j]
    inv_m = k(1.0) / k(float(torch.tensor(M, dtype=dt)))
    # float32: the header's literals; other dtypes: the constants they stand for
    half_log_2pi, log2, sqrt2 = ((0.918938533, 0.693147181, 1.41421354) if f32 else
                                 (0.5 * math.log(2.0 * math.pi), math.log(2.0), math.sqrt(2.0)))
    ent0 = 1.418938533 if f32 else 0.5 + half_log_2pi
    ec = k(entropy_cost)
    scale = ops.softplus(p) + k(0.001)
    inv, ls = 1.0 / scale, ops.log(scale)
    e = (raw - loc) * inv
    t1 = (((-0.5 * e) * e) - ls) - k(half_log_2pi)
    ldx = 2.0 * ((k(log2) - raw) - ops.softplus(-2.0 * raw))
    term = t1 - ldx
    u = torch.where(u > _U_MIN, u, k(_U_MIN))
    eps = k(sqrt2) * ops.erfinv(u)
    y = ops.fma(scale, eps, loc)
    ldy = 2.0 * ((k(log2) - y) - ops.softplus(-2.0 * y))
    en = (k(ent0) + ls) + ldy
    dlp_loc = e * inv
    dlp_sc = ops.fma(e, e, k(-1.0)) * inv
    den_loc = -2.0 * ops.tanh(y)
    den_sc = ops.fma(eps, den_loc, inv)
    sig = ops.sigmoid(p)
    logp, ent = torch.zeros_like(values), torch.zeros_like(values)
    for a in range(A):  # a ascending from +0
        logp = logp + term[:, a]
        ent = ent + en[:, a]
    rho = ops.exp(logp - old_logp)
    lo, hi = k(1.0) - k(ppo_epsilon), k(1.0) + k(ppo_epsilon)
    c = torch.where(rho < lo, lo, rho)
    c = torch.where(c > hi, hi, c)
    s1, s2 = rho * advantages, c * advantages
    unclipped = s1 <= s2
    neg_surr = -torch.where(unclipped, s1, s2)
    g_lp = torch.where(unclipped, -(s1 * inv_m), k(0.0))
    verr = vs - values
    vl = (verr * verr) * 0.25
    dvalues = (-0.5 * verr) * inv_m
    g_ent = -(ec * inv_m)
    g = g_lp[:, None]
    dlogits = torch.cat([ops.fma(g, dlp_loc, g_ent * den_loc), ops.fma(g, dlp_sc, g_ent * den_sc) * sig], dim=1)
    S = _chunk_sums(torch.stack([neg_surr, vl, ent]))
    m = float(M)
    policy, value = (S[0] / m).to(dt), (S[1] / m).to(dt)
    entropy = (-ec.double() * (S[2] / m)).to(dt)
    return torch.stack([(policy + value) + entropy, policy, value, entropy]), dlogits.contiguous(), dvalues


def _entropy_draws(key: torch.Tensor, M: int, A: int) -> torch.Tensor:
    """uniform(split(key)[1], (M, A), -1, 1): the device threefry on a device key, the host's otherwise."""
    if key.is_cuda:
        from .. import jumpy
        return jumpy.random_uniform(jumpy.random_split(key)[1], (M, A), -1.0, 1.0)
    sub = _networks._host_split(key)[1]
    return _networks._host_uniform(sub, M * A, -1.0, 1.0).reshape(M, A)


def _advance_key(key: torch.Tensor) -> None:
    """key <- split(key)[0], in place."""
    if key.is_cuda:
        check(lib.pob_random_split(ptr(key), 2, 0, 1, ptr(key), _lib.stream_handle(key.device)))
    else:
        key.copy_(_networks._host_split(key)[0].to(torch.uint32))


class _PPOLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, values, raw, old_logp, advantages, vs, key, idx, entropy_cost, ppo_epsilon):
        M, A = int(logits.shape[0]), int(logits.shape[1]) // 2
        ins = (logits, values, raw, old_logp, advantages, vs)
        fused = (all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ins) and key.is_cuda
                 and (idx is None or idx.is_contiguous()))
        if fused:
            dev = logits.device
            need = C.c_longlong()
            check(lib.pob_ppo_loss_workspace_bytes(M, C.byref(need)))
            workspace = torch.empty(need.value // 8, dtype=torch.float64, device=dev)
            dlogits, dvalues = torch.empty_like(logits), torch.empty_like(values)
            losses = torch.empty(4, dtype=torch.float32, device=dev)
            check(lib.pob_ppo_loss(M, A, ptr(logits), ptr(values), ptr(idx), ptr(raw), ptr(old_logp), ptr(advantages),
                                   ptr(vs), ptr(key), float(entropy_cost), float(ppo_epsilon), ptr(dlogits), ptr(dvalues),
                                   ptr(losses), ptr(workspace), _lib.stream_handle(dev)))
        else:
            u = _entropy_draws(key, M, A).to(device=logits.device, dtype=logits.dtype)
            losses, dlogits, dvalues = _ppo_torch(logits, values, raw, old_logp, advantages, vs, u, idx,
                                                  float(entropy_cost), float(ppo_epsilon))
        ctx.save_for_backward(dlogits, dvalues)
        total, policy, value, entropy = losses.unbind(0)
        ctx.mark_non_differentiable(policy, value, entropy)
        return total, policy, value, entropy

    @staticmethod
    def backward(ctx, grad, *_):
        dlogits, dvalues = ctx.saved_tensors
        return (dlogits * grad, dvalues * grad) + (None,) * 8


def ppo_loss(logits: torch.Tensor, values: torch.Tensor, raw: torch.Tensor, old_logp: torch.Tensor,
             advantages: torch.Tensor, vs: torch.Tensor, key: torch.Tensor, idx: Optional[torch.Tensor] = None,
             entropy_cost: float = 1e-4, ppo_epsilon: float = 0.3) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """brax's ``compute_ppo_loss`` from the networks' outputs: ``(total, metrics)``.

    ``logits`` (M, 2 A) and ``values`` (M,) are in minibatch order; ``raw`` (N, A), ``old_logp``,
    ``advantages`` and ``vs`` (N,) in trajectory order: row i reads trajectory row ``idx[i]``
    (int32, every entry in [0, N): not checked), or row i without ``idx`` (then N == M).  ``total =
    policy_loss + value_loss + entropy_loss`` with the clipped surrogate, ``mean((vs - values)^2) / 4``
    and ``-entropy_cost`` times the entropy sampled with ``uniform(split(key)[1], (M, A), -1, 1)``;
    ``metrics`` holds the three parts as 0-d tensors.  ``total`` is differentiable in ``logits`` and
    ``values`` only.  ``key`` (2 uint32 words) is advanced in place: ``key <- split(key)[0]``.  No host
    synchronisation on the kernel path: capturable."""
    named = (("logits", logits), ("values", values), ("raw", raw), ("old_logp", old_logp), ("advantages", advantages),
             ("vs", vs))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype}")
        if t.dtype != logits.dtype or t.device != logits.device:
            raise TypeError(f"{name} is {t.dtype} on {t.device}, logits {logits.dtype} on {logits.device}")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 2 or logits.shape[1] % 2:
        raise ValueError("logits must be (M, 2 A) with M >= 1 and A >= 1")
    M, A = int(logits.shape[0]), int(logits.shape[1]) // 2
    if A > MAX_ACTION_SIZE:
        raise ValueError(f"the action size A must be in 1 .. {MAX_ACTION_SIZE}, got {A}")
    if M * A >= 2 ** 32 - 1:
        raise ValueError("too many action elements (M A must be below 2^32 - 1)")
    if tuple(values.shape) != (M,):
        raise ValueError(f"values must be ({M},), got {tuple(values.shape)}")
    if raw.dim() != 2 or raw.shape[1] != A or raw.shape[0] < 1:
        raise ValueError(f"raw must be (N, {A}), got {tuple(raw.shape)}")
    N = int(raw.shape[0])
    for name, t in named[3:]:
        if tuple(t.shape) != (N,):
            raise ValueError(f"{name} must be ({N},) like raw's rows, got {tuple(t.shape)}")
    if idx is None:
        if N != M:
            raise ValueError(f"without idx the trajectory arrays must have M = {M} rows, got {N}")
    else:
        if not (isinstance(idx, torch.Tensor) and idx.dtype == torch.int32 and tuple(idx.shape) == (M,)
                and idx.device == logits.device):
            raise ValueError(f"idx must be an int32 tensor ({M},) on {logits.device}")
    key = _networks._key_words(key)
    total, policy, value, entropy = _PPOLoss.apply(logits, values, raw.detach(), old_logp.detach(), advantages.detach(),
                                                   vs.detach(), key, idx, float(entropy_cost), float(ppo_epsilon))
    _advance_key(key)
    return total, {"policy_loss": policy, "value_loss": value, "entropy_loss": entropy}


class _DeviceLearner:
    """What both learners share of the device-resident update: the optimiser and permutation options
    (DESIGN.md "Learner on the device")."""

    def _init_options(self, key, learning_rate: float, optimizer: str, permutation: str) -> None:
        if optimizer not in ("torch", "fused"):
            raise ValueError(f"optimizer must be 'torch' or 'fused', got {optimizer!r}")
        if permutation not in ("torch", "threefry"):
            raise ValueError(f"permutation must be 'torch' or 'threefry', got {permutation!r}")
        dev = self.policy.theta.device
        self.key = _networks._key_words(key).to(dev).clone()
        words = _networks._key_words(key).cpu()
        self._generator = torch.Generator(device=dev)
        self._generator.manual_seed((int(words[0]) << 32) | int(words[1]))
        # leaves over the actors' own storage: the optimiser steps in place
        self._theta = [self.policy.theta.detach().requires_grad_(True), self.value_fn.theta.detach().requires_grad_(True)]
        if optimizer == "fused":
            from .optim import FusedAdam
            self.optimizer = FusedAdam(self._theta, lr=float(learning_rate))
        else:
            self.optimizer = torch.optim.Adam(self._theta, lr=float(learning_rate))
        self.permutation = permutation
        self.perm_key = None
        if permutation == "threefry":  # random_split(key, 3)[2], on the key's device
            if dev.type == "cuda":
                from .. import jumpy
                self.perm_key = jumpy.random_split_rows(self.key, 3, 2, 1).reshape(2)
            else:
                self.perm_key = _networks._host_split(words, 3)[2].to(torch.uint32)

    def _draw_permutation(self, n: int, dev) -> torch.Tensor:
        """One epoch's int32 permutation of n items on ``dev``."""
        if self.permutation == "threefry":
            from .. import jumpy
            perm = jumpy.random_permutation(self.perm_key, n).to(dev)
            _advance_key(self.perm_key)
            return perm
        return torch.randperm(n, device=dev, generator=self._generator).to(torch.int32)


class PPOLearner(_DeviceLearner):
    """The minibatch loop of brax v1 PPO over one replay of an ``ActorRollout(..., critic=value_fn)``:

        learner = PPOLearner(policy, value_fn, key=jumpy.random_prngkey(7))
        for _ in range(n):
            roll.replay()
            metrics = learner.update(roll)

    ``policy`` is a feed-forward ``NormalTanhPolicy``, ``value_fn`` a ``ValueFunction``.  Per epoch one
    device permutation of the T B rows; per minibatch the observation rows are gathered with the
    ``idx`` slice, normalised with the policy's normaliser (torch ``apply``; the statistics are the
    replay's business), both networks run their torch-op ``apply`` under grad, ``ppo_loss`` reads the
    rollout's flattened ``raw``, ``logp``, ``advantages`` and ``vs`` through the same ``idx``, and one
    Adam step updates both ``theta`` vectors IN PLACE: their storage never moves, so a captured
    rollout graph sees the update.  ``key`` seeds the entropy draws and the permutations.

    ``backward`` chooses each network's forward-with-grad and backward pass: ``"torch"`` (the default:
    the torch-op ``apply`` under autograd), ``"native"`` (``model.apply_native``: ``pob_mlp_forward_train``
    and ``pob_mlp_backward``, the fused forward's bits and a fixed summation order), or a pair
    ``(policy, value)`` of those.  Measured on an MI355X at 40 960 rows a minibatch (DESIGN.md "MLP
    backward"): the policy network ``[32] * 4`` should use ``"native"`` (4.0 x faster than the torch
    ops), the 256-wide value network ``"torch"`` (the native pass is 2.4 x slower than the vendor
    GEMMs), i.e. ``backward=("native", "torch")``: one update in 78 ms against 108 ms for the default.

    ``optimizer``: ``"torch"`` (the default: ``torch.optim.Adam``) or ``"fused"`` (``training.optim.FusedAdam``:
    both parameter vectors in one launch, the step count on the device).  ``permutation``: ``"torch"`` (the
    default: ``randperm`` from a generator seeded with ``key``) or ``"threefry"``: ``perm_key =
    random_split(key, 3)[2]`` lives on the device, each epoch draws ``jumpy.random_permutation(perm_key, T B)``
    (jax's shuffle, [ext]) and then ``perm_key <- split(perm_key)[0]``; ``key`` and the entropy draws are the
    same either way.  With both nothing of an update is decided on the host (DESIGN.md "Learner on the
    device").

    Not brax's: advantages and value targets are the replay's (not recomputed per minibatch), and
    by default the permutation is torch's (``randperm``), not jax's."""

    def __init__(self, policy, value_fn, learning_rate: float = 3e-4, entropy_cost: float = 1e-4,
                 ppo_epsilon: float = 0.3, num_minibatches: int = 32, num_update_epochs: int = 4, key=None,
                 backward="torch", optimizer: str = "torch", permutation: str = "torch"):
        pair = (backward, backward) if isinstance(backward, str) else backward
        if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and all(b in ("torch", "native") for b in pair)):
            raise ValueError(f"backward must be 'torch', 'native' or a (policy, value) pair of those, got {backward!r}")
        self.backward = tuple(pair)
        if not isinstance(policy, _networks.NormalTanhPolicy):
            raise TypeError("policy must be a training.networks.NormalTanhPolicy (the feed-forward actor)")
        if not isinstance(value_fn, ValueFunction):
            raise TypeError("value_fn must be a training.ValueFunction")
        if key is None:
            raise ValueError("key is required (jumpy.random_prngkey)")
        if int(num_minibatches) < 1 or int(num_update_epochs) < 1:
            raise ValueError("num_minibatches and num_update_epochs must be positive")
        if policy.obs_size != value_fn.obs_size or policy.theta.device != value_fn.theta.device:
            raise ValueError("policy and value_fn must share the observation width and the device")
        self.policy, self.value_fn = policy, value_fn
        self.entropy_cost, self.ppo_epsilon = float(entropy_cost), float(ppo_epsilon)
        self.num_minibatches, self.num_update_epochs = int(num_minibatches), int(num_update_epochs)
        self._init_options(key, learning_rate, optimizer, permutation)

    def update(self, roll) -> Dict[str, torch.Tensor]:
        """One learning phase over ``roll``'s buffers as the last replay left them; returns the last
        minibatch's metrics (``total_loss`` and the three parts, 0-d device tensors)."""
        for name in ("obs", "raw", "logp", "advantages", "vs"):
            if not isinstance(getattr(roll, name, None), torch.Tensor):
                raise ValueError(f"roll has no {name}: build the ActorRollout with critic=")
        T, B = int(roll.logp.shape[0]), int(roll.logp.shape[1])
        N, A, D = T * B, self.policy.action_size, self.policy.obs_size
        if N % self.num_minibatches:
            raise ValueError(f"T B = {N} rows are not divisible by num_minibatches = {self.num_minibatches}")
        M = N // self.num_minibatches
        obs, raw = roll.obs.reshape(N, D), roll.raw.reshape(N, A)
        logp, adv, vs = roll.logp.reshape(N), roll.advantages.reshape(N), roll.vs.reshape(N)
        norm, v_norm = self.policy.normalizer, self.value_fn.normalizer
        p_params = types.SimpleNamespace(theta=self._theta[0])
        v_params = types.SimpleNamespace(theta=self._theta[1])
        p_apply, v_apply = (m.apply_native if b == "native" else m.apply
                            for m, b in zip((self.policy.model, self.value_fn.model), self.backward))
        metrics = None
        for _ in range(self.num_update_epochs):
            perm = self._draw_permutation(N, obs.device)
            for m in range(self.num_minibatches):
                idx = perm[m * M:(m + 1) * M]
                x = obs.index_select(0, idx)
                x_p = x if norm is None else norm.apply(x)
                x_v = x_p if v_norm is norm else (x if v_norm is None else v_norm.apply(x))
                with torch.enable_grad():
                    logits = p_apply(p_params, x_p)
                    values = v_apply(v_params, x_v).reshape(M)
                    total, metrics = ppo_loss(logits, values, raw, logp, adv, vs, self.key, idx=idx,
                                              entropy_cost=self.entropy_cost, ppo_epsilon=self.ppo_epsilon)
                self.optimizer.zero_grad(set_to_none=True)
                total.backward()
                self.optimizer.step()
                metrics = dict(metrics, total_loss=total.detach())
        return metrics


class RecurrentPPOLearner(_DeviceLearner):
    """``PPOLearner`` for the recurrent actor: "replay, learn, replay" over a
    ``RecurrentActorRollout(..., critic=value_fn)``:

        learner = RecurrentPPOLearner(policy, value_fn, key=jumpy.random_prngkey(7), backward=("native", "torch"))
        for _ in range(n):
            roll.replay()
            metrics = learner.update(roll)

    ``policy`` is a ``RecurrentTanhPolicy``, ``value_fn`` a ``ValueFunction`` (or a recurrent one: below).  Minibatches
    are drawn over ENVS, not rows: per epoch one device permutation of the B envs, cut into
    ``num_minibatches`` slices of M = B / num_minibatches envs; a minibatch is the whole T-step window
    of its envs, run through the recurrent network from ``roll.hidden[0]`` (the post-reset state step 0
    started from) with ``reset[0] = 0`` and ``reset[t] = done[t - 1]``, truncated BPTT over the window.
    The logits are (T M, 2 A) in (t, m) order; ``ppo_loss`` reads the trajectory in place through the
    row index ``t B + idx[m]``, and the value network sees the same rows.  One Adam step per minibatch
    updates both ``theta`` vectors IN PLACE, so the captured rollout graph acts under the new
    parameters at its next replay.

    ``backward``: ``"torch"``, ``"native"`` or a ``(policy, value)`` pair.  For the policy ``"torch"`` is
    ``model.apply_sequence`` under autograd on the gathered, normalised rows (CPU tensors too) and
    ``"native"`` is ``model.apply_sequence_native`` (``pob_gru_sequence_forward_train`` /
    ``pob_gru_sequence_backward``, the trajectory read in place: DESIGN.md "Recurrent backward"); for
    a feed-forward value network they are ``PPOLearner``'s.  The default (``"auto"``) is then ``("native",
    "torch")``.  Measured on an
    MI355X (DESIGN.md "Recurrent backward"): a window of T = 20 steps of 2 048 envs, forward with grad plus
    backward, takes 3.09 ms natively against 12.3 ms in torch ops (114 -> GRU 64 -> 16; 2.35 against 12.4 ms
    at 30 columns), and one update of 32 such minibatches 172 ms against 403 ms for ``"torch"`` and 254 ms
    for ``"native"``; the value half stays ``"torch"`` (DESIGN.md "MLP backward": the vendor GEMMs win at
    width 256).

    ``value_fn`` may be a ``RecurrentValueFunction`` (DESIGN.md "Recurrent critic"): the value network is
    then unrolled over the same windows as the policy, from ``roll.value_hidden0`` (the post-reset state
    the critic's row 0 started from) with the same ``reset`` and ``idx``; its ``"torch"`` is
    ``apply_sequence`` on the gathered, normalised rows, its ``"native"`` ``apply_sequence_native``, (T, M, 1)
    read as the loss's T M rows.  The default is then ``("native", "native")``: the GRU window is 4 - 5.3 x
    faster natively, and the vendor-GEMM argument holds for 256-wide dense layers only.  There is no
    gradient to ``value_hidden0``.

    ``optimizer`` and ``permutation`` are ``PPOLearner``'s; the threefry permutation is over the B envs.

    Not brax's: advantages and value targets are the replay's, minibatches never cut a window shorter
    than T, and by default the permutation is torch's."""

    def __init__(self, policy, value_fn, learning_rate: float = 3e-4, entropy_cost: float = 1e-4,
                 ppo_epsilon: float = 0.3, num_minibatches: int = 32, num_update_epochs: int = 4, key=None,
                 backward="auto", optimizer: str = "torch", permutation: str = "torch"):
        if not isinstance(policy, _networks.RecurrentTanhPolicy):
            raise TypeError("policy must be a training.networks.RecurrentTanhPolicy (the recurrent actor)")
        if not isinstance(value_fn, (ValueFunction, RecurrentValueFunction)):
            raise TypeError("value_fn must be a training.ValueFunction or a training.RecurrentValueFunction")
        self.recurrent_critic = isinstance(value_fn, RecurrentValueFunction)
        if isinstance(backward, str) and backward == "auto":
            backward = ("native", "native") if self.recurrent_critic else ("native", "torch")
        pair = (backward, backward) if isinstance(backward, str) else backward
        if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and all(b in ("torch", "native") for b in pair)):
            raise ValueError("backward must be 'auto', 'torch', 'native' or a (policy, value) pair of the last two, "
                             f"got {backward!r}")
        self.backward = tuple(pair)
        if key is None:
            raise ValueError("key is required (jumpy.random_prngkey)")
        if int(num_minibatches) < 1 or int(num_update_epochs) < 1:
            raise ValueError("num_minibatches and num_update_epochs must be positive")
        if policy.obs_size != value_fn.obs_size or policy.theta.device != value_fn.theta.device:
            raise ValueError("policy and value_fn must share the observation width and the device")
        self.policy, self.value_fn = policy, value_fn
        self.entropy_cost, self.ppo_epsilon = float(entropy_cost), float(ppo_epsilon)
        self.num_minibatches, self.num_update_epochs = int(num_minibatches), int(num_update_epochs)
        self._init_options(key, learning_rate, optimizer, permutation)

    def update(self, roll) -> Dict[str, torch.Tensor]:
        """One learning phase over ``roll``'s buffers as the last replay left them; returns the last
        minibatch's metrics (``total_loss`` and the three parts, 0-d device tensors)."""
        for name in ("obs", "raw", "logp", "advantages", "vs", "hidden", "done"):
            if not isinstance(getattr(roll, name, None), torch.Tensor):
                raise ValueError(f"roll has no {name}: build a RecurrentActorRollout with critic=")
        if self.recurrent_critic and not isinstance(getattr(roll, "value_hidden0", None), torch.Tensor):
            raise ValueError("roll has no value_hidden0: build the RecurrentActorRollout with "
                             "critic=RecurrentValueFunction(...)")
        T, B = int(roll.logp.shape[0]), int(roll.logp.shape[1])
        N, A, D = T * B, self.policy.action_size, self.policy.obs_size
        if B % self.num_minibatches:
            raise ValueError(f"B = {B} envs are not divisible by num_minibatches = {self.num_minibatches} "
                             "(minibatches are drawn over envs)")
        M = B // self.num_minibatches
        obs3, dev = roll.obs, roll.obs.device
        obs, raw = obs3.reshape(N, D), roll.raw.reshape(N, A)
        logp, adv, vs = roll.logp.reshape(N), roll.advantages.reshape(N), roll.vs.reshape(N)
        h0 = roll.hidden[0]
        reset = torch.cat([torch.zeros_like(roll.done[:1]), roll.done[:-1]], dim=0).contiguous()  # once per update
        row0 = (torch.arange(T, device=dev, dtype=torch.int32) * B).reshape(T, 1)
        norm, v_norm = self.policy.normalizer, self.value_fn.normalizer
        model, v_model = self.policy.model, self.value_fn.model
        p_params = types.SimpleNamespace(theta=self._theta[0])
        v_params = types.SimpleNamespace(theta=self._theta[1])
        v_h0 = roll.value_hidden0 if self.recurrent_critic else None
        # the native windows read the trajectory in place: no gathered rows when both halves are such
        gathered = not (self.recurrent_critic and self.backward == ("native", "native"))
        v_apply = None if self.recurrent_critic else (v_model.apply_native if self.backward[1] == "native" else v_model.apply)
        metrics = None
        for _ in range(self.num_update_epochs):
            perm = self._draw_permutation(B, dev)
            for m in range(self.num_minibatches):
                idx = perm[m * M:(m + 1) * M].contiguous()
                rows = (row0 + idx.reshape(1, M)).reshape(T * M)  # (t, m) order: trajectory row t B + idx[m]
                if gathered:
                    x = obs.index_select(0, rows)
                    x_p = x if norm is None else norm.apply(x)
                    x_v = x_p if v_norm is norm else (x if v_norm is None else v_norm.apply(x))
                with torch.enable_grad():
                    if self.backward[0] == "native":
                        y, _ = model.apply_sequence_native(p_params, obs3, h0, reset, idx, norm)
                    else:
                        j = idx.long()
                        y, _ = model.apply_sequence(p_params, x_p.reshape(T, M, D), h0.index_select(0, j),
                                                    reset.index_select(1, j))
                    logits = y.reshape(T * M, 2 * A)
                    if not self.recurrent_critic:
                        values = v_apply(v_params, x_v).reshape(T * M)
                    elif self.backward[1] == "native":
                        values = v_model.apply_sequence_native(v_params, obs3, v_h0, reset, idx, v_norm)[0].reshape(T * M)
                    else:
                        j = idx.long()
                        values = v_model.apply_sequence(v_params, x_v.reshape(T, M, D), v_h0.index_select(0, j),
                                                        reset.index_select(1, j))[0].reshape(T * M)
                    total, metrics = ppo_loss(logits, values, raw, logp, adv, vs, self.key, idx=rows,
                                              entropy_cost=self.entropy_cost, ppo_epsilon=self.ppo_epsilon)
                self.optimizer.zero_grad(set_to_none=True)
                total.backward()
                self.optimizer.step()
                metrics = dict(metrics, total_loss=total.detach())
        return metrics
