"""The learner's optimiser on the device: ``FusedAdam``, optax's ``adam`` [ext] (what brax v1 PPO
uses: no weight decay, no amsgrad) with every parameter vector stepped by ONE launch and the step
count kept on the device.

Contiguous float32 CUDA leaves (and gradients) take ``pob_adam_step`` (``k_adam_step`` and its
one-lane ``k_adam_advance``; ``adam_step_ref`` of csrc/pob_mlp.h bit for bit); anything else takes the
same operation order in torch ops, float32 with the header's fmaf spelled out (``_fma`` of
training/ppo.py), so CPU float32 leaves give ``adam_step_ref``'s bits.  Operation order and what is
pinned: DESIGN.md "Learner on the device".

The bias corrections come from ``bias``, a (2,) float64 tensor next to the moments that holds
``beta1^t`` and ``beta2^t`` as running products (1.0 before the first step).  There is no host step
count: a captured ``step()`` counts on at every replay.
"""
from __future__ import annotations

from typing import Dict, Iterable, List

import torch

from .. import _lib
from .._lib import check, lib


class FusedAdam:
    """Adam over a list of leaf tensors, stepped in place:

        opt = FusedAdam([policy_theta, value_theta], lr=3e-4)
        loss.backward(); opt.step(); opt.zero_grad()

    ``step()`` reads each leaf's ``.grad`` (a leaf without one is left alone; the step still counts)
    and updates the leaf, ``m`` and ``v`` in place: no storage moves, so a captured graph that reads
    the parameters sees the update.  No allocation on the kernel path, no synchronisation:
    capturable."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 3e-4, betas=(0.9, 0.999), eps: float = 1e-8):
        self.params: List[torch.Tensor] = list(params)
        if not self.params:
            raise ValueError("FusedAdam needs at least one parameter tensor")
        for p in self.params:
            if not (isinstance(p, torch.Tensor) and p.is_floating_point()):
                raise TypeError("parameters must be floating-point tensors")
            if p.device != self.params[0].device:
                raise ValueError("parameters must share one device")
        if not (lr >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0):
            raise ValueError("lr and eps must be non-negative, the betas in [0, 1)")
        # torch.optim's layout, as far as this project's helpers read it
        self.param_groups = [dict(params=self.params, lr=float(lr), betas=(float(betas[0]), float(betas[1])),
                                  eps=float(eps))]
        self.m = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.v = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.bias = torch.ones(2, dtype=torch.float64, device=self.params[0].device)

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    def _native(self, live) -> bool:
        return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                   for p, m, v in live for t in (p, p.grad, m, v))

    @torch.no_grad()
    def step(self) -> None:
        g = self.param_groups[0]
        lr, (beta1, beta2), eps = g["lr"], g["betas"], g["eps"]
        live = [(p, m, v) for p, m, v in zip(self.params, self.m, self.v) if p.grad is not None]
        if live and self._native(live):
            stream = _lib.stream_handle(self.bias.device)
            chunks = [live[i:i + _lib.ADAM_MAX_SEG] for i in range(0, len(live), _lib.ADAM_MAX_SEG)]
            for k, chunk in enumerate(chunks):
                segs = (_lib.pob_adam_seg * len(chunk))()
                for s, (p, m, v) in zip(segs, chunk):
                    s.theta, s.grad, s.m, s.v, s.n = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
                # every chunk of a step reads the same products: only the last launch leaves them advanced
                bias = self.bias if k == len(chunks) - 1 else self.bias.clone()
                check(lib.pob_adam_step(segs, len(chunk), bias.data_ptr(), lr, beta1, beta2, eps, stream))
            return
        # adam_step_ref in torch ops (float32: its bits; other dtypes: the same order in that dtype)
        from .ppo import _fma
        p_new = self.bias * torch.tensor([beta1, beta2], dtype=torch.float32, device=self.bias.device).double()
        for p, m, v in live:
            dt, f32 = p.dtype, p.dtype == torch.float32
            fma = _fma if f32 else (lambda a, b, c: a * b + c)
            k = lambda x: torch.tensor(x, dtype=dt, device=p.device)  # noqa: E731
            b1, b2 = k(beta1), k(beta2)
            ic = 1.0 / (1.0 - p_new).to(device=p.device, dtype=dt)
            grad = p.grad.to(dt)
            m_new = fma(b1, m, (1.0 - b1) * grad)
            v_new = fma(b2, v, ((1.0 - b2) * grad) * grad)
            m_hat, v_hat = m_new * ic[0], v_new * ic[1]
            den = torch.sqrt(v_hat) + k(eps)
            p.copy_(fma(-k(lr), m_hat * (1.0 / den), p))
            m.copy_(m_new)
            v.copy_(v_new)
        self.bias.copy_(p_new)

    def state_dict(self) -> Dict:
        g = self.param_groups[0]
        return dict(state=dict(m=[t.clone() for t in self.m], v=[t.clone() for t in self.v], bias=self.bias.clone()),
                    param_groups=[dict(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"])])

    def load_state_dict(self, state: Dict) -> None:
        """Copies m, v and the bias block INTO the optimiser's own tensors (no storage moves)."""
        st = state["state"]
        if len(st["m"]) != len(self.m) or len(st["v"]) != len(self.v):
            raise ValueError(f"the state holds {len(st['m'])} moment pairs, the optimiser {len(self.m)} parameters")
        for mine, theirs in zip(self.m + self.v + [self.bias], list(st["m"]) + list(st["v"]) + [st["bias"]]):
            if tuple(mine.shape) != tuple(theirs.shape):
                raise ValueError(f"shape {tuple(theirs.shape)} does not fit {tuple(mine.shape)}")
        with torch.no_grad():
            for mine, theirs in zip(self.m + self.v + [self.bias], list(st["m"]) + list(st["v"]) + [st["bias"]]):
                mine.copy_(theirs)
        g = state["param_groups"][0]
        self.param_groups[0].update(lr=float(g["lr"]), betas=(float(g["betas"][0]), float(g["betas"][1])),
                                    eps=float(g["eps"]))


__all__ = ["FusedAdam"]
