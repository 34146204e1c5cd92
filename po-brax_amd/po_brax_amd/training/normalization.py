"""Running observation normaliser (brax <= 0.0.12 ``training/normalization.py``:
``create_observation_normalizer``), fused into the native actors.

The state lives on the device: ``count`` (float64, 1 element) and ``table`` (float32, (3, D):
``mean``, ``scale``, ``m2``).  The actor kernels read ``mean`` / ``scale`` at launch time and
feed the network ``clip((obs - mean) * scale, +-clip)`` straight from the observation tile they
load anyway (``pob_*_norm``); ``update`` folds observation rows into the statistics with one
streaming reduction and a one-block finish (``pob_obsnorm_accumulate`` / ``pob_obsnorm_update``),
in place, stream-ordered and capturable.  Formulas, summation order and what is pinned:
DESIGN.md "Observation normaliser".
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from .._lib import check, lib, ptr

MAX_WIDTH = 256


class ObservationNormalizer:
    """``count``, ``table`` and the update's buffers for observations of width ``obs_size``.

        norm = ObservationNormalizer(env.observation_size)
        policy = NormalTanhPolicy(model, params, key, normalizer=norm)   # acts on apply(obs)
        norm.update(roll.obs)                                            # any leading dims

    ``mean``, ``scale`` (= 1 / std) and ``m2`` (the running variance sum) are views into
    ``table``.  A fresh normaliser is the identity up to the clamp.  ``clip=0`` turns the clamp
    off (brax's ``apply_clipping=False``)."""

    def __init__(self, obs_size: int, clip: float = 5.0, device=None):
        obs_size = int(obs_size)
        if not 1 <= obs_size <= MAX_WIDTH:
            raise ValueError(f"obs_size must be in 1 .. {MAX_WIDTH}, got {obs_size}")
        if not float(clip) >= 0.0:
            raise ValueError("clip must be >= 0 (0: no clamp)")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise ValueError("the observation normaliser lives on the GPU (no CPU fallback)")
        self.count = torch.zeros(1, dtype=torch.float64, device=dev)
        dev = self.count.device  # with its index
        self.obs_size, self.clip, self.device = obs_size, float(clip), dev
        self.table = torch.zeros((3, obs_size), dtype=torch.float32, device=dev)
        self.table[1:].fill_(1.0)
        self.sums = torch.zeros((2, obs_size), dtype=torch.float64, device=dev)
        self._workspace = None

    @property
    def mean(self) -> torch.Tensor:
        return self.table[0]

    @property
    def scale(self) -> torch.Tensor:
        return self.table[1]

    @property
    def m2(self) -> torch.Tensor:
        return self.table[2]

    def reserve(self, n_rows: int) -> None:
        """Size the chunk-partial workspace for updates of up to ``n_rows`` rows (an allocation:
        call it before a capture; ``update`` outside a capture does it itself)."""
        need = C.c_longlong()
        check(lib.pob_obsnorm_workspace_bytes(int(n_rows), self.obs_size, C.byref(need)))
        if self._workspace is None or self._workspace.numel() * 8 < need.value:
            self._workspace = torch.empty(need.value // 8, dtype=torch.float64, device=self.device)

    def _rows(self, obs: torch.Tensor) -> torch.Tensor:
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.dim() >= 1 and obs.shape[-1] == self.obs_size
                and obs.device == self.table.device):
            raise ValueError(f"obs must be a float32 tensor (..., {self.obs_size}) on {self.table.device}")
        x = obs.detach().reshape(-1, self.obs_size)
        if not x.is_contiguous():
            x = x.contiguous()
        if x.shape[0] < 1:
            raise ValueError("obs has no rows")
        return x

    def accumulate(self, obs: torch.Tensor) -> torch.Tensor:
        """``self.sums`` (2, D) float64 <- sum d, sum d^2 of the rows against the current mean."""
        x = self._rows(obs)
        if not torch.cuda.is_current_stream_capturing():
            self.reserve(x.shape[0])
        need = C.c_longlong()
        check(lib.pob_obsnorm_workspace_bytes(x.shape[0], self.obs_size, C.byref(need)))
        if self._workspace is None or self._workspace.numel() * 8 < need.value:
            raise RuntimeError("reserve(n_rows) before capturing an update")
        check(lib.pob_obsnorm_accumulate(ptr(x), x.shape[0], self.obs_size, ptr(self.table), ptr(self._workspace),
                                         ptr(self.sums), _lib.stream_handle(self.device)))
        return self.sums

    def update(self, obs: torch.Tensor, group=None) -> "ObservationNormalizer":
        """Fold the rows of ``obs`` (..., D) into the statistics, in place and stream-ordered.
        ``group is None``: two launches for the sums and one for the finish, capturable.  With a
        ``torch.distributed`` group every rank's (2, D) sums and row count are all-gathered and
        the update runs from all of them in rank order, so every rank ends with the same table
        bit for bit (the ranks must start from the same one); not capturable."""
        n = self._rows(obs).shape[0]
        self.accumulate(obs)
        if group is None:
            sums, R, n_new = self.sums, 1, n
        else:
            import torch.distributed as dist
            R = dist.get_world_size(group)
            sums = torch.empty((R, 2, self.obs_size), dtype=torch.float64, device=self.device)
            dist.all_gather_into_tensor(sums, self.sums, group=group)
            counts = torch.empty(R, dtype=torch.int64, device=self.device)
            dist.all_gather_into_tensor(counts, torch.tensor([n], dtype=torch.int64, device=self.device), group=group)
            n_new = int(counts.sum().item())
        check(lib.pob_obsnorm_update(ptr(self.count), ptr(self.table), self.obs_size, ptr(sums), R, n_new,
                                     _lib.stream_handle(self.device)))
        return self

    def apply(self, obs: torch.Tensor) -> torch.Tensor:
        """``clip((obs - mean) * scale, +-clip)`` in torch ops (differentiable in ``obs``): one
        rounded subtract and one rounded multiply, the values the kernels stage."""
        t = (obs - self.mean) * self.scale
        return torch.clamp(t, -self.clip, self.clip) if self.clip > 0.0 else t

    def state_dict(self) -> dict:
        return {"count": self.count.clone(), "table": self.table.clone(), "clip": self.clip}

    def load_state_dict(self, state: dict) -> None:
        table, count = torch.as_tensor(state["table"]), torch.as_tensor(state["count"])
        if tuple(table.shape) != (3, self.obs_size):
            raise ValueError(f"table must be (3, {self.obs_size})")
        self.table.copy_(table.to(torch.float32))  # in place: a captured graph keeps reading this buffer
        self.count.copy_(count.to(torch.float64).reshape(1))
        self.clip = float(state.get("clip", self.clip))


def create_observation_normalizer(obs_size: int, normalize_observations: bool = True, apply_clipping: bool = True,
                                  device=None):
    """brax's spelling: ``(data, update_fn, apply_fn)``.  ``data`` is the ``ObservationNormalizer``
    (None without normalisation); ``update_fn(data, obs)`` updates it in place and returns it;
    ``apply_fn(data, obs)`` normalises.  ``normalize_observations=False``: identity functions."""
    if not normalize_observations:
        return None, (lambda data, obs, *a, **k: data), (lambda data, obs: obs)
    data = ObservationNormalizer(obs_size, clip=5.0 if apply_clipping else 0.0, device=device)
    return data, (lambda d, obs, group=None: d.update(obs, group)), (lambda d, obs: d.apply(obs))


def attach(normalizer: Optional[ObservationNormalizer], obs_size: int, device) -> Optional[ObservationNormalizer]:
    """The check a policy makes on its ``normalizer=`` argument."""
    if normalizer is None:
        return None
    if not isinstance(normalizer, ObservationNormalizer):
        raise TypeError("normalizer must be a training.normalization.ObservationNormalizer")
    if normalizer.obs_size != obs_size:
        raise ValueError(f"the normaliser is for observations of width {normalizer.obs_size}, the policy's are {obs_size}")
    if normalizer.table.device != device:
        raise ValueError(f"the normaliser is on {normalizer.table.device}, the policy on {device}")
    return normalizer
