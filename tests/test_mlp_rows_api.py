"""CPU: the public side of the row-indexed training pass (DESIGN.md "Row-indexed training pass"):
``apply_native(idx=, normalizer=)`` off the kernel path, the argument checks of the ``pob_mlp_*_rows`` entries
(made before any HIP call), and the host restatement against the existing one on materialised rows."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from test_mlp_bwd_host import (CSRC, HERE, SWISH, _p, _sizes, build_mlp_bwd_host, make_problem, param_count,
                               ref_train_and_back, same_bits)


class _Norm:
    """``ObservationNormalizer``'s table, clip and ``apply`` on the host (the real one lives on the GPU)."""

    def __init__(self, rng, D):
        mean, scale = rng.standard_normal(D), rng.uniform(0.5, 4.0, D)
        self.table, self.clip = torch.from_numpy(np.stack([mean, scale, np.ones(D)]).astype(np.float32)), 5.0

    def apply(self, obs):
        return torch.clamp((obs - self.table[0]) * self.table[1], -self.clip, self.clip)


def _case(rng, D, M, N):
    x = rng.uniform(-3.0, 3.0, (N, D)).astype(np.float32)
    idx = rng.integers(0, N, M).astype(np.int32)
    idx[:3] = (0, N - 1, N - 1)
    return x, idx, _Norm(rng, D)


def test_torch_fallback_and_value_errors():
    from po_brax_amd.training import make_model
    x, idx, norm = _case(np.random.default_rng(0), 5, 9, 28)
    model = make_model([7, 2], 5)
    theta = model.init(torch.tensor([1, 2], dtype=torch.uint32)).theta
    x, idx = torch.from_numpy(x), torch.from_numpy(idx)
    for kw in (dict(idx=idx, normalizer=norm), dict(idx=idx), dict(normalizer=norm)):
        rows = x if "idx" not in kw else x[idx.long()]
        rows = norm.apply(rows) if "normalizer" in kw else rows
        got, want = (theta.clone().requires_grad_(True) for _ in range(2))
        y = model.apply_native(types.SimpleNamespace(theta=got), x, **kw)
        y_want = model.apply(types.SimpleNamespace(theta=want), rows)
        y.sum().backward()
        y_want.sum().backward()
        assert torch.equal(y, y_want) and torch.equal(got.grad, want.grad)
        with torch.no_grad():
            assert torch.equal(model.apply_native(types.SimpleNamespace(theta=got), x, **kw), y_want)
        with pytest.raises(ValueError, match="no gradient to x"):
            model.apply_native(types.SimpleNamespace(theta=got), x.clone().requires_grad_(True), **kw)
        with pytest.raises(ValueError, match="mixed"):
            model.apply_native(types.SimpleNamespace(theta=got), x, kernel="mixed", **kw)


def test_exports_and_argument_checks():
    """POB_EINVAL (a ValueError through check) for N < 1, NULL pointers and dx with idx or norm: all before any HIP call,
    so the addresses are never read."""
    from po_brax_amd import _lib
    from po_brax_amd._lib import check, lib
    from po_brax_amd.training.networks import MLPHandle
    mlp = MLPHandle([5, 7, 2], SWISH)  # kept: the handle dies with it
    h, a = mlp.handle, 4096  # a: a stand-in for every address
    for names in (("pob_mlp_forward_train_rows", "pob_mlp_backward_rows"),
                  ("pob_mlp_forward_train_wide_rows", "pob_mlp_backward_wide_rows")):
        assert all(name in _lib.EXPORTS for name in names)
        fwd, bwd = (getattr(lib, name) for name in names)
        for M, N in ((4, 0), (4, -1), (0, 4)):
            with pytest.raises(ValueError):
                check(fwd(h, M, N, a, a, a, a, a, a, 5.0, None))
            with pytest.raises(ValueError):
                check(bwd(h, M, N, a, a, a, a, a, a, None, a, 5.0, a, None))
        for missing in range(6):  # forward: x, theta, y, saved; backward: x, theta, saved, dy, dtheta, workspace
            p = [None if k == missing else a for k in range(6)]
            if missing < 4:
                with pytest.raises(ValueError, match="NULL argument"):
                    check(fwd(h, 4, 9, p[0], a, p[1], p[2], p[3], a, 5.0, None))
            with pytest.raises(ValueError, match="NULL argument"):
                check(bwd(h, 4, 9, p[0], a, p[1], p[2], p[3], p[4], None, a, 5.0, p[5], None))
        for idx, norm in ((a, None), (None, a)):
            with pytest.raises(ValueError, match="no dx"):
                check(bwd(h, 4, 9, a, idx, a, a, a, a, a, norm, 5.0, a, None))


@pytest.mark.parametrize("sizes", [[5, 7, 6, 2], [114, 256, 1]])
def test_host_rows_ref_equals_the_refs_on_materialised_rows(tmp_path, sizes):
    so = os.path.join(str(tmp_path), "mlp_rows_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared", "-o", so,
                           os.path.join(HERE, "host", "mlp_rows_host.cpp")])
    rows_lib, host = C.CDLL(so), build_mlp_bwd_host(tmp_path)
    rng, M = np.random.default_rng(2), 37
    x, idx, norm = _case(rng, sizes[0], M, 112)
    _, theta, dy = make_problem(rng, sizes, M)
    want = ref_train_and_back(host, sizes, SWISH, 0, norm.apply(torch.from_numpy(x[idx])).numpy(), theta, dy, want_dx=False)
    y, saved = np.full_like(want["y"], np.nan), np.full_like(want["saved"], np.nan)
    dtheta = np.full(param_count(sizes), np.nan, np.float32)
    table = np.ascontiguousarray(norm.table.numpy())
    head = (len(sizes) - 1, _sizes(sizes), SWISH, 0, C.c_longlong(M), _p(x), _p(idx, C.POINTER(C.c_int32)), _p(table),
            C.c_float(norm.clip), _p(theta))
    assert rows_lib.mlp_rows_ref_forward_train(*head, _p(y), _p(saved)) == 0
    assert rows_lib.mlp_rows_ref_backward(*head, _p(saved), _p(dy), _p(dtheta)) == 0
    assert same_bits(y, want["y"]) and same_bits(saved, want["saved"]) and same_bits(dtheta, want["dtheta"])
