"""CPU: the bf16 forward's argument checks and workspace size; ``apply(kernel="bf16")`` in torch ops is the definition."""
import ctypes as C

import pytest
import torch

TOL = 5.8e-3  # DESIGN.md "Bf16 forward": 4 x 1.45e-3, the torch-op path's largest error over the GPU tests' cases


def reference(sizes, act, x, theta, hidden=None):
    """The definition in float64; ``hidden`` (a list) receives the rounded hidden activations."""
    fn = (torch.relu, torch.nn.functional.silu, torch.tanh)[act]
    r = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    h, off = r(x.float()), 0
    for i, (n_in, n_out) in enumerate(zip(sizes[:-1], sizes[1:])):
        W, b = theta[off:off + n_in * n_out].view(n_in, n_out), theta[off + n_in * n_out:off + (n_in + 1) * n_out]
        off += (n_in + 1) * n_out
        h = b.double() + h @ r(W)
        if i != len(sizes) - 2:
            h = r(fn(h).float())
            if hidden is not None:
                hidden.append(h)
    return h


def metric(y, want):
    return float((y.double() - want).abs().max() / max(1.0, float(want.abs().max())))


def test_bf16_entry_points_reject_bad_arguments():
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import MLPHandle
    mlp = MLPHandle([5, 7, 2], 1, False)
    h, n = mlp.handle, C.c_longlong()
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    for bad in ((None, 4, p, p, p, p), (h, 0, p, p, p, p), (h, -3, p, p, p, p), (h, 4, None, p, p, p), (h, 4, p, None, p, p),
                (h, 4, p, p, None, p), (h, 4, p, p, p, None)):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib.pob_mlp_forward_bf16(*bad, None))
        with pytest.raises(ValueError):
            _lib.check(_lib.lib.pob_mlp_forward_bf16_norm(*bad[:5], p, 1.0, bad[5], None))
    assert b"mlp" in _lib.lib.pob_last_error()
    for bad in ((None, C.byref(n)), (h, None)):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib.pob_mlp_bf16_workspace_bytes(*bad))


@pytest.mark.parametrize("sizes", [[5, 7, 2], [114, 256, 256, 256, 256, 256, 1]])
def test_bf16_workspace_bytes(sizes):
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import MLPHandle
    mlp, n = MLPHandle(sizes, 0, False), C.c_longlong()
    _lib.check(_lib.lib.pob_mlp_bf16_workspace_bytes(mlp.handle, C.byref(n)))
    assert n.value == sum(-(-a // 16) * 16 * -(-b // 32) * 32 * 2 for a, b in zip(sizes[:-1], sizes[1:]))


def test_apply_bf16_on_cpu_is_the_definition_and_has_no_training_pass():
    from po_brax_amd.training import networks
    model = networks.make_model([160, 256, 1], 114)
    p = model.init(torch.tensor([0, 7], dtype=torch.uint32))
    x = torch.randn((65, 114), generator=torch.Generator().manual_seed(5))
    y = model.apply(p, x, kernel="bf16")
    assert metric(y, reference(model.layer_sizes, model.activation, x, p.theta)) <= TOL
    assert not torch.equal(y, model.apply(p, x, kernel="tile"))  # not silently f32
    with pytest.raises(ValueError, match="kernel"):
        networks.train_entries("bf16")
    with pytest.raises(ValueError, match="kernel"):
        model.apply_native(p, x, kernel="bf16")
