"""CPU: pob_mlp_forward_wide / _norm reject bad arguments before any HIP call; ``apply(kernel=)`` where the torch ops run."""
import ctypes as C

import pytest
import torch


def test_wide_entry_points_reject_bad_arguments():
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import MLPHandle
    mlp = MLPHandle([5, 7, 2], 1, False)
    h = mlp.handle
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    plain, norm = _lib.lib.pob_mlp_forward_wide, _lib.lib.pob_mlp_forward_wide_norm
    for bad in ((None, 4, p, p, p), (h, 0, p, p, p), (h, -3, p, p, p), (h, 4, None, p, p), (h, 4, p, None, p),
                (h, 4, p, p, None)):
        with pytest.raises(ValueError):
            _lib.check(plain(*bad, None))
        with pytest.raises(ValueError):
            _lib.check(norm(*bad, p, 1.0, None))
    assert b"mlp" in _lib.lib.pob_last_error()


def test_apply_kernel_keyword_on_cpu():
    from po_brax_amd.training import networks
    model = networks.make_model([9, 3], 6)
    p = model.init(torch.tensor([0, 7], dtype=torch.uint32))
    x = torch.rand((4, 6)) - 0.5
    assert torch.equal(model.apply(p, x, kernel="resident"), model.apply(p, x, kernel="tile"))
    assert torch.equal(model.apply(p, x), model.apply(p, x, kernel="tile"))
    with pytest.raises(ValueError, match="kernel"):
        model.apply(p, x, kernel="bogus")
