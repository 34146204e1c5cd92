"""CPU: the public side of the wide training pass: ``apply_native(kernel=)``, ``backward="resident"`` on both
learners, and the argument checks of pob_mlp_forward_train_wide / pob_mlp_backward_wide (before any HIP call)."""
import ctypes as C

import pytest
import torch


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32)


def test_apply_native_kernel_keyword_on_cpu():
    from po_brax_amd.training import make_model
    model = make_model([9, 3], 6)
    p = model.init(_key(0))
    p.theta.requires_grad_(True)
    x = torch.rand((4, 6)) - 0.5
    for kernel in ("resident", "tile"):  # the torch ops run: the keyword selects nothing
        assert torch.equal(model.apply_native(p, x, kernel=kernel), model.apply_native(p, x))
    with pytest.raises(ValueError, match="kernel"):
        model.apply_native(p, x, kernel="bogus")


def test_learners_accept_resident():
    from po_brax_amd.training import PPOLearner, RecurrentPPOLearner
    for good in ("resident", ("native", "resident"), ("resident", "torch")):
        with pytest.raises(TypeError, match="NormalTanhPolicy"):  # past the keyword's check
            PPOLearner(None, None, key=_key(0), backward=good)
    with pytest.raises(ValueError, match="backward"):
        PPOLearner(None, None, key=_key(0), backward=("native", "wide"))
    # the recurrent learner checks its networks' types first: bare instances, and no key, which it asks for next
    from po_brax_amd.training import RecurrentValueFunction, ValueFunction
    from po_brax_amd.training.networks import RecurrentTanhPolicy
    policy, ff, gru = (c.__new__(c) for c in (RecurrentTanhPolicy, ValueFunction, RecurrentValueFunction))
    with pytest.raises(ValueError, match="key is required"):
        RecurrentPPOLearner(policy, ff, backward=("native", "resident"))
    for critic, bad in ((ff, ("native", "wide")), (ff, ("resident", "torch")), (ff, "resident"), (gru, ("native", "resident"))):
        with pytest.raises(ValueError, match="backward must"):
            RecurrentPPOLearner(policy, critic, backward=bad)


def test_wide_training_entry_points_reject_bad_arguments():
    from po_brax_amd import _lib
    from po_brax_amd.training.networks import MLPHandle
    lib, mlp = _lib.lib, MLPHandle([27, 33, 16], 1, False)
    h = mlp.handle
    p = C.cast((C.c_float * 64)(), C.c_void_p)  # never dereferenced
    for bad in ((None, 4, p, p, p, p), (h, 0, p, p, p, p), (h, -3, p, p, p, p), (h, 2 ** 31 // 33 - 1024, p, p, p, p),
                (h, 4, None, p, p, p), (h, 4, p, None, p, p), (h, 4, p, p, None, p), (h, 4, p, p, p, None)):
        assert lib.pob_mlp_forward_train_wide(*bad, None) == _lib.POB_EINVAL, bad  # mlp, M, x, theta, y, saved
    for bad in ((None, 4, p, p, p, p, p, p), (h, 0, p, p, p, p, p, p), (h, 4, None, p, p, p, p, p), (h, 4, p, None, p, p, p, p),
                (h, 4, p, p, None, p, p, p), (h, 4, p, p, p, None, p, p), (h, 4, p, p, p, p, None, p), (h, 4, p, p, p, p, p, None)):
        with pytest.raises(ValueError, match="mlp"):  # mlp, M, x, theta, saved, dy, dtheta, (dx,) workspace
            _lib.check(lib.pob_mlp_backward_wide(*bad[:7], None, bad[7], None))
    assert _lib.ABI_VERSION == 8 and lib.pob_abi_version() == 8
