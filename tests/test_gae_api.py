"""CPU: the public GAE interface (po_brax_amd.training.gae) and the argument checks of pob_gae.

``compute_gae`` on CPU tensors takes the torch-op spelling; it is compared with ``gae_ref`` in the
bound form of test_gae_host.py with the restatement as the reference: max |torch - ref| <= 4 x max
|f32 numpy - f64| + ulp32(max |f64|) (the torch spelling rounds each product and sum separately,
like the float32 numpy spelling of brax's formula, so it carries errors of that size)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gae_host import brax_gae, build_gae_host, ref_gae, trajectory, ulp32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_gae_host(tmp_path_factory.mktemp("gae_host_api"))


def _tensors(d):
    return [torch.from_numpy(d[k]) for k in ("trunc", "term", "reward", "values", "boot")]


@pytest.mark.parametrize("T,lam,disc,scale", [(1, 0.95, 0.99, 1.0), (20, 0.95, 0.99, 0.1), (33, 1.0, 1.0, 1.0), (7, 0.0, 0.99, 2.0)])
def test_compute_gae_on_cpu_tensors(host, T, lam, disc, scale):
    from po_brax_amd.training import compute_gae
    d = trajectory(np.random.default_rng(T), T, 65)
    out = compute_gae(*_tensors(d), lambda_=lam, discount=disc, reward_scaling=scale)
    assert isinstance(out, tuple) and len(out) == 2
    want = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], scale, d["values"], d["boot"], lam, disc)
    scaled = d["reward"] * np.float32(scale)
    f64 = brax_gae(d["trunc"], d["term"], scaled, d["values"], d["boot"], lam, disc, np.float64)
    f32 = brax_gae(d["trunc"], d["term"], scaled, d["values"], d["boot"], lam, disc, np.float32)
    for k, name in enumerate(("vs", "advantages")):
        got = out[k].numpy()
        assert got.dtype == np.float32 and got.shape == (T, 65)
        err = float(np.abs(got.astype(np.float64) - want[k].astype(np.float64)).max())
        bound = 4.0 * float(np.abs(f32[k].astype(np.float64) - f64[k]).max()) + ulp32(np.abs(f64[k]).max())
        print(f"T {T} {name}: torch spelling against gae_ref {err:.3e} bound {bound:.3e}")
        assert err <= bound, name


def test_return_order_and_no_grad():
    """(vs, advantages), in brax's order: at a truncated step vs == values and advantages == 0."""
    from po_brax_amd.training import compute_gae
    d = trajectory(np.random.default_rng(3), 20, 33)
    trunc, term, reward, values, boot = _tensors(d)
    values.requires_grad_(True)
    boot.requires_grad_(True)
    vs, adv = compute_gae(trunc, term, reward, values, boot)
    cut = trunc != 0
    assert bool(cut.any()) and bool((vs[cut] == values.detach()[cut]).all()) and bool((adv[cut] == 0).all())
    assert not vs.requires_grad and not adv.requires_grad and vs.grad_fn is None and adv.grad_fn is None
    # float64 inputs keep their dtype on the torch path
    vs64, adv64 = compute_gae(*[t.detach().double() for t in (trunc, term, reward, values, boot)])
    assert vs64.dtype == torch.float64 and adv64.dtype == torch.float64
    torch.testing.assert_close(vs64.float(), vs, rtol=1e-5, atol=1e-3)
    # out= is written and returned
    bufs = (torch.empty(20, 33), torch.empty(20, 33))
    got = compute_gae(trunc, term, reward, values.detach(), boot.detach(), out=bufs)
    assert got[0] is bufs[0] and got[1] is bufs[1] and torch.equal(bufs[0], vs) and torch.equal(bufs[1], adv)


def test_shape_and_dtype_errors():
    from po_brax_amd.training import compute_gae
    d = trajectory(np.random.default_rng(4), 5, 9)
    trunc, term, reward, values, boot = _tensors(d)
    with pytest.raises(ValueError, match="rewards"):
        compute_gae(trunc, term, reward[:4], values, boot)
    with pytest.raises(ValueError, match="truncation"):
        compute_gae(trunc[:, :8], term, reward, values, boot)
    with pytest.raises(ValueError, match="bootstrap_value"):
        compute_gae(trunc, term, reward, values, boot[:8])
    with pytest.raises(ValueError, match="values"):
        compute_gae(trunc[0], term[0], reward[0], values[0], boot)
    with pytest.raises(TypeError, match="termination"):
        compute_gae(trunc, term.bool(), reward, values, boot)
    with pytest.raises(TypeError, match="rewards"):
        compute_gae(trunc, term, reward.double(), values, boot)
    with pytest.raises(TypeError, match="values"):
        compute_gae(trunc, term, reward, values.numpy(), boot)
    with pytest.raises(ValueError, match=r"out\[1\]"):
        compute_gae(trunc, term, reward, values, boot, out=(torch.empty(5, 9), torch.empty(5, 8)))


def test_pob_gae_rejects_bad_arguments_without_a_gpu():
    from po_brax_amd import _lib
    lib = _lib.lib
    a = np.zeros((2, 3), np.float32)
    p = a.ctypes.data_as(C.c_void_p)  # never dereferenced: every call below is rejected before any HIP call
    ok = dict(T=2, B=3, trunc=p, second=p, reward=p, values=p, boot=p, vs=p, adv=p)

    def call(**kw):
        k = {**ok, **kw}
        return lib.pob_gae(k["T"], k["B"], k["trunc"], k["second"], 1, k["reward"], 1.0, k["values"], k["boot"], 0.95, 0.99,
                           k["vs"], k["adv"], None)

    for kw, word in ((dict(T=0), "T"), (dict(T=-1), "T"), (dict(B=0), "B"), (dict(second=None), "NULL"),
                     (dict(reward=None), "NULL"), (dict(values=None), "NULL"), (dict(boot=None), "NULL"),
                     (dict(vs=None, adv=None), "both NULL")):
        assert call(**kw) != 0, kw
        msg = lib.pob_last_error().decode()
        assert msg.startswith("gae:") and word in msg, (kw, msg)
        with pytest.raises(ValueError, match="gae:"):
            _lib.check(call(**kw))
    assert "pob_gae" in _lib.EXPORTS and _lib.ABI_VERSION == 8 and lib.pob_abi_version() == 8


def test_value_function_checks():
    from po_brax_amd import jumpy  # noqa: F401
    from po_brax_amd.training import ValueFunction, make_model, make_models
    from po_brax_amd.training.normalization import ObservationNormalizer
    D = 14
    policy_model, value_model = make_models(16, D)
    assert value_model.layer_sizes == (D, 256, 256, 256, 256, 256, 1)
    key = torch.tensor([0, 1], dtype=torch.uint32)
    with pytest.raises(ValueError, match="last width must be 1"):
        ValueFunction(policy_model, policy_model.init(key))
    with pytest.raises(ValueError, match="last width must be 1"):
        ValueFunction(make_model([8, 2], D), make_model([8, 2], D).init(key))
    # a normaliser of another width (its device state needs a GPU: only the fields the check reads)
    norm = ObservationNormalizer.__new__(ObservationNormalizer)
    norm.obs_size, norm.table = D + 1, torch.zeros((3, D + 1))
    small = make_model([8, 1], D)
    with pytest.raises(ValueError, match="width"):
        ValueFunction(small, small.init(key), normalizer=norm)
    with pytest.raises(TypeError, match="ObservationNormalizer"):
        ValueFunction(small, small.init(key), normalizer=object())
    # parameters on the host: the native path has no CPU fallback
    with pytest.raises(ValueError, match="CUDA"):
        ValueFunction(small, small.init(key))


def test_rollout_gae_options():
    from po_brax_amd.training.gae import gae_options
    assert gae_options(None) == {"lambda_": 0.95, "discount": 0.99, "reward_scaling": 1.0}
    assert gae_options({"discount": 0.9})["discount"] == 0.9 and gae_options({"discount": 0.9})["lambda_"] == 0.95
    with pytest.raises(ValueError, match="gamma"):
        gae_options({"gamma": 0.9})
