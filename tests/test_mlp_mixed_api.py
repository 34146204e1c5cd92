"""CPU: the mixed-precision training pass (``kernel="mixed"``): its torch-op form against the float64 statement of
the definition."""
import pytest
import torch

# DESIGN.md "Mixed training pass": 4 x the largest error of the torch-op path on the CPU over 45 random cases (three
# activations x the four networks of tests/test_gpu_mlp_bf16.py and one with the last layer activated x M = 1, 65, 161;
# per tensor: max|g - ref| / max|ref|; y: max|y - ref| / max(1, max|ref|)).  Measured: y 2.867e-3, gradients
# 2.646e-3 (both eight layers of 40, M = 161: one flipped bf16 tie; 30 of the 45 cases are below 3e-7).  For scale, the
# same metric between the mixed gradient and the float64 gradient of the unrounded network: 2.6e-3 .. 1.7e-2 for swish
# and tanh, up to 0.97 for relu (a unit's mask flips at M = 1).
TOL = 1.15e-2


def reference(sizes, act, x, theta, dy, act_final=False):
    """y, dtheta, dx of the definition in float64."""
    fn = (torch.relu, torch.nn.functional.silu, torch.tanh)[act]
    r = lambda t: t.float().to(torch.bfloat16).double()  # noqa: E731
    n, off, hs, zs, Ws = len(sizes) - 1, 0, [r(x)], [], []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        Ws.append(r(theta[off:off + a * b].view(a, b)))
        bias = theta[off + a * b:off + (a + 1) * b].double()
        off += (a + 1) * b
        zs.append(bias + hs[-1] @ Ws[-1])
        hs.append(r(fn(zs[-1])) if i != n - 1 else (fn(zs[-1]) if act_final else zs[-1]))
    y, g, parts = hs.pop(), dy.double(), []
    for i in reversed(range(n)):
        if i != n - 1 or act_final:
            z = zs[i]  # mlp_activate_grad of csrc/pob_mlp.h: relu' is 0 at z = 0
            s, t = torch.sigmoid(z), torch.tanh(z)
            g = (torch.where(z > 0, g, 0 * g), g * (s + z * s * (1 - s)), g * (1 - t * t))[act]
        d = r(g)
        parts[:0] = [(hs[i].t() @ d).ravel(), d.sum(0)]
        g = d @ Ws[i].t()
    return y, torch.cat(parts), g


def metrics(sizes, y, dtheta, dx, want):
    """The largest error of y (DESIGN.md "Bf16 forward"'s metric) and of the gradients, per tensor: each dW, db, dx."""
    rel = lambda g, w: float((g.double() - w).abs().max() / max(float(w.abs().max()), 1e-30))  # noqa: E731
    ey = float((y.double() - want[0]).abs().max() / max(1.0, float(want[0].abs().max())))
    eg, off = rel(dx, want[2]) if dx is not None else 0.0, 0
    for a, b in zip(sizes[:-1], sizes[1:]):
        for n in (a * b, b):
            eg = max(eg, rel(dtheta[off:off + n], want[1][off:off + n]))
            off += n
    return ey, eg


def _key(seed):
    return torch.tensor([seed, 12345 + seed], dtype=torch.uint32)


@pytest.mark.parametrize("act", ["relu", "swish", "tanh"])
def test_mixed_torch_ops_are_the_definition(act):
    from po_brax_amd.training import networks
    model = networks.make_model([160, 256, 1], 114, activation=act)
    p = model.init(_key(3))
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn((65, 114), generator=g).requires_grad_(True), torch.randn((65, 1), generator=g)
    theta = p.theta.clone().requires_grad_(True)
    params = networks.Params(theta, model.layer_sizes)
    y = model.apply_native(params, x, kernel="mixed")
    y.backward(dy)
    want = reference(model.layer_sizes, model.activation, x.detach(), p.theta, dy)
    ey, eg = metrics(model.layer_sizes, y.detach(), theta.grad, x.grad, want)
    assert ey <= TOL and eg <= TOL, (ey, eg)
    assert torch.equal(y.detach(), model.apply(p, x.detach(), kernel="bf16"))  # the values of the bf16 forward
    assert torch.equal(model.apply_native(p, x.detach(), kernel="mixed"), y.detach())  # without grad: apply(kernel="bf16")
    t32 = p.theta.clone().requires_grad_(True)
    model.apply_native(networks.Params(t32, model.layer_sizes), x.detach()).backward(dy)
    assert not torch.equal(t32.grad, theta.grad)  # not silently the f32 path
    views = {k: {n: t.detach().clone().requires_grad_(True) for n, t in v.items()} for k, v in p.items()}
    model.apply_native(views, x.detach(), kernel="mixed").backward(dy)  # the dict-of-views form: the same function
    n = 114 * 160
    assert torch.equal(views["hidden_0"]["kernel"].grad.ravel(), theta.grad[:n])
    assert torch.equal(views["hidden_0"]["bias"].grad, theta.grad[n:n + 160])


def test_mixed_keyword():
    from po_brax_amd.training import networks
    with pytest.raises(ValueError, match="kernel"):  # no entry points: the definition only
        networks.train_entries("mixed")
    with pytest.raises(ValueError, match="kernel"):
        networks.make_model([3], 2).apply_native(None, torch.zeros(1, 2), kernel="Mixed")
