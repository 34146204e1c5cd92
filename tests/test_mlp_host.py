"""CPU: the shared scalar math and the restatement of the policy-network kernels
(po-brax_amd/csrc/pob_mlp.h, built for the host by tests/host/mlp_host.cpp).

Scalar functions: max error in ulp against float64 numpy / scipy on fixed grids, bounded by
2 x (the error of glibc's float32 function on the same grid) + 1 ulp -- what a table-free
polynomial is allowed.  erfinv has no glibc function: its yardstick is scipy's float32 erfinv.
mlp_forward_ref: max abs error against the float64 forward, bounded by 4 x (the error of torch's
CPU float32 forward of the same network and inputs) + 1e-7; the 4 x covers a different but
fixed summation order and the polynomial activations.
The stand-alone program (-DMLP_MAIN) runs once under -fsanitize=address,undefined.

Measured (this grid, x86-64 glibc 2.35), ours / yardstick in ulp: see DESIGN.md "Policy
networks"; the test prints each figure before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "mlp_host.cpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
WHICH = {"exp": 0, "log": 1, "tanh": 2, "softplus": 3, "sigmoid": 4, "swish": 5, "erfinv": 6}


def build_host(d):
    so = os.path.join(str(d), "mlp_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    lib.mlp_scalar.argtypes = [C.c_int, C.c_longlong, FP, FP]
    lib.mlp_scalar_libm.argtypes = [C.c_int, C.c_longlong, FP, FP]
    lib.mlp_ref_param_count.argtypes = [C.c_int, IP]
    lib.mlp_ref_param_count.restype = C.c_longlong
    lib.mlp_ref_forward.argtypes = [C.c_int, IP, C.c_int, C.c_int, C.c_int, FP, FP, FP]
    lib.mlp_ref_head.argtypes = [C.c_int, C.c_int, FP, FP, C.c_int, FP, FP, FP]
    lib.mlp_ref_kfeat.argtypes = [C.c_int, C.c_int]
    return lib


def fp(a):
    return a.ctypes.data_as(FP)


def ref_forward(lib, sizes, act, act_final, x, theta):
    """mlp_forward_ref on numpy arrays: x (B, sizes[0]) float32, theta flat float32."""
    x = np.ascontiguousarray(x, np.float32)
    theta = np.ascontiguousarray(theta, np.float32)
    sz = np.asarray(sizes, np.int32)
    assert theta.size == lib.mlp_ref_param_count(len(sizes) - 1, sz.ctypes.data_as(IP))
    y = np.empty((x.shape[0], sizes[-1]), np.float32)
    rc = lib.mlp_ref_forward(len(sizes) - 1, sz.ctypes.data_as(IP), act, int(act_final), x.shape[0], fp(x), fp(theta), fp(y))
    assert rc == 0
    return y


def ref_head(lib, logits, u, deterministic=False):
    """policy_head_ref: logits (B, 2A), u (B, A) -> action, logp, raw."""
    logits = np.ascontiguousarray(logits, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    B, A = u.shape
    action, raw = np.empty((B, A), np.float32), np.empty((B, A), np.float32)
    logp = np.full(B, np.nan, np.float32)
    lib.mlp_ref_head(B, A, fp(logits), fp(u), int(deterministic), fp(action), fp(logp), fp(raw))
    return action, logp, raw


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("mlp_host"))


def _floats_between(lo, hi, step=256):
    """Every step-th float32 of [lo, hi] (0 < lo < hi), ascending."""
    a, b = np.float32(lo).view(np.uint32), np.float32(hi).view(np.uint32)
    return np.arange(int(a), int(b) + 1, step, dtype=np.uint32).view(np.float32)


def _dense(hi=30.0):
    p = _floats_between(2.0 ** -126, hi)
    return np.concatenate([-p[::-1], np.zeros(1, np.float32), p])


def _ulp_err(y, exact):
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(y.astype(np.float64) - exact) / ulp))


def _grids():
    from scipy import special
    d30 = _dense(30.0)
    d88 = np.concatenate([d30, _floats_between(30.0, 88.0), -_floats_between(30.0, 88.0)])
    sp64 = lambda x: np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))  # noqa: E731
    one = np.float32(1.0)
    near = one - np.arange(1, 1 << 16, dtype=np.float32) * np.float32(2.0 ** -24)  # 1 - 2^-24 .. in 2^-24 steps
    inner = _floats_between(2.0 ** -126, 1.0 - 2.0 ** -8)
    ei = np.concatenate([near, inner, np.zeros(1, np.float32), -inner, -near])
    return {
        "exp": (d88, np.exp),
        "log": (_floats_between(2.0 ** -20, 2.0 ** 20), np.log),
        "tanh": (d30, np.tanh),
        "softplus": (d88, sp64),
        "sigmoid": (d30, lambda x: 1.0 / (1.0 + np.exp(-x))),
        "swish": (d30, lambda x: x / (1.0 + np.exp(-x))),
        "erfinv": (ei, special.erfinv),
    }


@pytest.mark.parametrize("name", list(WHICH))
def test_scalar_function_error(host, name):
    from scipy import special
    x, f64 = _grids()[name]
    x = np.ascontiguousarray(x, np.float32)
    exact = f64(x.astype(np.float64))
    ours = np.empty_like(x)
    assert host.mlp_scalar(WHICH[name], x.size, fp(x), fp(ours)) == 0
    if name == "erfinv":
        yard = special.erfinv(x)
        assert yard.dtype == np.float32
    else:
        yard = np.empty_like(x)
        assert host.mlp_scalar_libm(WHICH[name], x.size, fp(x), fp(yard)) == 0
    assert np.isfinite(ours).all()
    e_ours, e_yard = _ulp_err(ours, exact), _ulp_err(yard, exact)
    print(f"{name}: n = {x.size}  ours {e_ours:.3f} ulp  yardstick {e_yard:.3f} ulp")
    assert e_ours <= 2.0 * e_yard + 1.0, (name, e_ours, e_yard)


def test_scalar_edges(host):
    x = np.array([-200.0, 100.0, np.nan, 0.0, -0.0], np.float32)
    y = np.empty_like(x)
    host.mlp_scalar(0, x.size, fp(x), fp(y))
    assert y[0] == 0.0 and np.isinf(y[1]) and np.isnan(y[2]) and y[3] == 1.0 and y[4] == 1.0
    x = np.array([0.0, -1.0, np.inf, 1.0, 2.0 ** -140], np.float32)
    host.mlp_scalar(1, x.size, fp(x), fp(y))
    assert y[0] == -np.inf and np.isnan(y[1]) and y[2] == np.inf and y[3] == 0.0
    assert abs(y[4] - np.log(2.0 ** -140)) < 1e-5
    x = np.array([50.0, -50.0, 0.0, 1e-20, -1e-20], np.float32)
    host.mlp_scalar(2, x.size, fp(x), fp(y))
    assert y[0] == 1.0 and y[1] == -1.0 and y[2] == 0.0 and y[3] == x[3] and y[4] == x[4]
    host.mlp_scalar(3, x.size, fp(x), fp(y))  # softplus: x for large x, exp(x) for very negative x
    assert y[0] == 50.0 and abs(y[1] / np.exp(-50.0) - 1.0) < 1e-6 and abs(y[2] - np.log(2.0)) < 1e-7


def test_summation_order_is_natural(host):
    assert [host.mlp_ref_kfeat(s, h) for s in range(3) for h in range(2)] == [0, 1, 2, 3, 4, 5]


NETS = [([27, 33, 16], False), ([114, 32, 32, 32, 32, 16], False), ([114, 256, 256, 1], False), ([5, 7], True)]


def random_net(sizes, rng, B):
    """Inputs uniform in [-3, 3], weights uniform in +-sqrt(3 / in), small biases."""
    x = rng.uniform(-3, 3, (B, sizes[0])).astype(np.float32)
    parts = []
    for i, o in zip(sizes[:-1], sizes[1:]):
        lim = np.sqrt(3.0 / i)
        parts += [rng.uniform(-lim, lim, i * o), rng.uniform(-0.1, 0.1, o)]
    return x, np.concatenate(parts).astype(np.float32)


def forward_np(sizes, act, act_final, x, theta, dtype=np.float64):
    fn = {0: lambda v: np.maximum(v, 0), 1: lambda v: v / (1 + np.exp(-v)), 2: np.tanh}[act]
    a, off = x.astype(dtype), 0
    for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
        W = theta[off:off + i * o].reshape(i, o).astype(dtype); off += i * o
        b = theta[off:off + o].astype(dtype); off += o
        a = a @ W + b
        if l != len(sizes) - 2 or act_final:
            a = fn(a)
    return a


def forward_torch(sizes, act, act_final, x, theta):
    import torch
    fn = {0: torch.relu, 1: torch.nn.functional.silu, 2: torch.tanh}[act]
    a, off, th = torch.from_numpy(x), 0, torch.from_numpy(theta)
    for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
        W = th[off:off + i * o].reshape(i, o); off += i * o
        b = th[off:off + o]; off += o
        a = torch.addmm(b, a, W)
        if l != len(sizes) - 2 or act_final:
            a = fn(a)
    return a.numpy()


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("net", range(len(NETS)))
def test_restatement_against_float64(host, net, act):
    sizes, act_final = NETS[net]
    rng = np.random.default_rng(100 + 10 * net + act)
    x, theta = random_net(sizes, rng, 257)
    exact = forward_np(sizes, act, act_final, x, theta)
    ours = ref_forward(host, sizes, act, act_final, x, theta)
    tor = forward_torch(sizes, act, act_final, x, theta)
    e_ours = float(np.abs(ours - exact).max())
    e_torch = float(np.abs(tor - exact).max())
    print(f"net {sizes} act {act}: restatement {e_ours:.3e}  torch f32 {e_torch:.3e}")
    assert e_ours <= 4.0 * e_torch + 1e-7


def test_head_against_float64(host):
    """The head's formulas against float64: action = tanh(loc + scale eps), logp = the normal's
    log-density minus log(1 - tanh^2), from the restatement's own raw (so that only the formula
    is compared, not the noise)."""
    from scipy import special
    rng = np.random.default_rng(5)
    B, A = 512, 8
    logits = rng.uniform(-2, 2, (B, 2 * A)).astype(np.float32)
    u = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    u[0, 0] = -1.0  # the draw's lower end: clamped, finite
    action, logp, raw = ref_head(host, logits, u)
    assert np.isfinite(action).all() and np.isfinite(logp).all()
    loc, s = logits[:, :A].astype(np.float64), logits[:, A:].astype(np.float64)
    scale = np.log1p(np.exp(s)) + 0.001
    eps = np.sqrt(2.0) * special.erfinv(np.maximum(u.astype(np.float64), -1 + 2.0 ** -24))
    raw64 = loc + scale * eps
    # raw: erfinv (bound above: <= 2 x 2.9 + 1 ulp), softplus and one fmaf rounding, about 8 ulp
    # = 1e-6 relative on |scale eps| <= max |raw|; twice that
    assert np.abs(raw - raw64).max() <= 2e-6 * max(1.0, np.abs(raw64).max())
    r = raw.astype(np.float64)
    z = (r - loc) / scale
    lp = (-0.5 * z * z - np.log(scale) - 0.5 * np.log(2 * np.pi) - 2 * (np.log(2) - r - np.logaddexp(0.0, -2 * r))).sum(-1)
    # z re-derived from the float32 raw: |raw| < 16 here, so raw carries up to 2^-21 / 2 of rounding,
    # dz = that / scale (scale >= softplus(-2) = 0.127), d(z^2 / 2) = |z| dz with |z| <= 5.3 (u's last
    # step before 1): 1e-5 per component, 8 components, and as much again for the other terms
    assert np.abs(logp - lp).max() <= 2e-4
    assert np.abs(action - np.tanh(r)).max() <= 3e-7  # tanh: bound above <= 2 x 2.2 + 1 ulp of [0.5, 1)
    a_det, lp_det, raw_det = ref_head(host, logits, u, deterministic=True)
    assert np.isnan(lp_det).all() and np.array_equal(raw_det, logits[:, :A])
    assert np.abs(a_det - np.tanh(loc)).max() <= 3e-7


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "mlp_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DMLP_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
