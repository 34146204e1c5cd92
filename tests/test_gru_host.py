"""CPU: the restatement of the recurrent-actor kernels (gru_forward_ref / gru_policy_ref of
po-brax_amd/csrc/pob_mlp.h, built for the host by tests/host/gru_host.cpp).

One step of the cell plus a post layer against an independent float64 numpy spelling of the
equations, bounded by 4 x (the error of torch.nn.GRUCell + Linear in float32 with the same
weights) + 1e-7, the rule of test_mlp_host.py.  Layout: exact gates and exact integers that a
row / column or x / h swap would change.  reset: any non-zero entry (a NaN too) starts the env
from h = +0.  The stand-alone program (-DGRU_MAIN) runs once under -fsanitize=address,undefined.

Measured (x86-64, torch 2.x CPU), max abs error against float64, restatement / torch float32:
see DESIGN.md "Recurrent actor"; the test prints each figure before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "gru_host.cpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)


def build_gru_host(d):
    so = os.path.join(str(d), "gru_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    lib.gru_ref_param_count.argtypes = [C.c_int, IP, C.c_int, C.c_int, IP]
    lib.gru_ref_param_count.restype = C.c_longlong
    lib.gru_ref_forward.argtypes = [C.c_int, IP, C.c_int, C.c_int, IP, C.c_int, C.c_int, FP, FP, FP, FP, FP, FP, FP]
    lib.gru_ref_policy.argtypes = [C.c_int, IP, C.c_int, C.c_int, IP, C.c_int, C.c_int, FP, FP, FP, FP, FP, C.c_int,
                                   FP, FP, FP, FP, FP, FP]
    lib.gru_ref_cell.argtypes = [C.c_int, C.c_int, C.c_int, FP, FP, FP, FP, FP, FP, FP, FP]
    lib.gru_ref_sigmoid.argtypes = [C.c_float]
    lib.gru_ref_sigmoid.restype = C.c_float
    return lib


def fp(a):
    return None if a is None else a.ctypes.data_as(FP)


def _ints(v):
    a = np.asarray(v, np.int32)
    return a, a.ctypes.data_as(IP)


def ref_param_count(lib, pre, H, post):
    pa, pp = _ints(pre)
    qa, qp = _ints(post)
    return int(lib.gru_ref_param_count(len(pre) - 1, pp, H, len(post), qp))


def ref_forward(lib, pre, H, post, act, x, theta, reset, h):
    """gru_forward_ref on numpy arrays: pre = [D, *pre widths]; returns y, h_out, h_in_copy."""
    x, theta, h = (np.ascontiguousarray(a, np.float32) for a in (x, theta, h))
    reset = None if reset is None else np.ascontiguousarray(reset, np.float32)
    pa, pp = _ints(pre)
    qa, qp = _ints(post)
    assert theta.size == ref_param_count(lib, pre, H, post)
    B = x.shape[0]
    y, h_out, h_copy = np.empty((B, post[-1]), np.float32), np.empty((B, H), np.float32), np.empty((B, H), np.float32)
    rc = lib.gru_ref_forward(len(pre) - 1, pp, H, len(post), qp, act, B, fp(x), fp(theta), fp(reset), fp(h), fp(y),
                             fp(h_out), fp(h_copy))
    assert rc == 0
    return y, h_out, h_copy


def ref_policy(lib, pre, H, post, act, obs, theta, reset, h, u, deterministic=False):
    """gru_policy_ref: returns a dict of logits, h_out, h_in_copy, action, logp, raw."""
    obs, theta, h, u = (np.ascontiguousarray(a, np.float32) for a in (obs, theta, h, u))
    reset = None if reset is None else np.ascontiguousarray(reset, np.float32)
    pa, pp = _ints(pre)
    qa, qp = _ints(post)
    B, A = u.shape
    assert post[-1] == 2 * A
    o = {"logits": np.empty((B, 2 * A), np.float32), "h_out": np.empty((B, H), np.float32),
         "h_in_copy": np.empty((B, H), np.float32), "action": np.empty((B, A), np.float32),
         "logp": np.full(B, np.nan, np.float32), "raw": np.empty((B, A), np.float32)}
    rc = lib.gru_ref_policy(len(pre) - 1, pp, H, len(post), qp, act, B, fp(obs), fp(theta), fp(reset), fp(h), fp(u),
                            int(deterministic), fp(o["logits"]), fp(o["h_out"]), fp(o["h_in_copy"]), fp(o["action"]),
                            fp(o["logp"]), fp(o["raw"]))
    assert rc == 0
    return o


def gru_layout(pre, H, post):
    """(n_in, n_out) of every weight matrix in theta order."""
    I = pre[-1]
    widths = [H] + list(post)
    return (list(zip(pre[:-1], pre[1:])) + [(I + H, 2 * H), (I, H), (H, H)] + list(zip(widths[:-1], widths[1:])))


def random_gru(pre, H, post, rng, B, bias=0.1):
    """Inputs uniform in [-3, 3], h in [-1, 1], weights uniform in +-sqrt(3 / in), small biases."""
    x = rng.uniform(-3, 3, (B, pre[0])).astype(np.float32)
    h = rng.uniform(-1, 1, (B, H)).astype(np.float32)
    parts = []
    for i, o in gru_layout(pre, H, post):
        lim = np.sqrt(3.0 / i)
        parts += [rng.uniform(-lim, lim, i * o), rng.uniform(-bias, bias, o)]
    return x, h, np.concatenate(parts).astype(np.float32)


def unpack(pre, H, post, theta):
    """[(W (in, out), b (out))] in theta order."""
    out, off = [], 0
    for i, o in gru_layout(pre, H, post):
        W = theta[off:off + i * o].reshape(i, o); off += i * o
        out.append((W, theta[off:off + o])); off += o
    assert off == theta.size
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_gru_host(tmp_path_factory.mktemp("gru_host"))


def _cell_f64(x, h, Wrz, brz, Wxn, bxn, Whn, bhn):
    H = h.shape[1]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    c = np.concatenate([x, h], axis=1)
    rz = sig(c @ Wrz + brz)
    r, z = rz[:, :H], rz[:, H:]
    n = np.tanh(r * (h @ Whn + bhn) + (x @ Wxn + bxn))
    return (1.0 - z) * n + z * h


@pytest.mark.parametrize("D,H,O", [(114, 64, 16), (30, 64, 16), (7, 5, 4), (128, 128, 2)])
def test_restatement_against_float64(host, D, H, O):
    import torch
    rng = np.random.default_rng(D * 1000 + H)
    pre, post, B = [D], [O], 257
    x, h, theta = random_gru(pre, H, post, rng, B)
    (Wrz, brz), (Wxn, bxn), (Whn, bhn), (Wp, bp) = unpack(pre, H, post, theta)
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    h64 = _cell_f64(f64(x), f64(h), f64(Wrz), f64(brz), f64(Wxn), f64(bxn), f64(Whn), f64(bhn))
    y64 = h64 @ f64(Wp) + f64(bp)
    y, h_out, h_copy = ref_forward(host, pre, H, post, 1, x, theta, None, h)
    assert np.array_equal(h_copy, h)
    # torch.nn.GRUCell in float32 with the same weights: its gate order is (r, z, n), weights (3 H, in)
    cell = torch.nn.GRUCell(D, H)
    t = torch.from_numpy
    with torch.no_grad():
        cell.weight_ih.copy_(t(np.concatenate([Wrz[:D, :H].T, Wrz[:D, H:].T, Wxn.T])))
        cell.weight_hh.copy_(t(np.concatenate([Wrz[D:, :H].T, Wrz[D:, H:].T, Whn.T])))
        cell.bias_ih.copy_(t(np.concatenate([brz, bxn])))
        cell.bias_hh.copy_(t(np.concatenate([np.zeros(2 * H, np.float32), bhn])))  # b_hr = b_hz = 0
        ht = cell(t(x), t(h))
        yt = torch.addmm(t(bp), ht, t(Wp))
    e_h, e_h_t = float(np.abs(h_out - h64).max()), float(np.abs(ht.numpy() - h64).max())
    e_y, e_y_t = float(np.abs(y - y64).max()), float(np.abs(yt.numpy() - y64).max())
    print(f"D {D} H {H} O {O}: h' restatement {e_h:.3e} torch f32 {e_h_t:.3e};  y restatement {e_y:.3e} torch f32 {e_y_t:.3e}")
    assert e_h <= 4.0 * e_h_t + 1e-7
    assert e_y <= 4.0 * e_y_t + 1e-7


def _cell(host, I, H, x, h, g):
    B = x.shape[0]
    outs = [np.empty((B, H), np.float32) for _ in range(5)]
    assert host.gru_ref_cell(I, H, B, fp(x), fp(h), fp(g), *(fp(o) for o in outs)) == 0
    return outs  # r, z, cx, ch, hn


def test_layout_exact_gates_and_integers(host):
    assert host.gru_ref_sigmoid(0.0) == 0.5  # exact: 1 / (1 + 1)
    I, H, B = 6, 5, 9
    rng = np.random.default_rng(0)
    x = rng.integers(-4, 5, (B, I)).astype(np.float32)
    h = rng.integers(-4, 5, (B, H)).astype(np.float32)
    Wrz, brz = np.zeros((I + H, 2 * H)), np.zeros(2 * H)
    Wxn, bxn = np.zeros((I, H)), np.arange(H) - 2.0
    Whn = np.arange(H)[:, None] + 100.0 * np.arange(H)[None, :]  # asymmetric
    bhn = 7.0 - np.arange(H)
    g = np.concatenate([Wrz.ravel(), brz, Wxn.ravel(), bxn, Whn.ravel(), bhn]).astype(np.float32)
    r, z, cx, ch, hn = _cell(host, I, H, x, h, g)
    assert (r == 0.5).all() and (z == 0.5).all()
    assert np.array_equal(cx, np.broadcast_to(bxn, (B, H)).astype(np.float32))
    want = h.astype(np.int64) @ Whn.astype(np.int64) + bhn.astype(np.int64)
    assert np.abs(want).max() < 2 ** 24 and np.array_equal(ch.astype(np.int64), want)
    assert not np.array_equal(want, h.astype(np.int64) @ Whn.T.astype(np.int64) + bhn.astype(np.int64))
    # x reaches cx through W_xn (row-major (I, H)), h does not; and r, z take column j and H + j of W_rz
    Wxn = np.arange(I)[:, None] * 10.0 + np.arange(H)[None, :]
    Wrz[:, 1] = 50.0   # r[1] -> sigmoid(50 sum c) in {0, 0.5, 1}
    Wrz[:, H + 2] = -50.0
    g = np.concatenate([Wrz.ravel(), brz, Wxn.ravel(), bxn, Whn.ravel(), bhn]).astype(np.float32)
    r, z, cx, ch, hn = _cell(host, I, H, x, h, g)
    assert np.array_equal(cx.astype(np.int64), x.astype(np.int64) @ Wxn.astype(np.int64) + bxn.astype(np.int64))
    s = x.sum(1) + h.sum(1)
    step = np.where(s > 0, 1.0, np.where(s < 0, 0.0, 0.5)).astype(np.float32)
    assert np.array_equal(r[:, 1], step) and np.array_equal(z[:, 2], 1 - step)
    assert (np.delete(r, 1, axis=1) == 0.5).all() and (np.delete(z, 2, axis=1) == 0.5).all()
    # z = 1 keeps h, z = 0 takes n: h' = fmaf(z, h - n, n)
    keep = s < 0
    assert np.array_equal(hn[keep, 2], h[keep, 2])


def test_reset_zeroes_the_state(host):
    pre, H, post, B = [6], 5, [4], 8
    rng = np.random.default_rng(3)
    x, h, theta = random_gru(pre, H, post, rng, B)
    reset = np.array([0.0, 1.0, -0.0, np.nan, -2.5, 1e-45, 0.0, np.inf], np.float32)
    zeroed = np.array([0, 1, 0, 1, 1, 1, 0, 1], bool)
    y, h_out, h_copy = ref_forward(host, pre, H, post, 1, x, theta, reset, h)
    assert (h_copy[zeroed].view(np.uint32) == 0).all()  # +0, not -0
    assert np.array_equal(h_copy[~zeroed], h[~zeroed])
    h0 = h.copy()
    h0[zeroed] = 0.0
    y2, h_out2, _ = ref_forward(host, pre, H, post, 1, x, theta, None, h0)
    assert np.array_equal(y, y2) and np.array_equal(h_out, h_out2)
    y3, _, _ = ref_forward(host, pre, H, post, 1, x, theta, None, h)
    assert not np.array_equal(y[zeroed], y3[zeroed])


def test_param_count(host):
    assert ref_param_count(host, [114], 64, [16]) == 3 * 64 * 114 + 3 * 64 ** 2 + 4 * 64 + 65 * 16
    assert ref_param_count(host, [114, 32], 64, [32, 16]) == 115 * 32 + 3 * 64 * 32 + 3 * 64 ** 2 + 4 * 64 + 65 * 32 + 33 * 16


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "gru_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DGRU_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
