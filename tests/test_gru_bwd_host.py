"""CPU: the restatement of the recurrent training forward and its truncated backward pass through
time (gru_sequence_forward_train_ref / gru_sequence_backward_ref of po-brax_amd/csrc/pob_mlp.h, built
for the host by tests/host/gru_bwd_host.cpp).

Accuracy: against float64 torch autograd of ``RecurrentModel.apply_sequence``, next to float32 torch
CPU autograd as the yardstick; per block of dtheta and for dh0, max |ours - f64| <= 4 x max |f32 -
f64| + ulp32(max |f64|) (DESIGN.md "MLP backward" has the rule; relu is left out for the reason given
there).  The test prints every ratio before it asserts; the table is in DESIGN.md "Recurrent
backward".

Exact properties are bitwise.  ``test_dh0_is_zero_exactly_behind_a_reset`` sends the gradient in
through ``dh_last`` alone: with a non-zero ``dy`` at every step, the steps before a reset still reach
h0, so "zero exactly where any reset" holds for the gradient that has to cross the whole window.  The
stand-alone program (-DGRU_BWD_MAIN) runs once under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "gru_bwd_host.cpp")
FP, IP, LP = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
I32P = C.POINTER(C.c_int32)
RELU, SWISH, TANH = 0, 1, 2
ACT_NAMES = {RELU: "relu", SWISH: "swish", TANH: "tanh"}
# (pre sizes with the observation width first, hidden, post sizes)
NETS = {
    "7-gru5-4": ([7], 5, [4]),
    "30-gru64-16": ([30], 64, [16]),
    "114-gru64-16": ([114], 64, [16]),
    "114-32-gru33-16-8": ([114, 32], 33, [16, 8]),
}
PLAN = ("xin", "pre", "xc", "hin", "gate", "hn", "post", "n_saved", "d_pre", "d_cell", "d_post", "n_delta")


def build_gru_bwd_host(d):
    so = os.path.join(str(d), "gru_bwd_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    net = [C.c_int, IP, C.c_int, C.c_int, IP]
    lib.gru_bwd_ref_param_count.argtypes = net
    lib.gru_bwd_ref_param_count.restype = C.c_longlong
    lib.gru_bwd_ref_layout.argtypes = net + [C.c_longlong, LP]
    lib.gru_bwd_ref_layout.restype = None
    lib.gru_bwd_ref_step.argtypes = net + [C.c_int, C.c_int, FP, FP, FP, FP, FP, FP, FP]
    lib.gru_bwd_ref_step.restype = None
    lib.gru_bwd_ref_forward.argtypes = net + [C.c_int, C.c_int, C.c_longlong, C.c_longlong, FP, I32P, FP, FP, FP, C.c_float,
                                              FP, FP, FP, FP]
    lib.gru_bwd_ref_forward.restype = None
    lib.gru_bwd_ref_backward.argtypes = net + [C.c_int, C.c_int, C.c_longlong, C.c_longlong, I32P, FP, FP, FP, FP, FP, FP, FP,
                                               FP]
    lib.gru_bwd_ref_mlp_backward.argtypes = [C.c_int, IP, C.c_int, C.c_int, C.c_longlong, FP, FP, FP, FP, FP, FP]
    lib.gru_bwd_ref_sum.argtypes = [C.c_longlong, FP, C.c_longlong, FP, C.c_longlong]
    lib.gru_bwd_ref_sum.restype = C.c_float
    lib.gru_bwd_ref_cell_grad.argtypes = [C.c_float] * 6 + [FP]
    lib.gru_bwd_ref_cell_grad.restype = None
    lib.gru_bwd_ref_obsnorm.argtypes = [FP, C.c_longlong, C.c_int, FP, C.c_float]
    lib.gru_bwd_ref_obsnorm.restype = None
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_gru_bwd_host(tmp_path_factory.mktemp("gru_bwd_host"))


def _p(a, t=FP):
    return None if a is None else a.ctypes.data_as(t)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _net(net):
    pre, H, post = net
    return (len(pre) - 1, (C.c_int * len(pre))(*pre), H, len(post), (C.c_int * len(post))(*post))


def param_count(net):
    return sum((a + 1) * b for _, _, a, b in blocks(net))


def blocks(net):
    """[(name, offset, in, out)] of the (in + 1, out) blocks of theta's packing."""
    pre, H, post = net
    I = pre[-1]
    shapes = [(f"pre_{i}", a, b) for i, (a, b) in enumerate(zip(pre[:-1], pre[1:]))]
    shapes += [("W_rz", I + H, 2 * H), ("W_xn", I, H), ("W_hn", H, H)]
    widths = [H] + list(post)
    shapes += [(f"post_{i}", a, b) for i, (a, b) in enumerate(zip(widths[:-1], widths[1:]))]
    out, off = [], 0
    for name, a, b in shapes:
        out.append((name, off, a, b))
        off += (a + 1) * b
    return out


def layout(lib, net, R):
    v = (C.c_longlong * 12)()
    lib.gru_bwd_ref_layout(*_net(net), R, v)
    return dict(zip(PLAN, (int(x) for x in v)))


def ref_forward(lib, net, act, obs, h0, theta, idx=None, reset=None, norm=None, clip=5.0, want_h_last=True):
    """(y (T, M, out), h_last (M, H) or None, saved) of gru_sequence_forward_train_ref."""
    pre, H, post = net
    obs, h0, theta, reset, norm = map(_f32, (obs, h0, theta, reset, norm))
    T, B = obs.shape[:2]
    idx = None if idx is None else np.ascontiguousarray(idx, np.int32)
    M = B if idx is None else idx.shape[0]
    assert obs.shape == (T, B, pre[0]) and h0.shape == (B, H) and theta.shape == (param_count(net),)
    n = layout(lib, net, T * M)["n_saved"]
    y, saved = np.full((T, M, post[-1]), np.nan, np.float32), np.full(n, np.nan, np.float32)
    h_last = np.full((M, H), np.nan, np.float32) if want_h_last else None
    lib.gru_bwd_ref_forward(*_net(net), act, T, M, B, _p(obs), _p(idx, I32P), _p(h0), _p(reset), _p(norm), clip, _p(theta),
                            _p(y), _p(h_last), _p(saved))
    assert not np.isnan(saved).any() or np.isnan(obs).any()
    return y, h_last, saved


def ref_backward(lib, net, act, T, M, B, theta, saved, dy, idx=None, reset=None, dh_last=None, want_dh0=True):
    """dict of dtheta (P,), dh0 (M, H) or None, delta (flat) of gru_sequence_backward_ref."""
    pre, H, post = net
    theta, saved, dy, reset, dh_last = map(_f32, (theta, saved, dy, reset, dh_last))
    idx = None if idx is None else np.ascontiguousarray(idx, np.int32)
    assert dy.shape == (T, M, post[-1])
    dtheta = np.full(param_count(net), np.nan, np.float32)
    dh0 = np.full((M, H), np.nan, np.float32) if want_dh0 else None
    delta = np.full(layout(lib, net, T * M)["n_delta"], np.nan, np.float32)
    assert lib.gru_bwd_ref_backward(*_net(net), act, T, M, B, _p(idx, I32P), _p(reset), _p(theta), _p(saved), _p(dy),
                                    _p(dh_last), _p(dtheta), _p(dh0), _p(delta)) == 0
    return dict(dtheta=dtheta, dh0=dh0, delta=delta)


def problem(rng, net, T, M, B=None, reset_p=0.2):
    """Inputs of the issue's accuracy cases: x ~ U[-3, 3], h0 ~ U[-1, 1], lecun-uniform weights, biases
    0.1 N(0, 1), resets on about ``reset_p`` of the entries, dy ~ N(0, 1) / (T M)."""
    pre, H, post = net
    B = M if B is None else B
    theta = np.zeros(param_count(net), np.float32)
    for _, off, a, b in blocks(net):
        lim = np.sqrt(3.0 / a)
        theta[off:off + a * b] = rng.uniform(-lim, lim, a * b)
        theta[off + a * b:off + (a + 1) * b] = 0.1 * rng.standard_normal(b)
    return dict(obs=rng.uniform(-3, 3, (T, B, pre[0])).astype(np.float32), h0=rng.uniform(-1, 1, (B, H)).astype(np.float32),
                theta=theta, reset=(rng.uniform(size=(T, B)) < reset_p).astype(np.float32),
                dy=(rng.standard_normal((T, M, post[-1])) / (T * M)).astype(np.float32))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("name", ["7-gru5-4", "114-32-gru33-16-8"])
@pytest.mark.parametrize("act", [RELU, SWISH, TANH])
def test_forward_is_the_chained_single_step(lib, name, act):
    """y, h_last = T chained gru_forward_ref calls on the gathered, normalised rows, with idx, a table
    and resets; the saved post-reset h of every step is the step's h_in_copy."""
    net = NETS[name]
    pre, H, post = net
    rng = np.random.default_rng(3)
    T, B, M = 4, 41, 35
    pr = problem(rng, net, T, M, B)
    idx = rng.permutation(B)[:M].astype(np.int32)
    norm = np.stack([0.5 * rng.standard_normal(pre[0]), rng.uniform(0.5, 2.0, pre[0]), np.ones(pre[0])]).astype(np.float32)
    y, h_last, saved = ref_forward(lib, net, act, pr["obs"], pr["h0"], pr["theta"], idx, pr["reset"], norm, 2.5)
    lay = layout(lib, net, T * M)
    hin = saved[lay["hin"]:lay["hin"] + T * M * H].reshape(T, M, H)
    h = np.ascontiguousarray(pr["h0"][idx])
    for t in range(T):
        x = np.ascontiguousarray(pr["obs"][t, idx])
        lib.gru_bwd_ref_obsnorm(_p(x), M, pre[0], _p(norm), 2.5)
        rs = np.ascontiguousarray(pr["reset"][t, idx])
        yt, h_new, h_copy = (np.full(s, np.nan, np.float32) for s in ((M, post[-1]), (M, H), (M, H)))
        lib.gru_bwd_ref_step(*_net(net), act, M, _p(x), _p(pr["theta"]), _p(rs), _p(h), _p(yt), _p(h_new), _p(h_copy))
        assert same_bits(y[t], yt) and same_bits(hin[t], h_copy)
        h = h_new
    assert same_bits(h_last, h)


def test_window_splits_at_any_step(lib):
    net = NETS["114-32-gru33-16-8"]
    rng = np.random.default_rng(4)
    T, T1, M = 5, 2, 33
    pr = problem(rng, net, T, M)
    y, h_last, _ = ref_forward(lib, net, SWISH, pr["obs"], pr["h0"], pr["theta"], None, pr["reset"])
    ya, ha, _ = ref_forward(lib, net, SWISH, pr["obs"][:T1], pr["h0"], pr["theta"], None, pr["reset"][:T1])
    yb, hb, _ = ref_forward(lib, net, SWISH, pr["obs"][T1:], ha, pr["theta"], None, pr["reset"][T1:])
    assert same_bits(y, np.concatenate([ya, yb])) and same_bits(h_last, hb)


@pytest.mark.parametrize("name", ["7-gru5-4", "114-32-gru33-16-8"])
def test_zero_gradient_in_gives_positive_zero_bits(lib, name):
    net = NETS[name]
    rng = np.random.default_rng(5)
    T, M = 3, 37
    pr = problem(rng, net, T, M)
    _, _, saved = ref_forward(lib, net, TANH, pr["obs"], pr["h0"], pr["theta"], None, pr["reset"])
    out = ref_backward(lib, net, TANH, T, M, M, pr["theta"], saved, np.zeros_like(pr["dy"]), None, pr["reset"],
                       np.zeros((M, net[1]), np.float32))
    assert not bits(out["dtheta"]).any() and not bits(out["dh0"]).any()


def test_dh0_is_zero_exactly_behind_a_reset(lib):
    """The gradient of h_last alone: dh0[m] is +0 in every feature exactly for the sequences with any
    reset[t][m] != 0; a NaN reset counts, a -0.0 reset does not."""
    net = NETS["7-gru5-4"]
    rng = np.random.default_rng(6)
    T, M = 5, 40
    pr = problem(rng, net, T, M)
    reset = pr["reset"] * (rng.uniform(size=(T, M)) < 0.5)  # about a tenth of the entries
    reset[2, 0] = np.nan   # sequence 0: a NaN counts
    reset[:, 1] = -0.0     # sequence 1: -0.0 everywhere does not
    reset[:, 2] = 0.0
    reset[3, 2] = -0.0     # sequence 2: one -0.0 among zeros does not
    assert np.signbit(reset[3, 2]) and np.isnan(reset[2, 0])
    _, _, saved = ref_forward(lib, net, SWISH, pr["obs"], pr["h0"], pr["theta"], None, reset)
    dh_last = rng.uniform(0.5, 1.5, (M, net[1])).astype(np.float32)
    out = ref_backward(lib, net, SWISH, T, M, M, pr["theta"], saved, np.zeros_like(pr["dy"]), None, reset, dh_last)
    any_reset = (reset != 0).any(axis=0)  # NaN != 0 is True, -0.0 != 0 is False
    assert any_reset[0] and not any_reset[1] and not any_reset[2] and 5 < any_reset.sum() < M - 5
    zero_rows = ~bits(out["dh0"]).any(axis=1)
    assert np.array_equal(zero_rows, any_reset)
    assert (out["dh0"][~any_reset] != 0).any(axis=1).all()


def _fma(a, b, c):
    from po_brax_amd.training.ppo import _fma as fma
    return fma(torch.from_numpy(np.ascontiguousarray(a, np.float32)), torch.from_numpy(np.ascontiguousarray(b, np.float32)),
               torch.from_numpy(np.ascontiguousarray(c, np.float32))).numpy()


def _deltas_by_formula(g_h, hin, r, z, ch, n):
    """The issue's formulas, one float32 rounding per spelled operation."""
    one = np.float32(1.0)
    dz = g_h * (hin - n)
    dn = g_h * (one - z)
    ds = dn * _fma(-n, n, np.ones_like(n))
    return ((ds * ch) * r) * (one - r), (dz * z) * (one - z), ds, ds * r


def _sum_block(lib, a, d):
    """(in + 1, out) = mlp_bwd_sum over the rows of a (R, in) (then the constant 1) against d (R, out)."""
    R, n_in = a.shape
    out = np.empty((n_in + 1, d.shape[1]), np.float32)
    a, d = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(d, np.float32)
    for i in range(n_in + 1):
        for j in range(d.shape[1]):
            ap = None if i == n_in else C.cast(C.addressof(_p(a).contents) + 4 * i, FP)
            dp = C.cast(C.addressof(_p(d).contents) + 4 * j, FP)
            out[i, j] = lib.gru_bwd_ref_sum(R, ap, n_in, dp, d.shape[1])
    return out


@pytest.mark.parametrize("act", [RELU, SWISH, TANH])
def test_one_step_cell_blocks_are_the_formulas(lib, act):
    """T = 1, no pre-MLP, reset = NULL: the cell blocks of dtheta and dh0 from a direct spelling."""
    net = ([6], 5, [4])
    pre, H, post = net
    I = pre[0]
    rng = np.random.default_rng(7)
    M = 70
    pr = problem(rng, net, 1, M)
    dh_last = rng.standard_normal((M, H)).astype(np.float32)
    _, _, saved = ref_forward(lib, net, act, pr["obs"], pr["h0"], pr["theta"])
    out = ref_backward(lib, net, act, 1, M, M, pr["theta"], saved, pr["dy"], None, None, dh_last)
    lay = layout(lib, net, M)
    gate = saved[lay["gate"]:lay["gate"] + M * 4 * H].reshape(M, 4, H)
    r, z, ch, n = (gate[:, q] for q in range(4))
    hin, xc = pr["h0"], pr["obs"][0]
    blk = {name: (off, a, b) for name, off, a, b in blocks(net)}
    off, a, b = blk["post_0"]
    W_post = pr["theta"][off:off + a * b].reshape(a, b)
    g_post = np.zeros((M, H), np.float32)
    for j in range(b):  # acc = +0, one fmaf per output feature in natural order
        g_post = _fma(np.broadcast_to(W_post[:, j], (M, H)), np.broadcast_to(pr["dy"][0][:, j:j + 1], (M, H)), g_post)
    g_h = g_post + dh_last
    d_r, d_z, d_xn, d_hn = _deltas_by_formula(g_h, hin, r, z, ch, n)
    d_rz = np.concatenate([d_r, d_z], axis=1)
    delta = out["delta"][lay["d_cell"]:lay["d_cell"] + M * 4 * H].reshape(M, 4 * H)
    assert same_bits(delta, np.concatenate([d_rz, d_xn, d_hn], axis=1))
    for name, A_rows, d in (("W_rz", np.concatenate([xc, hin], axis=1), d_rz), ("W_xn", xc, d_xn), ("W_hn", hin, d_hn)):
        off, a, b = blk[name]
        assert same_bits(out["dtheta"][off:off + (a + 1) * b].reshape(a + 1, b), _sum_block(lib, A_rows, d)), name
    off, a, b = blk["W_rz"]
    W_rz = pr["theta"][off:off + a * b].reshape(a, b)
    off, a, b = blk["W_hn"]
    W_hn = pr["theta"][off:off + a * b].reshape(a, b)
    acc = np.zeros((M, H), np.float32)
    for j in range(2 * H):
        acc = _fma(np.broadcast_to(W_rz[I:, j], (M, H)), np.broadcast_to(d_rz[:, j:j + 1], (M, H)), acc)
    for j in range(H):
        acc = _fma(np.broadcast_to(W_hn[:, j], (M, H)), np.broadcast_to(d_hn[:, j:j + 1], (M, H)), acc)
    assert same_bits(out["dh0"], _fma(g_h, z, acc))


@pytest.mark.parametrize("act", [RELU, SWISH, TANH])
def test_dense_blocks_are_mlp_backward_ref(lib, act):
    """The post-MLP's and the pre-MLP's blocks = mlp_backward_ref fed the same rows (the post-MLP: h'
    and dy; the pre-MLP: the normalised observation rows and g_x spelled from the cell's deltas)."""
    net = NETS["114-32-gru33-16-8"]
    pre, H, post = net
    I = pre[-1]
    rng = np.random.default_rng(8)
    T, M = 3, 45
    R = T * M
    pr = problem(rng, net, T, M)
    _, _, saved = ref_forward(lib, net, act, pr["obs"], pr["h0"], pr["theta"], None, pr["reset"])
    out = ref_backward(lib, net, act, T, M, M, pr["theta"], saved, pr["dy"], None, pr["reset"])
    lay = layout(lib, net, R)
    blk = {name: (off, a, b) for name, off, a, b in blocks(net)}

    def mlp_back(sizes, fin, x, theta, sv, dy):
        P = sum((a + 1) * b for a, b in zip(sizes[:-1], sizes[1:]))
        dth = np.full(P, np.nan, np.float32)
        x, theta, sv, dy = map(np.ascontiguousarray, (x, theta, sv, dy))
        assert lib.gru_bwd_ref_mlp_backward(len(sizes) - 1, (C.c_int * len(sizes))(*sizes), act, fin, R, _p(x), _p(theta),
                                            _p(sv), _p(dy), _p(dth), None) == 0
        return dth

    p0 = blk["post_0"][0]
    got = mlp_back([H] + post, 0, saved[lay["hn"]:lay["hn"] + R * H], pr["theta"][p0:], saved[lay["post"]:lay["n_saved"]],
                   pr["dy"].reshape(R, -1))
    assert same_bits(out["dtheta"][p0:], got)
    dc = out["delta"][lay["d_cell"]:lay["d_cell"] + R * 4 * H].reshape(R, 4 * H)
    off, a, b = blk["W_rz"]
    W_rz = pr["theta"][off:off + a * b].reshape(a, b)
    off, a, b = blk["W_xn"]
    W_xn = pr["theta"][off:off + a * b].reshape(a, b)
    g_x = np.zeros((R, I), np.float32)
    for j in range(2 * H):
        g_x = _fma(np.broadcast_to(W_rz[:I, j], (R, I)), np.broadcast_to(dc[:, j:j + 1], (R, I)), g_x)
    for j in range(H):
        g_x = _fma(np.broadcast_to(W_xn[:, j], (R, I)), np.broadcast_to(dc[:, 2 * H + j:2 * H + j + 1], (R, I)), g_x)
    n_pre_params = blk["W_rz"][0]
    got = mlp_back(pre, 1, saved[lay["xin"]:lay["xin"] + R * pre[0]], pr["theta"][:n_pre_params],
                   saved[lay["pre"]:lay["xc"]], g_x)
    assert same_bits(out["dtheta"][:n_pre_params], got)


def test_reset_everywhere_is_a_shorter_window(lib):
    """Every env reset at step k and dy[t < k] = 0: dtheta = that of the (T - k)-step window started at
    step k from h = 0 (k M = 1024 rows: the tiles and chunks of both sums line up)."""
    net = NETS["114-32-gru33-16-8"]
    rng = np.random.default_rng(9)
    T, k, M = 6, 4, 256
    pr = problem(rng, net, T, M)
    pr["reset"][k] = 1.0
    pr["dy"][:k] = 0.0
    _, _, saved = ref_forward(lib, net, SWISH, pr["obs"], pr["h0"], pr["theta"], None, pr["reset"])
    full = ref_backward(lib, net, SWISH, T, M, M, pr["theta"], saved, pr["dy"], None, pr["reset"])
    zeros = np.zeros_like(pr["h0"])
    _, _, saved2 = ref_forward(lib, net, SWISH, pr["obs"][k:], zeros, pr["theta"], None, pr["reset"][k:])
    part = ref_backward(lib, net, SWISH, T - k, M, M, pr["theta"], saved2, pr["dy"][k:], None, pr["reset"][k:])
    assert same_bits(full["dtheta"], part["dtheta"])
    assert not bits(full["dh0"]).any()


def test_integer_layout(lib):
    """Small integers in a hand-made ``saved`` (the layout is gru_seq_layout's) and in theta and dy:
    every product is exact, so dtheta is an integer matrix product in which a transposed block or
    swapped r / z halves shows."""
    net = ([3], 2, [5])
    pre, H, post = net
    I, out_w = pre[0], post[0]
    T, M = 2, 3
    R = T * M
    rng = np.random.default_rng(10)
    lay = layout(lib, net, R)
    blk = {name: (off, a, b) for name, off, a, b in blocks(net)}
    theta = rng.integers(-2, 3, param_count(net)).astype(np.float32)
    xc, hin = rng.integers(-3, 4, (R, I)), rng.integers(-3, 4, (R, H))
    r, z, ch, n = (rng.integers(-2, 3, (R, H)) for _ in range(4))
    hn = rng.integers(-3, 4, (R, H))
    saved = np.zeros(lay["n_saved"], np.float32)
    saved[lay["xc"]:lay["xc"] + R * I] = xc.ravel()
    saved[lay["hin"]:lay["hin"] + R * H] = hin.ravel()
    saved[lay["gate"]:lay["gate"] + R * 4 * H] = np.concatenate([r, z, ch, n], axis=1).ravel()
    saved[lay["hn"]:lay["hn"] + R * H] = hn.ravel()
    dy = rng.integers(-2, 3, (T, M, out_w))
    out = ref_backward(lib, net, TANH, T, M, M, theta, saved, dy.astype(np.float32))
    W = {name: theta[off:off + a * b].reshape(a, b).astype(np.int64) for name, (off, a, b) in blk.items()}
    g_post = dy.reshape(R, out_w) @ W["post_0"].T
    carry = np.zeros((M, H), np.int64)
    d_all = np.zeros((R, 4 * H), np.int64)
    for t in (1, 0):
        s = slice(t * M, (t + 1) * M)
        g_h = g_post[s] + carry
        ds = g_h * (1 - z[s]) * (1 - n[s] * n[s])
        d_r, d_z = ds * ch[s] * r[s] * (1 - r[s]), g_h * (hin[s] - n[s]) * z[s] * (1 - z[s])
        d_all[s] = np.concatenate([d_r, d_z, ds, ds * r[s]], axis=1)
        carry = g_h * z[s] + d_all[s, :2 * H] @ W["W_rz"][I:].T + d_all[s, 3 * H:] @ W["W_hn"].T
    assert np.abs(d_all).max() < 2 ** 20
    ones = np.ones((R, 1), np.int64)
    want = {"W_rz": np.concatenate([xc, hin, ones], axis=1).T @ d_all[:, :2 * H],
            "W_xn": np.concatenate([xc, ones], axis=1).T @ d_all[:, 2 * H:3 * H],
            "W_hn": np.concatenate([hin, ones], axis=1).T @ d_all[:, 3 * H:],
            "post_0": np.concatenate([hn, ones], axis=1).T @ dy.reshape(R, out_w)}
    for name, (off, a, b) in blk.items():
        got = out["dtheta"][off:off + (a + 1) * b].reshape(a + 1, b)
        assert np.array_equal(got.astype(np.int64), want[name]) and np.array_equal(got, np.rint(got)), name
    assert np.array_equal(out["dh0"].astype(np.int64), carry)
    assert len({w.shape for w in want.values()}) == 4  # no two blocks share a shape: a mix-up cannot hide


# ---------------------------------------------------------------------------- accuracy
def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def torch_grads(net, act, pr, dtype):
    from po_brax_amd.training import networks
    pre, H, post = net
    model = networks.make_recurrent_model(pre[1:], H, post, pre[0], ACT_NAMES[act])
    theta = torch.from_numpy(pr["theta"]).to(dtype).requires_grad_(True)
    h0 = torch.from_numpy(pr["h0"]).to(dtype).requires_grad_(True)
    y, _ = model.apply_sequence(types.SimpleNamespace(theta=theta), torch.from_numpy(pr["obs"]).to(dtype), h0,
                                torch.from_numpy(pr["reset"]))
    (y * torch.from_numpy(pr["dy"]).to(dtype)).sum().backward()
    return theta.grad.numpy().astype(np.float64), h0.grad.numpy().astype(np.float64)


@pytest.mark.parametrize("M", [33, 257])
@pytest.mark.parametrize("T", [1, 5, 20])
@pytest.mark.parametrize("act", [SWISH, TANH], ids=["swish", "tanh"])
@pytest.mark.parametrize("name", list(NETS))
def test_accuracy_against_float64(lib, name, act, T, M):
    net = NETS[name]
    rng = np.random.default_rng(1000 + 7 * T + M)
    pr = problem(rng, net, T, M)
    _, _, saved = ref_forward(lib, net, act, pr["obs"], pr["h0"], pr["theta"], None, pr["reset"])
    out = ref_backward(lib, net, act, T, M, M, pr["theta"], saved, pr["dy"], None, pr["reset"])
    th64, h64 = torch_grads(net, act, pr, torch.float64)
    th32, h32 = torch_grads(net, act, pr, torch.float32)
    parts = [(bname, slice(off, off + (a + 1) * b)) for bname, off, a, b in blocks(net)]
    rows = [(bname, out["dtheta"][s].astype(np.float64), th32[s], th64[s]) for bname, s in parts]
    rows.append(("dh0", out["dh0"].astype(np.float64), h32, h64))
    worst = 0.0
    for bname, ours, f32, f64 in rows:
        e, yard = np.abs(ours - f64).max(), np.abs(f32 - f64).max()
        bound = 4.0 * yard + ulp32(np.abs(f64).max())
        worst = max(worst, e / bound)
        print(f"{name} {ACT_NAMES[act]} T={T} M={M} {bname}: ours {e:.3e} float32 torch {yard:.3e} ratio {e / bound:.3f}")
    print(f"{name} {ACT_NAMES[act]} T={T} M={M}: worst ratio {worst:.3f}")
    for bname, ours, f32, f64 in rows:
        assert np.isfinite(ours).all()
        assert np.abs(ours - f64).max() <= 4.0 * np.abs(f32 - f64).max() + ulp32(np.abs(f64).max()), bname


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gru_bwd_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DGRU_BWD_MAIN", "-I", CSRC, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
