"""CPU: the restatement of the MLP training forward and backward pass (mlp_forward_train_ref /
mlp_backward_ref / mlp_bwd_sum of po-brax_amd/csrc/pob_mlp.h, built for the host by
tests/host/mlp_bwd_host.cpp).

Accuracy: against float64 torch autograd of the same network in torch ops, next to float32 torch
CPU autograd as the yardstick; per layer block of dtheta and for dx, max |ours - f64| <= 4 x max
|f32 - f64| + ulp32(max |f64|).  The last term is derived, not measured: the float32 rounding of
the result itself.  relu is left out of that comparison (a float32 and a float64 forward disagree
about the sign of a pre-activation near 0) and is covered by the bitwise properties.  The test
prints every figure before it asserts; the table is in DESIGN.md "MLP backward".

Exact properties are bitwise.  The stand-alone program (-DMLP_BWD_MAIN) runs once under
-fsanitize=address,undefined."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "mlp_bwd_host.cpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)
CHUNK, TILE = 1024, 32
RELU, SWISH, TANH = 0, 1, 2
POLICY = [114, 32, 32, 32, 32, 16]


def build_mlp_bwd_host(d):
    so = os.path.join(str(d), "mlp_bwd_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    lib.mlp_bwd_ref_param_count.argtypes = [C.c_int, IP]
    lib.mlp_bwd_ref_param_count.restype = C.c_longlong
    lib.mlp_bwd_ref_saved_count.argtypes = [C.c_int, IP, C.c_int, C.c_longlong]
    lib.mlp_bwd_ref_saved_count.restype = C.c_longlong
    lib.mlp_bwd_ref_forward.argtypes = [C.c_int, IP, C.c_int, C.c_int, C.c_int, FP, FP, FP]
    lib.mlp_bwd_ref_forward.restype = None
    lib.mlp_bwd_ref_forward_train.argtypes = [C.c_int, IP, C.c_int, C.c_int, C.c_longlong, FP, FP, FP, FP]
    lib.mlp_bwd_ref_forward_train.restype = None
    lib.mlp_bwd_ref_backward.argtypes = [C.c_int, IP, C.c_int, C.c_int, C.c_longlong, FP, FP, FP, FP, FP, FP, FP]
    lib.mlp_bwd_ref_sum.argtypes = [C.c_longlong, FP, C.c_longlong, FP, C.c_longlong, DP]
    lib.mlp_bwd_ref_sum.restype = C.c_float
    lib.mlp_bwd_ref_activate.argtypes = [C.c_int, C.c_float]
    lib.mlp_bwd_ref_activate.restype = C.c_float
    lib.mlp_bwd_ref_activate_grad.argtypes = [C.c_int, C.c_float, C.c_float]
    lib.mlp_bwd_ref_activate_grad.restype = C.c_float
    return lib


def _p(a, t=FP):
    return None if a is None else a.ctypes.data_as(t)


def _sizes(sizes):
    return (C.c_int * len(sizes))(*sizes)


def param_count(sizes):
    return sum((a + 1) * b for a, b in zip(sizes[:-1], sizes[1:]))


def blocks(sizes):
    """[(offset, in, out)] of the layers' (in + 1, out) blocks in theta's packing."""
    out, off = [], 0
    for a, b in zip(sizes[:-1], sizes[1:]):
        out.append((off, a, b))
        off += (a + 1) * b
    return out


def activated(sizes, fin, l):
    return l != len(sizes) - 2 or bool(fin)


def ref_forward(lib, sizes, act, fin, x, theta):
    x, theta = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(theta, np.float32)
    y = np.full((x.shape[0], sizes[-1]), np.nan, np.float32)
    lib.mlp_bwd_ref_forward(len(sizes) - 1, _sizes(sizes), act, int(fin), x.shape[0], _p(x), _p(theta), _p(y))
    return y


def ref_forward_train(lib, sizes, act, fin, x, theta):
    """(y (M, sizes[-1]), saved (flat)) of mlp_forward_train_ref."""
    x, theta = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(theta, np.float32)
    M = x.shape[0]
    assert x.shape == (M, sizes[0]) and theta.shape == (param_count(sizes),)
    n = lib.mlp_bwd_ref_saved_count(len(sizes) - 1, _sizes(sizes), int(fin), M)
    assert n == M * sum(sizes[l + 1] for l in range(len(sizes) - 1) if activated(sizes, fin, l))
    y, saved = np.full((M, sizes[-1]), np.nan, np.float32), np.full(max(n, 1), np.nan, np.float32)
    lib.mlp_bwd_ref_forward_train(len(sizes) - 1, _sizes(sizes), act, int(fin), M, _p(x), _p(theta), _p(y), _p(saved))
    return y, saved[:n]


def ref_backward(lib, sizes, act, fin, x, theta, saved, dy, want_dx=True):
    """dict of dtheta (P,), dx (M, sizes[0]) or None, delta (list of (M, out) per layer)."""
    x, theta, dy = (np.ascontiguousarray(a, np.float32) for a in (x, theta, dy))
    saved = np.ascontiguousarray(saved, np.float32)
    M = x.shape[0]
    assert dy.shape == (M, sizes[-1])
    dtheta = np.full(param_count(sizes), np.nan, np.float32)
    dx = np.full((M, sizes[0]), np.nan, np.float32) if want_dx else None
    delta = np.full(M * sum(sizes[1:]), np.nan, np.float32)
    assert lib.mlp_bwd_ref_backward(len(sizes) - 1, _sizes(sizes), act, int(fin), M, _p(x), _p(theta),
                                    _p(saved) if saved.size else None, _p(dy), _p(dtheta), _p(dx), _p(delta)) == 0
    deltas, off = [], 0
    for w in sizes[1:]:
        deltas.append(delta[off:off + M * w].reshape(M, w))
        off += M * w
    return dict(dtheta=dtheta, dx=dx, delta=deltas)


def ref_train_and_back(lib, sizes, act, fin, x, theta, dy, want_dx=True):
    y, saved = ref_forward_train(lib, sizes, act, fin, x, theta)
    out = ref_backward(lib, sizes, act, fin, x, theta, saved, dy, want_dx)
    out.update(y=y, saved=saved)
    return out


def saved_layers(sizes, fin, saved, M):
    """{l: z_l (M, out)} of the flat saved."""
    out, off = {}, 0
    for l in range(len(sizes) - 1):
        if activated(sizes, fin, l):
            out[l] = saved[off:off + M * sizes[l + 1]].reshape(M, sizes[l + 1])
            off += M * sizes[l + 1]
    return out


def make_problem(rng, sizes, M):
    """x ~ U[-3, 3], lecun-uniform weights, biases 0.1 N(0, 1), dy ~ N(0, 1) / M."""
    x = rng.uniform(-3.0, 3.0, (M, sizes[0])).astype(np.float32)
    parts = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        lim = math.sqrt(3.0 / a)
        parts += [rng.uniform(-lim, lim, a * b), 0.1 * rng.standard_normal(b)]
    theta = np.concatenate(parts).astype(np.float32)
    dy = (rng.standard_normal((M, sizes[-1])) / M).astype(np.float32)
    return x, theta, dy


_TORCH_ACT = {RELU: torch.relu, SWISH: torch.nn.functional.silu, TANH: torch.tanh}


def torch_grads(sizes, act, fin, x, theta, dy, dtype):
    """(dtheta, dx) of the network in torch ops of ``dtype`` by autograd on the CPU."""
    th = torch.from_numpy(np.asarray(theta)).to(dtype).requires_grad_(True)
    xx = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    h, off = xx, 0
    for l, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        W = th[off:off + a * b].view(a, b)
        off += a * b
        h = torch.addmm(th[off:off + b], h, W)
        off += b
        if activated(sizes, fin, l):
            h = _TORCH_ACT[act](h)
    (h * torch.from_numpy(np.asarray(dy)).to(dtype)).sum().backward()
    return th.grad.numpy(), xx.grad.numpy()


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def within_bound(ours, f32, f64, tag):
    """max |ours - f64| <= 4 max |f32 - f64| + ulp32(max |f64|); returns (ours, yardstick, bound)."""
    ours, f32, f64 = (np.atleast_1d(np.asarray(a, np.float64)) for a in (ours, f32, f64))
    e_ours, e_yard = float(np.abs(ours - f64).max()), float(np.abs(f32 - f64).max())
    bound = 4.0 * e_yard + ulp32(np.abs(f64).max())
    print(f"{tag}: ours {e_ours:.3e} float32 torch {e_yard:.3e} bound {bound:.3e} "
          f"ours/float32 {e_ours / e_yard if e_yard else float('nan'):.2f}")
    assert e_ours <= bound, tag
    return e_ours, e_yard, bound


def check_against_float64(sizes, act, fin, x, theta, dy, got_dtheta, got_dx, tag):
    d64, x64 = torch_grads(sizes, act, fin, x, theta, dy, torch.float64)
    d32, x32 = torch_grads(sizes, act, fin, x, theta, dy, torch.float32)
    for l, (off, a, b) in enumerate(blocks(sizes)):
        s = slice(off, off + (a + 1) * b)
        within_bound(got_dtheta[s], d32[s], d64[s], f"{tag} layer {l} ({a} + 1, {b})")
    if got_dx is not None:
        within_bound(got_dx, x32, x64, f"{tag} dx")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _round_frac(v):
    """Round an exact rational to the nearest float32 (ties to even)."""
    from fractions import Fraction
    if v == 0:
        return np.float32(0.0)
    sign = -1 if v < 0 else 1
    v = abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    e = max(e, -126)
    q = v / Fraction(2) ** (e - 23)  # an integer below 2^24 when v is representable
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))


def direct_sum(a, d):
    """One element in the tile / chunk order spelled directly: float32 fmaf chain from +0 over a
    tile's rows ascending; tile partials in float64 ascending from +0.0 inside a chunk; chunk
    partials in float64 ascending from +0.0; one rounding.  Returns (value, chunk partials)."""
    M = len(d)
    a = np.ones(M, np.float32) if a is None else a
    total, partials = np.float64(0.0), []
    for c0 in range(0, M, CHUNK):
        c1 = min(c0 + CHUNK, M)
        chunk = np.float64(0.0)
        for t0 in range(c0, c1, TILE):
            acc = np.float32(0.0)
            for r in range(t0, min(t0 + TILE, c1)):
                acc = _round_frac(_frac(a[r]) * _frac(d[r]) + _frac(acc))
            chunk = chunk + np.float64(acc)
        partials.append(chunk)
        total = total + chunk
    return np.float32(total), np.array(partials, np.float64)


def _frac(v):
    from fractions import Fraction
    return Fraction(float(v))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_mlp_bwd_host(tmp_path_factory.mktemp("mlp_bwd_host"))


NETS = [[5, 7, 4], [27, 33, 16], POLICY, [114, 256, 256, 1]]


@pytest.mark.parametrize("act", [SWISH, TANH])
@pytest.mark.parametrize("M", [33, 257, 1025])
@pytest.mark.parametrize("sizes", NETS, ids=lambda s: "-".join(map(str, s)))
def test_restatement_against_float64(host, sizes, M, act):
    rng = np.random.default_rng(1000 * M + 10 * len(sizes) + act)
    x, theta, dy = make_problem(rng, sizes, M)
    got = ref_train_and_back(host, sizes, act, 0, x, theta, dy)
    check_against_float64(sizes, act, 0, x, theta, dy, got["dtheta"], got["dx"], f"{sizes} M {M} act {act}")


@pytest.mark.parametrize("act", [RELU, SWISH, TANH])
@pytest.mark.parametrize("fin", [0, 1])
def test_training_forward_equals_forward_and_saves_the_preactivations(host, act, fin):
    sizes, M = [27, 33, 16, 5], 67
    x, theta, _ = make_problem(np.random.default_rng(3 + act), sizes, M)
    y, saved = ref_forward_train(host, sizes, act, fin, x, theta)
    assert same_bits(y, ref_forward(host, sizes, act, fin, x, theta))
    z = saved_layers(sizes, fin, saved, M)
    assert sorted(z) == ([0, 1, 2] if fin else [0, 1])
    # z_l is the un-activated output of the first l + 1 layers; the activation of it is the next input
    for l in z:
        sub = sizes[:l + 2]
        n = param_count(sub)
        assert same_bits(z[l], ref_forward(host, sub, act, 0, x, theta[:n]))
        a = np.array([host.mlp_bwd_ref_activate(act, float(v)) for v in z[l].ravel()], np.float32).reshape(z[l].shape)
        assert same_bits(a, ref_forward(host, sub, act, 1, x, theta[:n]))


def test_relu_delta_is_plus_zero_where_z_is_not_positive(host):
    sizes, M = [27, 33, 16, 5], 67
    x, theta, dy = make_problem(np.random.default_rng(5), sizes, M)
    got = ref_train_and_back(host, sizes, RELU, 1, x, theta, dy)
    z = saved_layers(sizes, 1, got["saved"], M)
    g_last = dy
    for l in (2, 1, 0):
        off = z[l] <= 0
        assert 0.1 < off.mean() < 0.9
        assert (got["delta"][l].view(np.uint32)[off] == 0).all()
        if l == 2:  # where z > 0 delta is the incoming gradient itself
            assert same_bits(got["delta"][l][~off], g_last[~off])
    assert host.mlp_bwd_ref_activate_grad(RELU, float("nan"), 1.0) == 0.0
    assert host.mlp_bwd_ref_activate_grad(RELU, -0.0, -1.0) == 0.0
    assert math.copysign(1.0, host.mlp_bwd_ref_activate_grad(RELU, -1.0, -1.0)) == 1.0


def test_activation_derivatives_spelled_out(host):
    rng = np.random.default_rng(6)
    for z, g in zip(rng.uniform(-6, 6, 200).astype(np.float32), rng.standard_normal(200).astype(np.float32)):
        z64 = float(z)
        s = 1.0 / (1.0 + math.exp(-z64))
        want = float(g) * (s + z64 * s * (1.0 - s))
        assert abs(host.mlp_bwd_ref_activate_grad(SWISH, z64, float(g)) - want) <= 4e-6 * max(abs(float(g)), 1e-30)
        want = float(g) * (1.0 - math.tanh(z64) ** 2)
        assert abs(host.mlp_bwd_ref_activate_grad(TANH, z64, float(g)) - want) <= 4e-6 * max(abs(float(g)), 1e-30)


@pytest.mark.parametrize("act", [RELU, SWISH, TANH])
def test_zero_dy_gives_plus_zero_bits(host, act):
    sizes, M = [5, 7, 4], 1057
    x, theta, dy = make_problem(np.random.default_rng(7), sizes, M)
    got = ref_train_and_back(host, sizes, act, 0, x, theta, np.zeros_like(dy))
    assert (got["dtheta"].view(np.uint32) == 0).all() and (got["dx"].view(np.uint32) == 0).all()


def test_row_order_inside_a_tile_matters_and_chunk_order_of_integers_does_not(host):
    rng = np.random.default_rng(8)
    sizes, M = [5, 7, 4], 2 * CHUNK
    x, theta, dy = make_problem(rng, sizes, M)
    plain = ref_train_and_back(host, sizes, SWISH, 0, x, theta, dy)
    perm = np.arange(M)
    perm[:TILE] = rng.permutation(TILE)  # the rows of the first tile among themselves
    moved = ref_train_and_back(host, sizes, SWISH, 0, x[perm], theta, dy[perm])
    assert same_bits(moved["dx"], plain["dx"][perm]) and same_bits(moved["y"], plain["y"][perm])
    assert not same_bits(moved["dtheta"], plain["dtheta"])
    np.testing.assert_allclose(moved["dtheta"], plain["dtheta"], rtol=1e-4, atol=1e-7)
    # one layer without activation on small integers: every partial is an exact integer, so the two
    # chunks may change places
    sizes = [5, 4]
    xi = rng.integers(-8, 9, (M, 5)).astype(np.float32)
    dyi = rng.integers(-8, 9, (M, 4)).astype(np.float32)
    th = rng.integers(-4, 5, param_count(sizes)).astype(np.float32)
    a = ref_train_and_back(host, sizes, SWISH, 0, xi, th, dyi)
    swap = np.concatenate([np.arange(CHUNK, M), np.arange(CHUNK)])
    b = ref_train_and_back(host, sizes, SWISH, 0, xi[swap], th, dyi[swap])
    assert same_bits(a["dtheta"], b["dtheta"]) and np.abs(a["dtheta"]).max() > 100


@pytest.mark.parametrize("M", [1023, 1024, 1025, 2049])
def test_tile_and_chunk_order_against_a_direct_spelling(host, M):
    rng = np.random.default_rng(M)
    sizes = [3, 2, 2]
    x, theta, dy = make_problem(rng, sizes, M)
    dy = (dy * M).astype(np.float32)  # order-1 summands: the float32 chains round at every step
    got = ref_train_and_back(host, sizes, TANH, 0, x, theta, dy)
    z0 = saved_layers(sizes, 0, got["saved"], M)[0]
    a1 = np.array([host.mlp_bwd_ref_activate(TANH, float(v)) for v in z0.ravel()], np.float32).reshape(z0.shape)
    inputs = [x, a1]
    for l, (off, n_in, n_out) in enumerate(blocks(sizes)):
        block = got["dtheta"][off:off + (n_in + 1) * n_out].reshape(n_in + 1, n_out)
        for i in range(n_in + 1):
            for j in range(n_out):
                a = None if i == n_in else np.ascontiguousarray(inputs[l][:, i])
                d = np.ascontiguousarray(got["delta"][l][:, j])
                want, partials = direct_sum(a, d)
                assert same_bits(block[i, j], want), (l, i, j)
                ps = np.full((M + CHUNK - 1) // CHUNK, np.nan, np.float64)
                one = host.mlp_bwd_ref_sum(M, _p(a), 1, _p(d), 1, _p(ps, DP))
                assert same_bits(np.float32(one), want) and np.array_equal(ps, partials)
    # the bias row equals the same order run on a constant-one feature
    ones = np.ones(M, np.float32)
    for l, (off, n_in, n_out) in enumerate(blocks(sizes)):
        for j in range(n_out):
            d = np.ascontiguousarray(got["delta"][l][:, j])
            assert same_bits(got["dtheta"][off + n_in * n_out + j], np.float32(host.mlp_bwd_ref_sum(M, _p(ones), 1, _p(d), 1, None)))


def integer_problem(rng, n_in, n_out, M):
    """One non-activated layer on asymmetric small integers: every product, sum and partial is exact."""
    x = rng.integers(-7, 12, (M, n_in)).astype(np.float32)
    dy = rng.integers(-5, 9, (M, n_out)).astype(np.float32)
    W = rng.integers(-6, 10, (n_in, n_out)).astype(np.float32)
    b = rng.integers(-3, 4, n_out).astype(np.float32)
    theta = np.concatenate([W.ravel(), b])
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    want_dtheta = np.concatenate([(x64.T @ dy64).ravel(), dy64.sum(0)]).astype(np.float32)
    want_dx = (dy64 @ W.astype(np.float64).T).astype(np.float32)
    want_y = (x64 @ W.astype(np.float64) + b).astype(np.float32)
    return x, theta, dy, want_y, want_dtheta, want_dx


@pytest.mark.parametrize("n_in,n_out,M", [(3, 5, 7), (35, 37, 70), (6, 4, 1100)])
def test_integer_layout(host, n_in, n_out, M):
    """A transpose, a swapped k order or a misplaced bias row shows as a wrong integer."""
    x, theta, dy, want_y, want_dtheta, want_dx = integer_problem(np.random.default_rng(n_in), n_in, n_out, M)
    got = ref_train_and_back(host, [n_in, n_out], SWISH, 0, x, theta, dy)
    assert got["saved"].size == 0
    assert same_bits(got["y"], want_y) and same_bits(got["dtheta"], want_dtheta) and same_bits(got["dx"], want_dx)
    assert same_bits(got["delta"][0], dy)
    assert same_bits(ref_train_and_back(host, [n_in, n_out], SWISH, 0, x, theta, dy, want_dx=False)["dtheta"], want_dtheta)


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "mlp_bwd_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DMLP_BWD_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
