"""CPU: the restatement of the fused Adam step (pob_adam_bias / pob_adam_elem / adam_step_ref of
po-brax_amd/csrc/pob_mlp.h, built for the host by tests/host/adam_host.cpp) and the torch-op path of
``training.optim.FusedAdam``.

Accuracy: every step against the textbook float64 Adam (``Adam64`` of learner_ref.py, its moments
carried in float64 over the 3 steps) from the restatement's own float32 theta before the step; per
element |after - want| <= ulp32(theta_before) + 1e-6 lr, the bound torch's Adam is held to in
learner_ref.check_update (DESIGN.md "Learner against a float64 learner").  The test prints the worst
ratio before it asserts.

Exact properties are bitwise.  The stand-alone program (-DADAM_MAIN) runs once under
-fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from learner_ref import Adam64

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "adam_host.cpp")
FP = C.POINTER(C.c_float)
LR, BETA1, BETA2, EPS = 3e-4, 0.9, 0.999, 1e-8
LENGTHS = [1, 3, 63, 64, 65, 255, 1027]


def build_adam_host(d):
    so = os.path.join(str(d), "adam_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    lib.adam_ref_run.argtypes = [C.c_int, C.POINTER(FP), C.POINTER(FP), C.POINTER(FP), C.POINTER(FP),
                                 C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.c_float, C.c_float, C.c_float, C.c_float]
    return lib


def ref_step(lib, theta, grad, m, v, state, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """adam_step_ref IN PLACE on lists of float32 arrays (one segment each) and state (2,) float64."""
    k = len(theta)
    for a in (*theta, *grad, *m, *v):
        assert a.dtype == np.float32 and a.flags.c_contiguous
    assert state.dtype == np.float64 and all(len(x) == k for x in (grad, m, v))
    arr = lambda xs: (FP * k)(*[x.ctypes.data_as(FP) for x in xs])  # noqa: E731
    n = (C.c_longlong * k)(*[x.size for x in theta])
    assert lib.adam_ref_run(k, arr(theta), arr(grad), arr(m), arr(v), n, state.ctypes.data_as(C.POINTER(C.c_double)),
                            lr, beta1, beta2, eps) == 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def problem(rng, n, grad_scale):
    theta = (0.5 * rng.standard_normal(n)).astype(np.float32)
    grads = [(grad_scale * rng.standard_normal(n)).astype(np.float32) for _ in range(3)]
    return theta, grads


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_adam_host(tmp_path_factory.mktemp("adam_host"))


@pytest.mark.parametrize("grad_scale", [1.0, 1e-3, 1e-8])
def test_restatement_against_float64(host, grad_scale):
    rng = np.random.default_rng(5)
    worst = 0.0
    for n in LENGTHS:
        theta, grads = problem(rng, n, grad_scale)
        m, v, state = np.zeros(n, np.float32), np.zeros(n, np.float32), np.ones(2, np.float64)
        opt = Adam64(LR)
        for g in grads:
            before = theta.copy()
            ref_step(host, [theta], [g], [m], [v], state)
            want = opt.step(before, g)
            bound = np.spacing(np.abs(before)).astype(np.float64) + 1e-6 * LR
            worst = max(worst, float((np.abs(theta.astype(np.float64) - want) / bound).max()))
            assert np.abs(theta - before).max() > 0
    print(f"adam_step_ref, gradients ~ {grad_scale:g}: worst step at {worst:.3f} of ulp32(theta) + 1e-6 lr")
    assert worst <= 1.0


def test_zero_gradient_and_zero_m_leave_theta(host):
    rng = np.random.default_rng(6)
    n = 257
    theta = (0.5 * rng.standard_normal(n)).astype(np.float32)
    theta[:4] = [0.0, -0.0, np.float32(1e-45), -np.float32(3e-39)]
    v = rng.uniform(0.0, 1.0, n).astype(np.float32)
    v[::3] = 0.0
    before, v_before = theta.copy(), v.copy()
    m, g, state = np.zeros(n, np.float32), np.zeros(n, np.float32), np.array([0.9, 0.999])
    ref_step(host, [theta], [g], [m], [v], state)
    assert np.array_equal(bits(theta), bits(before))
    assert not m.any() and np.array_equal(bits(v), bits(np.float32(BETA2) * v_before))


def test_segments_do_not_interact(host):
    rng = np.random.default_rng(7)
    segs = [problem(rng, n, 0.1) for n in (65, 1027, 3, 64)]
    state0 = np.array([0.9, 0.999]) ** 5
    together = [[t.copy() for t, _ in segs], [np.zeros_like(t) for t, _ in segs], [np.zeros_like(t) for t, _ in segs]]
    state = state0.copy()
    ref_step(host, together[0], [g[0] for _, g in segs], together[1], together[2], state)
    for k, (t, g) in enumerate(segs):
        alone = [t.copy(), np.zeros_like(t), np.zeros_like(t)]
        s = state0.copy()
        ref_step(host, [alone[0]], [g[0]], [alone[1]], [alone[2]], s)
        assert all(np.array_equal(bits(alone[j]), bits(together[j][k])) for j in range(3))
        assert np.array_equal(s, state)


def test_state_block_holds_the_running_products(host):
    rng = np.random.default_rng(8)
    theta, grads = problem(rng, 65, 0.1)
    m, v, state = np.zeros(65, np.float32), np.zeros(65, np.float32), np.ones(2, np.float64)
    b1, b2 = float(np.float32(BETA1)), float(np.float32(BETA2))  # beta widened from float32
    p1 = p2 = 1.0
    for k in range(7):
        ref_step(host, [theta], [grads[k % 3]], [m], [v], state)
        p1, p2 = p1 * b1, p2 * b2
        assert state[0] == p1 and state[1] == p2, k


@pytest.mark.parametrize("lengths", [(65,), (1027, 3), (1, 63, 64, 255, 5)])
def test_fused_adam_on_cpu_leaves_is_the_restatement(host, lengths):
    from po_brax_amd.training.optim import FusedAdam
    rng = np.random.default_rng(10)
    segs = [problem(rng, n, 0.1) for n in lengths]
    leaves = [torch.from_numpy(t.copy()).requires_grad_(True) for t, _ in segs]
    opt = FusedAdam(leaves, lr=LR, betas=(BETA1, BETA2), eps=EPS)
    ref = [[t.copy() for t, _ in segs], [np.zeros_like(t) for t, _ in segs], [np.zeros_like(t) for t, _ in segs]]
    state = np.ones(2, np.float64)
    ptrs = [p.data_ptr() for p in leaves]
    for step in range(3):
        for p, (_, g) in zip(leaves, segs):
            p.grad = torch.from_numpy(g[step].copy())
        opt.step()
        for lo in range(0, len(segs), 4):  # the restatement takes four segments a call
            s = state.copy()
            hi = lo + 4
            ref_step(host, ref[0][lo:hi], [g[step] for _, g in segs[lo:hi]], ref[1][lo:hi], ref[2][lo:hi], s)
        state = s
        for k, p in enumerate(leaves):
            assert np.array_equal(bits(p.detach().numpy()), bits(ref[0][k])), (step, k)
            assert np.array_equal(bits(opt.m[k].numpy()), bits(ref[1][k])), (step, k)
            assert np.array_equal(bits(opt.v[k].numpy()), bits(ref[2][k])), (step, k)
        assert np.array_equal(opt.bias.numpy(), state)
        opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in leaves)
    assert [p.data_ptr() for p in leaves] == ptrs
    # the state dict carries m, v and the bias block into another optimiser
    other = FusedAdam([torch.zeros_like(p).requires_grad_(True) for p in leaves], lr=1.0)
    other.load_state_dict(opt.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.m + other.v + [other.bias], opt.m + opt.v + [opt.bias]))
    assert other.param_groups[0]["lr"] == LR and other.m[0].data_ptr() != opt.m[0].data_ptr()


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "adam_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DADAM_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
