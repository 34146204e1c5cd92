"""CPU: the restatement of the inference window (gru_sequence_forward_ref of po-brax_amd/csrc/pob_mlp.h,
built for the host by tests/host/gru_seq_infer_host.cpp), the specification of k_gru_seq_infer and of
``pob_gru_sequence_forward`` (DESIGN.md "Recurrent critic").

Everything is bitwise.  The chain it is held to is the existing single-step reference, compiled from
gru_bwd_host.cpp (``gru_bwd_ref_step`` on the gathered rows normalised by ``gru_bwd_ref_obsnorm``), and
the existing training forward's ``y`` (``gru_bwd_ref_forward``).  ``problem``, ``chain`` and
``check_window`` are shared with test_gpu_gru_seq_infer.py, which runs the same checks on the kernel.
The stand-alone program (-DGRU_SEQ_INFER_MAIN) runs once under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gru_bwd_host import CSRC, FP, HERE, I32P, IP, _net, _p, bits, build_gru_bwd_host, param_count, ref_forward, same_bits
from test_gru_bwd_host import problem as bwd_problem

SRC = os.path.join(HERE, "host", "gru_seq_infer_host.cpp")
SWISH = 1
# (pre sizes with the observation width first, hidden, post sizes): the critic's last width is 1
NETS = {
    "7-gru5-1": ([7], 5, [1]),
    "30-gru64-1": ([30], 64, [1]),
    "114-32-gru33-16-1": ([114, 32], 33, [16, 1]),
}
CANARY = np.float32(-7.25e10)
GUARD = 2  # rows behind every output that must keep the canary
RESETS = ("none", "tenth", "nan", "negzero")


def build_seq_infer_host(d):
    so = os.path.join(str(d), "gru_seq_infer_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    lib.gru_seq_infer_ref.argtypes = [C.c_int, IP, C.c_int, C.c_int, IP, C.c_int, C.c_int, C.c_longlong, C.c_longlong, FP, I32P,
                                      FP, FP, FP, C.c_float, FP, FP, FP, FP, C.c_int]
    lib.gru_seq_infer_ref.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gru_seq_infer_host")
    return build_seq_infer_host(d), build_gru_bwd_host(d)


def problem(seed, net, S, M, use_idx, use_norm, reset_kind, act=SWISH):
    """One window: obs (S, B, D) ~ U[-3, 3], h0 (B, H) ~ U[-1, 1] (never exactly 0), lecun-uniform theta.
    ``use_idx``: B = M + 3 envs, idx a permutation's first M entries with the last one repeating the
    first (M >= 2).  ``reset_kind``: "none" (NULL); "tenth" (about a tenth of the entries set, entry
    [0][first env] clear); "nan" / "negzero": the tenth with entry [0][first env] a NaN (counts as set)
    / -0.0 (does not)."""
    pre, H, post = net
    rng = np.random.default_rng(seed)
    B = M + 3 if use_idx else M
    pr = bwd_problem(rng, net, S, M, B)
    idx = None
    if use_idx:
        idx = rng.permutation(B)[:M].astype(np.int32)
        if M >= 2:
            idx[-1] = idx[0]
    first = int(idx[0]) if use_idx else 0
    reset = None
    if reset_kind != "none":
        reset = (rng.uniform(size=(S, B)) < 0.1).astype(np.float32)
        reset[0, first] = {"tenth": 0.0, "nan": np.nan, "negzero": -0.0}[reset_kind]
    norm = None
    if use_norm:
        norm = np.stack([0.5 * rng.standard_normal(pre[0]), rng.uniform(0.5, 2.0, pre[0]), np.ones(pre[0])]).astype(np.float32)
    assert (pr["h0"] != 0).all()
    return dict(net=net, act=act, S=S, M=M, B=B, obs=pr["obs"], h0=pr["h0"], theta=pr["theta"], idx=idx, reset=reset,
                norm=norm, clip=2.5)


def host_runner(lib):
    """run(prob, h_out_step, alias) -> dict(y, h_first, h_out, h0_after) of gru_sequence_forward_ref, every
    output with GUARD canary rows behind it; ``alias``: h_out is h0 itself."""
    def run(pb, h_out_step, alias=False):
        pre, H, post = pb["net"]
        S, M, B = pb["S"], pb["M"], pb["B"]
        y = np.full(S * M * post[-1] + GUARD, CANARY, np.float32)
        h_first, h_out = (np.full((M + GUARD, H), CANARY, np.float32) for _ in range(2))
        h0 = pb["h0"].copy()
        assert lib.gru_seq_infer_ref(*_net(pb["net"]), pb["act"], S, M, B, _p(pb["obs"]), _p(pb["idx"], I32P), _p(h0),
                                     _p(pb["reset"]), _p(pb["norm"]), pb["clip"], _p(pb["theta"]), _p(y), _p(h_first),
                                     _p(h0 if alias else h_out), h_out_step) == 0
        return dict(y=y, h_first=h_first, h_out=h0 if alias else h_out, h0_after=h0)
    return run


def chain(bwd, pb):
    """(y (S, M, out), h_first (M, H), [state after s + 1 steps]) of S chained gru_forward_ref steps."""
    pre, H, post = pb["net"]
    S, M = pb["S"], pb["M"]
    sel = np.arange(M) if pb["idx"] is None else pb["idx"]
    h = np.ascontiguousarray(pb["h0"][sel])
    ys, states, h_first = [], [], None
    for s in range(S):
        x = np.ascontiguousarray(pb["obs"][s, sel])
        bwd.gru_bwd_ref_obsnorm(_p(x), M, pre[0], _p(pb["norm"]), pb["clip"])
        rs = None if pb["reset"] is None else np.ascontiguousarray(pb["reset"][s, sel])
        yt, h_new, h_copy = (np.full(sh, np.nan, np.float32) for sh in ((M, post[-1]), (M, H), (M, H)))
        bwd.gru_bwd_ref_step(*_net(pb["net"]), pb["act"], M, _p(x), _p(pb["theta"]), _p(rs), _p(h), _p(yt), _p(h_new),
                             _p(h_copy))
        h_first = h_copy if s == 0 else h_first
        ys.append(yt)
        states.append(h_new)
        h = h_new
    return np.stack(ys), h_first, states


def check_window(run, bwd, pb):
    """Every bitwise property of one window, for the host restatement and the kernel alike."""
    pre, H, post = pb["net"]
    S, M = pb["S"], pb["M"]
    n_y = S * M * post[-1]
    y_c, h_first_c, states = chain(bwd, pb)
    y_t, h_last_t, _ = ref_forward(bwd, pb["net"], pb["act"], pb["obs"], pb["h0"], pb["theta"], pb["idx"], pb["reset"],
                                   pb["norm"], pb["clip"])
    sel = np.arange(M) if pb["idx"] is None else pb["idx"]
    want_first = pb["h0"][sel].copy()
    if pb["reset"] is not None:
        want_first[pb["reset"][0, sel] != 0] = 0.0  # NaN != 0 is True, -0.0 != 0 is False
    outs = {step: run(pb, step) for step in sorted({1, S})}
    for step, o in outs.items():
        y = o["y"][:n_y].reshape(S, M, post[-1])
        assert same_bits(y, y_c), "y against the chained single step"
        assert same_bits(y, y_t), "y against the training forward's"
        assert same_bits(o["h_out"][:M], states[step - 1]), f"h_out at step {step}"
        assert same_bits(o["h_first"][:M], want_first) and same_bits(o["h_first"][:M], h_first_c)
        assert same_bits(o["h0_after"], pb["h0"])
        for name in ("y", "h_first", "h_out"):
            tail = o[name].reshape(-1)[-(GUARD if name == "y" else GUARD * H):]
            assert (bits(tail) == bits(np.full_like(tail, CANARY))).all(), f"{name}: a guard row was written"
    assert same_bits(outs[S]["h_out"][:M], h_last_t)
    if pb["idx"] is None:  # h_out = h0: nothing else changes
        for step, o in outs.items():
            a = run(pb, step, alias=True)
            assert same_bits(a["y"], o["y"]) and same_bits(a["h_first"], o["h_first"])
            assert same_bits(a["h_out"][:M], o["h_out"][:M])
    return outs


@pytest.mark.parametrize("M", [1, 31, 33])
@pytest.mark.parametrize("S", [1, 3, 9])
@pytest.mark.parametrize("name", list(NETS))
def test_window_is_the_chain(libs, name, S, M):
    """y = the chained single step = the training forward's y; h_out at steps 1 and S = the chain's state;
    h_first = h0 gathered, zero exactly where reset[0] is set; h_out = h0 changes nothing else; no guard
    row written -- with and without idx (a repeated env), a normaliser, and every reset variant."""
    lib, bwd = libs
    run = host_runner(lib)
    seed = 0
    for use_idx in (False, True):
        for use_norm in (False, True):
            for kind in RESETS:
                seed += 1
                pb = problem(1000 * S + 10 * M + seed, NETS[name], S, M, use_idx, use_norm, kind)
                outs = check_window(run, bwd, pb)
                first = outs[1]["h_first"][0]
                if kind == "nan":
                    assert not bits(first).any()
                else:
                    assert same_bits(first, pb["h0"][0 if pb["idx"] is None else pb["idx"][0]])


def test_resets_inside_the_window_matter(libs):
    """The reset rows are live: clearing them changes y (so a reference that ignored them would show)."""
    lib, bwd = libs
    run = host_runner(lib)
    pb = problem(5, NETS["30-gru64-1"], 9, 33, False, True, "tenth")
    assert pb["reset"][1:].any()
    y = run(pb, 9)["y"]
    y0 = run(dict(pb, reset=None), 9)["y"]
    assert not same_bits(y, y0)


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gru_seq_infer_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DGRU_SEQ_INFER_MAIN", "-I", CSRC, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
