"""CPU: the restatement of the PPO loss and its head gradient (pob_ppo_component / pob_ppo_row /
ppo_loss_ref of po-brax_amd/csrc/pob_mlp.h, built for the host by tests/host/ppo_host.cpp).

Accuracy: against float64 torch autograd of brax v1 ``compute_ppo_loss`` in brax's spelling
(``log_prob`` of the stored raw action, ``exp``, ``clamp``, ``minimum``, ``mean``, and the entropy
sampled with the same ``u``; recalled, [ext]), next to the same spelling in float32 as the yardstick;
per output, max |ours - f64| <= 4 x max |f32 - f64| + ulp32(max |f64|).  The last term is derived,
not measured: the float32 rounding of the result itself.  Rows whose float64 rho lies within
relative 1e-4 of 1 +- epsilon are left out of the dlogits comparison (the branch may legitimately
differ there); at most 1 % of the rows may be.  The maxima are taken over several independent
problems of a shape (problems_for): with one problem per shape two scalars missed the bound against
a yardstick of one lucky draw (policy_loss at M = 4096, A = 1: 3.4e-9 against 3.0e-9; entropy_loss
at M = 257, A = 1: 1.8e-12 against 1.1e-12).  The test prints every triple before it asserts; the
table is in DESIGN.md "PPO loss".

Exact properties are bitwise.  The stand-alone program (-DPPO_MAIN) runs once under
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
SRC = os.path.join(HERE, "host", "ppo_host.cpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)
DP = C.POINTER(C.c_double)
CHUNK = 1024
U_MIN = np.float32(-float.fromhex("0x1.fffffep-1"))


def build_ppo_host(d):
    so = os.path.join(str(d), "ppo_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    lib.ppo_ref_run.argtypes = [C.c_longlong, C.c_int, FP, FP, IP, FP, FP, FP, FP, FP, C.c_float, C.c_float, FP, FP, FP, DP]
    lib.ppo_ref_pieces.argtypes = [C.c_longlong, C.c_int, FP, FP, IP, FP, FP, FP, FP, FP, C.c_float, FP, FP]
    lib.ppo_ref_pieces.restype = None
    lib.ppo_ref_expf.argtypes = [C.c_float]
    lib.ppo_ref_expf.restype = C.c_float
    return lib


def _f(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _p(a, t=FP):
    return None if a is None else a.ctypes.data_as(t)


def ref_ppo(lib, d, entropy_cost=1e-4, eps=0.3, want_dlogits=True, want_dvalues=True):
    """ppo_loss_ref on the dict ``d`` (logits, values, raw, old_logp, adv, vs, u and optionally idx):
    dict of dlogits, dvalues (None when not asked for), losses (4,) and partials (n_chunks, 3)."""
    a = {k: _f(d[k]) for k in ("logits", "values", "raw", "old_logp", "adv", "vs", "u")}
    M, W = a["logits"].shape
    A = W // 2
    idx = None if d.get("idx") is None else np.ascontiguousarray(d["idx"], np.int32)
    N = a["raw"].shape[0]
    assert a["values"].shape == (M,) and a["u"].shape == (M, A) and a["raw"].shape == (N, A)
    assert all(a[k].shape == (N,) for k in ("old_logp", "adv", "vs"))
    assert (idx is None and N == M) or (idx.shape == (M,) and idx.min() >= 0 and idx.max() < N)
    dl = np.full((M, W), np.nan, np.float32) if want_dlogits else None
    dv = np.full((M,), np.nan, np.float32) if want_dvalues else None
    losses = np.full(4, np.nan, np.float32)
    partials = np.full(((M + CHUNK - 1) // CHUNK, 3), np.nan, np.float64)
    assert lib.ppo_ref_run(M, A, _p(a["logits"]), _p(a["values"]), _p(idx, IP), _p(a["raw"]), _p(a["old_logp"]),
                           _p(a["adv"]), _p(a["vs"]), _p(a["u"]), entropy_cost, eps, _p(dl), _p(dv), _p(losses),
                           _p(partials, DP)) == 0
    return dict(dlogits=dl, dvalues=dv, losses=losses, partials=partials)


def ref_pieces(lib, d, eps=0.3):
    """(factors (7, M, A), rows (6, M)) of ppo_ref_pieces."""
    a = {k: _f(d[k]) for k in ("logits", "values", "raw", "old_logp", "adv", "vs", "u")}
    M, W = a["logits"].shape
    A = W // 2
    idx = None if d.get("idx") is None else np.ascontiguousarray(d["idx"], np.int32)
    factors, rows = np.empty((7, M, A), np.float32), np.empty((6, M), np.float32)
    lib.ppo_ref_pieces(M, A, _p(a["logits"]), _p(a["values"]), _p(idx, IP), _p(a["raw"]), _p(a["old_logp"]), _p(a["adv"]),
                       _p(a["vs"]), _p(a["u"]), eps, _p(factors), _p(rows))
    return factors, rows


def _softplus(x):
    return torch.logaddexp(x, torch.zeros_like(x))


def brax_ppo(d, entropy_cost, eps, dtype, grads=True):
    """brax v1 compute_ppo_loss on NormalTanhDistribution in torch ops of ``dtype``; the gradients by
    autograd.  dict of dlogits, dvalues, losses (total, policy, value, entropy), logp, rho."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    logits, values = t(d["logits"]).requires_grad_(grads), t(d["values"]).requires_grad_(grads)
    raw, old_logp, adv, vs = t(d["raw"]), t(d["old_logp"]), t(d["adv"]), t(d["vs"])
    if d.get("idx") is not None:
        j = torch.as_tensor(np.asarray(d["idx"])).long()
        raw, old_logp, adv, vs = raw[j], old_logp[j], adv[j], vs[j]
    u = t(np.maximum(np.asarray(d["u"], np.float32), U_MIN))
    total, parts, logp, rho = brax_loss(logits, values, raw, old_logp, adv, vs, u, entropy_cost, eps)
    assert total.dtype == dtype
    out = dict(losses=torch.stack([total, *parts]).detach().numpy(), logp=logp.detach().numpy(), rho=rho.detach().numpy())
    if grads:
        total.backward()
        out.update(dlogits=logits.grad.numpy(), dvalues=values.grad.numpy())
    return out


def brax_loss(logits, values, raw, old_logp, adv, vs, u, entropy_cost, eps):
    """The formula on tensors of one dtype, rows already gathered: (total, (policy, value, entropy_loss), logp, rho)."""
    A = logits.shape[1] // 2
    loc, scale = logits[:, :A], _softplus(logits[:, A:]) + 0.001
    log_det = lambda z: 2.0 * (math.log(2.0) - z - _softplus(-2.0 * z))  # noqa: E731
    normal = -0.5 * ((raw - loc) / scale) ** 2 - torch.log(scale) - 0.5 * math.log(2.0 * math.pi)
    logp = (normal - log_det(raw)).sum(-1)
    y = loc + scale * (math.sqrt(2.0) * torch.erfinv(u))
    entropy = (0.5 + 0.5 * math.log(2.0 * math.pi) + torch.log(scale) + log_det(y)).sum(-1)
    rho = torch.exp(logp - old_logp)
    policy = -torch.minimum(rho * adv, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * adv).mean()
    v_error = vs - values
    value = (v_error * v_error).mean() * 0.5 * 0.5
    entropy_loss = -entropy_cost * entropy.mean()
    return policy + value + entropy_loss, (policy, value, entropy_loss), logp, rho


def make_inputs(rng, M, A, N=None):
    """loc, p ~ N(0, 1); raw = loc + scale N(0, 1); old_logp = the float64 new log-prob + N(0, 0.3^2);
    advantages ~ N(0, 1); vs ~ N(0, 30^2); values = vs + 3 N(0, 1); u uniform in [-1, 1).  N > M: the
    trajectory has N rows, ``idx`` (with repeats) picks the M that the logits belong to."""
    n = M if N is None else N
    idx = None if N is None else rng.integers(0, N, M).astype(np.int32)
    rows = np.arange(M) if idx is None else idx
    logits = rng.standard_normal((M, 2 * A)).astype(np.float32)
    scale = np.logaddexp(logits[:, A:].astype(np.float64), 0.0) + 0.001
    if N is None:
        raw = (logits[:, :A] + scale * rng.standard_normal((M, A))).astype(np.float32)
    else:  # a trajectory row serves several minibatch rows: their loc is drawn around ITS raw action
        raw = rng.standard_normal((n, A)).astype(np.float32)
        logits[:, :A] = (raw[rows] - scale * rng.standard_normal((M, A))).astype(np.float32)
    vs = (30.0 * rng.standard_normal(n)).astype(np.float32)
    d = dict(logits=logits, raw=raw, vs=vs, adv=rng.standard_normal(n).astype(np.float32), idx=idx,
             values=(vs[rows] + 3.0 * rng.standard_normal(M)).astype(np.float32),
             u=rng.uniform(-1.0, 1.0, (M, A)).astype(np.float32), old_logp=np.zeros(n, np.float32))
    logp64 = brax_ppo(d, 0.0, 0.3, torch.float64, grads=False)["logp"]
    old = (-3.0 * A + rng.standard_normal(n)).astype(np.float32)
    old[rows] = (logp64 + 0.3 * rng.standard_normal(M)).astype(np.float32)  # a repeated row keeps its last
    d["old_logp"] = old
    return d


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def within_bound(ours, f32, f64, tag):
    """max |ours - f64| <= 4 max |f32 - f64| + ulp32(max |f64|); returns (ours, yardstick, bound)."""
    ours, f32, f64 = (np.atleast_1d(np.asarray(a, np.float64)) for a in (ours, f32, f64))
    e_ours, e_yard = float(np.abs(ours - f64).max()), float(np.abs(f32 - f64).max())
    bound = 4.0 * e_yard + ulp32(np.abs(f64).max())
    print(f"{tag}: restatement {e_ours:.3e} float32 torch {e_yard:.3e} bound {bound:.3e} ratio {e_ours / bound:.2f}")
    assert e_ours <= bound, tag
    return e_ours, e_yard, bound


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def kept_rows(rho64, eps, M):
    """The rows whose float64 rho is NOT within relative 1e-4 of 1 +- eps; at most 1 % may be left out."""
    near = (np.abs(rho64 - (1.0 - eps)) <= 1e-4 * (1.0 - eps)) | (np.abs(rho64 - (1.0 + eps)) <= 1e-4 * (1.0 + eps))
    print(f"M {M}: {int(near.sum())} rows ({100.0 * near.mean():.3f} %) within 1e-4 of the clip edges, "
          f"{100.0 * ((rho64 < 1.0 - eps) | (rho64 > 1.0 + eps)).mean():.1f} % outside the clip range")
    assert near.sum() <= 0.01 * M
    return ~near


def check_against_float64(run, problems, entropy_cost, eps, tag):
    """``run(d)`` (dict of dlogits, dvalues, losses) within the bound of the float64 spelling, the
    maxima of the bound's three terms taken over every problem of the list (the bound compares
    maxima: a scalar output of ONE problem would be held against a yardstick of one sample)."""
    cols = {k: ([], [], []) for k in ("dlogits", "dvalues", "total", "policy_loss", "value_loss", "entropy_loss")}
    f64 = None
    for d in problems:
        got = run(d)
        f64 = brax_ppo(d, entropy_cost, eps, torch.float64)
        f32 = brax_ppo(d, entropy_cost, eps, torch.float32)
        keep = kept_rows(f64["rho"], eps, d["logits"].shape[0])
        for k, pick in (("dlogits", lambda r: r["dlogits"][keep].ravel()), ("dvalues", lambda r: r["dvalues"])):
            for col, r in zip(cols[k], (got, f32, f64)):
                col.append(np.asarray(pick(r), np.float64))
        for i, k in enumerate(("total", "policy_loss", "value_loss", "entropy_loss")):
            for col, r in zip(cols[k], (got, f32, f64)):
                col.append(np.asarray([r["losses"][i]], np.float64))
    for k, (ours, f32s, f64s) in cols.items():
        within_bound(np.concatenate(ours), np.concatenate(f32s), np.concatenate(f64s), f"{tag} {k}")
    return f64


def problems_for(M, A, seed):
    """Independent problems of M rows each: 32 at M = 1, 8 up to 1024 rows, 4 beyond.  Each of the four
    scalars is ONE number per problem, a mean whose terms cancel (the policy loss at M = 4096 is 0.016
    from terms of order 1), so its float32 error is a draw of a few ulp32 and a single problem would
    hold one draw against four times another; the bound's maxima are taken over the problems."""
    n = 32 if M == 1 else (8 if M <= 1024 else 4)
    return [make_inputs(np.random.default_rng(seed + 1000 * t), M, A) for t in range(n)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_ppo_host(tmp_path_factory.mktemp("ppo_host"))


@pytest.mark.parametrize("A", [1, 3, 8])
@pytest.mark.parametrize("M", [1, 257, 4096])
def test_restatement_against_float64(host, M, A):
    f64 = check_against_float64(lambda d: ref_ppo(host, d, 1e-4, 0.3), problems_for(M, A, 10 * M + A), 1e-4, 0.3,
                                f"M {M} A {A}")
    if M == 4096:  # both branches are covered
        clipped = (f64["rho"] < 0.7) | (f64["rho"] > 1.3)
        assert 0.1 < clipped.mean() < 0.6


def test_restatement_against_float64_large_entropy_cost(host):
    """entropy_cost = 0.01: the entropy part is no longer far below the policy part."""
    check_against_float64(lambda d: ref_ppo(host, d, 1e-2, 0.3), problems_for(257, 3, 5), 1e-2, 0.3,
                          "M 257 A 3 entropy_cost 0.01")


def test_idx_arange_equals_null_and_permutation(host):
    rng = np.random.default_rng(21)
    M, A = 257, 3
    d = make_inputs(rng, M, A)
    plain = ref_ppo(host, d)
    ar = ref_ppo(host, dict(d, idx=np.arange(M, dtype=np.int32)))
    for k in ("dlogits", "dvalues", "losses"):
        assert same_bits(plain[k], ar[k]), k
    assert np.array_equal(plain["partials"], ar["partials"])
    # minibatch row i holds what row perm[i] held and reads trajectory row perm[i]
    perm = rng.permutation(M).astype(np.int32)
    e = dict(d, logits=d["logits"][perm], values=d["values"][perm], u=d["u"][perm], idx=perm)
    shuffled = ref_ppo(host, e)
    assert same_bits(shuffled["dlogits"], plain["dlogits"][perm]) and same_bits(shuffled["dvalues"], plain["dvalues"][perm])
    assert not same_bits(shuffled["dlogits"], plain["dlogits"])


def test_branches_spelled_out(host):
    """Inside the range g_lp = -(rho adv) / M; on the clipped (inactive) side the policy gradient is
    exactly the entropy part; entropy_cost = 0 removes the den_* terms."""
    rng = np.random.default_rng(22)
    M, A, eps = 257, 3, 0.3
    d = make_inputs(rng, M, A)
    factors, rows = ref_pieces(host, d, eps)
    term, ent, dlp_loc, dlp_sc, den_loc, den_sc, sig = factors
    logp, _, neg_surr, _, g_lp, _ = rows
    inv_m = np.float32(1.0) / np.float32(M)
    rho = np.array([host.ppo_ref_expf(float(v)) for v in (logp - d["old_logp"]).astype(np.float32)], np.float32)
    lo, hi = np.float32(1.0) - np.float32(eps), np.float32(1.0) + np.float32(eps)
    inside = (rho > lo) & (rho < hi)
    s1 = rho * d["adv"]
    active = s1 <= np.clip(rho, lo, hi) * d["adv"]
    assert inside.sum() > 50 and (~active).sum() > 20 and (active & ~inside).sum() > 20 and active[inside].all()
    assert same_bits(g_lp[active], -(s1[active] * inv_m)) and (g_lp[~active] == 0).all()
    assert same_bits(neg_surr[active], -s1[active])
    prod = lambda a, b: (a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)  # noqa: E731  (one rounding)
    got = ref_ppo(host, d, 1e-4, eps)
    g_ent = -(np.float32(1e-4) * inv_m)
    off = ~active
    assert same_bits(got["dlogits"][off, :A], g_ent * den_loc[off])
    assert same_bits(got["dlogits"][off, A:], (g_ent * den_sc[off]) * sig[off])
    zero = ref_ppo(host, d, 0.0, eps)
    assert np.array_equal(zero["dlogits"][:, :A], prod(g_lp[:, None], dlp_loc))
    assert np.array_equal(zero["dlogits"][:, A:], prod(g_lp[:, None], dlp_sc) * sig)
    assert (zero["dlogits"][off] == 0).all() and zero["losses"][3] == 0
    assert same_bits(zero["dvalues"], got["dvalues"]) and same_bits(zero["losses"][1:3], got["losses"][1:3])


def test_nan_advantage_stays_in_its_row(host):
    d = make_inputs(np.random.default_rng(23), 257, 3)
    clean = ref_ppo(host, d)
    e = dict(d, adv=d["adv"].copy())
    e["adv"][100] = np.nan
    got = ref_ppo(host, e)
    others = np.arange(257) != 100
    assert same_bits(got["dlogits"][others], clean["dlogits"][others]) and same_bits(got["dvalues"], clean["dvalues"])
    assert np.isnan(got["losses"][1]) and np.isnan(got["losses"][0])
    assert same_bits(got["losses"][2:], clean["losses"][2:])


def test_null_outputs_leave_the_scalars(host):
    d = make_inputs(np.random.default_rng(24), 1025, 3, N=1500)
    full = ref_ppo(host, d)
    no_dl = ref_ppo(host, d, want_dlogits=False)
    no_dv = ref_ppo(host, d, want_dvalues=False)
    assert no_dl["dlogits"] is None and no_dv["dvalues"] is None
    assert same_bits(no_dl["losses"], full["losses"]) and same_bits(no_dv["losses"], full["losses"])
    assert same_bits(no_dl["dvalues"], full["dvalues"]) and same_bits(no_dv["dlogits"], full["dlogits"])
    assert np.array_equal(no_dl["partials"], full["partials"])


def test_u_at_the_clamp(host):
    """u = -1 (the uniform draw can return it) acts as -1 + 2^-24."""
    d = make_inputs(np.random.default_rng(25), 65, 3)
    d["u"][7, 1] = -1.0
    e = dict(d, u=d["u"].copy())
    e["u"][7, 1] = U_MIN
    a, b = ref_ppo(host, d), ref_ppo(host, e)
    assert same_bits(a["dlogits"], b["dlogits"]) and same_bits(a["losses"], b["losses"])
    assert np.isfinite(a["dlogits"]).all()


def direct_sums(terms):
    """(partials (n_chunks, 3), totals (3,)) of terms (3, M) float32: float64 adds in ascending row
    order from +0.0 inside chunks of 1024, chunk partials in ascending order from +0.0."""
    M = terms.shape[1]
    partials = []
    for r0 in range(0, M, CHUNK):
        S = [np.float64(0.0)] * 3
        for r in range(r0, min(r0 + CHUNK, M)):
            S = [S[q] + np.float64(terms[q, r]) for q in range(3)]
        partials.append(S)
    T = [np.float64(0.0)] * 3
    for S in partials:
        T = [T[q] + S[q] for q in range(3)]
    return np.array(partials, np.float64), np.array(T, np.float64)


@pytest.mark.parametrize("M", [1023, 1024, 1025, 2049])
def test_chunk_order_of_the_sums(host, M):
    d = make_inputs(np.random.default_rng(M), M, 1)
    got = ref_ppo(host, d, 1e-4, 0.3)
    _, rows = ref_pieces(host, d, 0.3)
    partials, T = direct_sums(rows[[2, 3, 1]])  # neg_surr, vl, ent
    assert got["partials"].shape == ((M + CHUNK - 1) // CHUNK, 3) and np.array_equal(got["partials"], partials)
    policy, value = np.float32(T[0] / M), np.float32(T[1] / M)
    entropy = np.float32(-np.float64(np.float32(1e-4)) * (T[2] / M))
    assert same_bits(got["losses"], np.array([(policy + value) + entropy, policy, value, entropy], np.float32))


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "ppo_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DPPO_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
