"""CPU: the restatement of generalised advantage estimation (pob_gae_step / gae_ref of
po-brax_amd/csrc/pob_mlp.h, built for the host by tests/host/gae_host.cpp).

Accuracy: against a float64 numpy spelling of brax v1 PPO's ``compute_gae`` (the scan plus the two
shifted passes, recalled, [ext]), next to the same spelling in float32 numpy as the yardstick; per
output, max |ours - f64| <= 4 x max |f32 - f64| + ulp32(max |f64|).  The last term is derived,
not measured: the float32 rounding of the result itself.  Measured over the 24 cases below
(the test prints each before it asserts): the restatement's error is at most 0.27 of the bound
(vs, T = 20, lambda 0.95, discount 0.99) and 0.25 (advantages, the same case); the largest
absolute errors are 3.9e-5 (vs) and 3.7e-5 (advantages) at T = 200, lambda = discount = 1, where
the float32 numpy spelling has the same.  DESIGN.md "Critic pass and GAE".

Exact properties are bitwise.  The stand-alone program (-DGAE_MAIN) runs once under
-fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "gae_host.cpp")
FP = C.POINTER(C.c_float)


def build_gae_host(d):
    so = os.path.join(str(d), "gae_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    lib.gae_ref_run.argtypes = [C.c_int, C.c_longlong, FP, FP, C.c_int, FP, C.c_float, FP, FP, C.c_float, C.c_float, FP, FP]
    return lib


def ref_gae(lib, truncation, second, done_input, reward, reward_scale, values, bootstrap, lam, disc, want_vs=True,
            want_adv=True):
    """gae_ref on float32 copies: (vs, advantages), None for an output that was not asked for."""
    arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (truncation, second, reward, values, bootstrap)]
    T, B = arrs[3].shape
    assert arrs[4].shape == (B,) and all(a is None or a.shape == (T, B) for a in arrs[:3])
    vs = np.full((T, B), np.nan, np.float32) if want_vs else None
    adv = np.full((T, B), np.nan, np.float32) if want_adv else None
    p = lambda a: None if a is None else a.ctypes.data_as(FP)  # noqa: E731
    assert lib.gae_ref_run(T, B, p(arrs[0]), p(arrs[1]), int(done_input), p(arrs[2]), reward_scale, p(arrs[3]), p(arrs[4]),
                           lam, disc, p(vs), p(adv)) == 0
    return vs, adv


def brax_gae(truncation, termination, rewards, values, bootstrap, lam, disc, dtype):
    """brax v1 ppo.compute_gae with every operation in ``dtype``: (vs, advantages)."""
    truncation, termination, rewards, values, bootstrap = (np.asarray(a, dtype) for a in (
        truncation, termination, rewards, values, bootstrap))
    lam, disc, one = dtype(lam), dtype(disc), dtype(1)
    mask = one - truncation
    v_tp1 = np.concatenate([values[1:], bootstrap[None]], axis=0)
    deltas = rewards + disc * (one - termination) * v_tp1 - values
    deltas = deltas * mask
    acc = np.zeros_like(bootstrap)
    vs_minus_v = np.empty_like(values)
    for t in range(values.shape[0] - 1, -1, -1):
        acc = deltas[t] + disc * (one - termination[t]) * mask[t] * lam * acc
        vs_minus_v[t] = acc
    vs = vs_minus_v + values
    vs_tp1 = np.concatenate([vs[1:], bootstrap[None]], axis=0)
    adv = (rewards + disc * (one - termination) * vs_tp1 - values) * mask
    assert vs.dtype == dtype and adv.dtype == dtype
    return vs, adv


def trajectory(rng, T, B):
    """done Bernoulli 0.1, half of the dones truncations; rewards N(0, 3^2), values N(0, 30^2)."""
    done = (rng.random((T, B)) < 0.1).astype(np.float32)
    trunc = (done * (rng.random((T, B)) < 0.5)).astype(np.float32)
    reward = (3.0 * rng.standard_normal((T, B))).astype(np.float32)
    values = (30.0 * rng.standard_normal((T, B))).astype(np.float32)
    boot = (30.0 * rng.standard_normal(B)).astype(np.float32)
    return dict(done=done, trunc=trunc, term=(done * (1 - trunc)).astype(np.float32), reward=reward, values=values, boot=boot)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def within_bound(ours, f32, f64, tag):
    """max |ours - f64| <= 4 max |f32 - f64| + ulp32(max |f64|); returns (ours, yardstick, bound)."""
    e_ours = float(np.abs(ours.astype(np.float64) - f64).max())
    e_yard = float(np.abs(f32.astype(np.float64) - f64).max())
    bound = 4.0 * e_yard + ulp32(np.abs(f64).max())
    print(f"{tag}: restatement {e_ours:.3e} float32 numpy {e_yard:.3e} bound {bound:.3e} ratio {e_ours / bound:.2f}")
    assert e_ours <= bound, tag
    return e_ours, e_yard, bound


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def fma32(a, b, c):
    """fmaf on float32 arrays through float64: the product is exact, the sum rounds twice (the
    double rounding differs from fmaf only on an exact float32 tie of the float64 sum)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_gae_host(tmp_path_factory.mktemp("gae_host"))


B_ACC = 257
LAM_DISC = [(0.95, 0.99), (1.0, 1.0), (0.0, 0.99), (0.95, 0.0)]


@pytest.mark.parametrize("lam,disc", LAM_DISC)
@pytest.mark.parametrize("T", [1, 2, 7, 20, 33, 200])
def test_restatement_against_float64(host, T, lam, disc):
    rng = np.random.default_rng(100 * T + LAM_DISC.index((lam, disc)))
    d = trajectory(rng, T, B_ACC)
    vs, adv = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], 1.0, d["values"], d["boot"], lam, disc)
    vs64, adv64 = brax_gae(d["trunc"], d["term"], d["reward"], d["values"], d["boot"], lam, disc, np.float64)
    vs32, adv32 = brax_gae(d["trunc"], d["term"], d["reward"], d["values"], d["boot"], lam, disc, np.float32)
    within_bound(vs, vs32, vs64, f"T {T} lambda {lam} discount {disc} vs")
    within_bound(adv, adv32, adv64, f"T {T} lambda {lam} discount {disc} advantages")


def test_termination_cuts_the_dependence(host):
    """A termination at t makes rows <= t independent of everything after t."""
    rng = np.random.default_rng(11)
    T, B, t_cut = 20, 65, 12
    d = trajectory(rng, T, B)
    d["term"][t_cut] = 1.0
    d["trunc"][t_cut] = 0.0
    vs, adv = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    e = trajectory(rng, T, B)  # other rewards, values, flags after the cut, another bootstrap
    for k in ("trunc", "term", "reward", "values"):
        e[k][:t_cut + 1] = d[k][:t_cut + 1]
    vs2, adv2 = ref_gae(host, e["trunc"], e["term"], 0, e["reward"], 1.0, e["values"], e["boot"], 0.95, 0.99)
    assert same_bits(vs[:t_cut + 1], vs2[:t_cut + 1]) and same_bits(adv[:t_cut + 1], adv2[:t_cut + 1])
    assert not same_bits(vs[t_cut + 1:], vs2[t_cut + 1:])


def test_two_episodes_back_to_back(host):
    """Rows 0 .. t1 end in a termination, rows t1 + 1 .. T - 1 are the next episode: each run alone
    with its bootstrap (the first one's is the value that follows it) gives the same rows."""
    rng = np.random.default_rng(12)
    T, B, t1 = 17, 65, 8
    d = trajectory(rng, T, B)
    d["term"][t1] = 1.0
    d["trunc"][t1] = 0.0
    args = lambda s, boot: (d["trunc"][s], d["term"][s], 0, d["reward"][s], 1.0, d["values"][s], boot, 0.95, 0.99)  # noqa: E731
    vs, adv = ref_gae(host, *args(slice(0, T), d["boot"]))
    vs_a, adv_a = ref_gae(host, *args(slice(0, t1 + 1), d["values"][t1 + 1]))
    vs_b, adv_b = ref_gae(host, *args(slice(t1 + 1, T), d["boot"]))
    assert same_bits(vs, np.concatenate([vs_a, vs_b])) and same_bits(adv, np.concatenate([adv_a, adv_b]))


def test_truncated_step(host):
    """A truncated step has advantages == 0 and vs == values, whichever spelling of the flags."""
    rng = np.random.default_rng(13)
    d = trajectory(rng, 33, 257)
    cut = d["trunc"] != 0
    assert cut.any() and (d["done"][cut] == 1).all()
    for second, done_input in ((d["term"], 0), (d["done"], 1)):
        vs, adv = ref_gae(host, d["trunc"], second, done_input, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
        assert (adv[cut] == 0).all() and (vs[cut] == d["values"][cut]).all()
        assert (adv[~cut] != 0).all()


def test_lambda_zero(host):
    """lambda = 0: vs[t] = (fmaf(g, v_{t+1}, r) - v) m + v."""
    rng = np.random.default_rng(14)
    T, B = 33, 257
    d = trajectory(rng, T, B)
    disc = np.float32(0.99)
    vs, _ = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], 1.0, d["values"], d["boot"], 0.0, float(disc))
    m = np.float32(1) - d["trunc"]
    g = disc * (np.float32(1) - d["term"])
    v_next = np.concatenate([d["values"][1:], d["boot"][None]])
    want = (fma32(g, v_next, d["reward"]) - d["values"]) * m + d["values"]
    assert want.dtype == np.float32 and np.array_equal(vs, want)


def test_reward_scale_is_a_premultiplication(host):
    rng = np.random.default_rng(15)
    d = trajectory(rng, 20, 65)
    s = np.float32(0.3)
    a = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], float(s), d["values"], d["boot"], 0.95, 0.99)
    b = ref_gae(host, d["trunc"], d["term"], 0, d["reward"] * s, 1.0, d["values"], d["boot"], 0.95, 0.99)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


def test_done_input_forms_the_termination(host):
    rng = np.random.default_rng(16)
    d = trajectory(rng, 20, 65)
    a = ref_gae(host, d["trunc"], d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    b = ref_gae(host, d["trunc"], d["done"] * (np.float32(1) - d["trunc"]), 0, d["reward"], 1.0, d["values"], d["boot"],
                0.95, 0.99)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


def test_null_truncation_is_zeros_and_null_outputs(host):
    rng = np.random.default_rng(17)
    d = trajectory(rng, 20, 65)
    z = np.zeros_like(d["trunc"])
    for done_input in (0, 1):
        a = ref_gae(host, None, d["done"], done_input, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
        b = ref_gae(host, z, d["done"], done_input, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    only_vs = ref_gae(host, z, d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99, want_adv=False)
    only_adv = ref_gae(host, z, d["done"], 1, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99, want_vs=False)
    assert only_vs[1] is None and only_adv[0] is None and same_bits(only_vs[0], b[0]) and same_bits(only_adv[1], b[1])


def test_nan_stays_in_its_env(host):
    rng = np.random.default_rng(18)
    d = trajectory(rng, 20, 65)
    clean = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    d["reward"][9, 5] = np.nan
    d["term"][:, 5] = 0.0
    d["trunc"][:, 5] = 0.0
    vs, adv = ref_gae(host, d["trunc"], d["term"], 0, d["reward"], 1.0, d["values"], d["boot"], 0.95, 0.99)
    others = np.arange(65) != 5
    assert same_bits(vs[:, others], clean[0][:, others]) and same_bits(adv[:, others], clean[1][:, others])
    assert np.isnan(vs[:10, 5]).all() and np.isnan(adv[:10, 5]).all() and np.isfinite(vs[10:, 5]).all()


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "gae_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DGAE_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
