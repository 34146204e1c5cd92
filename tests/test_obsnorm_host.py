"""CPU: the restatement of the running observation normaliser (pob_obsnorm_apply,
obsnorm_accumulate_ref, obsnorm_update_ref of po-brax_amd/csrc/pob_mlp.h, built for the host by
tests/host/obsnorm_host.cpp).

Three chained updates against a float64 numpy spelling of brax's two-pass ``update_fn``
(``training/normalization.py`` of brax <= 0.0.12, recalled, [ext]), next to a float32 numpy
spelling of the same formula as the yardstick: max abs error of mean, m2 and scale per column
kind, asserted ours <= 4 x yardstick + floor.  The floor is the rounding of the float32 state
itself: mean and m2 are rounded to float32 once per update (three roundings, relative 3 x 2^-24),
scale adds the rounding of the variance, of the square root and of the reciprocal (4 x 2^-24 in
all, the square root halving what came before), so floor = 2^-22 |float64 value|.  Column kinds:
mean 0 / std 1, mean 100 / std 0.01 (S2 - S1^2 / total would cancel in float32), constant.
Beyond the floor, the rounding of the stored float32 mean moves the next update's m2 to first
order (2 S1 count / total per unit of it: 3e-6 .. 8e-6 on the mean-100 columns); the float32
spelling has the same term and far larger ones, so the 4 x yardstick part covers it.

Measured figures: DESIGN.md "Observation normaliser"; the test prints each before it asserts.
The stand-alone program (-DOBSNORM_MAIN) runs once under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "obsnorm_host.cpp")
FP = C.POINTER(C.c_float)
DP = C.POINTER(C.c_double)
FLOOR = 2.0 ** -22  # relative: see the module docstring


def build_obsnorm_host(d):
    so = os.path.join(str(d), "obsnorm_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-I", CSRC, "-shared",
                           "-o", so, SRC])
    lib = C.CDLL(so)
    lib.obsnorm_ref_accumulate.argtypes = [FP, C.c_longlong, C.c_int, FP, DP]
    lib.obsnorm_ref_update.argtypes = [DP, FP, C.c_int, DP, C.c_int, C.c_longlong]
    lib.obsnorm_ref_apply.argtypes = [FP, C.c_longlong, C.c_int, FP, C.c_float]
    lib.obsnorm_ref_apply1.argtypes = [C.c_float] * 4
    lib.obsnorm_ref_apply1.restype = C.c_float
    return lib


def fresh_table(D):
    t = np.zeros((3, D), np.float32)
    t[1:] = 1.0
    return t


def ref_accumulate(lib, x, table):
    """obsnorm_accumulate_ref: x (N, D) float32 -> sums (2, D) float64."""
    x = np.ascontiguousarray(x, np.float32)
    N, D = x.shape
    sums = np.full((2, D), np.nan, np.float64)
    assert lib.obsnorm_ref_accumulate(x.ctypes.data_as(FP), N, D, table.ctypes.data_as(FP), sums.ctypes.data_as(DP)) == 0
    return sums


def ref_update(lib, count, table, shards):
    """One update from a list of row blocks (one per shard, rank order): new (count, table, sums (R, 2, D))."""
    table = table.copy()
    sums = np.ascontiguousarray(np.stack([ref_accumulate(lib, s, table) for s in shards]))
    cnt = np.array([count], np.float64)
    n_new = sum(s.shape[0] for s in shards)
    assert lib.obsnorm_ref_update(cnt.ctypes.data_as(DP), table.ctypes.data_as(FP), table.shape[1],
                                  sums.ctypes.data_as(DP), len(shards), n_new) == 0
    return float(cnt[0]), table, sums


def ref_apply(lib, x, table, clip):
    """obsnorm_apply_ref on a copy of x (B, D); table None = the identity."""
    y = np.ascontiguousarray(x, np.float32).copy()
    t = None if table is None else np.ascontiguousarray(table, np.float32)
    assert lib.obsnorm_ref_apply(y.ctypes.data_as(FP), y.shape[0], y.shape[1], None if t is None else t.ctypes.data_as(FP),
                                 clip) == 0
    return y


def brax_update(state, obs, dtype):
    """brax's two-pass update_fn on state = (steps, mean, variance-sum), every operation in ``dtype``."""
    steps, mean, var = state
    obs = obs.astype(dtype)
    total = dtype(steps + obs.shape[0])
    to_old = obs - mean
    new_mean = mean + np.sum(to_old / total, axis=0, dtype=dtype)
    to_new = obs - new_mean
    return (steps + obs.shape[0], new_mean.astype(dtype), (var + np.sum(to_new * to_old, axis=0, dtype=dtype)).astype(dtype))


def brax_scale(state, dtype):
    steps, _, var = state
    v = np.clip(var / dtype(steps + 1.0), dtype(1e-6), dtype(1e6)).astype(dtype)
    return (dtype(1.0) / np.sqrt(v)).astype(dtype)


def columns(rng, N, D):
    """Column f is of kind (f + 1) % 3: 0 mean 0 / std 1, 1 mean 100 / std 0.01, 2 constant."""
    x = rng.standard_normal((N, D))
    kind = (np.arange(D) + 1) % 3
    x[:, kind == 1] = 100.0 + 0.01 * x[:, kind == 1]
    x[:, kind == 2] = 3.25
    return x.astype(np.float32), kind


def within_bound(table, s64, s32, kind, tag):
    """ours <= 4 x (the float32 numpy spelling's error) + floor, per column kind and quantity."""
    want = {"mean": s64[1], "m2": s64[2], "scale": brax_scale(s64, np.float64)}
    ours = {"mean": table[0], "m2": table[2], "scale": table[1]}
    yard = {"mean": s32[1], "m2": s32[2], "scale": brax_scale(s32, np.float32)}
    for k in range(3):
        cols = kind == k
        if not cols.any():
            continue
        for q in ("mean", "m2", "scale"):
            w = want[q][cols]
            e_ours = np.abs(ours[q][cols].astype(np.float64) - w)
            e_yard = np.abs(yard[q][cols].astype(np.float64) - w)
            print(f"{tag} kind {k} {q}: restatement {e_ours.max():.3e} float32 numpy {e_yard.max():.3e}")
            assert (e_ours <= 4.0 * e_yard.max() + FLOOR * np.abs(w)).all(), (tag, k, q)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_obsnorm_host(tmp_path_factory.mktemp("obsnorm_host"))


@pytest.mark.parametrize("N", [1, 7, 1023, 1024, 1025, 3000])
@pytest.mark.parametrize("D", [1, 30, 114, 256])
def test_restatement_against_float64(host, D, N):
    rng = np.random.default_rng(1000 * D + N)
    count, table = 0.0, fresh_table(D)
    s64 = (0, np.zeros(D, np.float64), np.ones(D, np.float64))
    s32 = (0, np.zeros(D, np.float32), np.ones(D, np.float32))
    for step in range(3):
        x, kind = columns(rng, N, D)
        count, table, _ = ref_update(host, count, table, [x])
        s64, s32 = brax_update(s64, x, np.float64), brax_update(s32, x, np.float32)
        assert count == s64[0] == N * (step + 1)
    within_bound(table, s64, s32, kind, f"D {D} N {N}")
    # the constant column: m2 stays at its initial 1 exactly, so the variance is 1 / (count + 1)
    const = kind == 2
    if const.any():
        v = np.float32(np.clip(1.0 / (3.0 * N + 1.0), 1e-6, 1e6))
        assert (table[2][const] == 1.0).all() and (table[0][const] == np.float32(3.25)).all()
        assert (table[1][const] == np.float32(1.0) / np.sqrt(v)).all()


def test_constant_column_reaches_the_variance_floor(host):
    """With m2 = 1 the variance m2 / (count + 1) falls below the 1e-6 clamp once count passes
    1e6: scale is then 1 / sqrt(1e-6) = 1000 in the float32 steps the kernels take."""
    D, N = 4, 1025
    table = fresh_table(D)
    table[0] = 3.25
    x = np.full((N, D), 3.25, np.float32)
    count, table, _ = ref_update(host, 2.0e6, table, [x])
    clamp = np.float32(1.0) / np.sqrt(np.float32(1e-6))
    assert count == 2.0e6 + N and (table[2] == 1.0).all() and (table[0] == np.float32(3.25)).all()
    assert (table[1] == clamp).all() and abs(float(clamp) - 1000.0) <= 1000.0 * FLOOR
    # and the upper clamp 1e6: scale 1 / sqrt(1e6) = 0.001
    table = fresh_table(D)
    table[2] = 3e38
    _, table, _ = ref_update(host, 0.0, table, [x * 0])
    assert (table[1] == np.float32(1.0) / np.sqrt(np.float32(1e6))).all()


def test_sums_order_is_chunked(host):
    """The (2, D) sums are the chunk partials added in ascending chunk order: recomputed here
    chunk by chunk with Python floats (float64), fma spelled exactly through integers."""
    import math
    rng = np.random.default_rng(5)
    N, D = 2 * 1024 + 5, 3
    x = rng.integers(-50, 50, (N, D)).astype(np.float32) / 8.0  # d and d^2 exact: every order agrees
    table = fresh_table(D)
    table[0] = [0.0, 1.5, -2.25]
    sums = ref_accumulate(host, x, table)
    d = x.astype(np.float64) - table[0].astype(np.float64)
    assert np.array_equal(sums[0], d.sum(0)) and np.array_equal(sums[1], (d * d).sum(0))
    # inexact data: equal to the chunked order, and not to one long chain
    x = rng.standard_normal((N, D)).astype(np.float32)
    sums = ref_accumulate(host, x, table)
    d = x.astype(np.float64) - table[0].astype(np.float64)
    for f in range(D):
        T1, chain = 0.0, 0.0
        for c0 in range(0, N, 1024):
            S1 = 0.0
            for v in d[c0:c0 + 1024, f]:
                S1 = S1 + float(v)
            T1 = T1 + S1
        for v in d[:, f]:
            chain = chain + float(v)
        assert sums[0, f] == T1
        assert math.isclose(chain, T1, rel_tol=1e-12)
    assert host.obsnorm_ref_chunk() == 1024


def test_initial_table_is_the_identity(host):
    rng = np.random.default_rng(6)
    x = rng.uniform(-5, 5, (9, 30)).astype(np.float32)
    x[0, :4] = [5.0, -5.0, 0.0, -0.0]
    y = ref_apply(host, x, fresh_table(30), 5.0)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(ref_apply(host, x * 3, None, 5.0), x * 3)  # no table: untouched


def test_apply_edges(host):
    f = lambda x, m, s, c: np.float32(host.obsnorm_ref_apply1(x, m, s, c))  # noqa: E731
    # the clamp's edges: +-clip pass, the next float beyond is clamped
    up, dn = np.nextafter(np.float32(5), np.float32(9)), np.nextafter(np.float32(5), np.float32(0))
    assert f(5.0, 0.0, 1.0, 5.0) == 5.0 and f(up, 0.0, 1.0, 5.0) == 5.0 and f(dn, 0.0, 1.0, 5.0) == dn
    assert f(-5.0, 0.0, 1.0, 5.0) == -5.0 and f(-up, 0.0, 1.0, 5.0) == -5.0 and f(-dn, 0.0, 1.0, 5.0) == -dn
    assert f(np.inf, 0.0, 1.0, 5.0) == 5.0 and f(-np.inf, 0.0, 1.0, 5.0) == -5.0
    # clip = 0: no clamp
    assert f(1e6, 1.0, 2.0, 0.0) == np.float32((np.float32(1e6) - np.float32(1)) * np.float32(2))
    assert f(np.inf, 0.0, 1.0, 0.0) == np.inf
    # NaN stays NaN with and without the clamp
    assert np.isnan(f(np.nan, 0.0, 1.0, 5.0)) and np.isnan(f(np.nan, 0.0, 1.0, 0.0))
    assert np.isnan(f(1.0, np.nan, 1.0, 5.0))
    # -0.0 keeps its sign; x == mean gives +0
    assert np.signbit(f(-0.0, 0.0, 1.0, 5.0)) and f(-0.0, 0.0, 1.0, 5.0) == 0.0
    assert not np.signbit(f(2.5, 2.5, 3.0, 5.0))
    # two roundings, not one fused: (x - m) rounds before the multiply
    x, m, s = np.float32(1.0000001), np.float32(1e-8), np.float32(3.0000002)
    assert f(x, m, s, 0.0) == np.float32(np.float32(x - m) * s)


def test_two_shards_update(host):
    """R = 2: the halves accumulated separately and updated together stay within the same bound
    of float64."""
    rng = np.random.default_rng(8)
    N, D = 2055, 30
    count, table = 0.0, fresh_table(D)
    s64 = (0, np.zeros(D, np.float64), np.ones(D, np.float64))
    s32 = (0, np.zeros(D, np.float32), np.ones(D, np.float32))
    for _ in range(3):
        x, kind = columns(rng, N, D)
        count, table, sums = ref_update(host, count, table, [x[:N // 2], x[N // 2:]])
        assert sums.shape == (2, 2, D)
        s64, s32 = brax_update(s64, x, np.float64), brax_update(s32, x, np.float32)
    assert count == 3 * N
    within_bound(table, s64, s32, kind, f"R 2 D {D} N {N}")


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "obsnorm_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DOBSNORM_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
