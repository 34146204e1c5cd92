"""``bench.py --dump-outputs DIR``: the State the last timed step left, written as DIR/<name>.npy.

CPU: ``bench.dump_outputs`` on a hand-made State -- names, dtypes (float32; the uint32 PRNG keys
exact in float64), the size cap and its seeded row sample.  GPU: a plain ``bench.py`` run's dump
equals, bit for bit, the State of W + K functional ``env.step`` calls from the same keys and
actions (same kernels, same inputs: nothing to tolerate), so ``--steps`` sets the step count and
the dump is the last timed step's; the plain line carries none of the ``--full`` figures."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _state(B, N=5, D=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    rng = torch.randint(0, 2 ** 32, (B, 2), generator=g, dtype=torch.int64)
    rng[0, 0] = 2 ** 32 - 1
    return types.SimpleNamespace(
        qp=types.SimpleNamespace(pos=r(B, N, 3), rot=r(B, N, 4), vel=r(B, N, 3).half(), ang=r(B, N, 3)),
        obs=r(B, D), reward=r(B), done=r(B) > 0,
        metrics={"apples": torch.arange(B, dtype=torch.int32)},
        info={"rng": rng.to(torch.uint32), "steps": r(B), "first_obs": r(B, D), "first_qp": object()}), rng


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_state(tmp_path):
    import bench
    s, rng = _state(33)
    rep = bench.dump_outputs(str(tmp_path / "d"), s, None, 0, 1)
    got = _load(tmp_path / "d")
    assert sorted(got) == ["done", "info_rng", "info_steps", "metrics_apples", "obs", "qp_ang", "qp_pos",
                           "qp_rot", "qp_vel", "reward"]
    assert rep["files"] == 10 and rep["rows"] == {"all": 33}
    assert rep["bytes"] == sum(a.nbytes for a in got.values())
    assert {k: a.dtype for k, a in got.items() if k != "info_rng"} == {k: np.float32 for k in got if k != "info_rng"}
    assert got["info_rng"].dtype == np.float64 and np.array_equal(got["info_rng"], rng.numpy().astype(np.float64))
    assert np.array_equal(got["obs"], s.obs.numpy()) and np.array_equal(got["qp_rot"], s.qp.rot.numpy())
    assert np.array_equal(got["qp_vel"], s.qp.vel.float().numpy())
    assert np.array_equal(got["done"], s.done.numpy().astype(np.float32))
    assert np.array_equal(got["metrics_apples"], np.arange(33, dtype=np.float32))


def test_dump_cap_takes_a_fixed_row_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100_000)
    s, rng = _state(1000)  # 76 float32 + 2 float64 per row: 320 000 bytes in all, so < 100 000 / 320 rows
    rep = bench.dump_outputs(str(tmp_path / "a"), s, None, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), s, None, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    rows = a.pop("sample_rows")
    assert rows.dtype == np.float64
    rows = rows.astype(np.int64)
    n = len(rows)
    assert rep["rows"] == {"all": n} and 250 <= n <= 312 and len(set(rows)) == n and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.sort(np.random.default_rng(0).choice(1000, size=n, replace=False)))
    assert all(v.shape[0] == n for v in a.values())
    disk = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert rep["bytes"] <= 100_000 and disk <= 100_000 + 128 * (len(a) + 1)
    assert np.array_equal(a["obs"], s.obs.numpy()[rows]) and np.array_equal(a["qp_pos"], s.qp.pos.numpy()[rows])
    assert np.array_equal(a["info_rng"], rng.numpy()[rows].astype(np.float64))


def test_dump_mixed_prefixes_each_kind(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100_000)
    states = [_state(B, seed=i)[0] for i, B in enumerate((700, 300, 40))]
    rep = bench.dump_outputs(str(tmp_path / "m"), states, bench.MIXED, 0, 1)
    got = _load(tmp_path / "m")
    assert rep["bytes"] <= 100_000 and sorted(rep["rows"]) == sorted(bench.MIXED)
    for kind, s in zip(bench.MIXED, states):
        rows = got[f"{kind}.sample_rows"].astype(np.int64)
        assert len(rows) == rep["rows"][kind]
        assert np.array_equal(got[f"{kind}.obs"], s.obs.numpy()[rows])
        assert np.array_equal(got[f"{kind}.reward"], s.reward.numpy()[rows])


@pytest.mark.gpu
@pytest.mark.parametrize("env,extra", [("ant_heavenhell", []), ("ant_tag", ["--no-graph"]),
                                       ("ant_gather", ["--groups", "2"])])
def test_plain_run_dumps_the_last_timed_step(tmp_path, env, extra):
    import bench
    from po_brax_amd import envs, jumpy
    from po_brax_amd.sharding import shard_keys
    B, W, K = 200, 3, 6
    d = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                          "--warmup", str(W), "--env", env, "--global-batch", str(B), "--dump-outputs", str(d),
                          *extra], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == K and line["warmup"] == W and line["ms_per_step"] > 0
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(B * 1e3 / line["ms_per_step"], rel=1e-2)
    assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None
    assert line["outputs"]["rows"] == {"all": B}
    got = _load(d)

    dev = torch.device("cuda", 0)
    key = jumpy.random_prngkey(0, device=dev)
    e = envs.create(env, batch_size=B, episode_length=1000, device=dev)
    s = e.reset(shard_keys(key, B, 1, 0))
    act_key = jumpy.random_split(key, B + 1)[0].contiguous()
    act = torch.empty((B, 8), dtype=torch.float32, device=dev)
    for _ in range(W + K):
        s = e.step(s, jumpy.random_actions_(act_key, B, 0, act))
    want = bench.output_arrays(s)
    assert sorted(got) == sorted(want)
    for name, t in want.items():
        if t.dtype == torch.uint32:
            w = (t.view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF).astype(np.float64)
        else:
            w = t.to(torch.float32).cpu().numpy()
        assert got[name].dtype == w.dtype and got[name].shape == w.shape, name
        assert np.array_equal(got[name], w, equal_nan=True), name
    assert np.isfinite(got["obs"]).all() and got["info_steps"].max() == W + K
