"""GPU: the four-lane kernel's block-cooperative wall walk (pob_quad.h qwalls_detect_block:
the fast launch of AntHeavenHell and AntTag in 256-thread blocks, whose four waves pool a
collide substep's face items in LDS and share the walk rounds out), bit-exact against the
oracle.  The sixteen- and eight-lane kernels are switched off, so the four-lane kernel runs at
batches just above 4 096, in 256-thread blocks:
  * ragged last blocks -- one live wave holding one env and three waves past the batch
    (B = 4 097), one full live wave (4 160), two live and two past (4 224): the waves past the
    batch stay for the block's barriers and store nothing;
  * ants teleported onto the walls (many items per block);
  * the block's item capacity lowered to 16 (POB_QUAD_BLOCK_CAP), so that some blocks overflow
    at ordinary states and go to the fix-up launch while others do not."""
import numpy as np
import pytest
import torch

import orc
from test_gpu_headline_parity import FLAGS, NT, _actions, _envs, _per_step
from test_gpu_parity import _keys, _near_wall, _state_np, _walls, compare_states

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _four_lane_only(monkeypatch):
    monkeypatch.setenv("POB_HEXA_MAX_B", "0")
    monkeypatch.setenv("POB_OCTET_MAX_B", "0")


@pytest.mark.parametrize("name", ["ant_heavenhell", "ant_tag"])
@pytest.mark.parametrize("B", [4097, 4160, 4224])
def test_per_step_parity_ragged_blocks(name, B):
    _per_step(name, B, T=4, L=3, seed=B)


@pytest.mark.parametrize("name", ["ant_heavenhell", "ant_tag"])
def test_wall_stress(name):
    """test_gpu_headline_parity.test_wall_stress_256_thread_blocks' teleport at B = 4 352."""
    B, T = 4352, 4
    env = _envs().create(name, batch_size=B, episode_length=1000)
    s = env.reset(torch.from_numpy(_keys(B, 5)).cuda())
    walls = _walls(name)
    ext = np.array([[abs(c[0]) + max(h), abs(c[1]) + max(h)] for c, _, h in walls]).max(0)
    lo = np.array([-ext[0], min(c[1] - max(h) for c, _, h in walls)])
    hi = np.array([ext[0], max(c[1] + max(h) for c, _, h in walls)])
    rng = np.random.default_rng(9)
    cand = rng.uniform(lo, hi, (16 * B, 2))
    near = cand[_near_wall(cand, walls, 1.0)]
    assert len(near) >= 3 * B // 4
    xy = np.concatenate([near[: 3 * B // 4], cand[: B - 3 * B // 4]]).astype(np.float32)[rng.permutation(B)]
    off = torch.from_numpy(xy - s.qp.pos[:, 0, :2].cpu().numpy()).cuda()
    s.qp.pos[:, :9, :2] += off[:, None, :]
    o = orc.OracleEnv(name)
    for t, act in enumerate(_actions(13, B, T)):
        so = o.step(_state_np(s), act, flags=FLAGS, episode_length=1000, nthreads=NT)
        s = env.step(s, torch.from_numpy(act).cuda())
        compare_states(s, so, f"{name} wall B={B} step {t}")


@pytest.mark.parametrize("cap", [16, 28])
def test_lowered_capacity_overflows_some_blocks(monkeypatch, cap):
    """HH at spawn loads a 64-env block with a median of 15 and a p90 of 26 face items per collide
    substep (oracle statistic, scripts/walk_balance.py), so at a capacity of 16 both kinds of
    substep occur: parity stays bit-exact through the fix-up launch, and the marks show marked
    and unmarked waves.  A block is marked when ANY of the step's five collide substeps overflows
    (and the kernel counts the torso's items once per leg lane), so at 16 nearly every block is
    marked in a step (measured: 272, 272, 268, 272 of 272 waves) and the unmarked ones are few;
    the second capacity, 28, is the median over blocks of a step's LARGEST substep load in the
    same oracle statistic (26 .. 30 over these four steps), where every step must show both
    (measured: 228, 192, 216, 220 of 272)."""
    monkeypatch.setenv("POB_QUAD_BLOCK_CAP", str(cap))
    name, B, L = "ant_heavenhell", 4352, 3
    env = _envs().create(name, batch_size=B, episode_length=L)
    keys = _keys(B, 17)
    s = env.reset(torch.from_numpy(keys).cuda())
    o = orc.OracleEnv(name)
    marks = []
    for t, act in enumerate(_actions(18, B, 4)):
        so = o.step(_state_np(s), act, flags=FLAGS, episode_length=L, nthreads=NT)
        s = env.step_(s, torch.from_numpy(act).cuda())
        compare_states(s, so, f"{name} B={B} cap {cap} step {t}")
        m = s.aux["ovf_mark"][::16].cpu().numpy() != 0
        print(f"step {t}: {int(m.sum())} of {m.size} waves marked")
        # (a block overflows as a whole: its four waves carry the same mark)
        assert (m.reshape(-1, 4) == m.reshape(-1, 4)[:, :1]).all()
        marks.append(m)
    marks = np.stack(marks)
    assert marks.any() and not marks.all(), marks.sum(1)  # some but not all waves marked
    if cap == 28:
        assert marks.any(1).all() and not marks.all(1).any(), marks.sum(1)  # in every step
