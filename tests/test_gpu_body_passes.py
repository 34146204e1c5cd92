"""GPU: the per-body publish and apply passes of the four-lane kernel's block-cooperative wall
walk (pob_quad.h qwalls_detect_block, qcontacts_position / _velocity COOP: a lane's items are
published and its contact slots applied body by body -- torso, Aux, lower leg -- each in a loop
of its own, pob_blockwalk.h bw_body_ranges), bit-exact against the oracle on every field.  The
sixteen- and eight-lane kernels are switched off, so the four-lane kernel runs at batches just
above 4 096, in 256-thread blocks, for T = 4 steps.

What can go wrong is a lane whose contacts span bodies, so every test asserts -- from the
oracle's own item record of the very states the kernel stepped (the FLOP build's statistics
hook, scripts/walk_balance.py; one (env, leg) lane holds the torso's, its Aux's and its lower
leg's items) -- that its states hold at least one lane-substep of each kind it is there for:
  (a) items on the Aux and on the lower leg at once;
  (b) a torso item;
  (c) items on all three bodies at once;
  (d) three or more items on one body;
  (e) a lane with items in a ragged last block (waves past the batch beside it).
AntHeavenHell's spawn states give (a) and, at a ragged batch, (e), never (b) .. (d) (their
largest lane load is 3 items); ants teleported onto the walls (test_gpu_block_walk.py
test_wall_stress) give all five, for AntTag too, whose spawn states hold almost no items.  The
teleported batches also load a block with a median of 160 and a p90 of 244 items per collide
substep against its capacity of 200, so overflowed blocks (empty ranges, the fix-up launch) and
normal ones mix there; the last test lowers the capacity (POB_QUAD_BLOCK_CAP) to mix them at
spawn states.  Seeds and batches were chosen on the CPU oracle alone.
(The torso's record is taken under leg 0's wall mask, so (b) and (c) count leg-0 lanes only.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from test_gpu_headline_parity import FLAGS, NT, _actions, _envs
from test_gpu_parity import _keys, _near_wall, _state_np, _walls, compare_states

pytestmark = pytest.mark.gpu
NSUB = 5  # collide substeps per step


@pytest.fixture(autouse=True)
def _four_lane_only(monkeypatch):
    monkeypatch.setenv("POB_HEXA_MAX_B", "0")
    monkeypatch.setenv("POB_OCTET_MAX_B", "0")


class _ItemRecord:
    """The oracle's face items per env, collide substep and body of one step from a state."""

    def __init__(self, name):
        self.o = orc.OracleEnv(name, count_flops=True)
        self.L = self.o._L
        self.L.orc_items_record.argtypes = [C.POINTER(C.c_int), C.c_int]

    def step(self, state, act, episode_length):
        buf = np.zeros((act.shape[0], NSUB, 9), np.int32)
        self.L.orc_items_record(buf.ctypes.data_as(C.POINTER(C.c_int)), NSUB)
        self.L.orc_flops_set_mode(orc.FLOPS_EXECUTED)
        try:
            self.o.step(state, act, flags=FLAGS, episode_length=episode_length, nthreads=1)  # (the hook is single-threaded)
        finally:
            self.L.orc_items_record(None, 0)
            self.L.orc_flops_set_mode(orc.FLOPS_REF_PAIRS)
        lanes = np.zeros((act.shape[0], 4, NSUB, 3), np.int64)  # (env, leg, substep, body slot)
        for k in range(4):
            lanes[:, k, :, 0] = buf[:, :, 0]
            lanes[:, k, :, 1] = buf[:, :, 2 * k + 1]
            lanes[:, k, :, 2] = buf[:, :, 2 * k + 2]
        return lanes


def _kinds(lanes, B):
    """lane-substeps of the kinds (a) .. (e) in the records (steps, env, leg, substep, slot)"""
    leg0 = lanes[:, :, 0]
    ragged = lanes[:, 64 * (B // 64):]
    return dict(a=int(((lanes[..., 1] > 0) & (lanes[..., 2] > 0)).sum()),
                b=int((leg0[..., 0] > 0).sum()),
                c=int((leg0 > 0).all(-1).sum()),
                d=int((lanes >= 3).any(-1).sum()),
                e=int((ragged.sum(-1) > 0).sum()))


def _teleport_onto_walls(name, s, B):
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


def _run(name, B, key_seed, act_seed, L, teleport=False, marks=None):
    env = _envs().create(name, batch_size=B, episode_length=L)
    s = env.reset(torch.from_numpy(_keys(B, key_seed)).cuda())
    if teleport:
        _teleport_onto_walls(name, s, B)
    o, rec = orc.OracleEnv(name), _ItemRecord(name)
    lanes = []
    for t, act in enumerate(_actions(act_seed, B, 4)):
        before = _state_np(s)
        so = o.step(before, act, flags=FLAGS, episode_length=L, nthreads=NT)
        lanes.append(rec.step(before, act, L))
        s = env.step_(s, torch.from_numpy(act).cuda())
        compare_states(s, so, f"{name} B={B} step {t}")
        if marks is not None:
            marks.append(s.aux["ovf_mark"][::16].cpu().numpy() != 0)
    kinds = _kinds(np.stack(lanes), B)
    print(f"{name} B={B}: lane-substeps (a) {kinds['a']} (b) {kinds['b']} (c) {kinds['c']} (d) {kinds['d']} (e) {kinds['e']}")
    return kinds


def test_spawn_states_ragged_block():
    """HH from reset at B = 4 130 = 64 blocks + 34 envs (two full waves, one with two envs, one
    past the batch).  Oracle alone: (a) 2 801, (e) 126 lane-substeps."""
    k = _run("ant_heavenhell", 4130, 4130, 4131, L=3)
    assert k["a"] > 0 and k["e"] > 0, k


def test_spawn_states_tag():
    """AntTag from reset (almost no items: the passes' early exits), same ragged batch."""
    _run("ant_tag", 4130, 4130, 4131, L=3)


@pytest.mark.parametrize("name", ["ant_heavenhell", "ant_tag"])
def test_teleported_onto_walls(name):
    """B = 4 290 = 67 blocks + 2 envs.  Oracle alone: HH (a) 33 026 (b) 8 968 (c) 1 839 (d) 2 392
    (e) 49, TAG (a) 30 959 (b) 14 683 (c) 2 952 (d) 2 929 (e) 28; a lane holds up to 13 items."""
    k = _run(name, 4290, 5, 13, L=1000, teleport=True)
    assert min(k.values()) > 0, k


def test_lowered_capacity_mixes_overflowed_and_normal_blocks(monkeypatch):
    """test_gpu_block_walk.py's capacity 28 (the median over blocks of a step's largest substep
    load at HH spawn states): every step marks some blocks for the fix-up launch -- their lanes'
    ranges are empty from the overflowing substep on -- and leaves others."""
    monkeypatch.setenv("POB_QUAD_BLOCK_CAP", "28")
    marks = []
    k = _run("ant_heavenhell", 4352, 17, 18, L=3, marks=marks)
    assert k["a"] > 0, k
    marks = np.stack(marks)
    assert marks.any(1).all() and not marks.all(1).any(), marks.sum(1)
