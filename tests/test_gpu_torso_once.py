"""GPU: the torso's items once per lane quad in the four-lane kernel's block-cooperative wall walk
(pob_quad.h qwalls_detect_block: the four lanes of an env hold the same
torso, so only quad lane 0 counts and publishes the torso's face items and all four lanes apply
the torso's contacts from that lane's slots, pob_blockwalk.h bw_quad_ranges), and the one hit
scan per collide substep (bw_hit_bits: a 32-bit hit mask per body, a body past its width
sends the block to the fix-up launch), bit-exact against the oracle on every field.  The
sixteen- and eight-lane kernels are switched off, so the four-lane kernel runs at batches just
above 4 096, in 256-thread blocks, for T = 4 steps.

Every test asserts -- from the oracle's own item record of the very states the kernel stepped
(the FLOP build's statistics hook, as tests/test_gpu_body_passes.py; the torso's record is taken
under leg 0's wall mask, the mask of the quad's lane 0) -- that its states hold the kinds it is
there for:
  (a) an env-substep with a torso item where leg 0 (quad lane 0: the publisher) holds no item of
      its own but another leg does;
  (b) an env-substep where the torso holds the env's only items;
  (c) a torso item in env B - 1 of a ragged batch (the lanes and waves past the batch replay
      that env): B = 4 097, one env in the last block, and B = 4 113, two live waves there;
  (d) with the capacity lowered (POB_QUAD_BLOCK_CAP), a block that overflows in a substep in
      which it holds torso items, beside blocks that never overflow;
  (e) with the hit mask's width lowered (POB_QUAD_HIT_WIDTH), bodies with more items than fit,
      on HH and TAG.
Ants teleported onto the walls (test_gpu_body_passes.py's recipe) give torso items in quantity;
for (c) env B - 1 is placed by hand with its torso centre 0.2235 from a wall face (the torso's
radius is 0.25), where it holds a torso item and few enough others for its replayed wave.  Block loads are modelled with the torso counted once per env, as the kernel
now counts it.  Seeds, batches and capacities were chosen on the CPU oracle alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from test_gpu_headline_parity import FLAGS, NT, _actions, _envs
from test_gpu_parity import _keys, _near_wall, _state_np, _walls, compare_states

pytestmark = pytest.mark.gpu
NSUB = 5    # collide substeps per step
WCAP = 50   # QBW_WCAP: items of a wave's segment


@pytest.fixture(autouse=True)
def _four_lane_only(monkeypatch):
    monkeypatch.setenv("POB_HEXA_MAX_B", "0")
    monkeypatch.setenv("POB_OCTET_MAX_B", "0")


class _ItemRecord:
    """The oracle's face items per env, collide substep and body (0 torso, 2 k + 1 Aux k + 1,
    2 k + 2 lower leg k) of one step from a state."""

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
        return buf.astype(np.int64)


def _kinds(rec, B, cap=200, width=16):
    """rec (steps, env, substep, body) -> counts of the kinds (a) .. (e)"""
    torso = rec[..., 0]                                            # (steps, env, substep)
    legs = rec[..., 1:].reshape(*rec.shape[:3], 4, 2).sum(-1)      # (.., leg): Aux + lower leg of leg k
    others = legs[..., 1:].sum(-1)
    # the kernel's blocks: env B - 1 replayed by the lanes past the batch of its wave, the waves
    # past the batch empty; the torso once per env
    S = rec.shape[0]
    per_env = rec.sum(-1)
    n_wave_envs = -(-B // 16) * 16
    n_blk_envs = -(-B // 64) * 64
    pad = lambda a: np.concatenate([a, np.repeat(a[:, -1:], n_wave_envs - B, 1),
                                    np.zeros((S, n_blk_envs - n_wave_envs, NSUB), a.dtype)], 1)
    items, tor = pad(per_env), pad(torso)
    wave = items.reshape(S, -1, 16, NSUB).sum(2)                   # (steps, waves, substep)
    blk = wave.reshape(S, -1, 4, NSUB).sum(2)
    blk_torso = tor.reshape(S, -1, 64, NSUB).sum(2)
    ovf = (blk > cap) | (wave.reshape(S, -1, 4, NSUB) > WCAP).any(2)  # (steps, blocks, substep)
    wide = pad((rec > width).any(-1)).reshape(S, -1, 64, NSUB).any(2)  # a body past the hit mask's width
    return dict(a=int(((torso > 0) & (legs[..., 0] == 0) & (others > 0)).sum()),
                b=int(((torso > 0) & (legs.sum(-1) == 0)).sum()),
                c=int((torso[:, B - 1] > 0).sum()),
                # .. of them in steps in which that env's block never overflows (its lanes apply
                # the torso's contacts themselves; the fix-up launch steps an overflowed block)
                c_applied=int(((torso[:, B - 1] > 0) & ~ovf[:, (B - 1) // 64].any(-1)[:, None]).sum()),
                d_ovf_with_torso=int((ovf & (blk_torso > 0)).sum()),
                d_blocks_never_ovf=int((~ovf.any(-1)).sum()),
                e=int((rec > width).sum()),
                e_blocks_by_width_alone=int((wide.any(-1) & ~ovf.any(-1)).sum()),
                e_blocks_unmarked=int((~wide.any(-1) & ~ovf.any(-1)).sum()),
                torso_items=int(torso.sum()), lane_max=int(max(torso.max(), rec[..., 1:].max())))


def _teleport_offsets(name, xy0, B):
    """test_gpu_body_passes.py _teleport_onto_walls: three ants of four onto the walls"""
    walls = _walls(name)
    ext = np.array([[abs(c[0]) + max(h), abs(c[1]) + max(h)] for c, _, h in walls]).max(0)
    lo = np.array([-ext[0], min(c[1] - max(h) for c, _, h in walls)])
    hi = np.array([ext[0], max(c[1] + max(h) for c, _, h in walls)])
    rng = np.random.default_rng(9)
    cand = rng.uniform(lo, hi, (16 * B, 2))
    near = cand[_near_wall(cand, walls, 1.0)]
    assert len(near) >= 3 * B // 4
    xy = np.concatenate([near[: 3 * B // 4], cand[: B - 3 * B // 4]]).astype(np.float32)[rng.permutation(B)]
    return xy - xy0


def _last_env_onto_wall(name, xy0, B):
    """env B - 1 alone: its torso centre 0.2235 (radius 0.25) outside the long face of HH's wall
    4 -- the wall behind the spawn -- that looks at the spawn, 1.053 along it from its middle: found
    on the oracle among 4 096 random placements as one where the env holds a torso item and at
    most 3 items in every collide substep of all four steps (its wave replays it up to sixteen
    times over, and 16 x 4 items would overflow the wave's segment of 50)"""
    (cx, cy), rz, (hx, hy) = _walls(name)[4]
    a = np.deg2rad(rz)
    lx, ly = -0.4213 * hx, -(hy + 0.2235)
    p = np.array([cx + lx * np.cos(a) - ly * np.sin(a), cy + lx * np.sin(a) + ly * np.cos(a)], np.float32)
    off = np.zeros((B, 2), np.float32)
    off[B - 1] = p - xy0[B - 1]
    return off


def _run(name, B, key_seed, act_seed, L, place, cap=200, width=16, marks=None):
    env = _envs().create(name, batch_size=B, episode_length=L)
    s = env.reset(torch.from_numpy(_keys(B, key_seed)).cuda())
    off = place(name, s.qp.pos[:, 0, :2].cpu().numpy(), B)
    s.qp.pos[:, :9, :2] += torch.from_numpy(off).cuda()[:, None, :]
    o, rec = orc.OracleEnv(name), _ItemRecord(name)
    recs = []
    for t, act in enumerate(_actions(act_seed, B, 4)):
        before = _state_np(s)
        so = o.step(before, act, flags=FLAGS, episode_length=L, nthreads=NT)
        recs.append(rec.step(before, act, L))
        s = env.step_(s, torch.from_numpy(act).cuda())
        compare_states(s, so, f"{name} B={B} step {t}")
        if marks is not None:
            m = s.aux["ovf_mark"][::16].cpu().numpy() != 0        # per live wave
            m = np.concatenate([m, np.repeat(m[-1:], -m.size % 4)])   # (the last block's waves past the batch)
            assert (m.reshape(-1, 4) == m.reshape(-1, 4)[:, :1]).all()  # (a block overflows as a whole)
            marks.append(m)
    kinds = _kinds(np.stack(recs), B, cap, width)
    print(f"{name} B={B}: {kinds}")
    return kinds


@pytest.mark.parametrize("name", ["ant_heavenhell", "ant_tag"])
def test_teleported_onto_walls(name):
    """B = 4 290 = 67 blocks + 2 envs (the last block: one live wave of two envs, their quads
    replayed 8 times over, and three waves past the batch).  Oracle alone: HH (a) 2 446 (b) 215
    env-substeps, 11 964 torso items; TAG (a) 1 945 (b) 24, 15 780."""
    k = _run(name, 4290, 5, 13, L=1000, place=_teleport_offsets)
    assert k["a"] > 0 and k["b"] > 0 and k["torso_items"] > 0, k


@pytest.mark.parametrize("B,seed", [(4097, 4097), (4113, 4)])
def test_torso_item_in_last_env_of_ragged_batch(B, seed):
    """HH from reset, env B - 1 placed onto a wall face: the only env of the last block
    (B = 4 097: its wave's sixteen quads all replay it) / the only env of the last block's second
    wave (B = 4 113).  Oracle alone: B = 4 097 (c) 10 env-substeps, 8 of them in steps in which
    the last block does not overflow; B = 4 113 (c) 8, 7 (key seeds 2 and 3 of six tried gave
    none of the second kind there: the seed was chosen for it)."""
    k = _run("ant_heavenhell", B, seed, seed + 1, L=1000, place=_last_env_onto_wall)
    assert k["c"] > 0 and k["c_applied"] > 0, k


def test_lowered_capacity_overflows_blocks_with_torso_items(monkeypatch):
    """Teleported HH states at capacity 160 (about the median block load there): blocks that
    overflow in a substep in which they hold torso items beside blocks that never overflow, in
    the oracle's record (545 block-substeps of the first kind, 134 of 272 block-steps of the
    second) and in the marks."""
    cap = 160
    monkeypatch.setenv("POB_QUAD_BLOCK_CAP", str(cap))
    marks = []
    k = _run("ant_heavenhell", 4290, 5, 13, L=1000, place=_teleport_offsets, cap=cap, marks=marks)
    assert k["d_ovf_with_torso"] > 0 and k["d_blocks_never_ovf"] > 0, k
    marks = np.stack(marks)
    assert marks.any() and not marks.all(), marks.sum(1)


@pytest.mark.parametrize("name", ["ant_heavenhell", "ant_tag"])
def test_lowered_hit_width(monkeypatch, name):
    """The hit mask's width lowered to 3 items per body: the teleported states hold bodies with
    up to 5 (HH) and 7 (TAG) items, whose blocks go to the fix-up launch; the others keep the mask
    walk.  Oracle alone: HH 732 bodies past the width, 70 of 272 block-steps marked for them
    alone (133 overflow by their counts, 69 stay unmarked); TAG 1 022, 122 (88, 62)."""
    monkeypatch.setenv("POB_QUAD_HIT_WIDTH", "3")
    marks = []
    k = _run(name, 4290, 5, 13, L=1000, place=_teleport_offsets, width=3, marks=marks)
    assert k["e"] > 0 and k["e_blocks_by_width_alone"] > 0 and k["e_blocks_unmarked"] > 0, k
    marks = np.stack(marks)
    assert marks.any() and not marks.all(), marks.sum(1)
