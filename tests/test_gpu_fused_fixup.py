"""GPU: the four-lane step kernel's fix-up inside the fast pass (pob_kernels.hip quad_fixup: a block
of the block-cooperative kernels whose wall-contact store overflows writes its marks and then
steps again, from the step's inputs, in the same launch; the per-wave kernels keep the fix-up
launch: with the call in them their fast loops spilled, a build variant since removed).  The sixteen- and eight-lane
kernels are switched off, so the four-lane kernel runs at these batches; T = 4 steps.

* HH in 256-thread blocks (the block-cooperative walk: a block overflows as a whole and its live
  waves all run the fix-up) at teleported states with the block capacity lowered to 160, where
  the oracle's item record shows overflowing blocks beside blocks that never overflow: bit-exact
  against the oracle, the in-place and the functional step alike;
* HH B = 4 097 with every wave forced through the fix-up: the last block has one live wave
  (one env) and three waves past the batch;
* the mixed launch (binary16 qp, the per-wave kernel: single waves go to the fix-up) as the
  one-pass kernel, the default and forced, bit for bit the same -- from reset, and with one HH
  block arranged so that one of its waves overflows its contact pool and the other three hold
  no contact at all, both asserted from the oracle's contact statistics of the very states;
* six captured steps (GraphRollout) at the lowered capacity against the eager loop.

The per-wave kernel's overflow rule: a wave's contacts of one collide substep go to its LDS pool
of POOL = 93 (pob_quad.h QPOOL_N), every lane walking its own replica of the torso; more than
that marks the wave.  The oracle counts the torso once, so a wave whose 16 envs hold more than
93 x (detections per env) triangle contacts in a step overflows in some substep for certain,
and one whose envs hold none does not.  Seeds, placements and the capacity were chosen on the
CPU oracle alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from test_gpu_headline_parity import FLAGS, NT, _actions, _envs
from test_gpu_parity import _keys, _near_wall, _state_np, _walls, compare_states
from test_gpu_torso_once import _ItemRecord, _kinds, _teleport_offsets
from test_gpu_variants import _state_np32

pytestmark = pytest.mark.gpu
POOL = (39 * 64 - (27 * 64 + 13 * 16)) // 6  # QPOOL_N
CAP = 160                                    # POB_QUAD_BLOCK_CAP of the lowered-capacity tests


@pytest.fixture(autouse=True)
def _four_lane_only(monkeypatch):
    monkeypatch.setenv("POB_HEXA_MAX_B", "0")
    monkeypatch.setenv("POB_OCTET_MAX_B", "0")


def _wave_marks(s):
    """the mark of every live wave (a wave's mark is at its first env)"""
    return s.aux["ovf_mark"][::16].cpu().numpy() != 0


def _teleported(name, B, key_seed, L):
    env = _envs().create(name, batch_size=B, episode_length=L)
    s = env.reset(torch.from_numpy(_keys(B, key_seed)).cuda())
    off = _teleport_offsets(name, s.qp.pos[:, 0, :2].cpu().numpy(), B)
    s.qp.pos[:, :9, :2] += torch.from_numpy(off).cuda()[:, None, :]
    return env, s


def _equal_bits(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                      b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k],
                                      err_msg=f"{what}: {k}")


def test_marked_and_unmarked_blocks_in_one_launch(monkeypatch):
    """HH B = 4 290 (67 blocks + 2 envs), teleported, capacity 160.  Oracle alone (the record of
    test_gpu_torso_once.py's same states): 134 of 272 block-steps never overflow, the others do,
    in every step some of each."""
    monkeypatch.setenv("POB_QUAD_BLOCK_CAP", str(CAP))
    name, B, L = "ant_heavenhell", 4290, 1000
    env, s = _teleported(name, B, 5, L)
    o, rec = orc.OracleEnv(name), _ItemRecord(name)
    recs, marks = [], []
    for t, act in enumerate(_actions(13, B, 4)):
        before = _state_np(s)
        so = o.step(before, act, flags=FLAGS, episode_length=L, nthreads=NT)
        recs.append(rec.step(before, act, L))
        a = torch.from_numpy(act).cuda()
        f = env.step(s, a)    # functional: s is left as it was
        s = env.step_(s, a)   # in place
        compare_states(s, so, f"{name} B={B} in place, step {t}")
        _equal_bits(_state_np(f), _state_np(s), f"functional against in place, step {t}")
        m = _wave_marks(s)
        m = np.concatenate([m, np.repeat(m[-1:], -m.size % 4)]).reshape(-1, 4)
        assert (m == m[:, :1]).all()  # (a block overflows as a whole)
        marks.append(m[:, 0])
        np.testing.assert_array_equal(_wave_marks(f), _wave_marks(s))
    k = _kinds(np.stack(recs), B, CAP)
    n_blocks = -(-B // 64)
    print(f"{name} B={B}: {k}, marked blocks per step {[int(m.sum()) for m in marks]} of {n_blocks}")
    # the record: block-steps that never overflow, and block-substeps that do (with torso items)
    assert k["d_blocks_never_ovf"] > 0 and k["d_ovf_with_torso"] > 0, k
    marks = np.stack(marks)
    assert marks.any() and not marks.all(), marks.sum(1)


def test_ragged_batch_every_wave_through_the_fixup(monkeypatch):
    """HH B = 4 097, POB_QUAD_FORCE_FIXUP=1: 64 full blocks and a block with one live wave of one
    env and three waves past the batch (they leave after the block's last barrier; the live
    wave runs the fix-up).  Episode length 3: step 3 autoresets every env."""
    monkeypatch.setenv("POB_QUAD_FORCE_FIXUP", "1")
    name, B, L = "ant_heavenhell", 4097, 3
    env = _envs().create(name, batch_size=B, episode_length=L)
    keys = _keys(B, 61)
    s = env.reset(torch.from_numpy(keys).cuda())
    o = orc.OracleEnv(name)
    n_done = 0
    for t, act in enumerate(_actions(62, B, 4)):
        so = o.step(_state_np(s), act, flags=FLAGS, episode_length=L, nthreads=NT)
        s = env.step_(s, torch.from_numpy(act).cuda())
        compare_states(s, so, f"{name} B={B} forced, step {t}")
        assert _wave_marks(s).all()
        n_done += int(so["done"].sum())
    assert n_done >= B


# ------------------------------------------------------------------ the mixed launch (per-wave kernel)
NAMES = ["ant_heavenhell", "ant_gather", "ant_tag"]
SIZES = [600, 500, 401]
HEAVY = slice(64, 80)    # HH block 1's first wave ..
LIGHT = slice(80, 128)   # .. and its other three


class _ContactCount:
    """Triangle contacts (the torso once per env) and detections of one oracle step of some envs."""

    def __init__(self, name):
        self.o = orc.OracleEnv(name)
        self.L = orc.lib()
        self.buf = (C.c_longlong * 16)()

    def step(self, state, act, rows, L):
        se = {k: np.ascontiguousarray(v[rows]) for k, v in state.items()}
        self.L.orc_contact_stats_enable(1)
        try:
            self.L.orc_contact_stats(self.buf)  # (the read zeroes the counters)
            self.o.step(se, np.ascontiguousarray(act[rows]), flags=FLAGS, episode_length=L, nthreads=1)
            self.L.orc_contact_stats(self.buf)
        finally:
            self.L.orc_contact_stats_enable(0)
        return int(self.buf[2]), int(self.buf[7])


def _arranged_offsets(st, act0, L):
    """HH block 1 of the mix: each env of its first wave onto the wall point -- of 24 seeded
    candidates within 0.3 of a wall -- where the oracle counts the most contacts for that env's
    own state (st: the oracle's float32 layout) and first action; the 48 envs of its other waves
    onto a point 3 clear of every wall.  Returns the xy offsets per env (zero elsewhere)."""
    name = NAMES[0]
    walls = _walls(name)
    ext = np.array([[abs(c[0]) + max(h), abs(c[1]) + max(h)] for c, _, h in walls]).max(0)
    lo = np.array([-ext[0], min(c[1] - max(h) for c, _, h in walls)])
    hi = np.array([ext[0], max(c[1] + max(h) for c, _, h in walls)])
    rng = np.random.default_rng(3)
    cand = rng.uniform(lo, hi, (4096, 2))
    near = cand[_near_wall(cand, walls, 0.3)][:24]
    free = cand[~_near_wall(cand, walls, 3.0)][0]
    cc = _ContactCount(name)
    off = np.zeros((st["pos"].shape[0], 2), np.float32)
    for e in range(HEAVY.start, HEAVY.stop):
        best, best_n = None, -1
        for p in near:
            trial = {k: v[e:e + 1].copy() for k, v in st.items()}
            trial["pos"][0, :9, :2] += (p - st["pos"][e, 0, :2]).astype(np.float32)
            n, _ = cc.step(trial, act0[e:e + 1], slice(0, 1), L)
            if n > best_n:
                best, best_n = p, n
        off[e] = (best - st["pos"][e, 0, :2]).astype(np.float32)
    for e in range(LIGHT.start, LIGHT.stop):
        off[e] = (free - st["pos"][e, 0, :2]).astype(np.float32)
    return off


@pytest.mark.parametrize("arranged", [False, True], ids=["from_reset", "marked_and_unmarked_waves_in_a_block"])
def test_mixed_fp16_one_pass_default_and_forced_agree(monkeypatch, arranged):
    """Sizes [600, 500, 401]: the HH segment ends in a block of one and a half waves, GA and TAG
    in ragged waves.  POB_QUAD_SPLIT=0 (the one-pass kernel with the inline re-walks) against the
    default (the fast pass, overflowing waves through the fix-up) against every wave forced
    through the fix-up.  Arranged (oracle alone: the first wave of HH block 1 holds 612 contacts
    in step 0, against 93 x 5 = 465; the segment's ordinary waves 14 to 82): the wave is marked
    for certain and its block's other three waves, without a contact, are not -- asserted from
    the contact statistics of the states the default run steps, and from its marks."""
    L, T = 3, 4
    total = sum(SIZES)
    keys = _keys(total, 9)
    acts = _actions(10, total, T)
    bounds = np.concatenate([[0], np.cumsum(SIZES)])
    outs, seen = [], []
    for split, force in ((None, "0"), ("0", "0"), (None, "1")):  # default; one pass; default, all fixed up
        if split is None:
            monkeypatch.delenv("POB_QUAD_SPLIT", raising=False)
        else:
            monkeypatch.setenv("POB_QUAD_SPLIT", split)
        monkeypatch.setenv("POB_QUAD_FORCE_FIXUP", force)
        mix = _envs().create_mixed(NAMES, episode_length=L, qp_dtype=torch.float16)
        mix.batch_sizes = list(SIZES)
        ms = [e.reset(torch.from_numpy(keys[a:b]).cuda()) for e, a, b in zip(mix.envs, bounds[:-1], bounds[1:])]
        default = split is None and force == "0"
        cc = _ContactCount(NAMES[0]) if arranged and default else None
        for t in range(T):
            act = torch.from_numpy(acts[t]).cuda()
            if arranged and t == 0:
                off = _arranged_offsets(_state_np32(ms[0]), acts[0][:SIZES[0]], L)
                pos = ms[0].qp.pos.float()
                pos[:, :9, :2] += torch.from_numpy(off).cuda()[:, None, :]
                ms[0].qp.pos.copy_(pos.half())
            if cc is not None:
                st, a = _state_np32(ms[0]), acts[t][:SIZES[0]]
                heavy, det = cc.step(st, a, HEAVY, L)
                light, _ = cc.step(st, a, LIGHT, L)
                per_env = det // (HEAVY.stop - HEAVY.start)
                ms = mix.step_(ms, [x.contiguous() for x in mix.split_actions(act)])
                m = _wave_marks(ms[0])[HEAVY.start // 16: LIGHT.stop // 16]
                seen.append((heavy, light, per_env, m.tolist()))
            else:
                ms = mix.step_(ms, [x.contiguous() for x in mix.split_actions(act)])
            if force == "1":
                assert all(_wave_marks(s).all() for s in ms)
        outs.append([_state_np32(s) for s in ms])
    for what, other in (("one pass", outs[1]), ("forced", outs[2])):
        for name, a, b in zip(NAMES, outs[0], other):
            _equal_bits(a, b, f"{name}: default against {what}")
    if arranged:
        print("HH block 1 (contacts of wave 0, of waves 1-3, detections per env, marks):", seen)
        heavy, light, per_env, m = seen[0]
        assert per_env == 5 and heavy > POOL * per_env and light == 0, seen[0]
        assert m == [True, False, False, False], seen[0]


def test_graph_capture_at_lowered_capacity(monkeypatch):
    """Six captured steps of the teleported HH states at capacity 160 (marked and unmarked blocks
    in every step, as above) replayed from the graph equal the eager loop, bit for bit."""
    from po_brax_amd.rollout import GraphRollout
    monkeypatch.setenv("POB_QUAD_BLOCK_CAP", str(CAP))
    name, B, T = "ant_heavenhell", 4290, 6
    (e1, s1), (e2, s2) = (_teleported(name, B, 5, 1000) for _ in range(2))
    acts = torch.from_numpy(np.stack(_actions(13, B, T))).cuda()
    marked = []
    for t in range(T):
        s1 = e1.step_(s1, acts[t])
        marked.append(int(_wave_marks(s1).sum()))
    s2 = GraphRollout(e2, s2, acts).replay()
    torch.cuda.synchronize()
    assert all(0 < n < -(-B // 16) for n in marked), marked
    _equal_bits(_state_np(s1), _state_np(s2), "graph replay against the eager loop")
    np.testing.assert_array_equal(_wave_marks(s1), _wave_marks(s2))
