#!/usr/bin/env python3
"""Walk-round statistics behind DESIGN.md §8 (round 6): from the oracle's per-body face items
(statistics hook, as scripts/wall_walk_stats.py) over a random-action rollout, the sixteen-lane
kernel's walk rounds per step -- per wave (4 envs, 8 items a round) against cooperation over a
block of 2 or 4 waves, two interleaved rounds per lane ("double rounds" at a relative cost D),
and an env-to-wave permutation balanced by the previous step's item counts.  What matters is
the slowest wave per step (the kernel waits for it).

    python scripts/walk_balance.py [env] [B] [steps]     (e.g. ant_heavenhell 4096 20)
"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import orc, pob_np as P
name = sys.argv[1] if len(sys.argv) > 1 else "ant_heavenhell"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
NSUB = 5
e = orc.OracleEnv(name, count_flops=True)
L = e._L
L.orc_items_record.argtypes = [C.POINTER(C.c_int), C.c_int]
s = e.reset(P.split(P.prngkey(0), B + 1)[1:], first=True)
rng = np.random.default_rng(0)
buf = np.zeros((B, NSUB, 9), np.int32)
L.orc_items_record(buf.ctypes.data_as(C.POINTER(C.c_int)), NSUB)
L.orc_flops_set_mode(orc.FLOPS_EXECUTED)
rec = []
try:
    for t in range(steps):
        buf[:] = 0
        s = e.step(s, rng.uniform(-1, 1, (B, 8)).astype(np.float32), flags=orc.F_EPISODE | orc.F_AUTORESET, nthreads=1, inplace=True)  # (the hook keeps its cursor in globals: one thread)
        rec.append(buf.copy())
finally:
    L.orc_items_record(None, 0); L.orc_flops_set_mode(orc.FLOPS_REF_PAIRS)
rec = np.stack(rec)  # (steps, B, NSUB, 9) items per body
items = rec.sum(-1)  # per env per substep
def rounds(env_items, epg, groups):
    # env_items (steps, B, NSUB); envs per cooperating unit epg, items per round `groups`
    S, Bn, N = env_items.shape
    u = env_items.reshape(S, Bn // epg, epg, N).sum(2)  # (steps, units, NSUB)
    r = np.ceil(u / groups).sum(-1)  # rounds per step per unit
    return r
for label, epg, groups in (("wave of 4 envs, 8 groups (hex now)", 4, 8),
                           ("block of 4 waves = 16 envs, 32 groups", 16, 32),
                           ("block of 2 waves = 8 envs, 16 groups", 8, 16)):
    r = rounds(items, epg, groups)
    print(f"{label:42s} rounds/step: mean {r.mean():.2f}  max over units per step (mean over steps) {r.max(1).mean():.2f}  max {r.max():.0f}")
# double rounds: a substep with k items costs ceil(k/8) rounds now; with two chains per lane,
# ceil(k/16) double rounds of cost D (relative to a single round) + a single round if the rest <= 8
def cost(u, D):
    full = np.floor(u / 16); rest = u - 16 * full
    return full * D + np.where(rest > 8, D, np.where(rest > 0, 1.0, 0.0))
u = items.reshape(items.shape[0], -1, 4, items.shape[2]).sum(2)  # per wave (4 envs)
for D in (1.3, 1.5, 1.7):
    c = cost(u, D).sum(-1)
    print(f"double-round cost {D}: slowest wave per step mean {c.max(1).mean():.2f} (single: {np.ceil(u/8).sum(-1).max(1).mean():.2f}), mean {c.mean():.2f}")
# env -> wave permutation from the previous step's per-env item totals: heavy envs dealt
# round-robin over the waves (sorted descending, snake order), light ones fill
S, Bn, NS = items.shape
W = Bn // 4
def rounds_for(perm, it):
    u = it[perm].reshape(W, 4, NS).sum(1)
    return np.ceil(u / 8).sum(-1)
base, bal = [], []
for t in range(1, S):
    prev = items[t - 1].sum(-1)
    order = np.argsort(-prev, kind="stable")
    # snake deal: rank r -> wave (r mod W) going forward, then backward
    waves = np.empty(Bn, int)
    r = np.arange(Bn); blk = r // W; pos = r % W
    waves[order] = np.where(blk % 2 == 0, pos, W - 1 - pos)
    perm = np.argsort(waves, kind="stable")  # envs grouped by wave
    bal.append(rounds_for(perm, items[t]).max())
    base.append(rounds_for(np.arange(Bn), items[t]).max())
print(f"slowest wave rounds per step: identity {np.mean(base):.2f}, balanced by previous step {np.mean(bal):.2f}")

# ---- the four-lane kernel (pob_quad.h): lane (env, leg k) holds three body slots -- the torso
# (its items once per leg lane), Aux k+1, lower leg k -- 16 envs per wave, 64 per 256-thread block.
# Per-wave walk (mesh_wave_walk): a round takes the next item of the first eight lanes holding
# one and, with groups to spare, the second item of the same slot of lanes holding two.
# Block-cooperative walk (pob_blockwalk.h): the block's T items make ceil(T / 8) rounds, wave w
# takes the rounds r = (w + substep) mod 4, + 4, ..
def lane_slots(rec_t):  # (B, NSUB, 9) -> (B, 4, NSUB, 3): per lane and slot
    Bn = rec_t.shape[0]
    out = np.zeros((Bn, 4, rec_t.shape[1], 3), np.int64)
    for k in range(4):
        out[:, k, :, 0] = rec_t[:, :, 0]
        out[:, k, :, 1] = rec_t[:, :, 2 * k + 1]
        out[:, k, :, 2] = rec_t[:, :, 2 * k + 2]
    return out
def wave_rounds(slots):  # (64, 3) item counts of a wave's lanes in a substep -> rounds of the per-wave walk
    s = [list(x) for x in slots if x.sum() > 0]
    rounds = 0
    while s:
        rounds += 1
        n1 = len(s)
        spare = 8 - min(8, n1)
        for i, x in enumerate(s):
            if i >= 8: break
            q = next(j for j in range(3) if x[j] > 0)
            x[q] -= 1
            if spare > 0 and x[q] > 0:
                x[q] -= 1
                spare -= 1
        s = [x for x in s if sum(x) > 0]
    return rounds
if Bn % 64 == 0:
    now_w, now_b, pool_w, pool_b, blk_items, wav_items = [], [], [], [], [], []
    once_b, once_w, once_items = [], [], []  # the torso's items once per quad (pob_quad.h qwalls_detect_block)
    for t in range(S):
        ls = lane_slots(rec[t]).reshape(Bn // 16, 64, NS, 3)  # (waves, lanes, NSUB, 3)
        wi = ls.sum((1, 3))  # (waves, NSUB) items per wave and substep
        bi = wi.reshape(-1, 4, NS).sum(1)  # (blocks, NSUB)
        r_now = np.array([[wave_rounds(ls[w, :, n]) if wi[w, n] else 0 for n in range(NS)] for w in range(ls.shape[0])])
        R = -(-bi // 8)  # (blocks, NSUB) pooled rounds
        r_pool = np.zeros_like(r_now)
        for w in range(4):
            first = (w + np.arange(NS)) % 4
            r_pool[w::4] = np.maximum(0, -(-(R - first[None, :]) // 4))
        now_w.append(r_now.sum(1)); pool_w.append(r_pool.sum(1))
        now_b.append(r_now.sum(1).reshape(-1, 4).sum(1)); pool_b.append(R.sum(1))
        blk_items.append(bi); wav_items.append(wi)
        # the torso's items published by leg lane 0 alone: the other three lanes hold their own only
        lo = ls.copy().reshape(-1, 16, 4, NS, 3)
        lo[:, :, 1:, :, 0] = 0
        bo = lo.sum((1, 2, 4)).reshape(-1, 4, NS).sum(1)  # (blocks, NSUB)
        Ro = -(-bo // 8)
        r_once = np.zeros_like(r_now)
        for w in range(4):
            first = (w + np.arange(NS)) % 4
            r_once[w::4] = np.maximum(0, -(-(Ro - first[None, :]) // 4))
        once_b.append(Ro.sum(1)); once_w.append(r_once.sum(1)); once_items.append(bo)
    now_w, pool_w, now_b, pool_b = map(np.stack, (now_w, pool_w, now_b, pool_b))
    bi, wi = np.concatenate(blk_items).ravel(), np.concatenate(wav_items).ravel()
    print(f"four-lane: items per wave and collide substep mean {wi.mean():.1f} p90 {np.percentile(wi, 90):.0f} max {wi.max()}; "
          f"substeps with an item {100 * (wi > 0).mean():.0f} %")
    print(f"four-lane: items per block and collide substep median {np.median(bi):.0f} p90 {np.percentile(bi, 90):.0f} "
          f"p99.9 {np.percentile(bi, 99.9):.0f} max {bi.max()}; largest substep of a block's step: median "
          f"{np.median(np.concatenate(blk_items).max(1)):.0f}")
    print(f"four-lane per-wave walk: rounds per wave per step mean {now_w.mean():.2f} p99 {np.percentile(now_w, 99):.0f} "
          f"max {now_w.max()}, slowest wave per step {now_w.max(1).mean():.2f}, per block {now_b.mean():.2f}")
    print(f"four-lane pooled walk:   rounds per wave per step mean {pool_w.mean():.2f}, slowest wave per step "
          f"{pool_w.max(1).mean():.2f}, per block {pool_b.mean():.2f} ({100 * (pool_b.mean() / now_b.mean() - 1):+.0f} %)")
    once_b, once_w, bo = np.stack(once_b), np.stack(once_w), np.concatenate(once_items).ravel()
    print(f"four-lane pooled walk, torso once per quad: items per env and collide substep {bi.sum() / (S * Bn * NS):.3f} -> "
          f"{bo.sum() / (S * Bn * NS):.3f}, rounds per block per step {pool_b.mean():.2f} -> {once_b.mean():.2f}, slowest block per step "
          f"{pool_b.max(1).mean():.2f} -> {once_b.max(1).mean():.2f}, slowest wave per step {pool_w.max(1).mean():.2f} -> "
          f"{once_w.max(1).mean():.2f}, largest block load {bi.max()} -> {bo.max()}")
