"""gae_bench.py -- what the critic pass costs: pob_gae alone and inside the actor rollout.

(a) pob_gae alone against the baseline a user has without it: brax's compute_gae spelled in eager
    torch ops as a reverse Python loop (that spelling lives here, not in the library), at
    (T, B) = (20, 65 536), (20, 4 096), (1000, 4 096); the two alternate call by call and the
    median of each is reported, with the kernel's achieved share of the 6.3 TB/s a streaming copy
    reaches on this chip (it moves 6 x 4 x T B bytes: four arrays in, two out).
(b) AntHeavenHell, B = 65 536, T = 20: rollout.ActorRollout with and without critic= (policy and
    critic sharing one ObservationNormalizer, update_normalizer=True), replayed in turn; the
    difference is the critic pass.  The value launch ([D -> 256 x 5 -> 1] over (T + 1) B rows) and
    the GAE launch are also timed on their own on the rollout's buffers.

Prints one JSON line.

    python scripts/gae_bench.py [--rounds 15] [--out FILE] [--skip-rollout]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "po-brax_amd"))

HBM_STREAM = 6.3e12  # bytes/s of a float4 copy on the MI355X (8.0e12 peak)


def torch_loop_gae(truncation, termination, rewards, values, bootstrap, lam, disc):
    """brax's compute_gae in eager torch ops: the reverse scan as a Python loop, then the shifted pass."""
    mask = 1.0 - truncation
    v_tp1 = torch.cat([values[1:], bootstrap[None]], 0)
    g = disc * (1.0 - termination)
    deltas = (rewards + g * v_tp1 - values) * mask
    acc = torch.zeros_like(bootstrap)
    out = []
    for t in range(values.shape[0] - 1, -1, -1):
        acc = deltas[t] + g[t] * mask[t] * lam * acc
        out.append(acc)
    vs = torch.stack(out[::-1]) + values
    vs_tp1 = torch.cat([vs[1:], bootstrap[None]], 0)
    adv = (rewards + g * vs_tp1 - values) * mask
    return vs, adv


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def interleaved(legs, rounds, warmup):
    for _ in range(warmup):
        for fn in legs.values():
            timed(fn)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    return ms


def bench_alone(T, B, rounds, warmup):
    from po_brax_amd.training import compute_gae
    g = torch.Generator(device="cuda").manual_seed(T * 131 + B)
    done = (torch.rand((T, B), device="cuda", generator=g) < 0.1).float()
    trunc = done * (torch.rand((T, B), device="cuda", generator=g) < 0.5).float()
    term = done * (1.0 - trunc)
    rewards = 3.0 * torch.randn((T, B), device="cuda", generator=g)
    values = 30.0 * torch.randn((T, B), device="cuda", generator=g)
    boot = 30.0 * torch.randn((B,), device="cuda", generator=g)
    out = (torch.empty((T, B), device="cuda"), torch.empty((T, B), device="cuda"))
    legs = {
        "kernel": lambda: compute_gae(trunc, term, rewards, values, boot, out=out),
        "torch_loop": lambda: torch_loop_gae(trunc, term, rewards, values, boot, 0.95, 0.99),
    }
    vs_t, adv_t = legs["torch_loop"]()
    legs["kernel"]()
    torch.cuda.synchronize()
    err = max(float((out[0] - vs_t).abs().max()), float((out[1] - adv_t).abs().max()))
    ms = interleaved(legs, rounds, warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_bytes = 6 * 4 * T * B
    return {
        "T": T, "B": B, "bytes": n_bytes,
        "kernel_us": round(med["kernel"] * 1e3, 2), "kernel_min_us": round(min(ms["kernel"]) * 1e3, 2),
        "kernel_max_us": round(max(ms["kernel"]) * 1e3, 2),
        "torch_loop_us": round(med["torch_loop"] * 1e3, 2), "torch_loop_min_us": round(min(ms["torch_loop"]) * 1e3, 2),
        "torch_loop_max_us": round(max(ms["torch_loop"]) * 1e3, 2),
        "speedup": round(med["torch_loop"] / med["kernel"], 2),
        "kernel_TBps": round(n_bytes / (med["kernel"] * 1e-3) / 1e12, 4),
        "kernel_share_of_6.3TBps": round(n_bytes / (med["kernel"] * 1e-3) / HBM_STREAM, 4),
        "hbm_us_at_6.3TBps": round(n_bytes / HBM_STREAM * 1e6, 2),
        "max_abs_difference_of_the_two": err,
    }


def bench_rollout(B, T, rounds, warmup):
    from po_brax_amd import _lib, envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import ValueFunction, networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    keys = jumpy.random_split(jumpy.random_prngkey(0), B + 1)[1:]
    es = [envs.create("ant_heavenhell", batch_size=B) for _ in range(2)]
    ss = [e.reset(keys) for e in es]
    A, D = es[0].action_size, es[0].observation_size
    rolls = {}
    for i, leg in enumerate(("plain", "critic")):
        norm = ObservationNormalizer(D)
        pm, vm = networks.make_models(2 * A, D)
        pol = networks.NormalTanhPolicy(pm, pm.init(jumpy.random_prngkey(1)), jumpy.random_prngkey(2), normalizer=norm)
        kw = {}
        if leg == "critic":
            critic = ValueFunction(vm, vm.init(jumpy.random_prngkey(3)), normalizer=norm)
            kw = {"critic": critic}
        rolls[leg] = ActorRollout(es[i], ss[i], pol, T, update_normalizer=True, **kw)
    r = rolls["critic"]

    def value_alone():
        critic.values_into(r._obs_buffer.view((T + 1) * B, D), r.values.view(-1))

    def gae_alone():
        _lib.check(_lib.lib.pob_gae(T, B, _lib.ptr(r.truncation), _lib.ptr(r.done), 1, _lib.ptr(r.reward), 1.0,
                                    _lib.ptr(r.values), _lib.ptr(r.values[T]), 0.95, 0.99, _lib.ptr(r.vs),
                                    _lib.ptr(r.advantages), _lib.stream_handle()))

    legs = {"plain": rolls["plain"].replay, "critic": r.replay, "value": value_alone, "gae": gae_alone}
    ms = interleaved(legs, rounds, warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    sizes = vm.layer_sizes
    flop = 2 * (T + 1) * B * sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))
    return {
        "env": "ant_heavenhell", "batch": B, "steps": T, "obs_width": D, "value_network": list(sizes),
        "plain_ms_per_replay": round(med["plain"], 4), "critic_ms_per_replay": round(med["critic"], 4),
        "critic_pass_ms": round(med["critic"] - med["plain"], 4),
        "value_launch_alone_ms": round(med["value"], 4), "gae_launch_alone_us": round(med["gae"] * 1e3, 2),
        "value_rows": (T + 1) * B, "value_flop": flop, "value_TFLOPs": round(flop / (med["value"] * 1e-3) / 1e12, 2),
        "min_ms": {k: round(min(v), 4) for k, v in ms.items()}, "max_ms": {k: round(max(v), 4) for k, v in ms.items()},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-rollout", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"bench": "gae_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "alone": [bench_alone(T, B, args.rounds, args.warmup) for T, B in ((20, 65536), (20, 4096), (1000, 4096))]}
    if not args.skip_rollout:
        res["rollout"] = bench_rollout(args.batch, args.steps, args.rounds, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
