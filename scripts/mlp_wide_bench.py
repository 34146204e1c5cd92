"""mlp_wide_bench.py -- the critic's value launch through the three fused forwards.

(a) ValueFunction.values_into alone, HH's value network [114 -> 256 x 5 -> 1] under a normaliser,
    kernel="tile" (pob_mlp_forward_norm) against kernel="resident" (pob_mlp_forward_wide_norm) and
    kernel="bf16" (pob_mlp_forward_bf16_norm, its pack pass included), at 2^10 .. 2^20 rows in
    powers of four and at the critic pass's (T + 1) B = 1 376 256; the three alternate call by call
    in one process; "tile" and "resident" are compared bit for bit, "bf16" (another function) by
    its largest |difference| from "resident".
(b) AntHeavenHell, B = 65 536, T = 20: one ActorRollout replay with each critic, in turn.

Prints one JSON line.

    python scripts/mlp_wide_bench.py [--rounds 15] [--out FILE] [--skip-rollout]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "po-brax_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gae_bench import interleaved  # noqa: E402

KERNELS = ("tile", "resident", "bf16")


def summary(ms):
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}


def critics(D, normalizer):
    from po_brax_amd import jumpy
    from po_brax_amd.training import ValueFunction, networks
    vm = networks.make_models(16, D)[1]
    params = vm.init(jumpy.random_prngkey(3))
    return vm, {k: ValueFunction(vm, params, normalizer=normalizer, kernel=k) for k in KERNELS}


def bench_alone(row_counts, rounds, warmup, D=114):
    from po_brax_amd.training.normalization import ObservationNormalizer
    norm = ObservationNormalizer(D, device="cuda")
    vm, vf = critics(D, norm)
    flop_per_row = 2 * sum(a * b for a, b in zip(vm.layer_sizes[:-1], vm.layer_sizes[1:]))
    g = torch.Generator(device="cuda").manual_seed(1)
    out = []
    for N in row_counts:
        rows = torch.randn((N, D), device="cuda", generator=g)
        y = {k: torch.empty((N,), device="cuda") for k in KERNELS}
        legs = {k: (lambda k=k: vf[k].values_into(rows, y[k])) for k in KERNELS}
        ms = interleaved(legs, rounds, warmup)
        s = summary(ms)
        for k in KERNELS:
            s[k]["TFLOPs"] = round(N * flop_per_row / (s[k]["median_ms"] * 1e-3) / 1e12, 2)
        out.append({"rows": N, **s, "tile_over_resident": round(s["tile"]["median_ms"] / s["resident"]["median_ms"], 3),
                    "resident_over_bf16": round(s["resident"]["median_ms"] / s["bf16"]["median_ms"], 3),
                    "bit_equal": bool(torch.equal(y["tile"], y["resident"])),
                    "bf16_max_abs_diff": float((y["bf16"] - y["resident"]).abs().max())})
    return out


def bench_rollout(B, T, rounds, warmup):
    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout
    from po_brax_amd.training import networks
    from po_brax_amd.training.normalization import ObservationNormalizer
    keys = jumpy.random_split(jumpy.random_prngkey(0), B + 1)[1:]
    rolls = {}
    for k in KERNELS:
        env = envs.create("ant_heavenhell", batch_size=B)
        D = env.observation_size
        norm = ObservationNormalizer(D)
        pm = networks.make_models(2 * env.action_size, D)[0]
        pol = networks.NormalTanhPolicy(pm, pm.init(jumpy.random_prngkey(1)), jumpy.random_prngkey(2), normalizer=norm)
        rolls[k] = ActorRollout(env, env.reset(keys), pol, T, update_normalizer=True, critic=critics(D, norm)[1][k])
    ms = interleaved({k: r.replay for k, r in rolls.items()}, rounds, warmup)
    same = all(bool(torch.equal(getattr(rolls["tile"], a), getattr(rolls["resident"], a))) for a in ("values", "vs", "advantages"))
    diff = {a: float((getattr(rolls["bf16"], a) - getattr(rolls["resident"], a)).abs().max()) for a in ("values", "advantages")}
    return {"env": "ant_heavenhell", "batch": B, "steps": T, "replay": summary(ms), "bit_equal": same,
            "bf16_max_abs_diff": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-rollout", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    counts = [1 << p for p in range(10, 21, 2)] + [(args.steps + 1) * args.batch]
    res = {"bench": "mlp_wide_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "alone": bench_alone(counts, args.rounds, args.warmup)}
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
