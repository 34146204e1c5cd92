"""permutation_bench.py -- what one epoch's shuffle costs on the device, and whether the native one is right
at the learner's size.

At n = 1 310 720 (HH B = 65 536, T = 20) and n = 65 536, two legs alternating call by call in one process,
the median of each reported with min .. max (a sample is --calls calls between two device events):

  native    jumpy.random_permutation(key, n, sort="native") into a preallocated workspace and out
            (pob_random_permutation: k_perm_subs, then k_sort_count / k_sort_scan / k_sort_scatter per pass)
  randperm  torch.randperm(n, device=...).to(torch.int32): the default learner's shuffle

The threefry leg through torch.sort (sort="torch") is NOT run: above n = 4 096 it takes the vendor radix
sort in which the captured update's fault was reported (DESIGN.md "Learner on the device"), cause unknown.

Once, at n = 1 310 720: the native result against numpy.  The rounds' sub keys come from random_split, their
words from random_bits (copied to the host), and numpy's stable argsort is applied round by round; the
comparison is exact.  Then one PPOLearner.update (one epoch, 32 minibatches of 40 960 rows of synthetic
buffers, backward=("native", "torch")) under permutation = "torch" and "native", alternating the same way
(--no-learner skips it).  Prints one JSON line.

    python scripts/permutation_bench.py [--rounds 15] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mlp_backward_bench import _Roll, interleaved, summary  # noqa: E402  (puts po-brax_amd on sys.path)


def check_full_size(n):
    from po_brax_amd import jumpy
    key = jumpy.random_prngkey(11)
    got = jumpy.random_permutation(key, n, sort="native").cpu().numpy()
    x, k = np.arange(n, dtype=np.int32), key
    for _ in range(jumpy.permutation_rounds(n)):
        k, sub = jumpy.random_split(k)
        x = x[np.argsort(jumpy.random_bits(sub, n).cpu().numpy(), kind="stable")]
    return bool(np.array_equal(got, x))


def bench_shuffle(n, rounds, warmup, calls):
    from po_brax_amd import jumpy
    key = jumpy.random_prngkey(3)
    ws, out = jumpy.sort_workspace(n, "cuda"), torch.empty(n, dtype=torch.int32, device="cuda")

    def native():
        for _ in range(calls):
            jumpy.random_permutation(key, n, sort="native", workspace=ws, out=out)

    def randperm():
        for _ in range(calls):
            torch.randperm(n, device="cuda").to(torch.int32)

    res = {"n": n, "calls_per_sample": calls, "rounds_of_sorting": jumpy.permutation_rounds(n),
           "workspace_bytes": ws.numel()}
    for k, v in summary(interleaved({"native": native, "randperm": randperm}, rounds, warmup)).items():
        res[k.replace("_ms", "_us_per_call")] = round(v * 1e3 / calls, 2)
    return res


def bench_learner(T, B, rounds, warmup):
    from po_brax_amd import jumpy
    from po_brax_amd.training import PPOLearner, ValueFunction, networks
    D, A = 114, 8
    p_model, v_model = networks.make_models(2 * A, D)
    g = torch.Generator(device="cuda").manual_seed(5)
    legs = {}
    for permutation in ("torch", "native"):
        policy = networks.NormalTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6))
        critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)))
        learner = PPOLearner(policy, critic, learning_rate=1e-5, num_minibatches=32, num_update_epochs=1,
                             key=jumpy.random_prngkey(7), backward=("native", "torch"), permutation=permutation)
        roll = _Roll(T, B, D, A, g)
        legs[permutation] = (lambda l=learner, r=roll: l.update(r))
    out = {"T": T, "B": B, "num_minibatches": 32, "num_update_epochs": 1, "backward": ["native", "torch"]}
    out.update(summary(interleaved(legs, rounds, warmup)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-learner", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"bench": "permutation_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "native_equals_numpy_at_1310720": check_full_size(1310720),
           "sort_torch_leg": "not run: the vendor radix sort behind torch.sort above n = 4096 is where the captured "
                             "update's fault was reported, cause unknown",
           "shuffle": [bench_shuffle(n, args.rounds, args.warmup, args.calls) for n in (1310720, 65536)]}
    if not args.no_learner:
        res["learner_update"] = bench_learner(20, 65536, args.rounds, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
