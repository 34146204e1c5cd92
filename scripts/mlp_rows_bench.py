"""mlp_rows_bench.py -- what reading a minibatch in place saves over gathering it (DESIGN.md "Row-indexed
training pass").

For the policy and the value network of make_models(16, 114), one of 32 minibatches (M = 40 960 rows drawn by a
permutation) of an (N = 1 310 720, 114) trajectory array (HH B = 65 536, T = 20) under a loaded normaliser: forward
with grad, then backward to theta.grad, two legs alternating call by call in one process, the median of each
reported with min .. max:

  gather  x.index_select(0, idx), normalizer.apply, model.apply_native(kernel=) on the rows (the route before)
  rows    model.apply_native(kernel=, idx=, normalizer=) on the whole array (pob_mlp_*_rows)

with kernel="tile" for the policy and "resident" for the value network, the legs' theta.grad compared bit for bit
first; then one PPOLearner.update (one epoch, 32 minibatches) under backward=("native", "resident") with
rows="gather" and rows="in_place", and ("native", "torch") as the control nothing of this touches (--no-learner
skips it).  Prints one JSON line.

    python scripts/mlp_rows_bench.py [--rounds 15] [--out FILE]
"""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mlp_backward_bench import _Roll, interleaved, summary  # noqa: E402  (puts po-brax_amd on the path)


def _normalizer(D, g):
    from po_brax_amd.training.normalization import ObservationNormalizer
    norm = ObservationNormalizer(D)
    table = torch.stack([torch.randn(D, device="cuda", generator=g), 0.5 + torch.rand(D, device="cuda", generator=g),
                         torch.ones(D, device="cuda")])
    norm.load_state_dict({"table": table, "count": torch.tensor([1000.0], dtype=torch.float64), "clip": 5.0})
    return norm


def bench_network(name, model, kernel, x, idx, norm, rounds, warmup):
    from po_brax_amd import jumpy
    sizes, M = model.layer_sizes, int(idx.shape[0])
    g = torch.Generator(device="cuda").manual_seed(M)
    dy = torch.randn((M, sizes[-1]), device="cuda", generator=g) / M
    theta = model.init(jumpy.random_prngkey(1)).theta.detach().requires_grad_(True)
    params = types.SimpleNamespace(theta=theta)

    def gather():
        theta.grad = None
        model.apply_native(params, norm.apply(x.index_select(0, idx)), kernel=kernel).backward(dy)

    def rows():
        theta.grad = None
        model.apply_native(params, x, kernel=kernel, idx=idx, normalizer=norm).backward(dy)

    legs, grads = {"gather": gather, "rows": rows}, {}
    for k, fn in legs.items():
        fn()
        grads[k] = theta.grad.clone()
    torch.cuda.synchronize()
    out = {"network": name, "sizes": list(sizes), "kernel": kernel, "M": M, "N": int(x.shape[0]),
           "rows_grad_equals_gather": bool(torch.equal(grads["rows"], grads["gather"])),
           "minibatch_bytes": 4 * M * sizes[0]}
    out.update(summary(interleaved(legs, rounds, warmup)))
    out["saved_us"] = round(1e3 * (out["gather_ms"] - out["rows_ms"]), 1)
    return out


def bench_learner(T, B, norm_of, rounds, warmup):
    from po_brax_amd import jumpy
    from po_brax_amd.training import PPOLearner, ValueFunction, networks
    D, A = 114, 8
    p_model, v_model = networks.make_models(2 * A, D)
    g = torch.Generator(device="cuda").manual_seed(5)
    roll, legs = _Roll(T, B, D, A, g), {}
    for name, backward, rows in (("native_resident_gather", ("native", "resident"), "gather"),
                                 ("native_resident_in_place", ("native", "resident"), "in_place"),
                                 ("native_torch", ("native", "torch"), "gather")):
        norm = norm_of(D, g)
        policy = networks.NormalTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6),
                                           normalizer=norm)
        critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)), normalizer=norm)
        learner = PPOLearner(policy, critic, learning_rate=1e-5, num_minibatches=32, num_update_epochs=1,
                             key=jumpy.random_prngkey(7), backward=backward, rows=rows)
        legs[name] = (lambda l=learner: l.update(roll))
    out = {"T": T, "B": B, "num_minibatches": 32, "num_update_epochs": 1, "rows_per_minibatch": T * B // 32}
    out.update(summary(interleaved(legs, rounds, warmup)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--no-learner", action="store_true")
    ap.add_argument("--learner-rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from po_brax_amd.training import networks
    p_model, v_model = networks.make_models(16, 114)
    N = args.T * args.B
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((N, 114), device="cuda", generator=g)
    idx = torch.randperm(N, device="cuda", generator=g).to(torch.int32)[:N // 32].contiguous()
    norm = _normalizer(114, g)
    res = {"bench": "mlp_rows_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "networks": [bench_network("policy", p_model, "tile", x, idx, norm, args.rounds, args.warmup),
                        bench_network("value", v_model, "resident", x, idx, norm, args.rounds, args.warmup)]}
    del x
    if not args.no_learner:
        res["learner_rounds"] = args.learner_rounds
        res["learner_update"] = bench_learner(args.T, args.B, _normalizer, args.learner_rounds, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
