"""gru_backward_bench.py -- what the recurrent network's forward-with-grad plus backward costs on the device.

For the masked (30 -> GRU 64 -> 16) and the full (114 -> GRU 64 -> 16) recurrent policy network over a
window of T = 20 steps and M = 2 048 sequences (one of 32 env-minibatches of HH B = 65 536): forward
with grad, then backward to theta.grad, two legs alternating call by call in one process, the median
of each reported with min .. max:

  native   model.apply_sequence_native: pob_gru_sequence_forward_train and pob_gru_sequence_backward
           (k_gru_seq_forward, k_gru_seq_backward, k_gru_bwd_weights, k_mlp_bwd_reduce) with their
           allocations
  torch    the torch-op model.apply_sequence under autograd (a loop over the single-step ops)

then one RecurrentPPOLearner.update (one epoch, 32 minibatches of 2 048 envs of synthetic rollout
buffers) under backward = "torch", ("native", "torch") and "native", alternating the same way
(--no-learner skips it).  Prints one JSON line.

    python scripts/gru_backward_bench.py [--rounds 15] [--out FILE]
"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "po-brax_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mlp_backward_bench import interleaved, summary  # noqa: E402

H, A = 64, 8


def bench_network(name, D, T, M, rounds, warmup):
    from po_brax_amd import jumpy
    from po_brax_amd.training import networks
    model = networks.make_recurrent_model([], H, [2 * A], D)
    g = torch.Generator(device="cuda").manual_seed(M)
    obs = torch.randn((T, M, D), device="cuda", generator=g)
    h0 = torch.rand((M, H), device="cuda", generator=g) * 2.0 - 1.0
    reset = (torch.rand((T, M), device="cuda", generator=g) < 0.05).float()
    dy = torch.randn((T, M, 2 * A), device="cuda", generator=g) / (T * M)
    theta = model.init(jumpy.random_prngkey(1)).theta.detach().requires_grad_(True)
    params = types.SimpleNamespace(theta=theta)

    def leg(fn):
        def run():
            theta.grad = None
            fn(params, obs, h0, reset)[0].backward(dy)
        return run

    legs = {"native": leg(model.apply_sequence_native), "torch": leg(model.apply_sequence)}
    grads = {}
    for k, fn in legs.items():  # the legs agree before they are timed
        fn()
        grads[k] = theta.grad.clone()
    torch.cuda.synchronize()
    out = {"network": name, "obs": D, "hidden": H, "out": 2 * A, "T": T, "M": M, "params": int(theta.numel()),
           "max_abs_grad_difference": float((grads["native"] - grads["torch"]).abs().max()),
           "largest_grad": float(grads["torch"].abs().max())}
    out.update(summary(interleaved(legs, rounds, warmup)))
    out["torch_over_native"] = round(out["torch_ms"] / out["native_ms"], 3)
    return out


class _Roll:
    """The buffers RecurrentPPOLearner.update reads, filled with synthetic values."""

    def __init__(self, T, B, D, g):
        rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
        self.obs = rn(T, B, D)
        self.raw, self.logp = rn(T, B, A), -8.0 + 0.3 * rn(T, B)
        self.advantages, self.vs = rn(T, B), rn(T, B)
        self.hidden = torch.rand((T, B, H), device="cuda", generator=g) * 2.0 - 1.0
        self.done = (torch.rand((T, B), device="cuda", generator=g) < 0.05).float()


def bench_learner(D, T, B, rounds, warmup):
    from po_brax_amd import jumpy
    from po_brax_amd.training import RecurrentPPOLearner, ValueFunction, networks
    p_model = networks.make_recurrent_model([], H, [2 * A], D)
    v_model = networks.make_models(2 * A, D)[1]
    g = torch.Generator(device="cuda").manual_seed(5)
    roll = _Roll(T, B, D, g)
    legs = {}
    for name, backward in (("torch", "torch"), ("native_torch", ("native", "torch")), ("native", "native")):
        policy = networks.RecurrentTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6))
        critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)))
        learner = RecurrentPPOLearner(policy, critic, learning_rate=1e-5, num_minibatches=32, num_update_epochs=1,
                                      key=jumpy.random_prngkey(7), backward=backward)
        legs[name] = (lambda l=learner: l.update(roll))
    out = {"obs": D, "T": T, "B": B, "num_minibatches": 32, "num_update_epochs": 1, "envs_per_minibatch": B // 32}
    out.update(summary(interleaved(legs, rounds, warmup)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--M", type=int, default=2048)
    ap.add_argument("--no-learner", action="store_true")
    ap.add_argument("--learner-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"bench": "gru_backward_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "networks": [bench_network("masked", 30, args.T, args.M, args.rounds, args.warmup),
                        bench_network("full", 114, args.T, args.M, args.rounds, args.warmup)]}
    if not args.no_learner:
        res["learner_rounds"] = args.learner_rounds
        res["learner_update"] = bench_learner(114, args.T, 32 * args.M, args.learner_rounds, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
