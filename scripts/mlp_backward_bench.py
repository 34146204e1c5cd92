"""mlp_backward_bench.py -- what the networks' forward-with-grad plus backward costs on the device.

For the policy and the value network of make_models(16, 114) at M = 40 960 (one of 32 minibatches of
HH B = 65 536, T = 20): forward with grad, then backward to theta.grad, two legs alternating call by
call in one process, the median of each reported with min .. max:

  native   model.apply_native: pob_mlp_forward_train and pob_mlp_backward (k_mlp_forward_train,
           k_mlp_bwd_delta, k_mlp_bwd_weights, k_mlp_bwd_reduce) with their allocations
  torch    the torch-op model.apply under autograd (addmm / silu and their backward)

then one PPOLearner.update (one epoch, 32 minibatches of 40 960 rows of synthetic rollout buffers)
under backward = "torch", "native" and ("native", "torch"), alternating the same way (--no-learner
skips it).  Prints one JSON line.

    python scripts/mlp_backward_bench.py [--rounds 15] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "po-brax_amd"))

F32_MFMA_PEAK = 157e12  # flop/s


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


def summary(ms):
    out = {}
    for k, v in ms.items():
        out[k + "_ms"] = round(statistics.median(v), 4)
        out[k + "_min_ms"] = round(min(v), 4)
        out[k + "_max_ms"] = round(max(v), 4)
    return out


def bench_network(name, model, M, rounds, warmup):
    from po_brax_amd import jumpy
    sizes = model.layer_sizes
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn((M, sizes[0]), device="cuda", generator=g)
    dy = torch.randn((M, sizes[-1]), device="cuda", generator=g) / M
    theta = model.init(jumpy.random_prngkey(1)).theta.detach().requires_grad_(True)
    params = types.SimpleNamespace(theta=theta)

    def leg(fn):
        def run():
            theta.grad = None
            fn(params, x).backward(dy)
        return run

    legs = {"native": leg(model.apply_native), "torch": leg(model.apply)}
    # the legs agree before they are timed
    grads = {}
    for k, fn in legs.items():
        fn()
        grads[k] = theta.grad.clone()
    torch.cuda.synchronize()
    flop = 6 * M * sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))  # forward, dW and dx (dx of layer 0 included)
    out = {"network": name, "sizes": list(sizes), "M": M, "gflop": round(flop / 1e9, 2),
           "ms_at_f32_mfma_peak": round(flop / F32_MFMA_PEAK * 1e3, 4),
           "max_abs_grad_difference": float((grads["native"] - grads["torch"]).abs().max()),
           "largest_grad": float(grads["torch"].abs().max())}
    out.update(summary(interleaved(legs, rounds, warmup)))
    out["torch_over_native"] = round(out["torch_ms"] / out["native_ms"], 3)
    return out


class _Roll:
    """The buffers PPOLearner.update reads, filled with synthetic values."""

    def __init__(self, T, B, D, A, g):
        rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
        self.obs = rn(T, B, D)
        self.raw, self.logp = rn(T, B, A), -8.0 + 0.3 * rn(T, B)
        self.advantages, self.vs = rn(T, B), rn(T, B)


def bench_learner(T, B, rounds, warmup):
    from po_brax_amd import jumpy
    from po_brax_amd.training import PPOLearner, ValueFunction, networks
    D, A = 114, 8
    p_model, v_model = networks.make_models(2 * A, D)
    g = torch.Generator(device="cuda").manual_seed(5)
    legs = {}
    for name, backward in (("torch", "torch"), ("native", "native"), ("native_torch", ("native", "torch"))):
        policy = networks.NormalTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6))
        critic = ValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)))
        learner = PPOLearner(policy, critic, learning_rate=1e-5, num_minibatches=32, num_update_epochs=1,
                             key=jumpy.random_prngkey(7), backward=backward)
        roll = _Roll(T, B, D, A, g)
        legs[name] = (lambda l=learner, r=roll: l.update(r))
    out = {"T": T, "B": B, "num_minibatches": 32, "num_update_epochs": 1, "rows_per_minibatch": T * B // 32}
    out.update(summary(interleaved(legs, rounds, warmup)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--M", type=int, default=40960)
    ap.add_argument("--no-learner", action="store_true")
    ap.add_argument("--learner-rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from po_brax_amd.training import networks
    p_model, v_model = networks.make_models(16, 114)
    res = {"bench": "mlp_backward_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "networks": [bench_network("policy", p_model, args.M, args.rounds, args.warmup),
                        bench_network("value", v_model, args.M, args.rounds, args.warmup)]}
    if not args.no_learner:
        res["learner_rounds"] = args.learner_rounds
        res["learner_update"] = bench_learner(20, 65536, args.learner_rounds, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
