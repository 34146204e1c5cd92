"""critic_pass_bench.py -- what the recurrent critic's pass and its learner cost on the device.

The critic pass alone, for the masked (30 -> GRU 64 -> 1) and the full (114 -> GRU 64 -> 1) critic over
S = T + 1 = 21 rows of B envs (B = 65 536 and 4 096), a normaliser table applied and resets on 5 % of the
entries.  Three routes to the same (S, B) values, each captured into a hipGraph of its own and replayed,
alternating replay by replay in one process; the median of each is reported with min .. max (device
events around a replay), after the three have been compared bit for bit:

  sequence   ONE pob_gru_sequence_forward launch (k_gru_seq_infer)
  chained    S pob_gru_forward_norm launches (k_gru_forward), h carried in place through HBM
  train      ONE pob_gru_sequence_forward_train launch (k_gru_seq_forward), which also stores every array
             the backward pass needs (skipped where `saved` does not fit in --max-saved-gib)

then one RecurrentPPOLearner.update with the recurrent critic (one epoch, 32 minibatches of B / 32 envs of
synthetic rollout buffers, 114 columns) under backward = "torch", ("native", "torch") and "native",
alternating the same way (--no-learner skips it).  Prints one JSON line.

    python scripts/critic_pass_bench.py [--rounds 15] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "po-brax_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mlp_backward_bench import interleaved, summary  # noqa: E402

H, A = 64, 8


def _graph(fn):
    fn()  # once eagerly: code objects are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def bench_pass(name, D, S, B, rounds, warmup, max_saved_gib):
    from po_brax_amd import _lib, jumpy
    from po_brax_amd._lib import check, lib, ptr
    from po_brax_amd.training import networks
    model = networks.make_recurrent_model([], H, [1], D)
    gru = model.gru.handle
    gen = torch.Generator(device="cuda").manual_seed(B + D)
    obs = torch.randn((S, B, D), device="cuda", generator=gen)
    h0 = torch.rand((B, H), device="cuda", generator=gen) * 2.0 - 1.0
    reset = (torch.rand((S, B), device="cuda", generator=gen) < 0.05).float()
    table = torch.stack([0.1 * torch.randn(D, device="cuda", generator=gen),
                         0.5 + torch.rand(D, device="cuda", generator=gen), torch.ones(D, device="cuda")]).contiguous()
    theta = model.init(jumpy.random_prngkey(1)).theta
    clip = 5.0
    y = {k: torch.empty((S, B), device="cuda") for k in ("sequence", "chained", "train")}
    h_seq, h_first, h_chain = (torch.empty((B, H), device="cuda") for _ in range(3))
    h_train = torch.empty((B, H), device="cuda")

    def stream():
        return _lib.stream_handle(obs.device)

    def sequence():
        check(lib.pob_gru_sequence_forward(gru, S, B, B, ptr(obs), None, ptr(h0), ptr(reset), ptr(theta), ptr(y["sequence"]),
                                           ptr(h_first), ptr(h_seq), S, ptr(table), clip, stream()))

    def chained():
        h_chain.copy_(h0)
        for s in range(S):
            check(lib.pob_gru_forward_norm(gru, B, ptr(obs[s]), ptr(theta), ptr(reset[s]), ptr(h_chain), ptr(y["chained"][s]),
                                           None, ptr(table), clip, stream()))

    legs = {"sequence": sequence, "chained": chained}
    need = C.c_longlong()
    check(lib.pob_gru_sequence_saved_bytes(gru, S, B, C.byref(need)))
    out = {"network": name, "obs": D, "hidden": H, "S": S, "B": B, "train_saved_gib": round(need.value / 2 ** 30, 3)}
    if need.value <= max_saved_gib * 2 ** 30:
        saved = torch.empty(need.value // 4, device="cuda")

        def train():
            check(lib.pob_gru_sequence_forward_train(gru, S, B, B, ptr(obs), None, ptr(h0), ptr(reset), ptr(theta),
                                                     ptr(y["train"]), ptr(h_train), ptr(saved), ptr(table), clip, stream()))
        legs["train"] = train
    graphs = {k: _graph(fn) for k, fn in legs.items()}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    same = all(torch.equal(y["sequence"].view(torch.int32), y[k].view(torch.int32)) for k in legs)
    same = same and torch.equal(h_seq.view(torch.int32), h_chain.view(torch.int32))
    out["routes_agree_bitwise"] = bool(same)
    if not same:
        raise SystemExit(f"{name} B={B}: the routes disagree: nothing is timed")
    out.update(summary(interleaved({k: g.replay for k, g in graphs.items()}, rounds, warmup)))
    out["chained_over_sequence"] = round(out["chained_ms"] / out["sequence_ms"], 3)
    if "train_ms" in out:
        out["train_over_sequence"] = round(out["train_ms"] / out["sequence_ms"], 3)
    return out


class _Roll:
    """The buffers RecurrentPPOLearner.update reads under a recurrent critic, filled with synthetic values."""

    def __init__(self, T, B, D, g):
        rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
        self.obs = rn(T, B, D)
        self.raw, self.logp = rn(T, B, A), -8.0 + 0.3 * rn(T, B)
        self.advantages, self.vs = rn(T, B), rn(T, B)
        self.hidden = torch.rand((T, B, H), device="cuda", generator=g) * 2.0 - 1.0
        self.value_hidden0 = torch.rand((B, H), device="cuda", generator=g) * 2.0 - 1.0
        self.done = (torch.rand((T, B), device="cuda", generator=g) < 0.05).float()


def bench_learner(D, T, B, rounds, warmup):
    from po_brax_amd import jumpy
    from po_brax_amd.training import RecurrentPPOLearner, RecurrentValueFunction, networks
    p_model = networks.make_recurrent_model([], H, [2 * A], D)
    v_model = networks.make_recurrent_model([], H, [1], D)
    g = torch.Generator(device="cuda").manual_seed(5)
    roll = _Roll(T, B, D, g)
    legs = {}
    for name, backward in (("torch", "torch"), ("native_torch", ("native", "torch")), ("native", "native")):
        policy = networks.RecurrentTanhPolicy(p_model, p_model.init(jumpy.random_prngkey(5)), jumpy.random_prngkey(6))
        critic = RecurrentValueFunction(v_model, v_model.init(jumpy.random_prngkey(9)))
        learner = RecurrentPPOLearner(policy, critic, learning_rate=1e-5, num_minibatches=32, num_update_epochs=1,
                                      key=jumpy.random_prngkey(7), backward=backward)
        legs[name] = (lambda l=learner: l.update(roll))
    out = {"critic": f"{D} -> GRU {H} -> 1", "T": T, "B": B, "num_minibatches": 32, "num_update_epochs": 1,
           "envs_per_minibatch": B // 32}
    out.update(summary(interleaved(legs, rounds, warmup)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--envs", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--max-saved-gib", type=float, default=24.0)
    ap.add_argument("--no-learner", action="store_true")
    ap.add_argument("--learner-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"bench": "critic_pass_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "lib": os.environ.get("POB_LIB", "in-tree"), "passes": []}
    for B in args.envs:
        for name, D in (("masked", 30), ("full", 114)):
            res["passes"].append(bench_pass(name, D, args.T + 1, B, args.rounds, args.warmup, args.max_saved_gib))
    if not args.no_learner:
        res["learner_rounds"] = args.learner_rounds
        res["learner_update"] = bench_learner(114, args.T, 65536, args.learner_rounds, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
