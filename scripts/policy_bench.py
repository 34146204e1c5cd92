"""policy_bench.py -- what the policy in the loop costs next to the fused env step.

AntHeavenHell, B = 65 536, T = 20 env-steps per replay, one process, three captured unrolls
replayed in turn (A, B, C, A, B, C, ..), the median replay time of each:

  A  rollout.PolicyRollout with the reference's policy network ([32] * 4 + [2 A], swish,
     tanh-normal head) written in torch ops (addmm, silu, softplus, randn, tanh)
  B  rollout.ActorRollout: the same network as ONE pob_policy_act launch per step (which also
     gives logp, raw and the trajectory's observation rows)
  C  rollout.GraphRollout on pre-drawn actions: the env step alone

Prints one JSON line: ms/step of each and the policy's share A - C and B - C.

    python scripts/policy_bench.py [--batch 65536] [--steps 20] [--rounds 15] [--out FILE]

--recurrent runs the same three legs with the recurrent actor (GRU cell of --hidden features,
no pre-MLP, one post layer of 2 A logits):

  A  rollout.PolicyRollout with that network in torch ops (cat, addmm, sigmoid, tanh, where),
     the hidden state carried and zeroed where the last step ended an episode
  B  rollout.RecurrentActorRollout: ONE pob_gru_policy_act launch per step
  C  rollout.GraphRollout on pre-drawn actions

--masked creates the envs with the standard observability mask (30 of HH's 114 columns, fused
into the step kernel) and both policies act on state.info["obs_masked"].

--normalize replaces leg A by two more native legs (with --recurrent the recurrent actor's):

  N  leg B's rollout whose policy carries an ObservationNormalizer (the table applied in the
     actor kernel's tile load)
  U  leg N with update_normalizer=True: the statistics update over the replay's T B observation
     rows as the graph's last nodes

and times normalizer.update(roll.obs) on its own; the JSON then holds the actor's share with
and without the table, the update per replay (U - N and alone) and its HBM time at 8 TB/s.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "po-brax_amd"))


class TorchNormalTanhPolicy:
    """The same actor in torch ops, on the same flat parameters (action only)."""

    def __init__(self, params, action_size):
        self.layers = [(params[f"hidden_{i}"]["kernel"], params[f"hidden_{i}"]["bias"]) for i in range(len(params))]
        self.A = action_size

    def __call__(self, obs):
        h = obs
        for i, (W, b) in enumerate(self.layers):
            h = torch.addmm(b, h, W)
            if i != len(self.layers) - 1:
                h = torch.nn.functional.silu(h)
        loc, s = h[:, :self.A], h[:, self.A:]
        scale = torch.nn.functional.softplus(s) + 0.001
        return torch.tanh(loc + scale * torch.randn_like(loc))


class TorchRecurrentPolicy:
    """The recurrent actor in torch ops on the same flat parameters (action only).  ``tap`` is
    the env proxy below: it holds the State the last step returned and writes its done into
    ``self.reset``."""

    def __init__(self, model, params, B, action_size, masked):
        self.model, self.theta, self.A, self.masked = model, params.theta, action_size, masked
        self.hidden = torch.zeros((B, model.hidden_size), device=params.theta.device)
        self.reset = torch.zeros((B,), device=params.theta.device)
        self.tap = None

    def __call__(self, obs):
        from po_brax_amd.training.networks import _recurrent_torch
        m = self.model
        if self.masked:
            obs = self.tap.state.info["obs_masked"]
        y, h = _recurrent_torch(m.pre_sizes, m.hidden_size, m.post_sizes, m.activation, self.theta, obs, self.hidden,
                                self.reset)
        self.hidden.copy_(h)
        loc, s = y[:, :self.A], y[:, self.A:]
        scale = torch.nn.functional.softplus(s) + 0.001
        return torch.tanh(loc + scale * torch.randn_like(loc))


class DoneTap:
    """An env whose step_ also copies the step's done into ``policy.reset`` (leg A's episode
    boundaries) and remembers the returned State."""

    def __init__(self, env, state, policy):
        self.env, self.state, self.policy = env, state, policy
        self.action_size = env.action_size
        policy.tap = self

    def step_(self, state, action):
        s = self.env.step_(state, action)
        self.policy.reset.copy_(s.aux["done"] if "done" in s.aux else s.done)
        self.state = s
        return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="ant_heavenhell")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--recurrent", action="store_true")
    ap.add_argument("--masked", action="store_true")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--normalize", action="store_true")
    args = ap.parse_args()

    from po_brax_amd import envs, jumpy
    from po_brax_amd.rollout import ActorRollout, GraphRollout, PolicyRollout, RecurrentActorRollout
    from po_brax_amd.training import networks

    B, T = args.batch, args.steps
    keys = jumpy.random_split(jumpy.random_prngkey(0), B + 1)[1:]
    mask = None
    if args.masked:
        if not args.recurrent:
            ap.error("--masked goes with --recurrent")
        from po_brax_amd import standard_observability_masks as M
        mask = M.po_env_mask(args.env, cfrc=False)
    es = [envs.create(args.env, batch_size=B, obs_mask=mask) for _ in range(4 if args.normalize else 3)]
    ss = [e.reset(keys) for e in es]
    A, D = es[0].action_size, es[0].observation_size
    if args.recurrent:
        D = es[0].masked_observation_size if args.masked else D
    if args.normalize:
        from po_brax_amd.training.normalization import ObservationNormalizer
        norms = [None, ObservationNormalizer(D), ObservationNormalizer(D)]
        legs = {}
        for i, (leg, upd) in enumerate((("B", False), ("N", False), ("U", True))):
            if args.recurrent:
                model = networks.make_recurrent_model([], args.hidden, [2 * A], D)
                pol = networks.RecurrentTanhPolicy(model, model.init(jumpy.random_prngkey(1)), jumpy.random_prngkey(2),
                                                   normalizer=norms[i])
                legs[leg] = RecurrentActorRollout(es[i], ss[i], pol, T, masked=args.masked, update_normalizer=upd)
            else:
                model = networks.make_models(2 * A, D)[0]
                pol = networks.NormalTanhPolicy(model, model.init(jumpy.random_prngkey(1)), jumpy.random_prngkey(2),
                                                normalizer=norms[i])
                legs[leg] = ActorRollout(es[i], ss[i], pol, T, update_normalizer=upd)
        roll_a, roll_b = None, legs["B"]
    elif args.recurrent:
        model = networks.make_recurrent_model([], args.hidden, [2 * A], D)
        params = model.init(jumpy.random_prngkey(1))
        torch_policy = TorchRecurrentPolicy(model, params, B, A, args.masked)
        with torch.no_grad():
            roll_a = PolicyRollout(DoneTap(es[0], ss[0], torch_policy), ss[0], torch_policy, T)
        roll_b = RecurrentActorRollout(es[1], ss[1], networks.RecurrentTanhPolicy(model, params, jumpy.random_prngkey(2)),
                                       T, masked=args.masked)
    else:
        model = networks.make_models(2 * A, D)[0]
        params = model.init(jumpy.random_prngkey(1))
        with torch.no_grad():
            roll_a = PolicyRollout(es[0], ss[0], TorchNormalTanhPolicy(params, A), T)
        roll_b = ActorRollout(es[1], ss[1], networks.NormalTanhPolicy(model, params, jumpy.random_prngkey(2)), T)
    acts = torch.rand((T, B, A), device="cuda") * 2 - 1
    roll_c = GraphRollout(es[-1], ss[-1], acts, warmup=True)
    rolls = {"A": roll_a, "B": roll_b, "C": roll_c}
    if args.normalize:
        rolls = {"B": legs["B"], "N": legs["N"], "U": legs["U"], "C": roll_c}

        class UpdateAlone:  # normalizer.update(roll.obs) outside the graph, timed like a replay
            def replay(self):
                norms[1].update(legs["N"].obs)
        rolls["update"] = UpdateAlone()

    def timed(roll):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        roll.replay()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / T

    for _ in range(args.warmup):
        for r in rolls.values():
            timed(r)
    ms = {k: [] for k in rolls}
    for _ in range(args.rounds):
        for k, r in rolls.items():
            ms[k].append(timed(r))
    med = {k: statistics.median(v) for k, v in ms.items()}
    if args.normalize:
        n_bytes = T * B * D * 4
        res = {
            "bench": "policy_bench", "normalize": True, "recurrent": args.recurrent, "masked": args.masked, "obs_width": D,
            "hidden": args.hidden if args.recurrent else None, "env": args.env, "batch": B, "steps": T, "rounds": args.rounds,
            "device": torch.cuda.get_device_name(0),
            "B_actor_ms_per_step": round(med["B"], 5), "N_actor_table_ms_per_step": round(med["N"], 5),
            "U_actor_table_update_ms_per_step": round(med["U"], 5), "C_graph_rollout_ms_per_step": round(med["C"], 5),
            "actor_share_ms": round(med["B"] - med["C"], 5), "actor_share_table_ms": round(med["N"] - med["C"], 5),
            "update_in_graph_us_per_replay": round((med["U"] - med["N"]) * T * 1e3, 2),
            "update_alone_us": round(med["update"] * T * 1e3, 2),
            "update_alone_min_us": round(min(ms["update"]) * T * 1e3, 2),
            "update_bytes": n_bytes, "update_hbm_us_at_8TBs": round(n_bytes / 8e12 * 1e6, 2),
            "min_ms_per_step": {k: round(min(v), 5) for k, v in ms.items()},
            "max_ms_per_step": {k: round(max(v), 5) for k, v in ms.items()},
        }
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    res = {
        "bench": "policy_bench", "recurrent": args.recurrent, "masked": args.masked,
        "obs_width": D, "hidden": args.hidden if args.recurrent else None, "env": args.env, "batch": B, "steps": T, "rounds": args.rounds,
        "device": torch.cuda.get_device_name(0),
        "A_policy_rollout_torch_ms_per_step": round(med["A"], 5),
        "B_actor_rollout_ms_per_step": round(med["B"], 5),
        "C_graph_rollout_ms_per_step": round(med["C"], 5),
        "policy_share_torch_ms": round(med["A"] - med["C"], 5),
        "policy_share_native_ms": round(med["B"] - med["C"], 5),
        "min_ms_per_step": {k: round(min(v), 5) for k, v in ms.items()},
        "max_ms_per_step": {k: round(max(v), 5) for k, v in ms.items()},
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
