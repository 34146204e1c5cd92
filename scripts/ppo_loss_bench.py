"""ppo_loss_bench.py -- what the PPO loss and its head gradient cost on the device.

Forward plus backward to dlogits and dvalues at A = 8, M = 40 960 (T = 20, B = 65 536 over 32
minibatches) and M = 1 310 720 (the whole unroll), four legs alternating call by call in one
process, the median of each reported with min .. max:

  kernel          training.ppo_loss on contiguous float32 device tensors and total.backward():
                  pob_ppo_loss plus the key advance, the output allocations and autograd's two
                  multiplications by the upstream gradient
  launches        pob_ppo_loss alone on preallocated buffers (k_ppo_loss, k_ppo_chunks, k_ppo_finish)
  torch_ops       the module's own torch-op spelling (ppo._ppo_torch: the header's scalar functions
                  in float32 torch ops, fmaf through float64) on the same tensors
  torch_autograd  brax's formula as a user writes it by hand: torch's softplus / erfinv / exp and
                  autograd (that spelling lives here, not in the library)

The yardstick column is the HBM time of the launches' (5 A + 5) x 4 x M bytes at the 6.3 TB/s a
streaming copy reaches on this chip.  Prints one JSON line.

    python scripts/ppo_loss_bench.py [--rounds 15] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "po-brax_amd"))

HBM_STREAM = 6.3e12  # bytes/s of a float4 copy on the MI355X (8.0e12 peak)


def torch_autograd_loss(logits, values, raw, old_logp, adv, vs, u, entropy_cost, eps):
    """brax's compute_ppo_loss on the tanh-normal head in eager torch ops."""
    A = logits.shape[1] // 2
    softplus = torch.nn.functional.softplus
    loc, scale = logits[:, :A], softplus(logits[:, A:]) + 0.001
    log_det = lambda z: 2.0 * (math.log(2.0) - z - softplus(-2.0 * z))  # noqa: E731
    logp = (-0.5 * ((raw - loc) / scale) ** 2 - torch.log(scale) - 0.5 * math.log(2.0 * math.pi) - log_det(raw)).sum(-1)
    y = loc + scale * (math.sqrt(2.0) * torch.erfinv(u))
    entropy = (0.5 + 0.5 * math.log(2.0 * math.pi) + torch.log(scale) + log_det(y)).sum(-1)
    rho = torch.exp(logp - old_logp)
    policy = -torch.minimum(rho * adv, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * adv).mean()
    v_error = vs - values
    return policy + (v_error * v_error).mean() * 0.25 - entropy_cost * entropy.mean()


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


def bench(M, A, rounds, warmup, ec=1e-4, eps=0.3):
    from po_brax_amd import _lib, jumpy
    from po_brax_amd.training import ppo, ppo_loss
    g = torch.Generator(device="cuda").manual_seed(M + A)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    logits = rn(M, 2 * A)
    scale = torch.nn.functional.softplus(logits[:, A:]) + 0.001
    raw = (logits[:, :A] + scale * rn(M, A)).contiguous()
    vs = 30.0 * rn(M)
    values = vs + 3.0 * rn(M)
    adv = rn(M)
    key = jumpy.random_prngkey(3)
    u = ppo._entropy_draws(key, M, A)
    with torch.no_grad():  # old_logp: the new log-probability + N(0, 0.3^2)
        e = (raw - logits[:, :A]) / scale
        log_det = 2.0 * (math.log(2.0) - raw - torch.nn.functional.softplus(-2.0 * raw))
        logp = (-0.5 * e * e - torch.log(scale) - 0.5 * math.log(2.0 * math.pi) - log_det).sum(-1)
        old_logp = logp + 0.3 * rn(M)
    lg, va = logits.clone().requires_grad_(True), values.clone().requires_grad_(True)

    def leg_kernel():
        lg.grad = va.grad = None
        total, _ = ppo_loss(lg, va, raw, old_logp, adv, vs, key, entropy_cost=ec, ppo_epsilon=eps)
        total.backward()

    need = C.c_longlong()
    _lib.check(_lib.lib.pob_ppo_loss_workspace_bytes(M, C.byref(need)))
    ws = torch.empty(need.value // 8, dtype=torch.float64, device="cuda")
    dl, dv, losses = torch.empty_like(logits), torch.empty_like(values), torch.empty(4, device="cuda")

    def leg_launches():
        _lib.check(_lib.lib.pob_ppo_loss(M, A, _lib.ptr(logits), _lib.ptr(values), None, _lib.ptr(raw), _lib.ptr(old_logp),
                                         _lib.ptr(adv), _lib.ptr(vs), _lib.ptr(key), ec, eps, _lib.ptr(dl), _lib.ptr(dv),
                                         _lib.ptr(losses), _lib.ptr(ws), _lib.stream_handle()))

    def leg_torch_ops():
        with torch.no_grad():
            uu = ppo._entropy_draws(key, M, A)
            ppo._ppo_torch(logits, values, raw, old_logp, adv, vs, uu, None, ec, eps)

    def leg_torch_autograd():
        lg.grad = va.grad = None
        uu = ppo._entropy_draws(key, M, A).clamp_(min=ppo._U_MIN)
        torch_autograd_loss(lg, va, raw, old_logp, adv, vs, uu, ec, eps).backward()

    # the legs agree before they are timed
    k0 = key.clone()
    leg_launches()
    uu = ppo._entropy_draws(k0, M, A).clamp_(min=ppo._U_MIN)
    torch_autograd_loss(lg, va, raw, old_logp, adv, vs, uu, ec, eps).backward()
    torch.cuda.synchronize()
    err = float((dl - lg.grad).abs().max())
    gmax = float(lg.grad.abs().max())
    legs = {"kernel": leg_kernel, "launches": leg_launches, "torch_ops": leg_torch_ops, "torch_autograd": leg_torch_autograd}
    ms = interleaved(legs, rounds, warmup)
    n_bytes = (5 * A + 5) * 4 * M
    out = {"M": M, "A": A, "bytes": n_bytes, "hbm_us_at_6.3TBps": round(n_bytes / HBM_STREAM * 1e6, 2),
           "max_abs_dlogits_difference_kernel_vs_autograd": err, "largest_dlogits": gmax}
    for k, v in ms.items():
        out[k + "_us"] = round(statistics.median(v) * 1e3, 2)
        out[k + "_min_us"] = round(min(v) * 1e3, 2)
        out[k + "_max_us"] = round(max(v) * 1e3, 2)
    out["launches_over_hbm_time"] = round(out["launches_us"] / out["hbm_us_at_6.3TBps"], 2)
    out["speedup_over_torch_ops"] = round(out["torch_ops_us"] / out["kernel_us"], 2)
    out["speedup_over_torch_autograd"] = round(out["torch_autograd_us"] / out["kernel_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"bench": "ppo_loss_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "shapes": [bench(M, 8, args.rounds, args.warmup) for M in (40960, 1310720)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
