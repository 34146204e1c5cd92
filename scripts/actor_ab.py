"""actor_ab.py -- pob_policy_act of two builds of libpob.so, interleaved in one process.

Both libraries are loaded side by side through ctypes (the C ABI only: pob_mlp_create,
pob_policy_act) and run the reference's policy network (obs -> [32] * 4 -> 2 A, swish) on the
same observations, parameters and key.  Per round and library: ``--calls`` launches between two
device events; the libraries alternate within a round.  Prints one JSON line: the median, min
and max of the per-round microseconds per call for each library (a library's own min .. max is
its run-to-run spread), and whether every output of the two agrees bit for bit.

    python scripts/actor_ab.py --lib this=po-brax_amd/po_brax_amd/libpob.so --lib parent=/path/to/libpob.so
"""
import argparse
import ctypes as C
import json
import os
import statistics

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True, help="name=path, twice or more")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--obs", type=int, default=114)
    ap.add_argument("--actions", type=int, default=8)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, D, A = args.batch, args.obs, args.actions
    sizes = [D, 32, 32, 32, 32, 2 * A]
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.rand((B, D), device="cuda", generator=g) * 6 - 3
    n_params = sum((i + 1) * o for i, o in zip(sizes[:-1], sizes[1:]))
    theta = (torch.rand(n_params, device="cuda", generator=g) - 0.5) * 0.6
    VP = C.c_void_p
    libs = {}
    for spec in args.lib:
        name, path = spec.split("=", 1)
        lib = C.CDLL(os.path.abspath(path))
        lib.pob_mlp_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(VP)]
        lib.pob_policy_act.argtypes = [VP, C.c_int, C.c_int, C.c_int, VP, VP, VP, C.c_int, VP, VP, VP, VP, VP, VP]
        h = VP()
        assert lib.pob_mlp_create(len(sizes) - 1, (C.c_int * len(sizes))(*sizes), 1, 0, C.byref(h)) == 0
        out = {"action": torch.zeros((B, A), device="cuda"), "logp": torch.zeros(B, device="cuda"),
               "raw": torch.zeros((B, A), device="cuda"), "obs_copy": torch.zeros((B, D), device="cuda")}
        libs[name] = (lib, h, out, torch.tensor([0, 42], dtype=torch.uint32, device="cuda"))

    def call(name):
        lib, h, out, key = libs[name]
        rc = lib.pob_policy_act(h, B, B, 0, obs.data_ptr(), theta.data_ptr(), key.data_ptr(), 0, out["action"].data_ptr(),
                                out["logp"].data_ptr(), out["raw"].data_ptr(), None, out["obs_copy"].data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0

    for name in libs:  # one call each from the same key: the outputs must agree
        call(name)
    torch.cuda.synchronize()
    first = next(iter(libs))
    same = all(torch.equal(libs[n][2][k].view(torch.int32), libs[first][2][k].view(torch.int32))
               for n in libs for k in libs[first][2]) and all(torch.equal(libs[n][3], libs[first][3]) for n in libs)
    for _ in range(3):
        for name in libs:
            for _ in range(args.calls):
                call(name)
    us = {n: [] for n in libs}
    for _ in range(args.rounds):
        for name in libs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                call(name)
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / args.calls)
    res = {"bench": "actor_ab", "batch": B, "sizes": sizes, "calls": args.calls, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "outputs_bit_equal": bool(same),
           "us_per_call": {n: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                           for n, v in us.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
