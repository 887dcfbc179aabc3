#!/usr/bin/env python3
"""Cost of msnake_copy_envs next to the host round trip it replaces.  19x19x3 snake_env at 4 096 and 32 768 envs, the
source some hundred steps into safe_greedy play (bodies of a dozen cells), the destination a clone of it.

The copy launch, two figures per leg, both from HIP events after a warm-up, legs alternating in one process:
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence,
            free of the host's submission cost;
  call_us:  CALLS back-to-back calls through the Python wrapper (validation + ctypes + the stream lookup): what a
            Python caller pays when nothing else is queued; mostly the host's submission rate.
Legs: "identity" (index None: env e <- env e), "permutation" (a random permutation as an int32 device tensor) and
"one_in_eight" (every eighth env selected, the rest -1), plus msnake_step on the source for scale.
The host path, dst.set_state_all(src.get_state_all()), blocks (three kernels, a host prefix sum, two blocking copies),
so it is timed with the host clock around the pair, after a device synchronise: host_ms per round trip.
The comparison is descriptive: nothing gates on it.
    python tools/copy_cost.py            # writes profiles/copy_cost.json"""
import argparse
import os
import time

import cost_harness as ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ch.ROOT, "profiles", "copy_cost.json"))
    args = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "calls_per_leg": args.calls,
           "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "median (min, max) over the rounds; graph_us / call_us: us per call, host_ms: ms per round trip",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "call_us": "calls through the Python wrapper (includes the host's submission cost), HIP events",
           "host_ms": "dst.set_state_all(src.get_state_all()): host clock around the blocking pair",
           "batches": {}}
    for n in args.envs:
        src, _ = ch.played_env(n, args.play_steps)
        dst = src.clone(seed=1, env_id_base=n)
        g = torch.Generator().manual_seed(n)
        perm = torch.randperm(n, generator=g).to(device=src.device, dtype=torch.int32)
        sparse = torch.where(torch.arange(n) % 8 == 0, torch.arange(n), torch.full((n,), -1)).to(device=src.device, dtype=torch.int32)
        ones = torch.ones((n, 3), dtype=torch.int32, device=src.device)
        legs = {
            "identity": lambda: dst.copy_envs_device(src),
            "permutation": lambda: dst.copy_envs_device(src, perm),
            "one_in_eight": lambda: dst.copy_envs_device(src, sparse),
            "msnake_step": lambda: src.step_device(ones),
        }
        blob = src.get_state_all()
        words = (len(blob) - 40 - 8 * (n + 1)) // 4
        # the step leg moves the source: every leg starts from the same state
        times = ch.graph_legs(legs, args.calls, args.rounds, restore=lambda: src.set_state_all(blob), eager=True)
        host = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.set_state_all(src.get_state_all())
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1000.0)
        ch.assert_unchanged(dst, blob)
        out = {k: {kind: ch.med(v) for kind, v in t.items()} for k, t in times.items()}
        out["host_round_trip"] = {"host_ms": ch.med(host), "state_words": words}
        res["batches"][str(n)] = out
        src.close(), dst.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
