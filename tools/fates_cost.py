#!/usr/bin/env python3
"""Cost of msnake_fate_actions next to safe_greedy, the mask-only call and msnake_step on the same handle, in the same
process.  19x19x3 snake_env at 4 096 and 32 768 envs, on a freshly reset batch and 500 steps into safe_greedy play
(longer bodies): the setup of tools/scripted_cost.py.

Two figures per leg, both from HIP events after a warm-up, legs alternating in one process:
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence;
  call_us:  CALLS back-to-back calls through the Python wrapper: mostly the host's submission rate.
The step leg plays the constant action 1 (with auto reset); the state is restored before every leg, and the legs that
only read are checked to have left it as it was.
    python tools/fates_cost.py --out profiles/fates_cost.json"""
import argparse
import sys

import cost_harness as ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=500)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import torch
    import msnake

    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "calls_per_leg": args.calls,
           "rounds": args.rounds, "unit": "us per call: median (min, max) over the rounds",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence)",
           "call_us": "calls through the Python wrapper (includes the host's submission cost)",
           "msnake_step": "plays the constant action 1 with auto reset: the batch drifts from the labelled state",
           "batches": {}}
    for n in args.envs:
        env, acts = ch.played_env(n, 0)
        ones = torch.ones((n, 3), dtype=torch.int32, device=env.device)
        safe = torch.zeros((n, 3), dtype=torch.uint8, device=env.device)
        all4 = env.move_fates_device(by=True, eat=True)
        masks = msnake.MoveFates(None, None, None, all4.mask)
        legs = {
            "safe_greedy": lambda: env.scripted_actions_device("safe_greedy", out=acts),
            "safe_greedy+mask": lambda: env.scripted_actions_device("safe_greedy", out=acts, safe_out=safe),
            "mask_only": lambda: env.safe_moves_device(out=safe),
            "wary_greedy": lambda: env.scripted_actions_device("wary_greedy", out=acts),
            "wary_greedy+fate+by+eat+mask": lambda: env.scripted_actions_device("wary_greedy", out=acts, fates_out=all4),
            "fate_masks_only": lambda: env.move_fates_device(out=masks),
            "fate+by+eat+mask": lambda: env.move_fates_device(out=all4),
            "msnake_step": lambda: env.step_device(ones),
            "safe_greedy->step": lambda: env.step_device(env.scripted_actions_device("safe_greedy", out=acts)),
            "wary_greedy->step": lambda: env.step_device(env.scripted_actions_device("wary_greedy", out=acts)),
        }
        out = {}
        for state in ("fresh_reset", f"after_{args.play_steps}_greedy_steps"):
            env.reset_device()
            ch.play(env, acts, 0 if state == "fresh_reset" else args.play_steps)
            blob = env.get_state_all()
            readers = {k: fn for k, fn in legs.items() if "step" not in k}
            for fn in readers.values():
                fn()
            ch.assert_unchanged(env, blob)
            times = ch.graph_legs(legs, args.calls, args.rounds, restore=lambda: env.set_state_all(blob), eager=True)
            out[state] = {k: {kind: ch.med(v) for kind, v in t.items()} for k, t in times.items()}
            print(f"{n} envs, {state}: done", file=sys.stderr, flush=True)
        res["batches"][str(n)] = out
        env.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
