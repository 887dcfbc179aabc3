#!/usr/bin/env python3
"""Cost of msnake_agent_outcomes next to the table-only msnake_render_cells, the composition that forms the same outcomes
without it, and msnake_step.  19x19x3 snake_env at 4 096 and 32 768 envs, some hundred steps into safe_greedy play on a
handle without auto reset (every step followed by a masked reset of the done envs).

One figure per leg, from HIP events after a warm-up, legs alternating in one process on one handle:
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence,
            free of the host's submission cost.
Legs: "outcomes_all" (rew, ate, flags and info: 22 bytes per snake written, the 32-byte tracker row read and written),
"outcomes_rew_flags" (5 bytes per snake), "arm" (the tracker row written), "cells_table_only" (msnake_render_cells with
no plane: the int32 [n_snakes][8] table, which reads the same record words and writes about as much -- the yardstick),
"torch_composition" (what a caller could do before this entry point: the table before and after a step and the torch
operations that form ate, died and rew from the two) and "msnake_step" (on a copy of the handle with auto reset, under
the constant action 1: snakes die and envs reset, as in untrained play).  The outcome legs run with done = 0 on an
armed tracker and only read the state, so every leg sees the same boards.  Descriptive: nothing gates on it.
    python tools/agents_cost.py            # writes profiles/agents_cost.json"""
import argparse
import os

import cost_harness as ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ch.ROOT, "profiles", "agents_cost.json"))
    args = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "calls_per_leg": args.calls,
           "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "graph_us: median (min, max) over the rounds, us per call",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "batches": {}}
    S = 3
    for n in args.envs:
        env, _ = ch.played_env(n, args.play_steps, masked_reset=True, n_snakes=S, auto_reset=False)
        stepper = env.clone(auto_reset=True)
        ones = torch.ones((n, S), dtype=torch.int32, device=env.device)
        zero_done = torch.zeros(n, dtype=torch.uint8, device=env.device)
        rew = torch.empty((n, S), dtype=torch.float32, device=env.device)
        ate, flags = (torch.empty((n, S), dtype=torch.uint8, device=env.device) for _ in range(2))
        info = torch.empty((n, S, 4), dtype=torch.int32, device=env.device)
        before, after = (torch.empty((n, S, 8), dtype=torch.int32, device=env.device) for _ in range(2))
        env.arm_agents_device()

        def composition():
            env.render_cells_device(views=[], snakes_out=before)
            env.render_cells_device(views=[], snakes_out=after)
            c_ate = (after[..., 5] - before[..., 5]).clamp_(min=0) >> 1
            died = (before[..., 0] > 0) & ~(after[..., 0] > 0)
            return torch.where(died, -1.0, c_ate.float()), c_ate, died

        legs = {
            "outcomes_all": (lambda: env.agent_outcomes_device(zero_done, rew, ate, flags, info), S * (4 + 1 + 1 + 16)),
            "outcomes_rew_flags": (lambda: env.agent_outcomes_device(zero_done, rew_out=rew, flags_out=flags), S * 5),
            "arm": (env.arm_agents_device, S * 32),
            "cells_table_only": (lambda: env.render_cells_device(views=[], snakes_out=after), S * 32),
            "torch_composition": (composition, 2 * S * 32 + S * (4 + 8 + 1)),
            "msnake_step": (lambda: stepper.step_device(ones), int(stepper.obs_shape[0] * stepper.obs_shape[1] * stepper.obs_shape[2])),
        }
        blob = env.get_state_all().tobytes()
        times = ch.graph_legs({k: fn for k, (fn, _) in legs.items()}, args.calls, args.rounds)
        ch.assert_unchanged(env, blob)   # every leg on `env` only read the state
        # a quiet step on an armed tracker: nothing eaten, nobody died, and the composition says the same
        c_rew, c_ate, c_died = composition()
        env.arm_agents_device()
        env.agent_outcomes_device(zero_done, rew, ate, flags, info)
        assert torch.equal(c_rew, rew) and torch.equal(c_ate.to(torch.uint8), ate) and not bool(c_died.any())
        assert torch.equal((flags & 1) != 0, after[..., 0] > 0) and not bool((flags & 4).any())
        res["batches"][str(n)] = {k: {"graph_us": ch.med(t["graph_us"]), "bytes_per_env": legs[k][1]} for k, t in times.items()}
        env.close(), stepper.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
