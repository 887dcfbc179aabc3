#!/usr/bin/env python3
"""Cost of msnake_render_cells next to msnake_render.  19x19x3 snake_env at 4 096 and 32 768 envs, some hundred steps
into safe_greedy play (bodies of a dozen cells); both calls only read the state, so every leg sees the same boards.

One figure per leg, from HIP events after a warm-up, legs alternating in one process on one handle:
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence,
            free of the host's submission cost.
Legs: "cells_one_view" (view 0: 361 bytes per env), "cells_all_views" (1 083 bytes per env), "cells_all_views_table"
(plus the int32 [n_snakes][8] table, 96 bytes per env) and "msnake_render" (the RGB frame, 3 969 bytes per env).
bytes_per_env is what each leg writes; the state it reads is the same for all.  The comparison is descriptive: nothing
gates on it.
    python tools/cells_cost.py            # writes profiles/cells_cost.json"""
import argparse
import math
import os

import cost_harness as ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ch.ROOT, "profiles", "cells_cost.json"))
    args = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "calls_per_leg": args.calls,
           "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "graph_us: median (min, max) over the rounds, us per call",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "batches": {}}
    for n in args.envs:
        env, _ = ch.played_env(n, args.play_steps)
        one = torch.empty((n, 1, 19, 19), dtype=torch.uint8, device=env.device)
        full = torch.empty((n, 3, 19, 19), dtype=torch.uint8, device=env.device)
        table = torch.empty((n, 3, 8), dtype=torch.int32, device=env.device)
        frame = torch.empty((n,) + env.obs_shape, dtype=torch.uint8, device=env.device)
        legs = {
            "cells_one_view": (lambda: env.render_cells_device(views=0, out=one), 361),
            "cells_all_views": (lambda: env.render_cells_device(out=full), 1083),
            "cells_all_views_table": (lambda: env.render_cells_device(out=full, snakes_out=table), 1083 + 96),
            "msnake_render": (lambda: env.render_device(out=frame), math.prod(env.obs_shape)),
        }
        blob = env.get_state_all().tobytes()
        times = ch.graph_legs({k: fn for k, (fn, _) in legs.items()}, args.calls, args.rounds)
        ch.assert_unchanged(env, blob)   # every leg only read the state
        # the planes are the frame: a cell of view 0 is black in the frame iff its code is 0
        assert torch.equal(full[:, :1], one) and torch.equal((frame[:, 1:-1, 1:-1, :3] != 0).any(-1), one[:, 0] != 0)
        res["batches"][str(n)] = {k: {"graph_us": ch.med(t["graph_us"]), "bytes_per_env": legs[k][1]} for k, t in times.items()}
        env.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
