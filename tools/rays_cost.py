#!/usr/bin/env python3
"""Cost of msnake_render_rays next to msnake_render_local and msnake_render_cells.  19x19x3 snake_env at 4 096 and
32 768 envs, 300 steps into greedy play (bodies of a dozen cells); every call only reads the state, so every leg sees the
same boards.

One figure per leg, from HIP events after a warm-up, legs alternating in one process on one handle:
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence,
            free of the host's submission cost.
Legs: "rays_three" (every snake, oriented, with headings: 96 + 3 bytes per env), "rays_one" (snake 0, oriented, no
headings: 32 bytes per env), "local_three_r5" and "local_one_r5" (the radius-5 windows of the same selections: 363 + 3 and
121 bytes per env) and "cells_three_views" (1 083 bytes per env).  bytes_per_env is what each leg writes.  The comparison
is descriptive: nothing gates on it.
    python tools/rays_cost.py                      # writes profiles/rays_cost.json"""
import argparse
import os

import cost_harness as ch

RADIUS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ch.ROOT, "profiles", "rays_cost.json"))
    args = ap.parse_args()
    import torch

    w = 2 * RADIUS + 1
    res = {"device": torch.cuda.get_device_name(0), "config": f"snake_env 19x19, 3 snakes, window radius {RADIUS}",
           "calls_per_leg": args.calls, "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "graph_us: median (min, max) over the rounds, us per call",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "batches": {}}
    for n in args.envs:
        env, _ = ch.played_env(n, args.play_steps)
        u8 = lambda *shape: torch.empty((n,) + shape, dtype=torch.uint8, device=env.device)
        rays3, rays1, head3 = u8(3, 8, 4), u8(1, 8, 4), u8(3)
        win3, win1, whead3, full = u8(3, w, w), u8(1, w, w), u8(3), u8(3, 19, 19)
        legs = {
            "rays_three": (lambda: env.render_rays_device(out=rays3, heading_out=head3), 3 * 32 + 3),
            "rays_one": (lambda: env.render_rays_device(snakes=0, out=rays1), 32),
            "local_three_r5": (lambda: env.render_local_device(RADIUS, out=win3, heading_out=whead3), 3 * w * w + 3),
            "local_one_r5": (lambda: env.render_local_device(RADIUS, snakes=0, out=win1), w * w),
            "cells_three_views": (lambda: env.render_cells_device(out=full), 3 * 361),
        }
        blob = env.get_state_all()
        times = ch.graph_legs({k: fn for k, (fn, _) in legs.items()}, args.calls, args.rounds)
        ch.assert_unchanged(env, blob)
        # snake 0's rays are the same whether they are rendered alone or with the others; a snake with a body (the centre
        # of its window is not 0) sees a wall in every direction; the step ahead of a head agrees with the window's entry
        # there; the headings agree
        torch.cuda.synchronize()
        body = win3[:, :, RADIUS, RADIUS] != 0
        assert torch.equal(rays3[:, :1], rays1) and torch.equal(rays3[..., 0] >= 1, body[..., None].expand(-1, -1, 8))
        assert int(rays3.max()) <= 20 and float(body.float().mean()) > 0.5
        ahead = win3[:, :, RADIUS + 1, RADIUS]
        assert torch.equal(rays3[:, :, 0, 0] == 1, ahead == 6) and torch.equal(rays3[:, :, 0, 1] == 1, ahead == 1)
        assert torch.equal(head3, whead3)
        res["batches"][str(n)] = {k: {"graph_us": ch.med(t["graph_us"]), "bytes_per_env": legs[k][1]} for k, t in times.items()}
        env.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
