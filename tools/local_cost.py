#!/usr/bin/env python3
"""Cost of msnake_render_local next to msnake_render_cells, msnake_render and msnake_step.  19x19x3 snake_env at 4 096
and 32 768 envs, some hundred steps into safe_greedy play (bodies of a dozen cells); the render calls only read the
state, so every such leg sees the same boards, and the step leg is rolled back to them after each of its replays.

One figure per leg, from HIP events after a warm-up, legs alternating in one process on one handle:
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence,
            free of the host's submission cost.
Legs: "local_three_oriented" (radius 5, every snake, oriented, with headings: 363 + 3 bytes per env), "local_one"
(radius 5, snake 0, oriented, no headings: 121 bytes per env), "cells_all_views" (1 083 bytes per env: the yardstick, it
reads the same state), "msnake_render" (the RGB frame, 3 969 bytes per env) and "msnake_step" (the step under the last
greedy actions, frame included).  bytes_per_env is what each leg writes.  The comparison is descriptive: nothing gates on
it.
    python tools/local_cost.py --out run1.json          # one process
    python tools/local_cost.py --merge run1.json run2.json run3.json    # writes profiles/local_cost.json: every process,
                                                        # and per leg the median, min and max of the processes' medians"""
import argparse
import json
import math
import os

import cost_harness as ch

RADIUS = 5


def merge(paths, out):
    runs = [json.load(open(p)) for p in paths]
    head = {k: v for k, v in runs[0].items() if k != "batches"}
    summary = {}
    for n, legs in runs[0]["batches"].items():
        summary[n] = {}
        for leg, rec in legs.items():
            meds = sorted(r["batches"][n][leg]["graph_us"][0] for r in runs)
            summary[n][leg] = {"graph_us_over_processes": [meds[len(meds) // 2], meds[0], meds[-1]], "bytes_per_env": rec["bytes_per_env"]}
    res = dict(head, processes=len(runs), summary_unit="median (min, max) of the processes' medians, us per call", summary=summary,
               per_process=[r["batches"] for r in runs])
    text = json.dumps(res, indent=1)
    with open(out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(summary, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ch.ROOT, "profiles", "local_cost.json"))
    ap.add_argument("--merge", nargs="+", metavar="JSON", help="combine the files of several processes into --out and exit")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    import torch

    w2 = (2 * RADIUS + 1) ** 2
    res = {"device": torch.cuda.get_device_name(0), "config": f"snake_env 19x19, 3 snakes, radius {RADIUS}", "calls_per_leg": args.calls,
           "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "graph_us: median (min, max) over the rounds, us per call",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "batches": {}}
    for n in args.envs:
        env, acts = ch.played_env(n, args.play_steps)
        env.scripted_actions_device("safe_greedy", out=acts)      # the actions the step leg replays
        win3 = torch.empty((n, 3, 2 * RADIUS + 1, 2 * RADIUS + 1), dtype=torch.uint8, device=env.device)
        head3 = torch.empty((n, 3), dtype=torch.uint8, device=env.device)
        win1 = torch.empty((n, 1, 2 * RADIUS + 1, 2 * RADIUS + 1), dtype=torch.uint8, device=env.device)
        full = torch.empty((n, 3, 19, 19), dtype=torch.uint8, device=env.device)
        frame = torch.empty((n,) + env.obs_shape, dtype=torch.uint8, device=env.device)
        legs = {
            "local_three_oriented": (lambda: env.render_local_device(RADIUS, out=win3, heading_out=head3), 3 * w2 + 3),
            "local_one": (lambda: env.render_local_device(RADIUS, snakes=0, out=win1), w2),
            "cells_all_views": (lambda: env.render_cells_device(out=full), 1083),
            "msnake_render": (lambda: env.render_device(out=frame), math.prod(env.obs_shape)),
            "msnake_step": (lambda: env.step_device(acts), math.prod(env.obs_shape)),
        }
        blob = env.get_state_all()
        # (the step leg moves the envs: back to the boards after the play before every leg and behind the last)
        times = ch.graph_legs({k: fn for k, (fn, _) in legs.items()}, args.calls, args.rounds, restore=lambda: env.set_state_all(blob))
        ch.assert_unchanged(env, blob)
        # snake 0's window is the same whether it is rendered alone or with the others; the centre of a window is the head's
        # own cell, and walls are in sight
        legs["cells_all_views"][0](), legs["local_three_oriented"][0](), legs["local_one"][0]()
        torch.cuda.synchronize()
        assert torch.equal(win3[:, :1], win1) and float((win3[:, :, RADIUS, RADIUS] == 3).float().mean()) > 0.5
        assert int((win3 == 6).sum()) > 0 and int(head3.max()) <= 3
        res["batches"][str(n)] = {k: {"graph_us": ch.med(t["graph_us"]), "bytes_per_env": legs[k][1]} for k, t in times.items()}
        env.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
