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
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_cost.json"))
    ap.add_argument("--merge", nargs="+", metavar="JSON", help="combine the files of several processes into --out and exit")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    import torch
    import msnake

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / args.calls

    med = lambda v: [round(sorted(v)[len(v) // 2], 3), round(min(v), 3), round(max(v), 3)]
    w2 = (2 * RADIUS + 1) ** 2
    res = {"device": torch.cuda.get_device_name(0), "config": f"snake_env 19x19, 3 snakes, radius {RADIUS}", "calls_per_leg": args.calls,
           "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "graph_us: median (min, max) over the rounds, us per call",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "batches": {}}
    for n in args.envs:
        env = msnake.MultiSnakeVecEnv(n, dim=19, n_snakes=3, rules="snake_env", seed=0)
        acts = torch.ones((n, 3), dtype=torch.int32, device=env.device)
        env.reset_device()
        for _ in range(args.play_steps):
            env.step_device(env.scripted_actions_device("safe_greedy", out=acts))
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
        graphs = {}
        side = torch.cuda.Stream()
        for name, (fn, _) in legs.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up on a side stream, as graph capture wants
                fn(), fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(args.calls):
                    fn()
            graphs[name] = gr
        env.set_state_all(blob)                # the step leg's warm-up aside: back to the boards after the play
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for name in legs:
                times[name].append(timed(graphs[name].replay))
                if name == "msnake_step":
                    env.set_state_all(blob)
        assert env.get_state_all().tobytes() == blob.tobytes() and env.stats()["errors"] == 0
        # snake 0's window is the same whether it is rendered alone or with the others; the centre of a window is the head's
        # own cell, and walls are in sight
        graphs["cells_all_views"].replay(), graphs["local_three_oriented"].replay(), graphs["local_one"].replay()
        torch.cuda.synchronize()
        assert torch.equal(win3[:, :1], win1) and float((win3[:, :, RADIUS, RADIUS] == 3).float().mean()) > 0.5
        assert int((win3 == 6).sum()) > 0 and int(head3.max()) <= 3
        res["batches"][str(n)] = {k: {"graph_us": med(v), "bytes_per_env": legs[k][1]} for k, v in times.items()}
        env.close()
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
