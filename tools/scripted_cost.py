#!/usr/bin/env python3
"""Cost of msnake_scripted_actions, msnake_space_actions, msnake_territory_actions, msnake_path_actions and msnake_timed_actions next to msnake_step on the same handle.  19x19x3 snake_env at
4 096 and 32 768 envs, on a freshly reset batch and 500 steps into safe_greedy play (longer bodies).  The Hamiltonian
cycle needs an even board: its legs run on a 20x20 handle of the same batch, in the same kind of state.  The "->step"
legs are one scripted call and one step per call (the self-play loop on the device).  `worst_case_62x62`: the flood
fill's longest runs, serpentine mazes of a 62x62 board (one corridor of 1 953 cells, along the rows and along the
columns, nine head positions each), copied over the whole batch; the territory race runs on the same states (the wall
snake is the opponent), and on `two_ends`, where two snakes enter the corridor from its two ends.  The fruits of these
states lie on the corridor's first cell, so the BFS of msnake_path_actions walks the corridor from that end up to the
head: with the field it runs to the end (up to 1 951 levels), without it it stops at the head's open target.
The wall snake of these states has its natural lifetimes (grow_to = its length), so under msnake_timed_actions the walls
dissolve from the tail while the fill runs; `lasting_walls_on_rows` / `_columns` are the same mazes with the wall's
grow_to at 2^31 - 1 (every lifetime clamped high), where the timed fill is the corridor, level by level.

Two figures per leg, both from HIP events after a warm-up, legs alternating in one process:
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence,
            free of the host's submission cost;
  call_us:  CALLS back-to-back calls through the Python wrapper (validation + ctypes + the stream lookup): what a
            Python caller pays when nothing else is queued; mostly the host's submission rate.
The step leg plays the constant action 1 (with auto reset), so over its CALLS calls the batch leaves the state the run
is labelled with; the scripted legs read the restored state every time.  The state is restored before every leg.
    python tools/scripted_cost.py --out profiles/timed_cost.json"""
import argparse
import sys

import cost_harness as ch


def serpentine_states(dim, transposed, wall_grow=None):
    """Canonical states of a two-snake snake_env: snake 1 is a serpentine wall (the odd rows, each with one gap at
    alternating ends; grow_to = wall_grow, by default its length), snake 0 a single cell at nine places of the corridor."""
    walls, path, right = [], [], True
    for y in range(dim):
        if y % 2 == 0:
            path += [(x, y) for x in (range(dim) if right else range(dim - 1, -1, -1))]
        else:
            gap = dim - 1 if right else 0
            walls += [(x, y) for x in range(dim) if x != gap]
            path.append((gap, y))
            right = not right
    if transposed:
        walls, path = [(y, x) for x, y in walls], [(y, x) for x, y in path]
    L = len(path)
    return [{"t": 0, "ctr": 0, "spare_fruits": 0, "ep_len": 0, "ep_return": 0.0, "fruits": [[0, 0], [0, 0]],
             "snakes": [[list(path[i])], [list(c) for c in walls]], "vels": [[1, 0]] * 2, "grow_to": [1, wall_grow or len(walls)],
             "alive": [True] * 2, "in_dead": [False] * 2} for i in (0, 1, L // 8, L // 4, L // 3, L // 2, 2 * L // 3, L - 2, L - 1)]


def two_ends(states):
    """The same mazes with the wall stacked under snake 0's head on one end of the corridor and snake 1 on the other: the
    two fronts meet in the middle after half the corridor's length in rounds."""
    first, last = states[0]["snakes"][0][0], states[-1]["snakes"][0][0]
    walls = states[0]["snakes"][1]
    return [dict(states[0], snakes=[[first] + walls, [last]], grow_to=[len(walls) + 1, 1])]


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
           "hamiltonian": "on a 20x20 handle of the same batch (the cycle needs an even board)",
           "msnake_step": "plays the constant action 1 with auto reset: the batch drifts from the labelled state",
           "batches": {}}
    for n in args.envs:
        env = msnake.MultiSnakeVecEnv(n, dim=19, n_snakes=3, rules="snake_env", seed=0)
        env20 = msnake.MultiSnakeVecEnv(n, dim=20, n_snakes=3, rules="snake_env", seed=0)
        acts = torch.ones((n, 3), dtype=torch.int32, device=env.device)
        ones = torch.ones((n, 3), dtype=torch.int32, device=env.device)
        safe = torch.zeros((n, 3), dtype=torch.uint8, device=env.device)
        space = torch.zeros((n, 3, 4), dtype=torch.uint16, device=env.device)
        terr = torch.zeros((n, 3, 4), dtype=torch.uint16, device=env.device)
        path = torch.zeros((n, 3, 4), dtype=torch.uint16, device=env.device)
        field = torch.zeros((n, 19, 19), dtype=torch.uint16, device=env.device)
        reach = torch.zeros((n, 3, 4), dtype=torch.uint16, device=env.device)
        life = torch.zeros((n, 19, 19), dtype=torch.uint16, device=env.device)
        legs = {
            "safe_greedy": lambda: env.scripted_actions_device("safe_greedy", out=acts),
            "safe_greedy+mask": lambda: env.scripted_actions_device("safe_greedy", out=acts, safe_out=safe),
            "hamiltonian_20x20": lambda: env20.scripted_actions_device("hamiltonian", out=acts),
            "hamiltonian_20x20+mask": lambda: env20.scripted_actions_device("hamiltonian", out=acts, safe_out=safe),
            "mask_only": lambda: env.safe_moves_device(out=safe),
            "space_greedy": lambda: env.scripted_actions_device("space_greedy", out=acts),
            "space_greedy+mask+space": lambda: env.scripted_actions_device("space_greedy", out=acts, safe_out=safe, space_out=space),
            "space_only": lambda: env.reachable_space_device(out=space),
            "territory_greedy": lambda: env.scripted_actions_device("territory_greedy", out=acts),
            "territory_greedy+mask+territory": lambda: env.scripted_actions_device("territory_greedy", out=acts, safe_out=safe,
                                                                                   territory_out=terr),
            "territory_only": lambda: env.territory_device(out=terr),
            "path_greedy": lambda: env.scripted_actions_device("path_greedy", out=acts),
            "path_greedy+mask+path+field": lambda: env.scripted_actions_device("path_greedy", out=acts, safe_out=safe, path_out=path,
                                                                               field_out=field),
            "path_only": lambda: env.path_device(out=path),
            "field_only": lambda: env.fruit_field_device(out=field),
            "timed_greedy": lambda: env.scripted_actions_device("timed_greedy", out=acts),
            "timed_greedy+mask+reach+life": lambda: env.scripted_actions_device("timed_greedy", out=acts, safe_out=safe, reach_out=reach,
                                                                                life_out=life),
            "reach_only": lambda: env.timed_reach_device(out=reach),
            "life_only": lambda: env.cell_lifetimes_device(out=life),
            "msnake_step": lambda: env.step_device(ones),
            "safe_greedy->step": lambda: env.step_device(env.scripted_actions_device("safe_greedy", out=acts)),
            "space_greedy->step": lambda: env.step_device(env.scripted_actions_device("space_greedy", out=acts)),
            "territory_greedy->step": lambda: env.step_device(env.scripted_actions_device("territory_greedy", out=acts)),
            "path_greedy->step": lambda: env.step_device(env.scripted_actions_device("path_greedy", out=acts)),
            "timed_greedy->step": lambda: env.step_device(env.scripted_actions_device("timed_greedy", out=acts)),
        }
        out = {}
        for state in ("fresh_reset", f"after_{args.play_steps}_greedy_steps"):
            for e in (env, env20):
                e.reset_device()
                ch.play(e, acts, 0 if state == "fresh_reset" else args.play_steps)
            blob = env.get_state_all()
            times = ch.graph_legs(legs, args.calls, args.rounds, restore=lambda: env.set_state_all(blob), eager=True)
            out[state] = {k: {kind: ch.med(v) for kind, v in t.items()} for k, t in times.items()}
            print(f"{n} envs, {state}: done", file=sys.stderr, flush=True)
        res["batches"][str(n)] = out
        env.close(), env20.close()
    from oracle.snake_oracle import state_to_flat
    res["worst_case_62x62"] = {}
    for n in args.envs:
        out = {}
        for name, transposed, ends, wall_grow in (("walls_on_rows", False, False, None), ("walls_on_columns", True, False, None),
                                                  ("two_ends_rows", False, True, None), ("two_ends_columns", True, True, None),
                                                  ("lasting_walls_on_rows", False, False, 2 ** 31 - 1),
                                                  ("lasting_walls_on_columns", True, False, 2 ** 31 - 1)):
            states = serpentine_states(62, transposed, wall_grow)
            if ends:
                states = two_ends(states)
            src = msnake.MultiSnakeVecEnv(len(states), dim=62, n_snakes=2, rules="snake_env", seed=0)
            env = msnake.MultiSnakeVecEnv(n, dim=62, n_snakes=2, rules="snake_env", seed=0)
            src.reset_device(), env.reset_device()
            for e, st in enumerate(states):
                src.set_state_words(e, state_to_flat(st, 2))
            env.copy_envs_device(src, torch.arange(n, dtype=torch.int32, device=env.device) % len(states))
            acts = torch.ones((n, 2), dtype=torch.int32, device=env.device)
            space = torch.zeros((n, 2, 4), dtype=torch.uint16, device=env.device)
            field = torch.zeros((n, 62, 62), dtype=torch.uint16, device=env.device)
            out[name] = {}
            for leg, pol, kw in (("space_greedy", "space_greedy", {"space_out": space}),
                                 ("territory_greedy", "territory_greedy", {"territory_out": space}),
                                 ("path_greedy", "path_greedy", {"path_out": space}),
                                 ("path_greedy+field", "path_greedy", {"path_out": space, "field_out": field}),
                                 ("timed_greedy", "timed_greedy", {"reach_out": space}),
                                 ("timed_greedy+life", "timed_greedy", {"reach_out": space, "life_out": field})):
                fn = lambda: env.scripted_actions_device(pol, out=acts, **kw)
                v = ch.graph_legs({leg: fn}, args.calls, args.rounds)[leg]["graph_us"]
                count = space.view(torch.int16).to(torch.int32) & 0xFFFF
                if pol == "path_greedy":  # the longest finite path (MSNAKE_PATH_NONE is no count)
                    count = torch.where(count == 0xFFFF, torch.zeros_like(count), count)
                out[name][leg] = {"graph_us": ch.med(v), "largest_count": int(count.max())}
            env.close(), src.close()
            print(f"{n} envs, worst case {name}: done", file=sys.stderr, flush=True)
        res["worst_case_62x62"][str(n)] = out
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
