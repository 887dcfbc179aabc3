#!/usr/bin/env python3
"""Cost of msnake_head_fields next to its yardsticks on the same handle: fruit_field_device() alone (one front, one staged
plane), territory_device() (five fronts per snake) and msnake_step.  19x19x3 snake_env at 4 096 and 32 768 envs, on a
freshly reset batch and 500 steps into safe_greedy play.  The legs: owner + counts alone (the race, no plane), all three
snakes' planes alone (the fronts, no race), one plane alone, and everything together.  `worst_case_62x62`: serpentine
mazes of a 62x62 board (one corridor of 1 953 cells, along the rows and along the columns) with snake 0 on one end and
snake 2 on the other, copied over the whole batch: the most levels a race can have.  `other_boards`: the plane legs 500
steps into greedy play at 32x32 and 44x44, on either side of the size up to which the planes are staged.

Figures are us per call from HIP events: CALLS back-to-back calls captured into one HIP graph and replayed, legs
alternating in one process, the state restored before every leg; the legs only read it (checked).

--ab LIB [LIB ...]: the same legs once more, each in a child process of its own, on other builds of the library
(MSNAKE_LIB), for the A/B of the plane store.  The shipped library stages the planes in LDS while they are small and
writes a new cell's level straight to HBM otherwise; `make -C <pkg>/csrc variant NAME=heads_direct
EXTRA=-DMSNAKE_HEADS_DIRECT` and `... NAME=heads_staged EXTRA=-DMSNAKE_HEADS_STAGED` do one or the other for every
shape.  The result carries the shipped library under "shipped" and the others under "variants".
    P=self-play-on-multi-snakes-environment_amd
    python tools/heads_cost.py --ab $P/libmsnake_heads_direct.so $P/libmsnake_heads_staged.so --out profiles/heads_cost.json"""
import argparse
import json
import os
import subprocess
import sys

import cost_harness as ch
from scripted_cost import serpentine_states


def maze_states(transposed):
    """The serpentine of scripted_cost with a third snake: snake 0 on the corridor's first cell, snake 1 the wall, snake 2
    on its last cell; the fruits lie in the corridor's middle, so that the field leg has a front to run as well."""
    st = serpentine_states(62, transposed)
    first, last = st[0], st[-1]
    return [dict(first, fruits=[st[5]["snakes"][0][0]] * 3, snakes=first["snakes"] + [last["snakes"][0]], vels=[[1, 0]] * 3,
                 grow_to=first["grow_to"] + [1], alive=[True] * 3, in_dead=[False] * 3)]


def measure(args):
    import torch
    import msnake
    res = {"library": os.path.basename(msnake._capi.LIB_PATH), "batches": {}, "other_boards": {}, "worst_case_62x62": {}}
    for n in args.envs:
        env = msnake.MultiSnakeVecEnv(n, dim=19, n_snakes=3, rules="snake_env", seed=0)
        acts = torch.ones((n, 3), dtype=torch.int32, device=env.device)
        ones = torch.ones((n, 3), dtype=torch.int32, device=env.device)
        dist = torch.zeros((n, 3, 19, 19), dtype=torch.uint16, device=env.device)
        one = torch.zeros((n, 1, 19, 19), dtype=torch.uint16, device=env.device)
        owner = torch.zeros((n, 19, 19), dtype=torch.uint8, device=env.device)
        counts = torch.zeros((n, 3), dtype=torch.uint16, device=env.device)
        terr = torch.zeros((n, 3, 4), dtype=torch.uint16, device=env.device)
        field = torch.zeros((n, 19, 19), dtype=torch.uint16, device=env.device)
        legs = {
            "owner+counts": lambda: env.head_fields_device(owner_out=owner, counts_out=counts, dist=False),
            "counts_only": lambda: env.owned_counts_device(out=counts),
            "planes_only": lambda: env.head_distances_device(out=dist),
            "one_plane_only": lambda: env.head_distances_device(1, out=one),
            "planes+owner+counts": lambda: env.head_fields_device(dist_out=dist, owner_out=owner, counts_out=counts),
            "field_only": lambda: env.fruit_field_device(out=field),
            "territory_only": lambda: env.territory_device(out=terr),
            "msnake_step": lambda: env.step_device(ones),
        }
        out = {}
        for state in ("fresh_reset", f"after_{args.play_steps}_greedy_steps"):
            env.reset_device()
            ch.play(env, acts, 0 if state == "fresh_reset" else args.play_steps)
            blob = env.get_state_all()
            times = ch.graph_legs(legs, args.calls, args.rounds, restore=lambda: env.set_state_all(blob))
            ch.assert_unchanged(env, blob)
            out[state] = {k: ch.med(t["graph_us"]) for k, t in times.items()}
            print(f"{n} envs, {state}: done", file=sys.stderr, flush=True)
        res["batches"][str(n)] = out
        env.close()
    # the plane store between the flagship board and the largest: where one wave's three planes grow from 6 to 12 KiB
    for dim in args.other_dims:
        res["other_boards"][f"{dim}x{dim}"] = {}
        for n in args.envs:
            env, acts = ch.played_env(n, args.play_steps, dim=dim)
            dist = torch.zeros((n, 3, dim, dim), dtype=torch.uint16, device=env.device)
            owner = torch.zeros((n, dim, dim), dtype=torch.uint8, device=env.device)
            counts = torch.zeros((n, 3), dtype=torch.uint16, device=env.device)
            field = torch.zeros((n, dim, dim), dtype=torch.uint16, device=env.device)
            legs = {
                "planes_only": lambda: env.head_distances_device(out=dist),
                "planes+owner+counts": lambda: env.head_fields_device(dist_out=dist, owner_out=owner, counts_out=counts),
                "field_only": lambda: env.fruit_field_device(out=field),
            }
            times = ch.graph_legs(legs, args.calls, args.rounds)
            res["other_boards"][f"{dim}x{dim}"][str(n)] = {k: ch.med(t["graph_us"]) for k, t in times.items()}
            env.close()
            print(f"{n} envs, {dim}x{dim}: done", file=sys.stderr, flush=True)
    from oracle.snake_oracle import state_to_flat
    for n in args.envs:
        out = {}
        for name, transposed in (("two_ends_rows", False), ("two_ends_columns", True)):
            states = maze_states(transposed)
            src = msnake.MultiSnakeVecEnv(len(states), dim=62, n_snakes=3, rules="snake_env", seed=0)
            env = msnake.MultiSnakeVecEnv(n, dim=62, n_snakes=3, rules="snake_env", seed=0)
            src.reset_device(), env.reset_device()
            for e, st in enumerate(states):
                src.set_state_words(e, state_to_flat(st, 3))
            env.copy_envs_device(src, torch.arange(n, dtype=torch.int32, device=env.device) % len(states))
            dist = torch.zeros((n, 3, 62, 62), dtype=torch.uint16, device=env.device)
            owner = torch.zeros((n, 62, 62), dtype=torch.uint8, device=env.device)
            counts = torch.zeros((n, 3), dtype=torch.uint16, device=env.device)
            terr = torch.zeros((n, 3, 4), dtype=torch.uint16, device=env.device)
            field = torch.zeros((n, 62, 62), dtype=torch.uint16, device=env.device)
            legs = {
                "owner+counts": lambda: env.head_fields_device(owner_out=owner, counts_out=counts, dist=False),
                "planes_only": lambda: env.head_distances_device(out=dist),
                "planes+owner+counts": lambda: env.head_fields_device(dist_out=dist, owner_out=owner, counts_out=counts),
                "field_only": lambda: env.fruit_field_device(out=field),
                "territory_only": lambda: env.territory_device(out=terr),
            }
            times = ch.graph_legs(legs, args.worst_calls, args.rounds)
            out[name] = {k: ch.med(t["graph_us"]) for k, t in times.items()}
            far = dist.view(torch.int16).to(torch.int32) & 0xFFFF
            out[name]["largest_distance"] = int(torch.where(far == 0xFFFF, torch.zeros_like(far), far).max())
            assert out[name]["largest_distance"] == 1951 and int(counts.view(torch.int16)[0].sum()) > 1900
            env.close(), src.close()
            print(f"{n} envs, worst case {name}: done", file=sys.stderr, flush=True)
        res["worst_case_62x62"][str(n)] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--worst-calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=500)
    ap.add_argument("--other-dims", type=int, nargs="*", default=[32, 44], help="boards for the planes-only legs besides 19x19")
    ap.add_argument("--ab", nargs="+", default=[], help="other builds of the library to run the same legs on, each in a child process")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    import torch
    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "calls_per_leg": args.calls,
           "calls_per_worst_case_leg": args.worst_calls, "rounds": args.rounds,
           "unit": "us per call, calls captured into one HIP graph and replayed: median (min, max) over the rounds",
           "msnake_step": "plays the constant action 1 with auto reset: the batch drifts from the labelled state",
           "shipped": measure(args)}
    for lib in args.ab:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--worst-calls", str(args.worst_calls),
               "--rounds", str(args.rounds), "--play-steps", str(args.play_steps), "--envs"] + [str(n) for n in args.envs] + ["--other-dims"] + [str(d) for d in args.other_dims]
        out = subprocess.run(cmd, env=dict(os.environ, MSNAKE_LIB=os.path.abspath(lib)), capture_output=True, text=True,
                             timeout=900)
        sys.stderr.write(out.stderr)
        assert out.returncode == 0, out.returncode
        res.setdefault("variants", {})[os.path.basename(lib)] = json.loads(out.stdout.strip().split("\n")[-1])
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
