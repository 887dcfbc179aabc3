#!/usr/bin/env python3
"""What one ply of playouts buys a scripted player.  Snake 0 plays the move with the best playout value
(playout_values_device: K = 16 steps, 4 reps per move, every snake on safe_greedy inside the playouts; ties go to
safe_greedy's own move), snakes 1 and 2 play safe_greedy; next to it the same batch with snake 0 on plain safe_greedy.
snake_env 10x10x3 and 19x19x3, 256 envs x 1 000 steps with auto reset; ended episodes, mean length and mean return of
both, from msnake_get_stats.  No threshold: the figures are recorded whichever way they go.
    python tools/playout_search.py --out profiles/playout_search.json

--explore: the same boards and counts against opponents that are not predictable.  Snakes 1 and 2 actually play safe_greedy
with eps 0.25 (explore_actions_device); snake 0 searches once with deterministic playouts -- today's model of them -- and
once with playouts in which snakes 1 and 2 explore as they do (explore = (0, 0.25, 0.25), under a salt of its own).
    python tools/playout_search.py --explore --out profiles/playout_explore_search.json"""
import argparse
import sys

import cost_harness as ch


OPPONENTS = (0.0, 0.25, 0.25)  # --explore: what snakes 1 and 2 actually play, and what the exploring search assumes of them


def run(dim, envs, steps, K, reps, search, seed, opponents=None, model=None):
    """opponents: the exploration probabilities the three snakes actually play with (None: plain safe_greedy); model: what the
    playouts of the search assume (None: deterministic playouts)."""
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(envs, dim=dim, n_snakes=3, rules="snake_env", seed=seed)
    scratch = env.clone(num_envs=envs * 4 * reps, auto_reset=False) if search else None
    acts = torch.zeros((envs, 3), dtype=torch.int32, device=env.device)
    rows = torch.arange(envs, device=env.device)
    env.reset_device()
    for _ in range(steps):
        if opponents is None:
            env.scripted_actions_device("safe_greedy", out=acts)
        else:
            env.explore_actions_device("safe_greedy", opponents, salt=1, out=acts)
        if search:
            value, _ = env.playout_values_device(scratch, K, snake=0, reps=reps, explore=model, salt=2)
            best = value.max(dim=1)
            own = acts[:, 0].long()
            keeps = (own > 0) & (value[rows, (own - 1).clamp(min=0)] >= best.values)
            acts[:, 0] = torch.where(keeps, own, best.indices + 1).to(torch.int32)
        env.step_device(acts)
    torch.cuda.synchronize()
    st = env.stats()
    assert st["errors"] == 0
    env.close()
    n = max(1, st["episodes"])
    return {"ended_episodes": st["episodes"], "mean_length": round(st["ep_len_sum"] / n, 2), "mean_return": round(st["ep_return_sum"] / n, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--dims", type=int, nargs="+", default=[10, 19])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    ap.add_argument("--explore", action="store_true", help="the search against exploring opponents (see the module docstring)")
    args = ap.parse_args()
    import torch
    if args.explore:
        res = {"device": torch.cuda.get_device_name(0), "envs": args.envs, "steps": args.steps, "playout_steps": args.k, "reps": args.reps,
               "players": "snakes 1, 2: safe_greedy with eps 0.25 (explore_actions_device); snake 0: argmax of playout_values_device, ties "
                          "to safe_greedy's move, with deterministic playouts / with explore = (0, 0.25, 0.25) inside the playouts",
               "figures": "episodes of snake 0 that ended within the steps played (msnake_get_stats)", "boards": {}}
        for dim in args.dims:
            res["boards"][f"{dim}x{dim}x3"] = {
                "deterministic_playouts": run(dim, args.envs, args.steps, args.k, args.reps, True, args.seed, OPPONENTS, None),
                "exploring_playouts": run(dim, args.envs, args.steps, args.k, args.reps, True, args.seed, OPPONENTS, OPPONENTS)}
            print(f"{dim}x{dim}: done", file=sys.stderr, flush=True)
        return ch.write_json(res, args.out)
    res = {"device": torch.cuda.get_device_name(0), "envs": args.envs, "steps": args.steps, "playout_steps": args.k, "reps": args.reps,
           "players": "snake 0: argmax of playout_values_device, ties to safe_greedy's move / plain safe_greedy; snakes 1, 2: safe_greedy",
           "figures": "episodes of snake 0 that ended within the steps played (msnake_get_stats)", "boards": {}}
    for dim in args.dims:
        res["boards"][f"{dim}x{dim}x3"] = {"playout_search": run(dim, args.envs, args.steps, args.k, args.reps, True, args.seed),
                                           "safe_greedy": run(dim, args.envs, args.steps, args.k, args.reps, False, args.seed)}
        print(f"{dim}x{dim}: done", file=sys.stderr, flush=True)
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
