#!/usr/bin/env python3
"""Play a policy against the on-device scripted opponents and report its episode returns (the reference's
evaluate_snake.py without the GUI).  Snake 0 is the policy, every other snake plays --opponent; all on the device.
    python tools/eval_vs_scripted.py --weights saved/snake_model_num2.pt --snakes 2 --opponent safe_greedy --episodes 2000
Every env plays the same number of episodes, ceil(--episodes / --envs), and all of them count: taking the first N
episodes to finish anywhere in the batch would favour short ones.
Prints one JSON line: mean / std of episode return and length, and the number of episodes."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")


def main():
    import msnake  # (no GPU is touched before an env is made)
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default=None, help="weights file written by selfplay.save_weights")
    ap.add_argument("--random", action="store_true", help="a freshly initialised policy instead of --weights")
    ap.add_argument("--opponent", choices=msnake._capi.SCRIPTED_OPPONENT_NAMES + (msnake._capi.TIMED_POLICY,) + (msnake._capi.WARY_POLICY,), default="safe_greedy")
    ap.add_argument("--eps", type=float, default=0.0, help="share of opponent actions replaced by a random one")
    ap.add_argument("--episodes", type=int, default=1000)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--snakes", type=int, default=2)
    ap.add_argument("--dim", type=int, default=19)
    ap.add_argument("--rules", default="snake_env")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-steps", type=int, default=1000000, help="give up after this many steps of the batch (each is --envs env steps)")
    args = ap.parse_args()
    if (args.weights is None) == (not args.random):
        ap.error("give exactly one of --weights FILE and --random")
    import torch
    from msnake import selfplay

    torch.manual_seed(args.seed)
    env = msnake.MultiSnakeVecEnv(args.envs, dim=args.dim, n_snakes=args.snakes, rules=args.rules, seed=args.seed,
                                  obs_scale=args.scale)
    H, W, _ = env.obs_shape
    model = selfplay.CnnPolicy((H, W, 3)).to(env.device)
    if args.weights:
        selfplay.load_weights(model, args.weights)
    gen = torch.Generator(device=env.device).manual_seed(args.seed)
    team = selfplay.ScriptedColumns(env)
    opps = [selfplay.ScriptedOpponent(env, args.opponent, s, eps=args.eps, generator=gen, columns=team) for s in range(1, args.snakes)]
    per_env = -(-args.episodes // args.envs)                 # every env contributes its first per_env episodes
    played = torch.zeros(args.envs, dtype=torch.int32, device=env.device)
    obs = env.reset_device()
    rets, lens, steps, finished = [], [], 0, False
    while not finished and steps < args.max_steps:
        team.refresh()
        acts = [model.step(obs[..., 0:3])[0]] + [o.step()[0] for o in opps]
        obs, rew, done, info = env.step_device(torch.stack(acts, dim=1).to(torch.int32))
        take = done.bool() & (played < per_env)
        rets.append(info[:, 0].view(torch.float32)[take]); lens.append(info[:, 1][take])
        played += done.to(torch.int32)
        steps += 1
        if steps % 16 == 0:  # one host sync every 16 steps
            finished = bool((played >= per_env).all())
    r, l = torch.cat(rets).float().cpu(), torch.cat(lens).float().cpu()
    k = int(r.numel())
    print(json.dumps({"opponent": args.opponent, "eps": args.eps, "episodes": k, "episodes_per_env": per_env,
                      "complete": finished, "env_steps": steps * args.envs,
                      "return_mean": float(r.mean()) if k else None, "return_std": float(r.std(unbiased=False)) if k else None,
                      "length_mean": float(l.mean()) if k else None, "length_std": float(l.std(unbiased=False)) if k else None}))
    env.close()


if __name__ == "__main__":
    main()
