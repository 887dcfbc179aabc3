#!/usr/bin/env python3
"""Self-play PPO on the HIP env (BASELINE.json configs[4]: 4096 envs, 2 snakes, 19x19).
    python tools/train_selfplay.py --envs 4096 --snakes 2 --timesteps 2000000 --csv ppo.csv"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")  # no exhaustive convolution search on first use


def main():
    import msnake  # (no GPU is touched before an env is made)
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--snakes", type=int, default=2)
    ap.add_argument("--dim", type=int, default=19)
    ap.add_argument("--rules", default="snake_env")
    ap.add_argument("--nsteps", type=int, default=64)
    ap.add_argument("--timesteps", type=int, default=int(2e6))
    ap.add_argument("--scale", type=int, default=1, help="4 = 84x84 frames (nature_cnn) at dim 19")
    ap.add_argument("--bf16", action="store_true", help="policy trunk under bf16 autocast (reference: fp32)")
    ap.add_argument("--csv", default=None)
    ap.add_argument("--monitor", default=None)
    ap.add_argument("--json", default=None, help="progress.json (baselines JSON log format)")
    ap.add_argument("--tensorboard", default=None, help="directory for a TensorBoard events file")
    ap.add_argument("--save", default=None, metavar="DIR", help="checkpoint directory (the reference's saved_models/<expr>/)")
    ap.add_argument("--save-interval", type=int, default=0, help="also save snake_model_num<N>_<k>.pt every this many updates")
    ap.add_argument("--load", default=None, metavar="FILE", help="initialise learner and opponents from a weights file")
    ap.add_argument("--resume", action="store_true", help="continue from <--save DIR>/trainer_state.pt")
    ap.add_argument("--opponent", choices=("pool",) + msnake._capi.SCRIPTED_OPPONENT_NAMES + (msnake._capi.TIMED_POLICY,) + (msnake._capi.WARY_POLICY,), default="pool",
                    help="who plays the other snakes: past selves from the pool, or a fixed on-device scripted policy")
    ap.add_argument("--local-radius", type=int, default=None, metavar="R",
                    help="train window policies on each snake's head-centred (2R+1)x(2R+1) cell-code window instead of the frame")
    ap.add_argument("--no-orient", action="store_true",
                    help="with --local-radius / --rays: windows / rays in board orientation and absolute actions (default: turned along the heading)")
    ap.add_argument("--rays", action="store_true",
                    help="train ray policies (an MLP) on each snake's eight-direction rays, 32 bytes per snake, instead of the frame")
    ap.add_argument("--all-snakes", action="store_true",
                    help="with --local-radius / --rays: the learner plays every snake and learns from every snake's transitions "
                         "(per-snake rewards and deaths from the device), instead of from snake 0 against opponents")
    ap.add_argument("--kill-bonus", type=float, default=0.0, metavar="B",
                    help="with --all-snakes (snake_env, adversarial): add B to a snake's reward for every snake that ran into its "
                         "body in the step, and log the deaths of every update by cause")
    ap.add_argument("--random-starts", type=float, default=0.0, metavar="P",
                    help="(snake_env, adversarial) an env whose episode ended starts its next one, with probability P, from a position "
                         "generated on the device instead of from the reset")
    ap.add_argument("--start-lengths", type=int, nargs=2, default=(3, 3), metavar=("LO", "HI"),
                    help="with --random-starts: every snake's body length in a generated position is uniform in [LO, HI]")
    args = ap.parse_args()
    if not 0.0 <= args.random_starts <= 1.0:
        ap.error("--random-starts needs a probability in [0, 1]")
    if not 0 <= args.start_lengths[0] <= args.start_lengths[1]:
        ap.error("--start-lengths needs 0 <= LO <= HI")
    if args.random_starts > 0.0 and args.rules == "new_world":
        ap.error("--random-starts needs snake_env or adversarial rules")
    if args.rays and args.local_radius is not None:
        ap.error("--rays and --local-radius are mutually exclusive")
    if args.no_orient and args.local_radius is None and not args.rays:
        ap.error("--no-orient needs --local-radius or --rays")
    if args.all_snakes and (args.local_radius is None and not args.rays or args.opponent != "pool"):
        ap.error("--all-snakes needs --local-radius or --rays, and no --opponent")
    if args.kill_bonus != 0.0 and not args.all_snakes:
        ap.error("--kill-bonus needs --all-snakes")
    import torch
    from msnake import selfplay

    # (--all-snakes: the step is followed by the per-snake outcomes and a masked reset, so the handle does not reset itself)
    env = msnake.MultiSnakeVecEnv(args.envs, dim=args.dim, n_snakes=args.snakes, rules=args.rules, seed=0,
                                  obs_scale=args.scale, auto_reset=not args.all_snakes)
    selfplay.learn(env, nsteps=args.nsteps, total_timesteps=args.timesteps, csv_path=args.csv,
                   monitor_path=args.monitor, json_path=args.json, tb_dir=args.tensorboard,
                   amp_dtype=torch.bfloat16 if args.bf16 else None, save_dir=args.save, save_interval=args.save_interval,
                   load_path=args.load, resume=args.resume, local_radius=args.local_radius, oriented=not args.no_orient, rays=args.rays,
                   all_snakes=args.all_snakes, kill_bonus=args.kill_bonus, random_starts=args.random_starts,
                   start_lengths=tuple(args.start_lengths), scripted_opponents=None if args.opponent == "pool" else {s: args.opponent for s in range(1, args.snakes)})
    print(env.stats())
    env.close()


if __name__ == "__main__":
    main()
