#!/usr/bin/env python3
"""Cadence of step_device() with terminal_obs False vs True (BASELINE configs[2]: 4 096 envs, 3 snakes, 19x19).

terminal_obs=True follows every msnake_step with msnake_reset_envs(done): a masked render of the finished envs'
terminal observations and a masked reset, i.e. two more launches per step on the same stream.  This leg is not part
of bench.py.  Both handles step the same seeded random action tape; the timed windows alternate between them (A B A B
...) so that drift on a shared box hits both alike.  Each window is K back-to-back step_device() calls between two HIP
events, after a warm-up of W steps.  Prints one JSON line: median / min / max us per step of each, over R windows.
usage: terminal_obs_cost.py [--envs 4096] [--steps 512] [--warmup 64] [--repeats 7]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import msnake  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("terminal_obs_cost.py needs a GPU")
    n, ns, K = a.envs, 3, a.steps
    envs = {flag: msnake.MultiSnakeVecEnv(n, dim=19, n_snakes=ns, rules="snake_env", seed=0, device="cuda:0",
                                          terminal_obs=flag) for flag in (False, True)}
    tape = torch.randint(0, 5, (K, n, ns), dtype=torch.int32, device="cuda:0",
                         generator=torch.Generator(device="cuda:0").manual_seed(0))
    for env in envs.values():
        env.reset_device()
        for t in range(a.warmup):
            env.step_device(tape[t % K])
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for _ in range(a.repeats):
        for flag, env in envs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(K):
                env.step_device(tape[t])
            e1.record()
            torch.cuda.synchronize()
            times[flag].append(e0.elapsed_time(e1) * 1e3 / K)
    assert torch.equal(envs[False]._obs, envs[True]._obs), "the two handles diverged"
    res = {"envs": n, "dim": 19, "n_snakes": ns, "steps_per_window": K, "windows": a.repeats,
           "device": torch.cuda.get_device_name(0)}
    for flag, key in ((False, "plain"), (True, "terminal_obs")):
        v = times[flag]
        res[key + "_us_per_step"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    res["added_us_per_step_median"] = round(statistics.median(times[True]) - statistics.median(times[False]), 3)
    print(json.dumps(res))
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
