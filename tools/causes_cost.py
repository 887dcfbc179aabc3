#!/usr/bin/env python3
"""Cost of msnake_death_causes next to msnake_copy_envs, msnake_agent_outcomes and msnake_step, and of the five-call chain
of step_agents_device(causes=True) next to the three-call chain without causes.  19x19x3 snake_env at 4 096 and 32 768
envs, some hundred steps into safe_greedy play on a handle without auto reset (every step followed by a masked reset of
the done envs); `before` is a snapshot of that handle, `after` the handle one more step on.

One figure per leg, from HIP events after a warm-up, legs alternating in one process on the same handles:
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence,
            free of the host's submission cost.
Legs: "causes_all" (cause, by, victims and where: 5 bytes per snake written, both envs read through the reader),
"causes_cause_only" (1 byte per snake), "copy_envs" (the snapshot the chain pays for, into a third handle: also one wave
per env, also a whole env through the reader, and it writes the env as well -- the yardstick), "outcomes_all"
(msnake_agent_outcomes with its four outputs), "msnake_step" (on a copy of the handle with auto reset, under the constant
action 1), "chain_3" (step_agents_device: step, outcomes, reset_envs(done)) and "chain_5" (the same with causes=True:
copy_envs in front, death_causes behind the outcomes), each chain on a copy of its own under the constant action 1.
The cause legs only read the two handles, so every round sees the same boards.  Descriptive: nothing gates on it.
    python tools/causes_cost.py            # writes profiles/causes_cost.json"""
import argparse
import os

import cost_harness as ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ch.ROOT, "profiles", "causes_cost.json"))
    args = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "calls_per_leg": args.calls,
           "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "graph_us: median (min, max) over the rounds, us per call",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "batches": {}}
    S = 3
    for n in args.envs:
        env, acts = ch.played_env(n, args.play_steps, masked_reset=True, n_snakes=S, auto_reset=False)
        before, scratch = env.clone(), env.clone()
        stepper, c3, c5 = env.clone(auto_reset=True), env.clone(), env.clone()
        env.step_device(env.scripted_actions_device("safe_greedy", out=acts))   # `env` is one step past `before` now
        ones = torch.ones((n, S), dtype=torch.int32, device=env.device)
        zero_done = torch.zeros(n, dtype=torch.uint8, device=env.device)
        cause, by, victims = (torch.empty((n, S), dtype=torch.uint8, device=env.device) for _ in range(3))
        where = torch.empty((n, S, 2), dtype=torch.int8, device=env.device)
        env.arm_agents_device()
        legs = {
            "causes_all": (lambda: env.death_causes_device(before, cause, by, victims, where), S * 5),
            "causes_cause_only": (lambda: env.death_causes_device(before, cause_out=cause), S),
            "copy_envs": (lambda: scratch.copy_envs_device(env), 256 + S * 128),
            "outcomes_all": (lambda: env.agent_outcomes_device(zero_done), S * (4 + 1 + 1 + 16)),
            "msnake_step": (lambda: stepper.step_device(ones), int(stepper.obs_shape[0] * stepper.obs_shape[1] * stepper.obs_shape[2])),
            "chain_3": (lambda: c3.step_agents_device(ones), None),
            "chain_5": (lambda: c5.step_agents_device(ones, causes=True), None),
        }
        blobs = [h.get_state_all().tobytes() for h in (env, before)]
        times = ch.graph_legs({k: fn for k, (fn, _) in legs.items()}, args.calls, args.rounds)
        for h, blob in zip((env, before), blobs):
            ch.assert_unchanged(h, blob)   # every leg on `env` and `before` only read the state
        # the step between the two handles: a snake has a cause exactly where the outcomes say it died
        env.arm_agents_device()   # (from `env`: the flags of a quiet step give who is alive after)
        alive_after = (env.agent_outcomes_device(zero_done).flags & 1) != 0
        before.arm_agents_device()
        alive_before = (before.agent_outcomes_device(zero_done).flags & 1) != 0
        env.death_causes_device(before, cause, by, victims, where)
        assert torch.equal(cause != 0, alive_before & ~alive_after)
        res["batches"][str(n)] = {k: dict({"graph_us": ch.med(t["graph_us"])}, **({} if legs[k][1] is None else {"bytes_per_env": legs[k][1]}))
                                  for k, t in times.items()}
        res["batches"][str(n)]["deaths_in_the_measured_step"] = int((cause != 0).sum())
        for h in (env, before, scratch, stepper, c3, c5):
            h.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
