#!/usr/bin/env python3
"""Cost of msnake_playout next to the loop it replaces, in the same process and from the same start states.  19x19x3
snake_env at 4 096 and 32 768 envs, 500 steps into safe_greedy play (the setup of tools/fates_cost.py).

For K in 1, 8, 64 steps, every leg captured into one HIP graph (a linear chain of `groups` repetitions) and replayed
between HIP events after a warm-up, the legs alternating over the rounds:
  playout:    one msnake_playout of K steps, every snake on safe_greedy / on wary_greedy, without and with the end words;
  yardstick:  K x [msnake_scripted_actions(safe_greedy, every snake) -> msnake_step with obs = NULL] on a twin handle with
              auto_reset = 0.  Every group starts from the start states again: msnake_copy_envs(twin <- env) heads each
              group inside the graph, and the cost of that copy, measured as a leg of its own, is taken off;
  step:       the same loop with the step alone (constant action 1), shown next to it as the sibling tools do.
Reported in us per call (one playout / one K-step loop) and per playout step.  At K = 64 the playout's time per step has to
be below the yardstick's at both batch sizes and for both policies: "below_yardstick_at_K64"; the tool exits 1 if not.
    python tools/playout_cost.py --out profiles/playout_cost.json

--explore measures what exploring playouts (msnake_playout_explore) cost, into a file of its own:
  (a) with --ab-libs OLD NEW ("default" = the in-tree libmsnake.so): msnake_playout, every snake on safe_greedy, on two
      builds of the library, one fresh process per build and round, alternating on the same box (the way tools/ab_libs.sh
      runs two libraries); both medians and the spread of the processes' medians are recorded, and whether NEW is slower
      than OLD beyond that spread;
  (b) in this process: msnake_playout next to msnake_playout_explore with eps 0.25 and 1.0 for all snakes, safe_greedy and
      wary_greedy.
The older build: check the parent commit out next to the tree and build it as a variant, which leaves
<parent tree>/self-play-on-multi-snakes-environment_amd/libmsnake_parent.so:
    git worktree add ../parent HEAD~1 && make -C ../parent/self-play-on-multi-snakes-environment_amd/csrc variant NAME=parent
    python tools/playout_cost.py --explore --ab-libs <parent tree>/self-play-on-multi-snakes-environment_amd/libmsnake_parent.so default \
        --out profiles/playout_explore_cost.json"""
import argparse
import json
import os
import subprocess
import sys

import cost_harness as ch


def capture(fn, groups):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as graph capture wants
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(groups):
            fn()
    return g


def explore_legs(env, K, out, policies=("safe_greedy", "wary_greedy"), eps=(0.25, 1.0)):
    legs = {}
    for pol in policies:
        legs[f"playout {pol}"] = lambda pol=pol: env.playout_device(K, pol, out=out)
        for x in eps:
            legs[f"playout {pol}, explore {x}"] = lambda pol=pol, x=x: env.playout_device(K, pol, out=out, explore=x, salt=1)
    return legs


def measure(args, legs_of):
    """legs_of(env, K, out) -> {name: fn}; us per call and per step of every leg, the legs alternating over the rounds."""
    import msnake
    res = {}
    for n in args.envs:
        env, _ = ch.played_env(n, args.play_steps)
        blob = env.get_state_all()
        small = msnake.Playout(*env.playout_device(1)[:4], None, None)
        out = {}
        for K in args.ks:
            groups = max(2, args.launches // (2 * K))
            legs = legs_of(env, K, small)
            graphs = {name: capture(fn, groups) for name, fn in legs.items()}
            times = {name: [] for name in legs}
            for _ in range(args.rounds):
                for name, g in graphs.items():
                    times[name].append(ch.timed(g.replay, groups))
            ch.assert_unchanged(env, blob)
            out[f"K={K}"] = {name: {"per_call_us": ch.med(v), "per_step_us": ch.med([x / K for x in v])} for name, v in times.items()}
            print(f"{n} envs, K={K}: done", file=sys.stderr, flush=True)
        res[str(n)] = out
        env.close()
    return res


def explore_main(args):
    import torch
    if args.ab_child:                                    # one process of leg (a): msnake_playout, all safe_greedy, on MSNAKE_LIB
        import msnake
        msnake._capi.load(optional=("msnake_explore_actions", "msnake_playout_explore"))  # the older build lacks them; the leg calls neither
        print(json.dumps(measure(args, lambda env, K, out: {"playout safe_greedy": lambda: env.playout_device(K, "safe_greedy", out=out)})))
        return
    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "rounds": args.rounds,
           "start_states": f"{args.play_steps} steps into safe_greedy play",
           "unit": "us: median (min, max) over the rounds; per_call = one playout, per_step = per_call / K"}
    if args.ab_libs:
        old, new = args.ab_libs
        runs = {old: [], new: []}
        base = [sys.executable, os.path.abspath(__file__), "--explore", "--ab-child", "--rounds", str(args.rounds), "--play-steps", str(args.play_steps),
                "--launches", str(args.launches), "--envs", *map(str, args.envs), "--ks", *map(str, args.ks)]
        for i in range(args.ab_rounds):
            for lib in (old, new):
                env = dict(os.environ, MSNAKE_LIB="" if lib == "default" else os.path.abspath(lib))
                r = subprocess.run(base, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit(f"A/B process on {lib} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                runs[lib].append(json.loads(r.stdout.strip().split("\n")[-1]))
                print(f"A/B round {i}, {lib}: done", file=sys.stderr, flush=True)
        ab = {}
        for n in map(str, args.envs):
            for K in args.ks:
                per = {lib: [run[n][f"K={K}"]["playout safe_greedy"]["per_step_us"][0] for run in runs[lib]] for lib in (old, new)}
                spread = max(max(v) - min(v) for v in per.values())
                m = {lib: sorted(v)[len(v) // 2] for lib, v in per.items()}
                ab[f"{n} envs, K={K}"] = {"old_per_step_us": ch.med(per[old]), "new_per_step_us": ch.med(per[new]), "spread_us": round(spread, 3),
                                          "new_slower_beyond_spread": bool(m[new] - m[old] > spread)}
        res["a_msnake_playout_old_vs_new"] = {"old": old, "new": new, "processes_per_library": args.ab_rounds,
                                              "figures": "median (min, max) over the processes of each process's median us per playout step; "
                                                         "spread = the larger max - min of the two libraries", "legs": ab}
    res["b_explore_vs_none"] = measure(args, explore_legs)
    ch.write_json(res, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--explore", action="store_true", help="the cost of exploring playouts (see the module docstring)")
    ap.add_argument("--ab-libs", nargs=2, default=None, metavar=("OLD", "NEW"), help="--explore: two builds of libmsnake.so to compare")
    ap.add_argument("--ab-rounds", type=int, default=3, help="--explore: processes per library")
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launches", type=int, default=256, help="kernel launches per yardstick graph, about")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--play-steps", type=int, default=500)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    if args.explore:
        return explore_main(args)
    import torch
    import msnake

    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "rounds": args.rounds,
           "start_states": f"{args.play_steps} steps into safe_greedy play",
           "unit": "us: median (min, max) over the rounds; per_call = one playout or one K-step loop, per_step = per_call / K",
           "yardstick": "K x [scripted_actions(safe_greedy) -> step(obs = NULL)] on an auto_reset = 0 twin, restarted from the start "
                        "states for every group (the copy's own cost taken off)",
           "batches": {}}
    ok = True
    for n in args.envs:
        env, acts = ch.played_env(n, args.play_steps)
        blob = env.get_state_all()
        twin = env.clone(auto_reset=False)
        ones = torch.ones((n, 3), dtype=torch.int32, device=env.device)
        stream = lambda: torch.cuda.current_stream(env.device).cuda_stream  # noqa: E731
        step = lambda a: msnake._capi.check(twin._L.msnake_step(twin._h, a.data_ptr(), 3, None, twin._p_rew, twin._p_done,  # noqa: E731
                                                                 twin._p_info, stream()), "msnake_step")
        small = msnake.Playout(*env.playout_device(1)[:4], None, None)
        full = env.playout_device(1, end_state=True)
        out = {}
        for K in args.ks:
            groups = max(2, args.launches // (2 * K))

            def loop(policy, K=K):
                twin.copy_envs_device(env)
                for _ in range(K):
                    step(twin.scripted_actions_device(policy, out=acts) if policy else ones)

            legs = {
                "playout safe_greedy": lambda K=K: env.playout_device(K, "safe_greedy", out=small),
                "playout safe_greedy + end words": lambda K=K: env.playout_device(K, "safe_greedy", out=full),
                "playout wary_greedy": lambda K=K: env.playout_device(K, "wary_greedy", out=small),
                "playout wary_greedy + end words": lambda K=K: env.playout_device(K, "wary_greedy", out=full),
                "yardstick safe_greedy->step": lambda: loop("safe_greedy"),
                "step alone": lambda: loop(None),
                "copy_envs": lambda: twin.copy_envs_device(env),
            }
            graphs = {name: capture(fn, groups) for name, fn in legs.items()}
            times = {name: [] for name in legs}
            for _ in range(args.rounds):
                for name, g in graphs.items():
                    times[name].append(ch.timed(g.replay, groups))
            ch.assert_unchanged(env, blob)
            copy = sorted(times["copy_envs"])[len(times["copy_envs"]) // 2]
            rows = {}
            for name, v in times.items():
                if name in ("yardstick safe_greedy->step", "step alone"):
                    v = [x - copy for x in v]
                rows[name] = {"per_call_us": ch.med(v), "per_step_us": ch.med([x / K for x in v])} if name != "copy_envs" else {"per_call_us": ch.med(v)}
            yard = rows["yardstick safe_greedy->step"]["per_step_us"][0]
            rows["yardstick_over_playout"] = {name: round(yard / rows[name]["per_step_us"][0], 2) for name in legs if name.startswith("playout")}
            if K == 64:
                below = all(rows[name]["per_step_us"][0] < yard for name in legs if name.startswith("playout"))
                rows["below_yardstick_at_K64"] = below
                ok = ok and below
            out[f"K={K}"] = dict(rows, groups_per_graph=groups)
            print(f"{n} envs, K={K}: done", file=sys.stderr, flush=True)
        res["batches"][str(n)] = out
        env.close(), twin.close()
    ch.write_json(res, args.out)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
