#!/usr/bin/env python3
"""Cost of building random positions on the device (msnake_generate_states) next to msnake_import_states, which installs
them, and to msnake_reset, the only other way to a fresh position.  19x19x3 snake_env at 4 096 and 32 768 envs, requests
of 3, 40 and 150 pieces per snake, compact, all legs in one process.

One figure per leg, from HIP events after a warm-up, legs alternating (tools/cost_harness.py):
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence.
Legs: "generate_<L>" (words at the full stride, state_words_max, counts and reached lengths; the handle is only read),
"generate_import_<L>" (the same followed by the import of every env into a second handle: what scatter_device() issues),
and the yardsticks on that second handle: "import" (every env, from rows exported some hundred steps into safe_greedy
play) and "reset" (msnake_reset with its observations).  `reached` is the share of snakes that got the requested length.
The comparison is descriptive: nothing gates on it.
    python tools/generate_cost.py            # writes profiles/generate_cost.json"""
import argparse
import os

import cost_harness as ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--lengths", type=int, nargs="+", default=[3, 40, 150])
    ap.add_argument("--play-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ch.ROOT, "profiles", "generate_cost.json"))
    args = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes, compact", "calls_per_leg": args.calls,
           "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "median (min, max) over the rounds; graph_us: us per call",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "batches": {}}
    for n in args.envs:
        src, _ = ch.played_env(n, args.play_steps)
        dst = src.clone()
        stride = src.state_words_max
        played_words, played_count = src.export_states_device()
        words = torch.zeros((n, stride), dtype=torch.int32, device=src.device)
        count = torch.zeros(n, dtype=torch.int32, device=src.device)
        got = torch.zeros((n, 3), dtype=torch.int32, device=src.device)
        status = torch.zeros(n, dtype=torch.uint8, device=src.device)
        blob = src.get_state_all()
        req = {L: torch.full((n, 3), L, dtype=torch.int32, device=src.device) for L in args.lengths}
        legs, reached = {}, {}
        for L in args.lengths:
            # what the legs compute installs cleanly: checked before anything is timed
            src.generate_states_device(req[L], salt=L, out=words, count_out=count, got_out=got)
            dst.import_states_device(words, count=count, status_out=status)
            torch.cuda.synchronize()
            assert int(status.max()) == 0 and int(got.min()) >= 1 and int(got.max()) <= L
            reached[L] = round(float((got == L).float().mean()), 4)

            def generate(L=L):
                src.generate_states_device(req[L], salt=L, out=words, count_out=count, got_out=got)

            def generate_import(L=L):
                generate(L)
                dst.import_states_device(words, count=count, status_out=status)

            legs[f"generate_{L}"], legs[f"generate_import_{L}"] = generate, generate_import
        legs["import"] = lambda: dst.import_states_device(played_words, count=played_count, status_out=status)
        legs["reset"] = lambda: dst.reset_device()
        times = ch.graph_legs(legs, args.calls, args.rounds)
        assert int(status.max()) == 0
        ch.assert_unchanged(src, blob)                      # generate only read its handle
        out = {k: {kind: ch.med(v) for kind, v in t.items()} for k, t in times.items()}
        out["reached"] = {str(L): r for L, r in reached.items()}
        out["stride_words"] = stride
        res["batches"][str(n)] = out
        src.close(), dst.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
