#!/usr/bin/env python3
"""Cost of the device-side state export, import and hashes (msnake_export_states, msnake_import_states,
msnake_hash_states) next to msnake_copy_envs, which moves the same state, and to the blocking host round trip.  19x19x3
snake_env at 4 096 and 32 768 envs, the handle some hundred steps into safe_greedy play (bodies of a dozen cells), all
legs in one process.

Two figures per leg, both from HIP events after a warm-up, legs alternating (tools/cost_harness.py):
  graph_us: CALLS back-to-back calls captured into one HIP graph (a linear chain) and replayed: the kernel's cadence;
  call_us:  CALLS back-to-back calls through the Python wrapper: mostly the host's submission rate.
Legs: "export" (words at the full stride, state_words_max, and counts), "export_counts" (counts only), "import" (every
env, from the exported rows with their counts, into a clone), "hash_full", "hash_board", "copy_envs" (the identity, into
the same clone) and "msnake_step" for scale.  The host path, dst.set_state_all(src.get_state_all()), blocks, so it is
timed with the host clock around the pair: host_ms per round trip.
The comparison is descriptive: nothing gates on it.
    python tools/state_cost.py            # writes profiles/state_cost.json"""
import argparse
import os
import time

import cost_harness as ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--play-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ch.ROOT, "profiles", "state_cost.json"))
    args = ap.parse_args()
    import torch
    import msnake

    res = {"device": torch.cuda.get_device_name(0), "config": "snake_env 19x19, 3 snakes", "calls_per_leg": args.calls,
           "rounds": args.rounds, "play_steps": args.play_steps,
           "unit": "median (min, max) over the rounds; graph_us / call_us: us per call, host_ms: ms per round trip",
           "graph_us": "calls captured into one HIP graph and replayed (kernel cadence), HIP events",
           "call_us": "calls through the Python wrapper (includes the host's submission cost), HIP events",
           "host_ms": "dst.set_state_all(src.get_state_all()): host clock around the blocking pair",
           "batches": {}}
    for n in args.envs:
        src, _ = ch.played_env(n, args.play_steps)
        dst = src.clone()
        stride = src.state_words_max
        words, count = src.export_states_device()
        full, board = src.hash_states_device("full"), src.hash_states_device("board")
        status = torch.zeros(n, dtype=torch.uint8, device=src.device)
        ones = torch.ones((n, 3), dtype=torch.int32, device=src.device)
        blob = src.get_state_all()
        state_words = (len(blob) - 40 - 8 * (n + 1)) // 4
        # what the legs compute is what the blocking path says: spot checks before anything is timed
        torch.cuda.synchronize()
        row0 = src.get_state_words(0)
        assert int(count.sum()) == state_words and words[0, :len(row0)].cpu().tolist() == row0.tolist()
        assert int(full[0]) & (2**64 - 1) == msnake.state_hash(row0) and int(board[0]) & (2**64 - 1) == msnake.state_hash(row0, "board")
        legs = {
            "export": lambda: src.export_states_device(out=words, count_out=count),
            "export_counts": lambda: src.export_states_device(words=False, count_out=count),
            "import": lambda: dst.import_states_device(words, count=count, status_out=status),
            "hash_full": lambda: src.hash_states_device("full", out=full),
            "hash_board": lambda: src.hash_states_device("board", out=board),
            "copy_envs": lambda: dst.copy_envs_device(src),
            "msnake_step": lambda: src.step_device(ones),
        }
        # the step leg moves the source: every leg starts from the same state
        times = ch.graph_legs(legs, args.calls, args.rounds, restore=lambda: src.set_state_all(blob), eager=True)
        assert int(status.max()) == 0
        host = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.set_state_all(src.get_state_all())
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1000.0)
        ch.assert_unchanged(dst, blob)
        ch.assert_unchanged(src, blob)
        out = {k: {kind: ch.med(v) for kind, v in t.items()} for k, t in times.items()}
        out["host_round_trip"] = {"host_ms": ch.med(host), "state_words": state_words, "stride_words": stride}
        res["batches"][str(n)] = out
        src.close(), dst.close()
    ch.write_json(res, args.out)


if __name__ == "__main__":
    main()
