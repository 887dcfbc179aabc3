#!/usr/bin/env python3
"""Generate tests/golden/death_causes.npz by RUNNING THE REFERENCE: the bodies its snakes were judged with.

The reference's step moves every snake, asks is_snake_alive for every snake and then clears the dead ones
(snake_multiple_test.py:166-197, snake_adversarial_env.py likewise).  Each env's bound is_snake_alive is wrapped here
so that the call for index 0 records state[0], the post-move bodies before any removal; the file holds, per step, the
actions, the canonical states before and after (after: before any reset), those recorded bodies and which snakes the
reference cleared.  Data only: loader, Philox shim, make_ref_env, canon_state and policy_actions are tools/gen_golden.py's,
which is imported and not edited.  Runs only where the reference exists.

Runs: snake_env and adversarial 6x6x3 and one snake_env 10x10x3, 4 envs each, eps-greedy walks at eps 0.15.  The seeds
were chosen on the CPU so that each rule set has at least 100 deaths, 10 of every cause class and 3 deaths on the body of
a snake that died in the same step (asserted below with tests/causes_play.py, the restatement the fixture pins).

Usage: python tools/gen_causes_golden.py   (rewrites tests/golden/death_causes.npz, byte-identical every time)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))

import gen_golden as gg  # noqa: E402

import causes_play as cp  # noqa: E402

EPS, NUM_ENVS = 0.15, 4
# name -> (rules, dim, steps, seed)
RUNS = {
    "S6": (gg.RULES_SNAKE_ENV, 6, 150, 11),
    "A6": (gg.RULES_ADVERSARIAL, 6, 300, 12),
    "S10": (gg.RULES_SNAKE_ENV, 10, 100, 13),
}
FLOORS = dict(deaths=100, wall=10, self=10, head_on=10, body=10, dead_owner=3)
PAD = -9   # fill of the cell arrays behind a body's last piece


def record_post_bodies(env):
    """Wrap the env's bound is_snake_alive: the call for index 0 keeps a copy of state[0] in env._post."""
    orig = env.is_snake_alive

    def wrapped(idx):
        if idx == 0:
            env._post = [[tuple(map(int, c)) for c in s] for s in env.state[0]]
        return orig(idx)

    env.is_snake_alive = wrapped


def play(rules, dim, steps, seed, n_snakes=3):
    """[T][E] of (actions, state before, state after, post-move bodies)."""
    envs = [gg.make_ref_env(rules, dim, n_snakes, n_snakes, seed, e) for e in range(NUM_ENVS)]
    rs = np.random.default_rng([seed, dim, rules])
    for env in envs:
        record_post_bodies(env)
        gg.quiet(env.reset)
    tape = []
    for _ in range(steps):
        row = []
        for env in envs:
            before = gg.canon_state(env)
            act = gg.policy_actions(env, n_snakes, rs, EPS)
            _, _, done, _ = gg.quiet(env.step, act)
            row.append((act, before, gg.canon_state(env), env._post))
            if done:
                gg.quiet(env.reset)
        tape.append(row)
    return tape


def pack(name, meta, tape, out):
    T, E, S = len(tape), NUM_ENVS, 3
    L = max(len(b) for row in tape for _, st0, st1, post in row for b in st0["snakes"] + st1["snakes"] + post)
    out[f"{name}_meta"] = np.array(meta, np.int32)
    act = np.zeros((T, E, S), np.int8)
    arr = {k: (np.zeros((T, E, S), np.int16), np.full((T, E, S, L, 2), PAD, np.int8)) for k in ("before", "after", "post")}
    vel = {k: np.zeros((T, E, S, 2), np.int8) for k in ("before", "after")}
    grow = {k: np.zeros((T, E, S), np.int16) for k in ("before", "after")}
    cleared = np.zeros((T, E, S), np.uint8)
    for t, row in enumerate(tape):
        for e, (a, st0, st1, post) in enumerate(row):
            act[t, e] = a
            for k, bodies in (("before", st0["snakes"]), ("after", st1["snakes"]), ("post", post)):
                for s, b in enumerate(bodies):
                    arr[k][0][t, e, s] = len(b)
                    if b:
                        arr[k][1][t, e, s, :len(b)] = b
            for k, st in (("before", st0), ("after", st1)):
                vel[k][t, e], grow[k][t, e] = st["vels"], st["grow_to"]
            cleared[t, e] = [len(b0) > 0 and len(b1) == 0 for b0, b1 in zip(st0["snakes"], st1["snakes"])]
    out[f"{name}_actions"] = act
    for k in arr:
        out[f"{name}_{k}_len"], out[f"{name}_{k}_cells"] = arr[k]
    for k in vel:
        out[f"{name}_{k}_vel"], out[f"{name}_{k}_grow"] = vel[k], grow[k]
    out[f"{name}_cleared"] = cleared


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    out, per_rules = {}, {}
    for name, (rules, dim, steps, seed) in RUNS.items():
        tape = play(rules, dim, steps, seed)
        ev = per_rules.setdefault(rules, {})
        for row in tape:
            for _, st0, st1, post in row:
                assert [b for b in cp.post_bodies(st0, st1) if b is not None] == [b for b in post if b], (name, st0, st1, post)
                cp.add_events(ev, cp.events(st0, st1, dim))
        pack(name, (rules, dim, 3, NUM_ENVS, steps, seed), tape, out)
        print(name, {k: v for k, v in cp.add_events({}, ev).items()})
    for rules, ev in per_rules.items():
        assert all(ev[k] >= v for k, v in FLOORS.items()), (gg.RULE_NAMES[rules], ev)
    path = os.path.join(gg.OUT, "death_causes.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 100_000


if __name__ == "__main__":
    main()
