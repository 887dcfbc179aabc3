"""The top of the documented ranges on the reference: boards up to 62x62, up to 32 new_world fruits, late-game bodies.

The run table of tests/golden/big_boards.npz, shared by tools/gen_golden.py (which plays the runs on the reference) and
by tests/test_oracle_big_boards.py and tests/test_big_boards_gpu.py (which replay them on the CPU oracle and on the
library).  Two kinds of run:

  random  the recipe of random_configs.npz: an eps-greedy walk towards the nearest fruit with invalid action codes mixed
          in, auto reset on or off with a reset by hand every 25 steps, env_id_base up to 2^40.  The dims sit on both
          sides of every board size at which a step kernel changes its number of envs per workgroup (boundaries() below
          restates the arithmetic of csrc/msnake_internal.h shape::lds_per_wave and of msnake_create / launch_k), for
          the 9 channels of snake_env, adversarial and 3-snake new_world handles and the 12 of 4-snake new_world ones.
  late    states installed into the reference (start_states), one body length per env, played by the scripted policies
          of tests/scripted_play.py from the reference's state: bodies along the Hamiltonian cycle with the fruit two
          cells ahead, a 62x62 board that fills, an adversarial snake of thousands of pieces that a scripted turn kills
          (its body becomes the fruit list), new_world bodies past 128 pieces among 25 fruits.

coverage() reads what a run is there for from the recorded arrays alone; check_coverage() holds the floors.  The
generator refuses to write a file that misses one and the host test asserts them again from the file.

A plain helper module like scripted_play; not collected.
"""
import json
import zlib

import numpy as np

import scripted_play as sp
from golden_util import state_view

S, N, A = 0, 1, 2
RESET_EVERY = 25      # auto_reset off: a reset by hand after every 25th step
LDS_BYTES = 64 * 1024
MAX_DIM = 62


# ----------------------------------------------------------------------------------------------- LDS bands
def channels(cfg):
    return 3 * cfg["n_snakes"] if cfg["rules"] == N else 9


def lds_per_wave(dim, C, tape):
    """shape::lds_per_wave at native size: the observation padded to whole KiB (+ 15 bytes of shift), the occupancy bytes
    behind it, and for the persistent tape kernel the pristine background image once more."""
    img = ((dim + 2) ** 2 * C + 15 + 1023) & ~1023
    return img + ((dim * dim + 15) & ~15) + (img if tape else 0)


def envs_per_workgroup(dim, C, tape, start=8):
    """8 envs per workgroup halved until their LDS fits 64 KB; 0 where one env alone does not (the persistent tape
    kernel: msnake_rollout_tape then runs per-step launches)."""
    per, epb = lds_per_wave(dim, C, tape), start
    while epb > 1 and epb * per > LDS_BYTES:
        epb >>= 1
    return 0 if per > LDS_BYTES else epb


def boundaries(C):
    """[(tape, dim, dim + 1)]: the neighbouring board sizes between which a kernel's envs per workgroup change."""
    return [(tape, d, d + 1) for tape in (False, True) for d in range(2, MAX_DIM)
            if envs_per_workgroup(d, C, tape) != envs_per_workgroup(d + 1, C, tape)]


# ----------------------------------------------------------------------------------------------- the run table
RUNS = {}


def _random(rules, dim, ns, nf=None, envs=3, steps=100, seed=1, eps=0.3, auto_reset=True, base=0):
    name = "SNA"[rules] + f"{dim}x{ns}" + (f"f{nf}" if rules == N else "")
    assert name not in RUNS
    RUNS[name] = dict(kind="random", rules=rules, dim=dim, n_snakes=ns, n_fruits=ns if nf is None else nf, num_envs=envs,
                      steps=steps, seed=seed, eps=eps, auto_reset=bool(auto_reset), env_id_base=base, max_steps=2000)


def _late(name, rules, dim, ns, nf, lengths, steps, seed, policy, base=0, **kw):
    RUNS[name] = dict(kind="late", rules=rules, dim=dim, n_snakes=ns, n_fruits=nf, num_envs=len(lengths), steps=steps,
                      seed=seed, eps=0.0, auto_reset=True, env_id_base=base, max_steps=2000, policy=policy,
                      lengths=[list(x) if isinstance(x, (tuple, list)) else x for x in lengths], **kw)


# 9 channels.  Per-step kernel: 8 envs per workgroup up to 26x26, 4 up to 37, 2 up to 55, 1 above; persistent tape
# kernel: 8 up to 16, 4 up to 26, 2 up to 39, 1 up to 56, none from 57 (asserted in tests/test_oracle_big_boards.py).
_random(S, 16, 3, seed=11, eps=0.3, base=(1 << 40) - 3)
_random(A, 17, 2, seed=12, eps=0.3, auto_reset=False, base=77)
_random(N, 24, 3, 10, seed=13, eps=0.3, auto_reset=False, base=1 << 33)
_random(S, 26, 1, seed=114, eps=0.3, auto_reset=False)
_random(A, 27, 3, seed=15, eps=0.3, base=4096)
_random(S, 31, 1, seed=16, eps=0.3, base=(1 << 32) - 1)
_random(S, 33, 2, seed=117, eps=0.3, auto_reset=False, base=9)
_random(S, 37, 3, seed=218, eps=0.3, base=1 << 39)
_random(A, 38, 1, seed=1019, eps=0.3, auto_reset=False, base=5)
_random(N, 39, 3, 16, seed=20, eps=0.3, base=123456789)
_random(S, 40, 2, seed=21, eps=0.3, base=31)
_random(A, 47, 3, seed=22, eps=0.3, auto_reset=False, base=1 << 20)
_random(A, 55, 2, seed=23, eps=0.3, base=3)
_random(S, 56, 3, seed=224, eps=0.3, auto_reset=False, base=(1 << 40) - 1)
_random(A, 57, 3, seed=125, eps=0.3, base=17)
_random(S, 62, 3, envs=3, steps=120, seed=126, eps=0.3, base=1 << 36)
_random(A, 62, 3, envs=3, steps=120, seed=427, eps=0.3, auto_reset=False, base=2)
# 12 channels (new_world, 4 snakes).  Per-step: 8 up to 22, 4 up to 32, 2 up to 47, 1 above; tape: 8 up to 13, 4 up to
# 22, 2 up to 33, 1 up to 48, none from 49.
_random(N, 13, 4, 10, seed=31, eps=0.3, auto_reset=False, base=8)
_random(N, 14, 4, 16, seed=32, eps=0.3, base=(1 << 40) - 2)
_random(N, 22, 4, 31, seed=33, eps=0.3, auto_reset=False, base=1 << 31)
_random(N, 23, 4, 0, seed=34, eps=0.5, base=6)
_random(N, 32, 4, 17, seed=35, eps=0.3, auto_reset=False, base=1000)
_random(N, 33, 4, 10, seed=36, eps=0.3, base=1 << 38)
_random(N, 34, 4, 16, seed=37, eps=0.3, auto_reset=False, base=4)
_random(N, 47, 4, 31, seed=38, eps=0.2, auto_reset=False, base=99)
_random(N, 48, 4, 32, seed=39, eps=0.2, base=1 << 35)
_random(N, 49, 4, 17, seed=40, eps=0.2, auto_reset=False, base=12)
_random(N, 62, 4, 32, envs=3, steps=150, seed=41, eps=0.1, auto_reset=False, base=1 << 37)
# 1 and 2 new_world snakes (3 and 6 channels), on the required dims: 32 | 33 is where both kernels change with 6
# channels, 61 | 62 where the per-step kernel does with 3
_random(N, 32, 2, 0, seed=51, eps=0.5, base=21)
_random(N, 33, 2, 31, seed=52, eps=0.3, auto_reset=False, base=1 << 34)
_random(N, 61, 1, 0, seed=54, eps=0.5, auto_reset=False, base=1 << 30)
_random(N, 62, 1, 17, seed=55, eps=0.2, auto_reset=False, base=7)

# late game: `lengths` holds one entry per env (adversarial: (snake, pieces) of the long snake; new_world: the lengths of
# snakes 1 and 2, snake 0 being dead from the start so that the episode runs on)
_late("L_S34", S, 34, 1, 1, (63, 127, 191, 1000), 100, 61, "hamiltonian", base=40)
_late("L_S62", S, 62, 1, 1, (2000, 3500, 3838, 3842), 100, 62, "hamiltonian", base=1 << 40)
_late("L_A62x3", A, 62, 3, 3, ((1, 2000), (2, 3000), (1, 1200)), 120, 63, "crash_then_safe_greedy", base=50, crash_at=3,
      fruit_floor=1000)
_late("L_A62x2", A, 62, 2, 2, ((1, 3400), (1, 1001)), 100, 64, "crash_then_safe_greedy", base=60, crash_at=5, fruit_floor=1000)
_late("L_N40", N, 40, 3, 25, ((129, 140), (200, 260), (300, 400)), 120, 65, "safe_greedy", base=70)


def step_bands():
    """One random run per per-step band of the 9-channel kernels (8, 4, 2 and 1 envs per workgroup): the runs of the
    launch-tuning test."""
    return {envs_per_workgroup(RUNS[n]["dim"], 9, False): n for n in ("S62x3", "A47x3", "S37x3", "S16x3")}


# ----------------------------------------------------------------------------------------------- late-game starts
def cycle(dim):
    """The cells of scripted_play.hamiltonian_table(dim) in walking order, from (0, 0)."""
    act, out, c = sp.hamiltonian_table(dim), [], (0, 0)
    for _ in range(dim * dim):
        out.append(c)
        d = sp.DIRS[act[c[0]][c[1]]]
        c = (c[0] + d[0], c[1] + d[1])
    assert c == (0, 0) and len(set(out)) == dim * dim
    return out


def _along(cyc, head, length):
    """A body of `length` pieces with its head on cycle cell `head` and the rest behind it, and its velocity."""
    n = len(cyc)
    cells = [list(cyc[(head - i) % n]) for i in range(length)]
    nxt = cyc[(head + 1) % n]
    return cells, [nxt[0] - cells[0][0], nxt[1] - cells[0][1]]


def start_states(cfg):
    """The canonical state dict installed into env e of a late-game run (the words of tools/gen_golden.py canon_state)."""
    dim, rules, ns = cfg["dim"], cfg["rules"], cfg["n_snakes"]
    cyc = cycle(dim)
    n2, out = dim * dim, []
    for e, spec in enumerate(cfg["lengths"]):
        ctr = 12 + e
        if rules == S:      # one body along the cycle, the fruit two cells ahead of the head
            head = (3 * dim + 7 * e + spec) % n2
            body, vel = _along(cyc, head, spec)
            st = dict(snakes=[body], fruits=[list(cyc[(head + 2) % n2])], vels=[vel], grow_to=[spec], t=0, ctr=ctr)
        elif rules == A:    # the long snake along the cycle, the others three pieces each well ahead of it
            long_s, pieces = spec
            head = pieces + 10 * e
            snakes, vels, ahead = [], [], 200
            for s in range(ns):
                body, vel = _along(cyc, head, pieces) if s == long_s else _along(cyc, head + ahead, 3)
                ahead += 0 if s == long_s else 200
                snakes.append(body)
                vels.append(vel)
            fruits = [list(cyc[(head + 250 + 50 * s) % n2]) for s in range(ns)]
            st = dict(snakes=snakes, fruits=fruits, vels=vels, grow_to=[len(b) for b in snakes], t=0, ctr=ctr, spare_fruits=0)
        else:               # snake 0 dead and gone; snakes 1 and 2 along the cycle, 25 fruits on free cycle cells
            l1, l2 = spec
            b1, v1 = _along(cyc, 500, l1)
            b2, v2 = _along(cyc, 1100, l2)
            assert ns == 3 and l1 <= 300 and l2 <= 400 and n2 == 1600
            fruits = [list(cyc[(1105 + 20 * i) % n2]) for i in range(cfg["n_fruits"])]
            st = dict(snakes=[[], b1, b2], fruits=fruits, vels=[[0, 0], v1, v2], grow_to=[3, l1, l2], t=0, ctr=ctr,
                      alive=[False, True, True], in_dead=[True, False, False])
        cells = [tuple(c) for b in st["snakes"] for c in b]
        assert len(cells) == len(set(cells)) and not set(cells) & {tuple(f) for f in st["fruits"]}, (cfg, e)
        out.append(st)
    return out


def crash_action(st, s, dim):
    """An action that ends snake s at once: a turn (no reversal, which the rules ignore) into a wall or a body."""
    body = st["snakes"][s]
    used = {(c[0], c[1]) for b in st["snakes"] for c in b}
    v = tuple(st["vels"][s])
    for a in (4, 3, 1, 2):
        d = sp.DIRS[a]
        if (d[0], d[1]) == (-v[0], -v[1]):
            continue
        x, y = body[0][0] + d[0], body[0][1] + d[1]
        if not (0 <= x < dim and 0 <= y < dim) or (x, y) in used:
            return a
    raise AssertionError("no crashing turn")


def late_actions(cfg, states, t):
    """The action rows of step t of a late-game run from the canonical states (no random numbers: eps is 0)."""
    dim, ns = cfg["dim"], cfg["n_snakes"]
    rows = []
    for e, st in enumerate(states):
        if cfg["policy"] == "hamiltonian":
            rows.append(sp.hamiltonian(st, dim, ns))
            continue
        a = sp.safe_greedy(st, dim, ns, None, 0.0)
        if cfg["policy"] == "crash_then_safe_greedy":
            s = cfg["lengths"][e][0]
            if len(st["snakes"]) > s and len(st["snakes"][s]) > 100:     # the long snake, while it lives
                a[s] = sp.hamiltonian(st, dim, ns)[s] if t < cfg["crash_at"] else crash_action(st, s, dim)
        rows.append(a)
    return np.array(rows, np.int32)


# ----------------------------------------------------------------------------------------------- tags, cuts, coverage
def state_tag(states, rules):
    """32 bits of the states alone (no observation, no history): what a path that delivers the state only at the end of a
    call is compared with."""
    return np.uint32(zlib.crc32(json.dumps([state_view(st, rules) for st in states], sort_keys=True, separators=(",", ":")).encode()))


def hand_resets(cfg):
    """The steps after which an auto_reset-off run is reset by hand."""
    return [] if cfg["auto_reset"] else [t for t in range(cfg["steps"]) if t % RESET_EVERY == RESET_EVERY - 1]


def segments(cfg):
    """[(first step, one past the last)]: the stretches of a run between its resets by hand (one tape call each)."""
    cuts = [0] + [t + 1 for t in hand_resets(cfg)]
    if cuts[-1] != cfg["steps"]:
        cuts.append(cfg["steps"])
    return list(zip(cuts[:-1], cuts[1:]))


def coverage(cfg, reward, done, body_max, n_fruits):
    """What a run is there for, from its recorded [T, E] arrays (the reference's numbers)."""
    reward, done = np.asarray(reward), np.asarray(done) != 0
    body_max, n_fruits = np.asarray(body_max, np.int64), np.asarray(n_fruits, np.int64)
    cov = dict(eaten=int(reward[reward > 0].sum()), episodes=int(done.sum()),
               grow_steps=int((body_max[1:] > body_max[:-1]).sum()), longest_body=[int(x) for x in body_max.max(axis=0)],
               longest_fruit_list=int(n_fruits.max()))
    if cfg.get("fruit_floor"):  # per env: the longest body after the step on which the list first passed the floor, less the one on it
        grown = []
        for e in range(body_max.shape[1]):
            over = np.nonzero(n_fruits[:, e] > cfg["fruit_floor"])[0]
            ends = np.nonzero(done[:, e])[0]
            if not len(over):
                grown.append(-1)
                continue
            t1 = int(over[0]) + 1   # (the step after: on t1 - 1 the long snake itself may still be the longest body)
            t2 = int(ends[ends >= t1][0]) if (ends >= t1).any() else body_max.shape[0]
            seg = body_max[t1:t2, e]
            grown.append(int(seg.max() - seg[0]) if len(seg) else 0)
        cov["grown_on_the_list"] = grown
    return cov


def check_coverage(cfg, cov):
    if cfg["kind"] == "random":
        if cfg["rules"] != N:
            assert cov["eaten"] >= 3 and cov["episodes"] >= 1, cov
        elif cfg["n_fruits"] > 0:
            assert cov["grow_steps"] >= 3, cov
        return
    if cfg["rules"] == A:       # the list passes the floor in every env and is eaten from afterwards
        assert cov["longest_fruit_list"] > cfg["fruit_floor"] and min(cov["grown_on_the_list"]) >= 2, cov
        return
    installed = [max(x) if isinstance(x, list) else x for x in cfg["lengths"]]
    assert all(got >= want + 2 for got, want in zip(cov["longest_body"], installed)), (cov, installed)


def check_table_coverage(covs):
    """The conditions on the file as a whole.  covs: name -> coverage()."""
    assert {c["rules"] for c in RUNS.values() if c["kind"] == "random"} == {S, N, A}
    for C in (9, 12):           # both sides of every boundary, per-step and tape kernel
        dims = {c["dim"] for c in RUNS.values() if c["kind"] == "random" and channels(c) == C}
        for tape, lo, hi in boundaries(C):
            assert lo in dims and hi in dims, (C, tape, lo, hi)
    assert {24, 31, 32, 33, 61, 62} <= {c["dim"] for c in RUNS.values() if c["kind"] == "random"}
    nw = [c for c in RUNS.values() if c["kind"] == "random" and c["rules"] == N]
    assert {c["n_fruits"] for c in nw} == {0, 10, 16, 17, 31, 32} and {c["n_snakes"] for c in nw} == {1, 2, 3, 4}
    assert {c["auto_reset"] for c in RUNS.values()} == {True, False}
    assert max(c["env_id_base"] for c in RUNS.values()) == 1 << 40
    assert all(2 <= c["num_envs"] <= 4 and 100 <= c["steps"] <= 150 for c in RUNS.values())
    # 64, 128 and 192 pieces are each crossed by some env; one 62x62 env fills its board
    for mark in (64, 128, 192):
        assert any(a < mark <= b for n in ("L_S34",) for a, b in zip(RUNS[n]["lengths"], covs[n]["longest_body"])), mark
    assert max(covs["L_S62"]["longest_body"]) == 62 * 62
