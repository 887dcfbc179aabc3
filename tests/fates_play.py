"""The one-step fate of every move, stated on canonical state dicts (Oracle.get_state): include/msnake.h,
msnake_fate_actions, restated without the library.

snake_env and adversarial move every snake and then judge every snake against the same post-move bodies.  Whether a
piece stays depends only on len, grow_to and the fruit list, so what happens to snake s under action a follows from the
state, but for two things that are named instead: what the others play (HEAD_ON) and whether another snake's last piece
goes (TAIL).  np_fates gives the four outputs of the call for one env, wary_greedy the opponent that plays by the two
masks.  check_guarantees steps copies of a state on the CPU oracle under every joint action of the others and holds the
header's four guarantees against what comes out.  new_world judges its snakes one after the other and is refused.
Nothing here asks the library under test.

A plain helper module in the style of causes_play and timed_play, which it imports and does not edit; imported by
tests/test_fates_host.py and tests/test_fates_gpu.py.  `python tests/fates_play.py` prints the share of deaths by cause
with every snake under wary_greedy next to safe_greedy, from the CPU oracle (the row of the README).
"""
import itertools

import numpy as np

import causes_play as cp
import scripted_play as sp
import timed_play as tp

DIRS = sp.DIRS
WALL, SELF, BODY, HEAD_ON, TAIL, EATS = 1, 2, 4, 8, 16, 32   # MSNAKE_FATE_*
CERTAIN, RISK = WALL | SELF | BODY, HEAD_ON | TAIL
BITS = dict(WALL=WALL, SELF=SELF, BODY=BODY, HEAD_ON=HEAD_ON, TAIL=TAIL, EATS=EATS)
NEW_WORLD = sp.RULES["new_world"]
BIG = 2 ** 31 - 1


def _refuse_new_world(rules):
    if rules is not None and (sp.RULES[rules] if isinstance(rules, str) else int(rules)) == NEW_WORLD:
        raise ValueError("new_world judges its snakes one after the other and clears bodies as it goes: the fate of a move "
                         "does not follow from the state")


def direction(v, a):
    """d(k, a): what turn() leaves of velocity v under action a."""
    v = (int(v[0]), int(v[1]))
    if a == 0:
        return v
    d = DIRS[a]
    return v if (d[0] == -v[0] and d[1] == -v[1] and v != (0, 0)) else d


def target(st, s, a):
    h = st["snakes"][s][0]
    d = direction(st["vels"][s], a)
    return (h[0] + d[0], h[1] + d[1]), d != (0, 0)


def np_fates(st, dim, n_snakes, rules=None):
    """One env.  Returns (fate uint8 [S, 5], by uint8 [S, 5], eat uint8 [S, 5], mask uint8 [S, 2])."""
    _refuse_new_world(rules)
    S = n_snakes
    fate, by, eat = np.zeros((S, 5), np.uint8), np.zeros((S, 5), np.uint8), np.zeros((S, 5), np.uint8)
    mask = np.zeros((S, 2), np.uint8)
    bodies = [[tuple(c) for c in (st["snakes"][s] if s < len(st["snakes"]) else [])] for s in range(S)]
    fruits = [tuple(f) for f in st["fruits"]]
    live = [s for s in range(S) if bodies[s]]
    for s in live:
        mine, grow = bodies[s], int(st["grow_to"][s])
        for a in range(5):
            T, moving = target(st, s, a)
            n_f = fruits.count(T)
            f = b = 0
            if not (0 <= T[0] < dim and 0 <= T[1] < dim):
                f |= WALL
            if moving:
                pop = len(mine) >= grow + 2 * n_f
                after = [T] + mine[:len(mine) - pop]
            else:
                after = mine
            if T in after[1:]:
                f |= SELF
            for k in live:
                if k == s:
                    continue
                other, grows = bodies[k], len(bodies[k]) < int(st["grow_to"][k])
                if T in other[:-1] or (grows and T == other[-1]):
                    f |= BODY
                if not grows and T == other[-1]:
                    f |= TAIL
                    b |= 16 << k
                for c in range(5):
                    Tk, k_moves = target(st, k, c)
                    if k_moves and Tk == T:
                        f |= HEAD_ON
                        b |= 1 << k
            if moving and n_f:
                f |= EATS
                eat[s, a] = min(255, n_f)
            fate[s, a], by[s, a] = f, b
            if not f & CERTAIN:
                mask[s, 0] |= 1 << a
            if not f & (CERTAIN | RISK):
                mask[s, 1] |= 1 << a
    return fate, by, eat, mask


def wary_choice(st, n_snakes, mask):
    """wary_greedy's action of every snake from the two masks [S, 2]."""
    fruits = st["fruits"]
    out = []
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        cand = [a for a in (1, 2, 3, 4) if mask[s, 1] >> a & 1] or [a for a in (1, 2, 3, 4) if mask[s, 0] >> a & 1]
        if not body or not cand:
            out.append(0)
            continue
        best, best_d = 0, None
        for a in cand:
            (x, y), _ = target(st, s, a)
            d = min((abs(f[0] - x) + abs(f[1] - y) for f in fruits), default=0)
            if best_d is None or d < best_d:
                best, best_d = a, d
        out.append(best)
    return out


def wary_greedy(st, dim, n_snakes, rs=None, eps=0.0):
    """Among the moves 1..4 that are survived whatever the others do -- if there is none, among those that can be
    survived -- the first whose target is closest (L1) to a fruit; 0 when there is none or the body is empty.  With
    probability eps a random action 0..4 instead (the POLICIES signature; the draws are safe_greedy's)."""
    choice = wary_choice(st, n_snakes, np_fates(st, dim, n_snakes)[3])
    if eps:
        for s in range(n_snakes):
            if rs.random() < eps:
                choice[s] = int(rs.integers(0, 5))
    return choice


POLICIES = dict(tp.POLICIES, wary_greedy=wary_greedy)


def choose_actions(cfg, states, rs):
    """timed_play.choose_actions with wary_greedy among the policies."""
    if cfg["policy"] != "wary_greedy":
        return tp.choose_actions(cfg, states, rs)
    return np.array([wary_greedy(st, cfg["dim"], cfg["n_snakes"], r, cfg["eps"]) for st, r in zip(states, rs)], np.int32)


def expected(cfg, states):
    """(actions int32 [E, S], fate, by, eat uint8 [E, S, 5], mask uint8 [E, S, 2]) for a batch of states."""
    S, dim = cfg["n_snakes"], cfg["dim"]
    outs = [np_fates(st, dim, S) for st in states]
    act = np.array([wary_choice(st, S, o[3]) for st, o in zip(states, outs)], np.int32).reshape(len(states), S)
    return (act,) + tuple(np.stack([o[k] for o in outs]) for k in range(4))


# ------------------------------------------------------------------------------------------ the guarantees on the oracle
def check_guarantees(cfg, states, seen=None, chunk=100):
    """For every state, snake and action: one oracle step of a copy of the state under every joint action of the others,
    and the header's guarantees 1-4 against the outcome.  `seen` collects, per bit name, how often it was set and clear.
    Returns the number of (state, snake, action, joint action) steps taken."""
    from oracle.snake_oracle import state_to_flat
    S, dim = cfg["n_snakes"], cfg["dim"]
    if len(states) > chunk:
        return sum(check_guarantees(cfg, states[i:i + chunk], seen, chunk) for i in range(0, len(states), chunk))
    E = len(states)
    joint = list(itertools.product(range(5), repeat=S - 1))
    # env (j, a, e): joint action j of the others, action a of the snake looked at, state e
    N = len(joint) * 5 * E
    ora = sp.make_oracle(dict(cfg, num_envs=N), auto_reset=False)
    ora.reset()
    flats = [state_to_flat(st, S) for st in states]
    buf = np.zeros(max(len(f) for f in flats) + 64, np.int32)

    def body_len(n, s):
        """len of snake s of env n, from the oracle's canonical words"""
        ora.L.orc_export_state(ora.h, n, buf.ctypes.data, len(buf))
        k = 8 + 2 * int(buf[6])
        for _ in range(s):
            k += 6 + 2 * int(buf[k])
        return int(buf[k])

    fates = [np_fates(st, dim, S) for st in states]
    steps = 0
    for s in range(S):
        act = np.zeros((len(joint), 5, E, S), np.int32)
        for j, others in enumerate(joint):
            for col, k in enumerate(k for k in range(S) if k != s):
                act[j, :, :, k] = others[col]
        act[:, :, :, s] = np.arange(5, dtype=np.int32)[None, :, None]
        for n in range(len(joint) * 5):
            for e, flat in enumerate(flats):
                assert ora.L.orc_import_state(ora.h, n * E + e, flat.ctypes.data, len(flat)) == 0
        _, rew, *_ = ora.step(act.reshape(-1, S), want_obs=False)
        rew = np.asarray(rew).reshape(len(joint), 5, E)
        alive = np.array([body_len(n, s) > 0 for n in range(N)]).reshape(len(joint), 5, E)
        for e, st in enumerate(states):
            fate, by, eat, _ = fates[e]
            if not st["snakes"][s]:
                assert not fate[s].any() and not alive[:, :, e].any(), (e, s)
                continue
            for a in range(5):
                f, where = int(fate[s, a]), (e, s, a, st)
                steps += len(joint)
                if seen is not None:
                    for name, bit in BITS.items():
                        seen.setdefault(name, [0, 0])[0 if f & bit else 1] += 1
                if f & CERTAIN:
                    assert not alive[:, a, e].any(), ("1: certain, yet alive", f, where)
                if not f & (CERTAIN | RISK):
                    assert alive[:, a, e].all(), ("2: no bit, yet dead", f, where)
                if f & HEAD_ON and not f & CERTAIN:
                    for k in range(S):
                        if k != s and by[s, a] >> k & 1:
                            col = k - (k > s)   # k's place among the others
                            assert any(not any(alive[j, a, e] for j, o in enumerate(joint) if o[col] == b) for b in range(5)), \
                                ("3: head-on, yet no action of k kills", f, k, where)
                if s == 0:
                    for j in range(len(joint)):
                        if alive[j, a, e]:
                            assert rew[j, a, e] == float(np_fruits_at(st, 0, a)), ("4: reward", f, where)
    return steps


def np_fruits_at(st, s, a):
    """fruits(T(s, a)) for a moving snake, 0 for a standing one."""
    T, moving = target(st, s, a)
    return [tuple(f) for f in st["fruits"]].count(T) if moving else 0


# ------------------------------------------------------------------------------------------ the hand-built states
def state(snakes, vels, fruits, grow_to=None):
    """A canonical state: grow_to = max(3, len) unless given."""
    n = len(snakes)
    grow = [max(3, len(b)) for b in snakes] if grow_to is None else list(grow_to)
    return {"t": 3, "ctr": 40, "spare_fruits": 0, "ep_len": 3, "ep_return": 0.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [list(v) for v in vels], "grow_to": grow,
            "alive": [True] * n, "in_dead": [False] * n}


HAND_DIM = 6
_F = [(0, 0), (0, 1), (0, 5)]            # three fruits out of everybody's way
_SQUARE = [(2, 2), (2, 3), (3, 3), (3, 2)]   # the head next to its own tail: move 1 from (2, 2) enters (3, 2)
_FAR1, _FAR2 = [(5, 5), (5, 4), (5, 3)], [(0, 3), (0, 4)]
# name -> (state, {(snake, action): (bits that must be set, bits that must be clear)}); 6x6, three snakes
HAND = {
    # the own tail pops: no SELF; growing: SELF
    "own_tail_pops": (state([_SQUARE, _FAR1, _FAR2], [(0, -1), (0, -1), (0, -1)], _F, grow_to=[4, 3, 3]),
                      {(0, 1): (0, SELF | WALL | BODY)}),
    "own_tail_stays": (state([_SQUARE, _FAR1, _FAR2], [(0, -1), (0, -1), (0, -1)], _F, grow_to=[5, 3, 3]),
                       {(0, 1): (SELF, WALL | BODY)}),
    # a fruit under the snake's own tail: it eats, so the tail stays
    "fruit_under_own_tail": (state([_SQUARE, _FAR1, _FAR2], [(0, -1), (0, -1), (0, -1)], [(3, 2), (0, 1), (0, 5)], grow_to=[4, 3, 3]),
                             {(0, 1): (SELF | EATS, WALL | BODY)}),
    # another snake's tail, popping (TAIL) and growing (BODY)
    "other_tail_pops": (state([[(2, 2), (1, 2), (0, 2)], [(3, 4), (3, 3), (3, 2)], _FAR2], [(1, 0), (0, 1), (0, -1)], _F),
                        {(0, 1): (TAIL, CERTAIN | HEAD_ON), (0, 0): (TAIL, CERTAIN | HEAD_ON)}),
    "other_tail_stays": (state([[(2, 2), (1, 2), (0, 2)], [(3, 4), (3, 3), (3, 2)], _FAR2], [(1, 0), (0, 1), (0, -1)], _F, grow_to=[3, 4, 3]),
                         {(0, 1): (BODY, TAIL | HEAD_ON)}),
    # two heads two cells apart, straight and diagonal
    "heads_straight": (state([[(1, 2), (0, 2)], [(3, 2), (4, 2)], _FAR1], [(1, 0), (-1, 0), (0, -1)], _F),
                       {(0, 1): (HEAD_ON, CERTAIN | TAIL), (1, 3): (HEAD_ON, CERTAIN | TAIL), (0, 2): (0, HEAD_ON | CERTAIN)}),
    "heads_diagonal": (state([[(1, 2), (0, 2)], [(2, 3), (2, 4)], _FAR1], [(1, 0), (0, -1), (0, -1)], _F),
                       {(0, 1): (HEAD_ON, CERTAIN), (0, 2): (HEAD_ON, CERTAIN), (1, 4): (HEAD_ON, CERTAIN), (1, 3): (HEAD_ON, CERTAIN)}),
    # a standing snake after a reset, next to a moving one: four cells in its head-on set, its own action 0 stands
    "standing": (state([[(2, 2), (1, 2), (0, 2)], [(3, 3)], [(5, 5)]], [(1, 0), (0, 0), (0, 0)], _F),
                 {(0, 1): (HEAD_ON, CERTAIN), (0, 2): (HEAD_ON, CERTAIN), (1, 0): (0, CERTAIN | HEAD_ON | EATS),
                  (1, 3): (HEAD_ON, CERTAIN), (1, 4): (HEAD_ON, CERTAIN)}),
    # heads at -1 and at dim
    "head_outside": (state([[(-1, 2)], [(6, 3)], [(2, 6)]], [(-1, 0), (1, 0), (0, 1)], _F),
                     {(0, 0): (WALL, 0), (0, 1): (WALL, 0), (0, 2): (WALL, 0), (1, 3): (WALL, 0), (2, 4): (WALL, 0), (2, 1): (WALL, 0)}),
    # a duplicated piece stacked on a tail: the tail goes, the duplicate stays
    "stacked_on_tail": (state([[(2, 2), (1, 2), (0, 2)], [(3, 4), (3, 3), (3, 2), (4, 2), (3, 2)], _FAR2], [(1, 0), (0, 1), (0, -1)], _F),
                        {(0, 1): (BODY | TAIL, WALL | SELF)}),
    # grow_to = 2^31 - 1: no overflow in the pop test, the tail stays
    "grow_to_max": (state([_SQUARE, [(3, 5), (3, 4), (4, 4)], _FAR2], [(0, -1), (0, 1), (0, -1)], _F, grow_to=[BIG, BIG, 3]),
                    {(0, 1): (SELF, WALL | BODY), (0, 3): (0, CERTAIN)}),
    # a dead snake among live ones: all zero, and nobody minds its cells
    "dead_among_live": (state([[(2, 2), (1, 2), (0, 2)], [], [(3, 3), (3, 4)]], [(1, 0), (0, 1), (0, -1)], _F),
                        {(1, 1): (0, 63), (1, 0): (0, 63), (0, 1): (HEAD_ON, CERTAIN)}),
}
# adversarial only: the list holds the same cell twice (eat = 2), len 3 < 3 + 4 so the tail stays
HAND_ADVERSARIAL = {
    "fruit_twice": (state([[(2, 2), (1, 2), (0, 2)], _FAR1, _FAR2], [(1, 0), (0, -1), (0, -1)], [(3, 2), (0, 1), (3, 2), (0, 5)]),
                    {(0, 1): (EATS, CERTAIN), (0, 0): (EATS, CERTAIN)}),
}


def hand_states(rules):
    """(names, states, expected bits) of the hand-built table for a rule set: adversarial adds the doubled list entry."""
    table = dict(HAND)
    if (sp.RULES[rules] if isinstance(rules, str) else int(rules)) == sp.RULES["adversarial"]:
        table.update(HAND_ADVERSARIAL)
    return list(table), [table[n][0] for n in table], [table[n][1] for n in table]


def hand_cfg(rules, num_envs=1):
    return sp.scenario(rules, HAND_DIM, 3, "wary_greedy", 1, num_envs, 1)


def long_body_state(grows, dim=10, length=70):
    """10x10, three snakes: snake 0 is a boustrophedon of `length` pieces (past the 64-slot ring) over the columns
    1..dim-2; its tail (0, 1) is the target of move 2 of snake 1, which stands at (0, 0).  `grows`: snake 0 is still
    growing, so its tail stays (BODY), else it goes if snake 0 does not eat (TAIL).  Snake 2 stands aside."""
    cells = []
    for x in range(dim):
        col = [(x, y) for y in range(1, dim - 1)]
        cells += col if x % 2 == 0 else col[::-1]
    body = cells[:length][::-1]                     # the head is the last cell laid, the tail is (0, 1)
    assert body[-1] == (0, 1) and len(body) == length
    v = (body[0][0] - body[1][0], body[0][1] - body[1][1])
    return state([body, [(0, 0)], [(dim - 1, dim - 1)]], [v, (0, 0), (0, 0)], [(dim - 1, 0), (5, 0), (5, dim - 1)],
                 grow_to=[length + bool(grows), 3, 3])


# ------------------------------------------------------------------------------------------ the behaviour table
def shares(dim, policy, num_envs=16, steps=1000, seed=1):
    """Deaths by cause when all three snakes play `policy` (eps 0) on a dim x dim snake_env board: the event counts."""
    cfg = sp.scenario("snake_env", dim, 3, policy, steps, num_envs, seed, eps=0.0, max_steps=2000)
    tw, total = Twin(cfg), {}
    for _ in range(steps):
        tw.step()
        cp.add_events(total, tw.events())
    return total


class Twin(cp.Twin):
    """causes_play.Twin that also plays wary_greedy."""

    def actions(self):
        return choose_actions(self.cfg, self.states, self.rs)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the oracle package
    print("| board | policy | deaths | wall | self | head-on | body |")
    print("|---|---|---|---|---|---|---|")
    for dim in (10, 19):
        for policy in ("safe_greedy", "wary_greedy"):
            ev = shares(dim, policy)
            pct = lambda k: f"{100.0 * ev[k] / max(1, ev['deaths']):.0f} %"
            print(f"| {dim}x{dim}x3 | {policy} | {ev['deaths']} | {pct('wall')} | {pct('self')} | {pct('head_on')} | {pct('body')} |")
