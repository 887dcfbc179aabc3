"""The top of the documented ranges: max_steps 60000, body rings of 60032 cells, bodies past 32767 pieces.

The scenario builders of tests/test_limits_host.py (which proves on the oracle alone that each does what it is there
for) and tests/test_limits_gpu.py, written from include/msnake.h.  Nothing here asks the library under test.

Every field of this range is 16 bits wide somewhere in the kernels and only safe while read as unsigned; the scenarios
put lengths, ring capacities, ring positions and step counts on both sides of 2^15:

- long bodies (cases "a" and "b"): new_world 12x12, 2 snakes, 1 fruit.  Snake 0 is dead with an empty body (the rule
  set ends the episode at every step at which snake 0 is alive); snake 1 has its head on a cell of the Hamiltonian cycle,
  its next ten pieces on the ten cycle cells behind it, and every further piece folded to and fro over those same ten
  cells.  Driven along the cycle the head has dim^2 - 11 = 133 free cells in front of it: pieces of a new_world body
  leave only at the tail, so the trail never clears and the head meets it on step 134.
- the capacity guard, the copy between capacities, the step cap and the longest body play can reach: see the functions.

A plain helper module like state_domain and scripted_play; not collected.
"""
import numpy as np

import scripted_play as sp
import state_domain as sd

DIM, NS, N2 = 12, 2, 144
SEED = 1                         # of every oracle here and of the handles compared with them (gpu_harness.install's)
FOLD = 10                        # the cycle cells behind the head that hold the whole body
CLEAR = N2 - FOLD - 1            # steps along the cycle before the head meets its trail
PLAY, BEYOND = 130, 10           # steps compared on a clear board, and steps through the self-hit after them
LONG = {
    # cap 60032: lengths around 2^15, one in the middle, the longest accepted, and one whose grow_to lies 6000 above the
    # length: it grows by one per step (to 59880 + 140 < cap - 1) and its lifetimes sit on the 0xFFFE clamp
    "a": dict(max_steps=60000, lens=(32767, 32768, 32769, 40000, 60030, 59880), grow=(3, 3, 3, 3, 3, 65880)),
    # cap 32832: the ring position comes down from 32831 past 32768 and 32767
    "b": dict(max_steps=32800, lens=(32830, 32829, 32768, 32830), grow=(3, 3, 3, 3)),
}


def cfg_of(max_steps, **kw):
    return dict(dict(rules="new_world", dim=DIM, n_snakes=NS, n_fruits=1, max_steps=max_steps), **kw)


def cycle(dim=DIM):
    """The cells of scripted_play.hamiltonian_table(dim) in walking order, from (0, 0)."""
    act, out, c = sp.hamiltonian_table(dim), [], (0, 0)
    for _ in range(dim * dim):
        out.append(c)
        d = sp.DIRS[act[c[0]][c[1]]]
        c = (c[0] + d[0], c[1] + d[1])
    assert c == (0, 0) and len(set(out)) == dim * dim
    return out


def folded_body(head, length, dim=DIM):
    """[[c0, c1]] * length: the head on cycle cell `head`, pieces 1..10 on the ten cycle cells behind it, the rest to and
    fro over those ten cells; neighbouring pieces are one step apart and none but piece 0 lies on the head's cell."""
    cyc = np.array(cycle(dim))
    period = np.array(list(range(1, FOLD + 1)) + list(range(FOLD - 1, 1, -1)))
    behind = period[np.arange(max(length - 1, 0)) % len(period)]
    idx = np.concatenate([[0], behind])[:length]
    return cyc[(head - idx) % (dim * dim)].tolist()


def head_of(e):
    """Env e's head start: cycle cell 20 + 17 e (the lanes and the ring phases of the envs differ)."""
    return (20 + 17 * e) % N2


def long_snake(head, length, grow, dim=DIM):
    cells = folded_body(head, length, dim)
    v = (cells[0][0] - cells[1][0], cells[0][1] - cells[1][1])
    return (cells, v, grow, 1, 0)


DEAD = ([], (0, 0), 3, 0, 1)


def long_words(head, length, grow, t=0, ctr=40, fruit_ahead=40, n_fruits=1):
    """Canonical words of one long-body env; the fruit lies `fruit_ahead` cells in front of the head on the cycle."""
    cyc = cycle()
    fruits = [list(cyc[(head + fruit_ahead) % N2])] * n_fruits
    return sd.state_words(NS, fruits, [DEAD, long_snake(head, length, grow)], t=t, ctr=ctr)


def long_states(case):
    """The installed words of every env of LONG[case]."""
    c = LONG[case]
    return [long_words(head_of(e), ln, g, ctr=40 + e, fruit_ahead=40 + 5 * e) for e, (ln, g) in enumerate(zip(c["lens"], c["grow"]))]


def snake_header(words, s=1):
    """The six header words of snake s (len, v0, v1, grow_to, alive, in_dead) and the index of its first cell, read in
    place: taking a 60000-piece state apart costs more than the step that made it."""
    w = np.asarray(words)
    k = 8 + 2 * int(w[6])
    for _ in range(s):
        k += 6 + 2 * int(w[k])
    return [int(x) for x in w[k:k + 6]], k + 6


def head_cell(words, s=1):
    """(c0, c1) of snake s's head, or None for an empty body."""
    hdr, k = snake_header(words, s)
    return (int(words[k]), int(words[k + 1])) if hdr[0] > 0 else None


def body_len(words, s=1):
    return snake_header(words, s)[0][0]


def alive_bit(words, s=1):
    return snake_header(words, s)[0][4]


def cycle_actions(ora, n_snakes=NS, dim=DIM):
    """scripted_play.hamiltonian for every env of the oracle, from the heads alone."""
    rows = []
    for e in range(ora.num_envs):
        w = sd.export(ora, e, False)
        heads = [head_cell(w, s) for s in range(n_snakes)]
        rows.append(sp.hamiltonian({"snakes": [[list(h)] if h else [] for h in heads]}, dim, n_snakes))
    return np.array(rows, np.int32)


def ohp_after(cap, k):
    """The ring position k steps after the install of a body over 64 pieces: every step evicts one piece into the ring
    and moves the position down by one (mod cap)."""
    return (cap - k) % cap


def make_oracle(cfg, words, seed=SEED, auto_reset=True):
    """An oracle of len(words) envs fresh from a reset, env e holding words[e]."""
    from oracle.snake_oracle import Oracle
    ora = Oracle(len(words), seed=seed, auto_reset=auto_reset, **cfg)
    ora.reset()
    for e, w in enumerate(words):
        assert sd.imports(ora, e, w) == 0, e
    return ora


def info_of(ora):
    """The msnake_info rows of the step the oracle just took: (ep_return bits, ep_len, num_snakes, done)."""
    return np.stack([ora.ep_return.view(np.int32), ora.ep_len, ora.num_snakes, ora.done.astype(np.int32)], 1).astype(np.int32)


class Record:
    """A play of the oracle alone.  Per step k = 1..steps (index k - 1): acts, obs, rew, done, info; headers[k] for
    k = 0..steps: every snake's six header words per env; words[k]: the canonical words of every env after step k, for
    the k in words_at (0 = as installed).  resets: every step on which an env is done is followed by the masked reset
    of the done envs: then obs holds the frames after it, final[k] / truncated[k] what it reported, and episodes /
    ep_len_sum the totals of the episodes that ended."""

    def __init__(self, cfg, ora, acts_fn, steps, words_at=(), resets=False):
        self.cfg, self.n, self.steps, ns = cfg, ora.num_envs, steps, cfg["n_snakes"]
        words_at = set(words_at)
        snap = lambda: [sd.export(ora, e) for e in range(self.n)]
        hdrs = lambda ws: [[snake_header(w, s)[0] for s in range(ns)] for w in ws]
        self.start = snap()
        self.words = {0: self.start} if 0 in words_at else {}
        self.headers = [hdrs(self.start)]
        self.acts, self.obs, self.rew, self.done, self.info = [], [], [], [], []
        self.final, self.truncated, self.episodes, self.ep_len_sum = {}, {}, 0, 0
        for k in range(1, steps + 1):
            act = acts_fn(ora, k)
            ora.step(act)
            self.acts.append(np.array(act, np.int32))
            self.rew.append(ora.rew.copy())
            self.done.append(ora.done.copy())
            self.info.append(info_of(ora))
            ws = snap()
            self.headers.append(hdrs(ws))
            if k in words_at:
                self.words[k] = ws
            if resets and ora.done.any():
                self.episodes += int(ora.done.sum())
                self.ep_len_sum += int(ora.ep_len[ora.done != 0].sum())
                _, final, trunc = ora.reset_envs(ora.done)
                self.final[k], self.truncated[k] = final.copy(), trunc.copy()
            self.obs.append(ora.obs.copy())
        for name in ("acts", "obs", "rew", "done", "info"):
            setattr(self, name, np.stack(getattr(self, name)))
        self.end = snap()

    def lens(self, k, s=1):
        return [h[s][0] for h in self.headers[k]]


_PLAYS = {}


def _once(key, make):
    if key not in _PLAYS:
        _PLAYS[key] = make()
    return _PLAYS[key]


def check_steps(case):
    """The steps (0 = straight after the install) at which the read-only entry points are compared.  Case a: the first
    step (the ring position is cap - 1), one in the middle, the last clear one.  Case b: the install, the first step, the
    two steps on which the ring position is 2^15 and 2^15 - 1, the last clear one."""
    if case == "a":
        return [1, PLAY // 2 + 6, PLAY]
    cap = sd.cap(cfg_of(LONG[case]["max_steps"]))
    return [0, 1, cap - 32768, cap - 32767, PLAY]


def long_play(case):
    """LONG[case] driven along the cycle for PLAY + BEYOND steps on the oracle, once per process."""
    def make():
        cfg = cfg_of(LONG[case]["max_steps"])
        ora = make_oracle(cfg, long_states(case))
        T = PLAY + BEYOND
        return Record(cfg, ora, lambda o, k: cycle_actions(o), T, words_at=check_steps(case) + [T])
    return _once(("long", case), make)


def long_expectations(case, k):
    """expectations() on the oracle's states k steps into long_play(case), once per process: the models take seconds
    on bodies of this length, and every kernel path is compared with the same states."""
    return _once(("expect", case, k), lambda: expectations(long_play(case).cfg, long_play(case).words[k]))


def too_long_words(declared, cells=None, head=20):
    """One env whose snake 1 declares `declared` pieces and brings `cells` of them (default: all)."""
    st = sd.St(long_words(head, declared if cells is None else cells, 3))
    st.snakes[1]["len"] = declared
    return st.flat()


# ------------------------------------------------------------------------------------------ C. the guard at the largest cap
GUARD_VICTIM, GUARD_STEPS = 2, 6
GROW_MAX = (1 << 31) - 1


def guard_states(max_steps=60000):
    """Four envs at cap 60032; env GUARD_VICTIM holds cap - 2 pieces with grow_to 2^31 - 1: cap - 1 after one step, held
    there by the guard from the second step on.  The others keep their length.  The fruits lie 60 cells ahead: nobody
    eats, so no grow_to moves."""
    cap = sd.cap(cfg_of(max_steps))
    lens = [40000, 32768, cap - 2, 33000]
    return [long_words(head_of(e), ln, GROW_MAX if e == GUARD_VICTIM else 3, ctr=50 + e, fruit_ahead=60) for e, ln in enumerate(lens)]


def guard_play():
    def make():
        cfg = cfg_of(60000)
        return Record(cfg, make_oracle(cfg, guard_states()), lambda o, k: cycle_actions(o), GUARD_STEPS, words_at=range(GUARD_STEPS + 1))
    return _once("guard", make)


# ------------------------------------------------------------------------------------------ D. copies between capacities
COPY_SRC_STEPS, COPY_ON = 40, 20
COPY = dict(src_max_steps=60000, dst_max_steps=32800,
            # source env -> length: dst cap - 1 fits (the guard's own limit), dst cap and the longest do not
            lens=(32831, 32832, 60030, 32767, 100),
            # the way back, after COPY_SRC_STEPS steps of the large handle: its env e receives env back[e] of the small one
            back=(-1, 0, 1, -1, 2))


def copy_states():
    return [long_words(head_of(e), ln, 3, ctr=60 + e, fruit_ahead=70) for e, ln in enumerate(COPY["lens"])]


def copy_back_states():
    """The small handle's envs for the way back: the longest body it accepts, one over 2^15, a short one."""
    cap = sd.cap(cfg_of(COPY["dst_max_steps"]))
    return [long_words(head_of(e + 2), ln, 3, ctr=80 + e, fruit_ahead=50) for e, ln in enumerate((cap - 2, 32769, 70))]


def fits(dst_cfg, words):
    """msnake_copy_envs' condition: every body of the source env has at most cap - 1 pieces in the destination."""
    return all(body_len(words, s) <= sd.cap(dst_cfg) - 1 for s in range(dst_cfg["n_snakes"]))


def copy_src_play():
    """The large handle's envs driven along the cycle for COPY_SRC_STEPS steps (its rings rotate)."""
    def make():
        cfg = cfg_of(COPY["src_max_steps"])
        return Record(cfg, make_oracle(cfg, copy_states()), lambda o, k: cycle_actions(o), COPY_SRC_STEPS, words_at=[COPY_SRC_STEPS])
    return _once("copy_src", make)


def copy_dst_play():
    """The envs that fit the small handle, played on there for COPY_ON steps."""
    def make():
        cfg = cfg_of(COPY["dst_max_steps"])
        words = [w for w in copy_states() if fits(cfg, w)]
        return Record(cfg, make_oracle(cfg, words), lambda o, k: cycle_actions(o), COPY_ON, words_at=[COPY_ON])
    return _once("copy_dst", make)


def copy_back_play():
    """The large handle after the way back: its envs after COPY_SRC_STEPS steps, those that COPY["back"] selects replaced
    by the small handle's, played on for COPY_ON steps."""
    def make():
        cfg = cfg_of(COPY["src_max_steps"])
        words, back = list(copy_src_play().words[COPY_SRC_STEPS]), copy_back_states()
        for e, i in enumerate(COPY["back"]):
            if i >= 0:
                words[e] = back[i]
        return Record(cfg, make_oracle(cfg, words), lambda o, k: cycle_actions(o), COPY_ON, words_at=[0, COPY_ON])
    return _once("copy_back", make)


# ------------------------------------------------------------------------------------------ E. the step cap
CAP_CONFIGS = {
    "S19x3": dict(rules="snake_env", dim=19, n_snakes=3, n_fruits=3),
    "S10x1": dict(rules="snake_env", dim=10, n_snakes=1, n_fruits=1),
    "A10x3": dict(rules="adversarial", dim=10, n_snakes=3, n_fruits=3),
    "N6x4": dict(rules="new_world", dim=6, n_snakes=4, n_fruits=5),
}
CAP_N, CAP_STEPS, CAP_WARM, CAP_POOL = 8, 6, 12, 512


def cap_states(key, max_steps):
    """(cfg, CAP_N states) from a short random play -- bodies and returns are not those of a reset --, whose episode is
    in progress and whose snakes survive the moves of cap_actions up to the cap (so that the cap is what ends them),
    with t = ep_len = max_steps - 4 + (e mod 4): the step cap falls on steps 4, 3, 2, 1 of the play that follows.  Under
    new_world the main snake is dead in every state: the rule set ends the episode at every step at which it is alive."""
    def make():
        cfg = dict(CAP_CONFIGS[key], max_steps=max_steps)
        ns, nw = cfg["n_snakes"], cfg["rules"] == "new_world"
        ora = sd.make_oracle(dict(cfg, max_steps=2000), CAP_POOL, seed=21, auto_reset=False)
        ora.reset()
        rs = np.random.default_rng([9, len(key)])
        for _ in range(CAP_WARM):
            ora.step(rs.integers(0, 5, (CAP_POOL, ns)).astype(np.int32))
        pool = []
        for e in range(CAP_POOL):
            w = sd.export(ora, e, False)
            hdr = [snake_header(w, s)[0] for s in range(ns)]
            if (hdr[0][4] == 0 and any(h[4] and h[0] for h in hdr[1:])) if nw else not ora.finished(e):
                pool.append(w)
        pool.sort(key=lambda w: int(w[5]) == 0)                # those with a return so far first
        # slot e gets the first unused candidate that lives through the moves slot e makes before its cap (tried on an
        # oracle of all candidates; the fruits it draws there are another slot's, so this is a choice, not a promise)
        acts, chosen, used = cap_actions(key, max_steps), [], set()
        for e in range(CAP_N):
            trial = make_oracle(dict(cfg, max_steps=2000), pool, auto_reset=False)
            ok = np.ones(len(pool), bool)
            for k in range(3 - e % 4):
                trial.step(np.repeat(acts[k, e][None], len(pool), 0))
                ok &= trial.done == 0
            i = next(i for i in range(len(pool)) if ok[i] and i not in used)
            used.add(i)
            w = pool[i].copy()
            w[0] = w[4] = max_steps - 4 + e % 4
            chosen.append(w)
        return cfg, chosen
    return _once(("cap_states", key, max_steps), make)


def cap_actions(key, max_steps):
    rs = np.random.default_rng([13, len(key), max_steps])
    return rs.integers(0, 5, (CAP_STEPS, CAP_N, CAP_CONFIGS[key]["n_snakes"])).astype(np.int32)


def cap_play(key, max_steps, resets, auto_reset=False):
    """cap_states played for CAP_STEPS random steps on the oracle: without a reset in between (a finished env stays
    done), with the masked reset of the done envs after every step, or on an oracle that resets by itself."""
    def make():
        cfg, words = cap_states(key, max_steps)
        acts = cap_actions(key, max_steps)
        ora = make_oracle(cfg, words, auto_reset=auto_reset)
        return Record(cfg, ora, lambda o, k: acts[k - 1], CAP_STEPS, words_at=[CAP_STEPS], resets=resets)
    return _once(("cap_play", key, max_steps, resets, auto_reset), make)


# ------------------------------------------------------------------------------------------ F. the longest body of play
REACH = dict(max_steps=60000, t0=59900, heads=(20, 37, 54, 71))


def reach_cfg():
    return cfg_of(REACH["max_steps"], n_fruits=0)


def reset_body():
    """(len, grow_to) of snake 1 straight after a reset of the no-fruit configuration, read from the oracle."""
    from oracle.snake_oracle import Oracle
    ora = Oracle(1, seed=SEED, **reach_cfg())
    ora.reset()
    hdr = snake_header(sd.export(ora, 0, False), 1)[0]
    return hdr[0], hdr[3]


def growth(steps):
    """[(len, grow_to)] of a lone snake 1 of the no-fruit configuration after 0..steps steps along the cycle from a
    reset body, measured on the oracle (snake 0 dead and empty, or the episode would end at once)."""
    ln, grow = reset_body()
    ora = make_oracle(reach_cfg(), [sd.state_words(NS, [], [DEAD, (folded_body(20, ln), (0, 0), grow, 1, 0)], t=0)])
    out = [(ln, grow)]
    for _ in range(steps):
        ora.step(cycle_actions(ora))
        hdr = snake_header(sd.export(ora, 0, False), 1)[0]
        out.append((hdr[0], hdr[3]))
    return out


def reach_body():
    """(len, grow_to) play from a reset has at t = REACH["t0"]: the reset body plus one piece per step (growth(), which
    tests/test_limits_host.py holds against this)."""
    ln, grow = reset_body()
    return ln + REACH["t0"], grow


def reach_states():
    """Snake 1 at t = 59900 with a folded body of the length play would have given it; snake 0 dead and empty; no fruit."""
    length, grow = reach_body()
    return [sd.state_words(NS, [], [DEAD, long_snake(h, length, grow)], t=REACH["t0"], ctr=70 + e) for e, h in enumerate(REACH["heads"])]


def reach_play():
    """reach_states driven along the cycle to the cap and two steps on (the auto reset, and the step after it)."""
    def make():
        cfg, T = reach_cfg(), REACH["max_steps"] - REACH["t0"] + 2
        return Record(cfg, make_oracle(cfg, reach_states()), lambda o, k: cycle_actions(o), T, words_at=[T - 3, T])
    return _once("reach", make)


# ------------------------------------------------------------------------------------------ the read-only entry points
def expectations(cfg, words):
    """What every read-only entry point returns on the states `words` (canonical words per env), from the *_play models:
    a dict of arrays in the dtypes and shapes of the library's outputs."""
    import cells_play as cp
    import heads_play as hp
    import local_play as lop
    import path_play as pp
    import rays_play as rp
    import space_play as spp
    import territory_play as tp
    import timed_play as tmp
    from oracle.snake_oracle import flat_to_state
    rules, dim, ns = sd.RULES[cfg["rules"]], cfg["dim"], cfg["n_snakes"]
    never = tmp.never_pops(dict(rules=rules, n_fruits=cfg["n_fruits"]))
    states = [flat_to_state(w) for w in words]
    E, every = len(states), list(range(ns))
    planes = lop.planes_all(states, dim, ns, rules)
    x = dict(cells=np.stack([cp.np_cells(st, dim, ns, rules, list(range(cp.n_views(rules, ns)))) for st in states]),
             table=np.stack([cp.np_snake_rows(st, ns) for st in states]).astype(np.int32),
             safe=np.stack([sp.np_safe_mask(st, dim, ns) for st in states]).astype(np.uint8),
             safe_greedy=np.array([sp.safe_greedy(st, dim, ns, None) for st in states], np.int32))
    space = np.stack([spp.np_space(st, dim, ns) for st in states])
    x["space"], x["space_greedy"] = space.astype(np.uint16), np.array([spp.space_greedy(st, dim, ns) for st in states], np.int32)
    terr = [tp.np_territory(st, dim, ns) for st in states]
    x["territory"] = np.stack(terr).astype(np.uint16)
    x["territory_greedy"] = np.array([tp.greedy_by_count(st, dim, ns, c) for st, c in zip(states, terr)], np.int32)
    field = [pp.np_field(st, dim) for st in states]
    x["field"] = np.stack(field).astype(np.uint16)
    x["path"] = np.stack([pp.np_path(st, dim, ns, f) for st, f in zip(states, field)]).astype(np.uint16)
    x["path_greedy"] = np.array([pp.path_greedy(st, dim, ns) for st in states], np.int32)
    life = [tmp.np_life(st, dim, never) for st in states]
    reach = [tmp.np_timed(st, dim, ns, L) for st, L in zip(states, life)]
    x["life"], x["reach"] = np.stack(life).astype(np.uint16), np.stack(reach).astype(np.uint16)
    x["timed_greedy"] = np.array([tmp.greedy_by_count(st, ns, r) for st, r in zip(states, reach)], np.int32)
    heads = [hp.np_heads(st, dim, ns) for st in states]
    x["dist"] = np.stack([h[0] for h in heads]).astype(np.uint16)
    x["owner"] = np.stack([h[1] for h in heads]).astype(np.uint8)
    x["counts"] = np.stack([h[2] for h in heads]).astype(np.uint16)
    for r in (2, 31):
        x[f"local{r}"], x["heading"] = lop.np_local_all(states, dim, ns, rules, every, r, True, planes=planes)
    x["rays"], _ = rp.np_rays_all(states, dim, ns, rules, every, True, planes=planes)
    assert all(v.shape[0] == E for v in x.values())
    return x
