"""Every kernel that reads bodies out of HBM, on a ROTATED overflow ring.

The kernels off the step path (state export on the host and on the device, the state hashes, render_cells, render_local,
render_rays, safe moves, reachable space, territory, path, timed reach, head fields, move fates, playouts, death causes,
copy_envs) all walk a body
the same way, most of them through msnake_envread.inc: piece i >= 64 sits at ovf[(ohp + i - 64) % cap].  A state
installed with set_state starts at ohp = 0, which is all that their own suites see of bodies over 64
cells.  Here a long body is installed and then DRIVEN: every step of a body over 64 cells evicts one piece into the overflow ring and moves ohp down by
one (mod cap), so k steps after the install ohp = (cap - k) % cap, and the walk wraps around the end of the ring
whenever ohp + len - 64 > cap -- from the first step on, until ohp has come down far enough, and again once ohp has
passed 0.

The CPU oracle is the master: it chooses the Hamiltonian move (scripted_play.hamiltonian), it steps next to the
handle, and every expectation is computed from its state (its exported words, the header's hash formula on them, and
the NumPy references of tests/*_play.py: expected() below, which needs no GPU).  Everything is compared bit for bit, for
all 8 envs.  What the header refuses under new_world (move fates, playouts, death causes) is left out of that case.

Both plays keep grow_to far below the body length: a fruit then raises grow_to and the body keeps its length, where
a body that grew by 2 per fruit would fill the 10 free cells, and end the episode, long before the ring has turned.

snake_env 10x10, 1 snake (cap 128): a 90-cell body along the Hamiltonian cycle, driven for cap + 8 = 136 steps: ohp
passes every value of the ring and the walk wraps a second time.
new_world 10x10, 2 snakes, 1 fruit, max_steps 126 (cap 128 as well): snake 0 is dead with an empty body -- the rule
set ends the episode at every step at which snake 0 is alive --, snake 1 has 70 + 3 e cells in env e.  new_world sizes
the ring from max_steps (cap >= max_steps + 2), so no episode can turn the ring once: the play stops one step short
of the episode's cap, at 125 steps, where ohp has passed 125 of the 128 values; the wrap of the walk is covered from
the first step on.  copy_envs goes into a handle with max_steps 300, whose ring holds 320 cells.
snake_env_noreset: the snake_env play on a handle created with auto_reset off, which msnake_death_causes asks of its
`after` handle (and which steps on the generic kernels, where the handle of the snake_env case steps on the ones
compiled for 10x10 x 1): the copy target is `before`, filled in front of a step, and the causes are read behind it.
No episode ends in these plays, so every cause is 0 -- from a kernel that compared the head with every piece of the body.
"""
import numpy as np
import pytest

import causes_play as cap_
import cells_play as cp
import fates_play as fp
import heads_play as hp
import local_play as lp
import path_play as pp
import playout_play as plp
import rays_play as rp
import scripted_play as sp
import space_play as spp
import territory_play as tp
import timed_play as tmp
from state_domain import assert_words, blob_words, export as ora_words, header_hash

pytestmark = pytest.mark.gpu

N, DIM, CAP, SEED = 8, 10, 128, 3
PLAYOUT_STEPS = 4
CASES = {
    "snake_env": dict(cfg=dict(rules="snake_env", dim=DIM, n_snakes=1, n_fruits=1), max_steps=2000, dst_max_steps=500,
                      lens=lambda e: (90,), steps=CAP + 8),
    "new_world": dict(cfg=dict(rules="new_world", dim=DIM, n_snakes=2, n_fruits=1), max_steps=126, dst_max_steps=300,
                      lens=lambda e: (0, 70 + 3 * e), steps=125),
}
CASES["snake_env_noreset"] = dict(CASES["snake_env"], auto_reset=False)


def cycle(dim):
    """The cells of scripted_play.hamiltonian_table(dim) in walking order, from (0, 0)."""
    act, out, c = sp.hamiltonian_table(dim), [], (0, 0)
    for _ in range(dim * dim):
        out.append(c)
        d = sp.DIRS[act[c[0]][c[1]]]
        c = (c[0] + d[0], c[1] + d[1])
    assert c == (0, 0) and len(set(out)) == dim * dim
    return out


def start_state(key, e):
    """Env e's installed state: the body lies along the cycle, its head at cycle cell 11 e + 95, the fruit on a free
    cell; grow_to is 3 whatever the length, and an empty body belongs to a dead snake."""
    case, cyc, n2 = CASES[key], cycle(DIM), DIM * DIM
    lens = case["lens"](e)
    snakes = [[list(cyc[(11 * e + 95 - i) % n2]) for i in range(ln)] for ln in lens]
    vels = [[b[0][0] - b[1][0], b[0][1] - b[1][1]] if b else [0, 0] for b in snakes]
    used = {tuple(c) for b in snakes for c in b}
    free = [c for c in cyc if c not in used]
    rng = np.random.default_rng([5, e, len(lens)])
    fruits = [list(free[i]) for i in rng.choice(len(free), case["cfg"]["n_fruits"], replace=False)]
    return {"t": 0, "ctr": 40 + e, "spare_fruits": 0, "ep_len": 0, "ep_return": 0.0, "fruits": fruits, "snakes": snakes,
            "vels": vels, "grow_to": [3] * len(lens), "alive": [bool(b) for b in snakes], "in_dead": [not b for b in snakes]}


def longest_body(st):
    return max(len(b) for b in st["snakes"])


def make_oracle(key):
    from oracle.snake_oracle import Oracle
    case = CASES[key]
    ora = Oracle(N, seed=SEED, max_steps=case["max_steps"], auto_reset=case.get("auto_reset", True), **case["cfg"])
    ora.reset()
    for e in range(N):
        ora.set_state(e, start_state(key, e))
    return ora


def cut(st, keep=64):
    """The state without the pieces of index >= keep: what a reader that never looked into the overflow ring would see."""
    return dict(st, snakes=[b[:keep] for b in st["snakes"]])


def expected(key, states, words):
    """name -> array (or list of word arrays) of everything the newer readers return, from the oracle's canonical states
    and words alone: the references of tests/*_play.py and the header's hash formula.  No GPU, no library."""
    cfg = CASES[key]["cfg"]
    ns, rules, snakes = cfg["n_snakes"], sp.RULES[cfg["rules"]], list(range(cfg["n_snakes"]))
    per_env = lambda fn, dtype: np.stack([np.asarray(fn(st)) for st in states]).astype(dtype)  # noqa: E731
    want = {"export": [np.asarray(w, np.int32) for w in words], "export_count": np.array([len(w) for w in words], np.int32),
            "hash_full": np.array([header_hash(w) for w in words], np.int64),
            "hash_board": np.array([header_hash(w, board=True) for w in words], np.int64)}
    planes = lp.planes_all(states, DIM, ns, rules)
    for o in (0, 1):
        want[f"local{o}"], want[f"local{o}_heading"] = lp.np_local_all(states, DIM, ns, rules, snakes, DIM, o, planes=planes)
        want[f"rays{o}"], want[f"rays{o}_heading"] = rp.np_rays_all(states, DIM, ns, rules, snakes, o, planes=planes)
    want["safe"] = per_env(lambda st: sp.np_safe_mask(st, DIM, ns), np.uint8)
    want["territory_act"] = per_env(lambda st: tp.territory_greedy(st, DIM, ns), np.int32)
    want["territory"] = per_env(lambda st: tp.np_territory(st, DIM, ns), np.uint16)
    want["path_act"] = per_env(lambda st: pp.path_greedy(st, DIM, ns), np.int32)
    want["path"] = per_env(lambda st: pp.np_path(st, DIM, ns), np.uint16)
    want["field"] = per_env(lambda st: pp.np_field(st, DIM), np.uint16)
    never = tmp.never_pops(dict(rules=rules, n_fruits=cfg["n_fruits"]))
    want["timed_act"] = per_env(lambda st: tmp.timed_greedy(st, DIM, ns, never=never), np.int32)
    want["reach"] = per_env(lambda st: tmp.np_timed(st, DIM, ns, never=never), np.uint16)
    want["life"] = per_env(lambda st: tmp.np_life(st, DIM, never), np.uint16)
    heads = [hp.np_heads(st, DIM, ns) for st in states]
    want["head_dist"] = np.stack([h[0] for h in heads]).astype(np.uint16)
    want["head_owner"] = np.stack([h[1] for h in heads]).astype(np.uint8)
    want["head_counts"] = np.stack([h[2] for h in heads]).astype(np.uint16)
    if rules == sp.RULES["snake_env"]:
        fates = fp.expected(dict(dim=DIM, n_snakes=ns), states)
        want.update(zip(("wary_act", "fate", "fate_by", "fate_eat", "fate_mask"), fates))
        ref = plp.np_playout(dict(rules=rules, dim=DIM, n_snakes=ns, n_fruits=cfg["n_fruits"], seed=SEED, env_id_base=0,
                                  max_steps=CASES[key]["max_steps"]), states, "hamiltonian", PLAYOUT_STEPS)
        want.update({"playout_" + k: v for k, v in ref.items()})
    return want


def shows_pieces_past_63(key, states, ref):
    """Per check, whether the expectation `ref` of at least one env depends on a piece of index >= 64: it differs from
    the expectation on the same states cut to 64 pieces."""
    cfg = CASES[key]["cfg"]
    ns, rules, snakes = cfg["n_snakes"], sp.RULES[cfg["rules"]], list(range(cfg["n_snakes"]))
    short = [cut(st) for st in states]
    assert all(len(b) <= 64 for st in short for b in st["snakes"]) and any(len(b) > 64 for st in states for b in st["snakes"])
    out = {"local": all(not np.array_equal(lp.np_local_all(short, DIM, ns, rules, snakes, DIM, o)[0], ref[f"local{o}"]) for o in (0, 1))}
    if rules == sp.RULES["snake_env"]:
        out["fates"] = not np.array_equal(fp.expected(dict(dim=DIM, n_snakes=ns), short)[1], ref["fate"])
    return out


def measured(env, key):
    """The same names from the handle, each entry point called once (twice where it has an `oriented`)."""
    import torch
    rules = sp.RULES[CASES[key]["cfg"]["rules"]]
    n, ns, dev = env.num_envs, env.n_snakes, env.device
    host = lambda t: t.cpu().numpy()  # noqa: E731
    new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
    rows = lambda words, count: [w[:c].copy() for w, c in zip(host(words), host(count))]  # noqa: E731
    got = {}
    words, count = env.export_states_device()
    got["export"], got["export_count"] = rows(words, count), host(count)
    got["hash_full"], got["hash_board"] = host(env.hash_states_device("full")), host(env.hash_states_device("board"))
    for o in (0, 1):
        got[f"local{o}"], got[f"local{o}_heading"] = map(host, env.render_local_device(DIM, oriented=bool(o), heading=True))
        got[f"rays{o}"], got[f"rays{o}_heading"] = map(host, env.render_rays_device(oriented=bool(o), heading=True))
    safes = []
    for pol, names, kws in (("territory_greedy", ("territory",), ("territory_out",)),
                            ("path_greedy", ("path", "field"), ("path_out", "field_out")),
                            ("timed_greedy", ("reach", "life"), ("reach_out", "life_out"))):
        outs = {kw: new((n, DIM, DIM) if kw in ("field_out", "life_out") else (n, ns, 4), torch.uint16) for kw in kws}
        safe, act = new((n, ns), torch.uint8), new((n, ns), torch.int32)
        env.scripted_actions_device(pol, out=act, safe_out=safe, **outs)
        got[pol.split("_")[0] + "_act"] = host(act)
        safes.append(host(safe))
        for name, kw in zip(names, kws):
            got[name] = host(outs[kw])
    assert all(np.array_equal(s, safes[0]) for s in safes)
    got["safe"] = safes[0]
    got["head_dist"], got["head_owner"], got["head_counts"] = map(host, env.head_fields_device())
    if rules == sp.RULES["snake_env"]:
        fates = [new((n, ns, 2 if name == "mask" else 5), torch.uint8) for name in ("fate", "by", "eat", "mask")]
        act = new((n, ns), torch.int32)
        env.scripted_actions_device("wary_greedy", out=act, fates_out=fates)
        got.update(zip(("wary_act", "fate", "fate_by", "fate_eat", "fate_mask"), map(host, [act] + fates)))
        res = env.playout_device(PLAYOUT_STEPS, "hamiltonian", end_state=True)
        got.update({"playout_" + k: host(t) for k, t in zip(("steps", "end", "ret", "info"), res[:4])})
        got["playout_words"], got["playout_count"] = rows(res[4], res[5]), host(res[5])
    return got


def walk_wraps(k, body_len):
    """k steps after the install: does the walk over pieces 64.. pass the end of the overflow ring?"""
    return (CAP - k) % CAP + body_len - 64 > CAP


def compare_at(key, steps):
    """The steps (0 = straight after the install) at which everything is compared: every 8th, the last, and the step
    at which the walk first wraps."""
    first_wrap = next(k for k in range(1, steps + 1) if all(walk_wraps(k, max(CASES[key]["lens"](e))) for e in range(N)))
    return sorted(set(range(0, steps + 1, 8)) | {steps, first_wrap}), first_wrap


@pytest.mark.parametrize("key", sorted(CASES))
def test_every_reader_on_a_rotated_overflow_ring(key):
    import msnake
    from oracle.snake_oracle import state_to_flat
    case = CASES[key]
    cfg, ns, steps = case["cfg"], case["cfg"]["n_snakes"], case["steps"]
    rules = sp.RULES[cfg["rules"]]
    views = list(range(cp.n_views(rules, ns)))
    assert sp.ring_cap(dict(rules=rules, dim=DIM, max_steps=case["max_steps"])) == CAP
    assert sp.ring_cap(dict(rules=rules, dim=DIM, max_steps=case["dst_max_steps"])) == (CAP if rules != 1 else 320)

    ora = make_oracle(key)
    env = msnake.MultiSnakeVecEnv(N, seed=SEED, max_steps=case["max_steps"], auto_reset=case.get("auto_reset", True), **cfg)
    dst = msnake.MultiSnakeVecEnv(N, seed=SEED, max_steps=case["dst_max_steps"], **cfg)
    with_causes = not case.get("auto_reset", True)        # msnake_death_causes refuses an `after` handle that resets itself
    if rules == 0:   # the two snake_env cases differ in the step kernels they run, as the module docstring says
        assert env.kernel_name().endswith(f", {DIM}>") == (not with_causes), env.kernel_name()
    env.reset()
    dst.reset()
    for e in range(N):
        env.set_state_words(e, state_to_flat(start_state(key, e), ns))
    read = sp._StateReader(ora)
    at, first_wrap = compare_at(key, steps)
    wrapped_at, straight_at, ohp_seen = [], [], set()
    fates_past_63, n_causes = [], []

    def compare(k):
        states = [read(e) for e in range(N)]
        longest = [longest_body(st) for st in states]
        assert min(longest) > 64, (k, longest)           # a body over 64 cells in every env
        (wrapped_at if all(walk_wraps(k, n) for n in longest) else straight_at).append(k)
        want = [ora_words(ora, e) for e in range(N)]
        assert_words(blob_words(env.get_state_all()), want, (k, "get_state_all"))
        cells, table = env.render_cells_device(snakes=True)
        assert np.array_equal(cells.cpu().numpy(), np.stack([cp.np_cells(st, DIM, ns, rules, views) for st in states])), (k, "cells")
        assert np.array_equal(table.cpu().numpy(), np.stack([cp.np_snake_rows(st, ns) for st in states])), (k, "table")
        assert np.array_equal(env.safe_moves_device().cpu().numpy(), np.stack([sp.np_safe_mask(st, DIM, ns) for st in states])), (k, "safe")
        assert np.array_equal(env.reachable_space_device().cpu().numpy().astype(np.int64),
                              np.stack([spp.np_space(st, DIM, ns) for st in states])), (k, "space")
        dst.copy_envs_device(env)
        assert_words(blob_words(dst.get_state_all()), want, (k, "copy_envs"))
        ref, got = expected(key, states, want), measured(env, key)
        assert sorted(got) == sorted(ref), (k, sorted(got), sorted(ref))
        for name in sorted(ref):
            if isinstance(ref[name], list):
                assert_words(got[name], ref[name], (k, name))
            else:
                assert got[name].shape == ref[name].shape and np.array_equal(got[name], ref[name]), (k, name, got[name], ref[name])
        # the checks above read the overflow ring: a reader that stopped at piece 63 would have been caught
        shown = shows_pieces_past_63(key, states, ref)
        assert shown["local"], (k, "local")
        fates_past_63.append(shown.get("fates", False))
        assert_words(blob_words(env.get_state_all()), want, (k, "the readers changed the state"))
        return states

    def compare_causes(k, before, after):
        """dst holds the state in front of step k (the copy of the comparison at k - 1), env the state behind it."""
        ref = [cap_.np_causes(b, a, DIM) for b, a in zip(before, after)]
        got = env.death_causes_device(dst)
        for j, name in enumerate(("cause", "by", "victims", "where")):
            want = np.stack([r[j] for r in ref])
            have = got[j].cpu().numpy()
            assert have.dtype == want.dtype and np.array_equal(have, want), (k, "causes", name, have, want)

    states = compare(0)
    for k in range(1, steps + 1):
        act = np.array([sp.hamiltonian(st, DIM, ns) for st in states], np.int32)
        obs, rew, done, _ = env.step(act)
        o_obs, o_rew, o_done = ora.step(act)[:3]
        assert np.array_equal(obs, o_obs) and np.array_equal(rew, o_rew) and np.array_equal(done, o_done.astype(bool)), k
        assert not o_done.any(), k
        if with_causes and k - 1 in at:
            compare_causes(k, states, [read(e) for e in range(N)])
            n_causes.append(k)
        if k in at:
            states = compare(k)
        else:
            states = [read(e) for e in range(N)]
            assert min(longest_body(st) for st in states) > 64, k    # every step evicts: ohp = (cap - k) % cap
        ohp_seen.add((CAP - k) % CAP)

    assert first_wrap in wrapped_at and straight_at, (first_wrap, wrapped_at, straight_at)
    if steps >= CAP + 8:   # the overflow position has passed every value, and the walk wraps a second time
        assert ohp_seen == set(range(CAP)) and max(wrapped_at) > max(straight_at) > first_wrap
    if rules == 0:     # at every comparison some env's head stands next to a piece of index >= 64, and the fates say so
        assert all(fates_past_63), (at, fates_past_63)
    assert len(n_causes) == (len(at) - 1 if with_causes else 0), (n_causes, at)
    assert env.stats()["errors"] == 0 and dst.stats()["errors"] == 0
    env.close()
    dst.close()
