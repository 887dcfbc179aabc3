"""Random interleavings of every entry point on one handle, and of device-side copies between it and a twin handle,
against the CPU oracle (tests/op_fuzz.py); and a state made on one record policy continued on the other, with no
randomness in the path.  Bit-exact throughout.

The adapter owns two handles: the main one and its twin (the neighbouring shard, another seed, the opposite record
policy, another envs_per_block; reset once at open).  Besides the older op kinds the sequences hold `space`
(msnake_space_actions: counts, safe mask and the space_greedy columns, whose actions drive the next step), `cells`
(msnake_render_cells: planes of a random view mask and the snake table), `fork` (msnake_copy_envs in either direction
with the identity, a permutation, a sparse map or one with out-of-range entries; both handles' states and stats() are
compared in full afterwards) and `swap` (main and twin exchange roles, so every later op runs on the handle the copy
kernel last wrote).  S10x1, S19x3_spec and S19x2_spec start on the step kernels compiled for the handle's shape: a
padded stride falls back to the generic kernel for the call, a migration or a swap hands the state to a generic
handle and back.  The adapter asserts at open that the full-record handle of these reports a kernel name that carries
the board size.  Every call goes through the C entry points on the adapter's one stream.

The entry points added since run in the same sequences: `local`, `rays`, `territory`, `path`, `timed`, `heads`, `fates`,
`export` and `hash` (readers, each also in a `sweep` directly behind every writer of state: the copy kernel and the swap
onto what it wrote, an import, a migration, a rollout with its parked draws, a masked reset, the set_state of a body
over 64 cells), `causes` (the main handle against the twin), `playout` (the handle's blob and stats() unchanged; its end
words imported into the twin, which is then stepped), `outcomes` (a tracker per handle, compared whole after every
call) and `import` (msnake_import_states: rows from the twin's device-side export, permuted, the handle's own with
edited counters, and rows to be refused; every env's status, the full blob and stats() afterwards).

Not fuzzed, host-only and tested elsewhere: msnake_state_blob_info, msnake_kernel_name_for_config (and
msnake_kernel_name beyond the assertion above; msnake_state_words_max is held against the header's formula).

The sequences are the ones tests/test_op_fuzz_host.py runs on the oracle alone, where their coverage is counted and
asserted, and where each of the twenty-three silent defects OracleAdapter can inject (among them fork_row_shifted,
space_off_by_one, import_refused_row_written, import_parked_kept, playout_counts_steps, outcomes_tracker_not_updated)
is shown to be caught.  Only calls that include/msnake.h documents as valid are issued.

Regression cases (a (configuration, seed, op index) that once exposed a product bug, kept by name): none so far."""
import numpy as np
import pytest

import op_fuzz as of

pytestmark = pytest.mark.gpu

CASES = of.cases()


@pytest.mark.parametrize("cfg,seed", CASES, ids=[f"{c['name']}-s{s}" for c, s in CASES])
def test_random_op_sequence_against_the_oracle(cfg, seed):
    of.run(of.HipAdapter(), cfg, of.gen_ops(cfg, seed, cfg["n_ops"]), count=False)


# ---------------------------------------------------------------------------------- full record <-> short record
def _mk(n, kw, **tuning):
    import msnake
    return msnake.MultiSnakeVecEnv(n, **kw, **tuning)


def _oracle(n, kw):
    from oracle.snake_oracle import Oracle
    return Oracle(n, **kw)


def _play(env, ora, rs, steps, what, rows=None):
    """Seeded random play of both; rew / done / info r, l, num_snakes of every env and the observations (of every env, or
    of `rows`) at every step."""
    import torch
    n, ns = env.num_envs, env.n_snakes
    ends = 0
    for t in range(steps):
        act = rs.integers(0, 5, (n, ns)).astype(np.int32)
        obs, rew, done, info = env.step_device(torch.from_numpy(act).to(env.device))
        o_obs, o_rew, o_done, o_ns, o_er, o_el = ora.step(act, threads=16)
        info = info.cpu().numpy()
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), (what, t)
        assert np.array_equal(info[:, 0].copy().view(np.float32), o_er) and np.array_equal(info[:, 1], o_el), (what, t)
        assert np.array_equal(info[:, 2], o_ns) and np.array_equal(info[:, 3], o_done), (what, t)
        if rows is None:
            assert np.array_equal(obs.cpu().numpy(), o_obs), (what, t)
        else:
            assert np.array_equal(obs[torch.as_tensor(rows, device=env.device)].cpu().numpy(), o_obs[rows]), (what, t)
        ends += int(o_done.sum())
    assert ends > 0, what
    return ends


def _same_states(env, ora, envs, what):
    from oracle.snake_oracle import flat_to_state
    for e in envs:
        assert flat_to_state(env.get_state_words(e)) == ora.get_state(e), (what, e)


@pytest.mark.parametrize("rules,dim", [("snake_env", 19), ("adversarial", 10)])
def test_a_state_made_on_one_record_policy_continues_on_the_other(rules, dim):
    """4 096 envs: 40 steps on the full record (parked draws, upper half live) -> the blob into a short-record handle
    with 4 envs per workgroup, 60 steps -> the blob into a fresh full-record handle, 60 more; every step against the
    oracle.  Then the same through set_state_words for 32 envs of a 16 384-env handle (short record by default) and
    back into a full-record one.  max_steps 25: episodes end and restart on both sides of every hand-over."""
    n, ns = 4096, 3
    kw = dict(dim=dim, n_snakes=ns, rules=rules, seed=(5 << 32) | 123, max_steps=25, env_id_base=640)
    rs = np.random.default_rng(dim)
    ora = _oracle(n, kw)
    a = _mk(n, kw, record_policy="full")
    assert np.array_equal(a.reset(), ora.reset())
    _play(a, ora, rs, 40, "full")
    blob = a.get_state_all()
    b = _mk(n, kw, record_policy="short", envs_per_block=4)
    b.reset()
    b.set_state_all(blob)
    assert np.array_equal(b.get_state_all(), blob)
    a.close()
    _play(b, ora, rs, 60, "full -> short")
    blob = b.get_state_all()
    c = _mk(n, kw, record_policy="full")
    c.reset()
    c.set_state_all(blob)
    assert np.array_equal(c.get_state_all(), blob)
    st_b = b.stats()
    assert st_b["errors"] == 0 and st_b["env_steps"] == 60 * n
    b.close()
    _play(c, ora, rs, 60, "short -> full")
    _same_states(c, ora, range(0, n, 37), "after short -> full")

    # ---- the same by words: 32 envs into a 16 384-env handle on the short record, played, and back onto a full record
    N = 16384
    rows = sorted(int(e) + n * int(k) for e, k in zip(rs.choice(n, 32, replace=False), rs.integers(0, N // n, 32)))
    src = sorted(int(e) for e in rs.choice(n, 32, replace=False))
    big, big_ora = _mk(N, kw), _oracle(N, kw)
    big.reset(), big_ora.reset()
    for e, s in zip(rows, src):
        w = c.get_state_words(s)
        big.set_state_words(e, w)
        big_ora.set_state(e, ora.get_state(s))
    _same_states(big, big_ora, rows, "words full -> short")
    _play(big, big_ora, rs, 60, "words on the short record", rows=rows)
    _same_states(big, big_ora, rows, "after the short record")
    back, back_ora = _mk(n, kw, record_policy="full"), _oracle(n, kw)
    back.reset(), back_ora.reset()
    dst = [e % n for e in rows]
    assert len(set(dst)) == 32
    for e, d in zip(rows, dst):
        back.set_state_words(d, big.get_state_words(e))
        back_ora.set_state(d, big_ora.get_state(e))
    _play(back, back_ora, rs, 60, "words short -> full")
    _same_states(back, back_ora, dst, "after words short -> full")
    for env in (c, big, back):
        assert env.stats()["errors"] == 0
        env.close()
