"""tests/op_fuzz.py on the CPU: the driver, its stats models and its guards against further Oracles (the null test), the
coverage the generated sequences reach (counted on the oracle alone, for every (configuration, seed) the GPU file runs:
op kinds, class pairs, the copies between the handle and its twin, the compiled-shape step kernels and the hand-overs
to and from the generic ones, the entry points added since: readers behind every writer of state, imports, playouts, death
causes, outcomes), the injected silent defects (each must be caught), and the generator's determinism."""
import ctypes
import hashlib
import re

import pytest

import op_fuzz as of

CASES = of.cases()
IDS = [f"{c['name']}-s{s}" for c, s in CASES]
_COV = {}


def _null(cfg, seed):
    """run(OracleAdapter()) of one case, once per process; passing at all is the null test."""
    key = (cfg["name"], seed)
    if key not in _COV:
        ops = of.gen_ops(cfg, seed, cfg["n_ops"])
        _COV[key] = (of.run(of.OracleAdapter(), cfg, ops), ops)
    return _COV[key]


SNAKE_ENV, NEW_WORLD, ADVERSARIAL = 0, 1, 2
# kind -> (the rule sets whose handles take the call, it needs a handle created with auto_reset off, its reference is a
# Python search per env and it is left out above 8 192 envs); a kind not listed applies everywhere ([N] migrates over
# envs_per_block; odd boards script safe_greedy)
TABLE = {
    "fates": ((SNAKE_ENV, ADVERSARIAL), False, True),
    "causes": ((SNAKE_ENV, ADVERSARIAL), True, True),
    "playout": ((SNAKE_ENV,), False, True),
    "outcomes": ((SNAKE_ENV, NEW_WORLD, ADVERSARIAL), True, False),
    "territory": ((SNAKE_ENV, NEW_WORLD, ADVERSARIAL), False, True),
    "path": ((SNAKE_ENV, NEW_WORLD, ADVERSARIAL), False, True),
    "timed": ((SNAKE_ENV, NEW_WORLD, ADVERSARIAL), False, True),
    "heads": ((SNAKE_ENV, NEW_WORLD, ADVERSARIAL), False, True),
    "sweep": ((SNAKE_ENV, NEW_WORLD, ADVERSARIAL), False, True),
}
QUIET_NEW = of.READERS + ("causes", "playout", "outcomes")


def _applicable(cfg):
    big = cfg["num_envs"] > 8192
    return {k for k in of.KINDS if k not in TABLE or (cfg["rules"] in TABLE[k][0] and not (TABLE[k][1] and cfg["auto_reset"])
                                                      and not (TABLE[k][2] and big))}


@pytest.mark.parametrize("cfg,seed", CASES, ids=IDS)
def test_null_run_and_coverage_of_every_case(cfg, seed):
    cov, ops = _null(cfg, seed)
    print(cfg["name"], seed, {k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items()})
    assert len(ops) == cfg["n_ops"]
    # 1. every op kind at least 3 times (above 8 192 envs: space, cells and fork at least once; swap follows fork); of the
    # kinds added since, every applicable one at least 2 times (above 8 192 envs: once), import at least 3 times, and
    # none that does not apply
    app, big = _applicable(cfg), cfg["num_envs"] > 8192
    assert app == of.applicable(cfg) and all(cov["kinds"][k] == 0 for k in set(of.KINDS) - app), (app, cov["kinds"])
    few = ("space", "cells", "fork", "swap") if big else ("swap",)
    newer = QUIET_NEW + ("sweep", "import")       # (import: condition 14)
    assert all(cov["kinds"][k] >= (1 if k in few else 3) for k in app if k not in newer), cov["kinds"]
    assert all(cov["kinds"][k] >= (1 if big else 2) for k in app if k in newer and k != "import"), cov["kinds"]
    # 14. imports: rows that are skipped, installed and refused for at least 3 of the six reasons; an import directly in
    # front of each of step, rollout and reset_mask
    # (above 8 192 envs the sequence stays the minimum: imports at all, one of them plain and one with a sparse mask)
    st = cov["import_status"]
    assert {of.STATE_SKIPPED, of.STATE_OK} <= st and (big or len(st & {1, 2, 3, 4, 5, 6}) >= 3), st
    assert cov["kinds"]["import"] >= (1 if big else 3) and (big or all(v >= 1 for v in cov["import_after"].values())), cov
    # 15. the blocks: death causes one step behind a copy, with the header's guarantee checked against the outcomes
    # (asserted by the driver); a playout whose end words go into the twin, which is then stepped
    assert cov["causes_blocks"] == ("causes" in app) and cov["playout_blocks"] == ("playout" in app), cov
    # 16. every reader directly behind each writer of state: the copy kernel (and the swap onto what it wrote), the
    # import, a migration, a rollout, a masked reset, the set_state of a body over 64 cells
    if "sweep" in app:
        want = {w: 1 for w in of.SWEEP_AFTER if w != "set_long" or of.long_body_allowed(cfg)}
        assert {w: v for w, v in cov["sweep_after"].items() if w in want} == want, cov["sweep_after"]
        for op in ops:
            if op["kind"] == "sweep":
                assert [o["kind"] for o in op["ops"]] == [k for k in of.READERS if k in app], op
    # 2. at least 2 migrations in each direction ([N] has no short record: envs_per_block only)
    if cfg["rules"] != 1:
        assert cov["migrate_dirs"].get("full>short", 0) >= 2 and cov["migrate_dirs"].get("short>full", 0) >= 2, cov["migrate_dirs"]
    else:
        assert cov["migrate_dirs"].get("full>full", 0) >= 3, cov["migrate_dirs"]
    # 3. every ordered pair of state-changing op classes, consecutively (here: for every seed, not only over the seeds)
    assert cov["pairs"] == {a + b for a in of.PAIR_CLASSES for b in of.PAIR_CLASSES}, sorted(cov["pairs"])
    # 4. episode ends and respawns inside the stepping ops
    assert cov["with_end"] >= 0.2 * cov["stepping"] and cov["with_respawn"] >= 0.2 * cov["stepping"], cov
    # 5. a rollout across a 16-step boundary with an episode end inside
    assert cov["rollout_cross16_end"] >= 1, cov
    # 9. copies in each direction at least twice, and a copy directly in front of each of step, rollout and reset_mask
    # on the handle it wrote
    assert all(cov["fork_dirs"][d] >= 2 for d in of.FORK_DIRS), cov["fork_dirs"]
    assert all(v >= 1 for v in cov["after_fork"].values()), cov["after_fork"]
    # 10. the step kernels compiled for the shape: stepping ops that run them, stepping ops that fall back to the
    # generic kernel for one call (padded stride), hand-overs of the state to a generic handle and back
    if cfg["name"] in SPEC:
        assert cov["compiled_steps"] >= 3 and cov["fallback_steps"] >= 2, cov
        assert cov["to_generic"] >= 2 and cov["to_compiled"] >= 2, cov


@pytest.mark.parametrize("cfg", of.CONFIGS, ids=[c["name"] for c in of.CONFIGS])
def test_coverage_over_the_seeds_of_a_configuration(cfg):
    covs = [_null(cfg, s)[0] for s in cfg["seeds"]]
    total = {k: sum(c[k] for c in covs) for k in ("wraps", "long_migrate", "long_checkpoint", "fin_across", "resets_of_finished",
                                                    "fork_dst_finished", "fork_src_finished", "fork_src_long", "stats_saw_errors")}
    modes = {m: sum(c["fork_modes"][m] for c in covs) for m in of.FORK_MODES}
    print(cfg["name"], total, modes)
    # 6. a 2^32 wrap of the draw counter (asked for per rule set; held per configuration)
    assert total["wraps"] >= 1, total
    # 7. a body over 64 cells survives a migration and a checkpoint_self, where the board has room for one
    if of.long_body_allowed(cfg):
        assert total["long_migrate"] >= 1 and total["long_checkpoint"] >= 1, total
    # 8. without auto reset: an env stays finished across a rollout and a checkpoint_self before it is reset
    if not cfg["auto_reset"]:
        assert total["fin_across"] >= 1 and total["resets_of_finished"] >= 1, total
    # 11. every index mode of the copy; an out-of-range one that a later stats() sees as errors > 0
    assert all(v >= 1 for v in modes.values()), modes
    assert total["stats_saw_errors"] >= 1, total
    # 12. a copy from a finished source env, and (without auto reset) onto a finished destination env
    if not cfg["auto_reset"]:
        assert total["fork_dst_finished"] >= 1 and total["fork_src_finished"] >= 1, total
    # 13. a copy of a body over 64 cells (the overflow ring), where the board has room for one
    if of.long_body_allowed(cfg):
        assert total["fork_src_long"] >= 1, total
    # 17. imports: all six refusal reasons; onto a finished env without auto reset; of a body over 64 cells
    more = {k: sum(c[k] for c in covs) for k in ("import_onto_finished", "import_long", "causes_nonzero", "outcomes_armed_died",
                                                  "outcomes_armed_ended", "outcomes_stale", "export_short", "board_twins")}
    status = set().union(*[c["import_status"] for c in covs])
    ends = set().union(*[c["playout_ends"] for c in covs])
    print(cfg["name"], more, sorted(status), sorted(ends))
    big = cfg["num_envs"] > 8192           # (the minimal sequence: see condition 14)
    assert big or {1, 2, 3, 4, 5, 6} <= status, status
    if not cfg["auto_reset"]:
        assert more["import_onto_finished"] >= 1, more
    if of.long_body_allowed(cfg):
        assert more["import_long"] >= 1, more
    app = _applicable(cfg)
    # 18. a death in a causes block; playouts that end in every way the configuration can reach
    if "causes" in app:
        assert more["causes_nonzero"] >= 1, more
    if "playout" in app:
        assert ends == {0, 1, 2} | ({3} if not cfg["auto_reset"] else set()), ends      # HORIZON, DEAD, CAP, FINISHED
    # 19. outcomes on an armed tracker with a death and with an ended snake, and on a stale tracker
    if "outcomes" in app:
        assert more["outcomes_armed_died"] >= 1 and more["outcomes_armed_ended"] >= 1 and more["outcomes_stale"] >= 1, more
    # 20. an export where a row does not fit the stride; two envs with equal BOARD and different FULL hashes (it takes two envs)
    assert big or more["export_short"] >= 1, more
    if cfg["num_envs"] > 1 and not big:
        assert more["board_twins"] >= 1, more


def test_every_reader_has_run_on_every_kind_of_handle():
    """Across all cases: each of the newer quiet kinds on the short record, on a handle that steps with the kernels compiled
    for its shape, and on handles with 1, 2, 4 and 8 envs per workgroup."""
    seen = set().union(*[_null(c, s)[0]["reader_on"] for c, s in CASES])
    for kind in QUIET_NEW:
        mine = {x[1:] for x in seen if x[0] == kind}
        assert any(rec == "short" for rec, _, _ in mine), (kind, "short record")
        assert {epb for _, _, epb in mine} >= {1, 2, 4, 8}, (kind, "envs_per_block", mine)
        if kind not in ("causes", "outcomes"):      # (a handle with auto_reset off never runs the compiled kernels)
            assert any(spec for _, spec, _ in mine), (kind, "compiled shape")


SPEC = ("S10x1", "S19x3_spec", "S19x2_spec")


@pytest.mark.parametrize("name", SPEC)
def test_the_compiled_shape_configurations_start_on_a_compiled_kernel(name):
    """Asked of the library's own host glue (no GPU), as tests/test_shape_spec_host.py does: the starting tuning names
    an instantiation with the fifth template argument, the same configuration on the short record names none."""
    import msnake
    C = msnake._capi
    cfg = of.BY_NAME[name]

    def kernel(record):
        c = C.MsnakeConfig(ctypes.sizeof(C.MsnakeConfig), 0, cfg["num_envs"], cfg["dim"], cfg["n_snakes"], cfg["n_fruits"],
                           cfg["rules"], cfg["max_steps"], int(cfg["auto_reset"]), cfg["obs_scale"], cfg["seed"],
                           cfg["env_id_base"], cfg["tuning"]["envs_per_block"], C.RECORD_POLICY[record],
                           C.STORE_POLICY[cfg["tuning"]["obs_store_policy"]], 0)
        return C.kernel_name_for_config(c)

    assert of.compiled_shape(cfg, cfg["tuning"]) and not of.compiled_shape(cfg, of.twin_cfg(cfg)["tuning"])
    assert kernel(cfg["tuning"]["record_policy"]) == "msnake_step_kernel<0, %d, 0, 1, %d>" % (cfg["n_snakes"], cfg["dim"])
    assert kernel("short") == "msnake_step_kernel<0, %d, 0, 1>" % cfg["n_snakes"]


def test_the_table_covers_what_it_is_there_for():
    C = of.CONFIGS
    assert {c["rules"] for c in C} == {0, 1, 2} and 10 <= len(C) <= 14
    assert {c["n_snakes"] for c in C if c["rules"] != 1} == {1, 2, 3} and any(c["n_snakes"] == 4 for c in C if c["rules"] == 1)
    assert min(c["dim"] for c in C) == 3 and max(c["dim"] for c in C) == 19
    assert all(5 <= c["max_steps"] <= 12 for c in C) and {c["max_steps"] for c in C} >= {5, 12}
    assert {c["obs_scale"] for c in C} == {1, 4}
    for r in (0, 1, 2):
        assert {c["auto_reset"] for c in C if c["rules"] == r} == {True, False}
    for r in (0, 2):
        assert {of.effective_record(c, c["tuning"]) for c in C if c["rules"] == r} == {"full", "short"}
    big = [c for c in C if c["num_envs"] > 8192]
    assert len(big) == 1 and big[0]["tuning"] == dict(record_policy="auto", envs_per_block=0, obs_store_policy="auto")
    assert len(big[0]["seeds"]) == 1 and big[0]["n_ops"] < min(c["n_ops"] for c in C if c is not big[0])
    assert {1, 130, 777} <= {c["num_envs"] for c in C} and any(c["num_envs"] % 4 for c in C)
    assert any(c["env_id_base"] >> 32 for c in C) and any(c["seed"] >> 32 for c in C) and any(c["env_id_base"] == 0 for c in C)


# ---------------------------------------------------------------------------------------------- sensitivity
FAULTS = [("ctr_lag", "S12x3", 1, 15), ("fruit_moved", "A10x2", 2, 15), ("fin_dropped", "A6x3", 1, 15), ("double_count", "N6x4", 3, 15),
          ("fork_row_shifted", "S19x2_spec", 1, 15), ("fork_touched_unselected", "A6x3", 2, 15), ("fork_totals_copied", "N10x2_x4", 1, 15),
          ("space_off_by_one", "S12x3", 3, 15), ("cells_head_as_body", "N6x4", 2, 15),
          ("local_shifted", "S3x2", 1, 15), ("rays_wrong_channel", "S3x2", 2, 15), ("territory_off_by_one", "S3x2", 1, 15),
          ("path_off_by_one", "S3x2", 3, 15), ("timed_life_off_by_one", "S3x2", 2, 15), ("heads_owner_tie_as_owner", "S3x2", 1, 15),
          ("fates_tail_as_body", "A6x3", 1, 15), ("export_row_written_when_short", "S3x2", 3, 15),
          ("hash_board_keeps_finished", "S3x2", 1, 15), ("import_refused_row_written", "N10x2_x4", 2, 15),
          ("import_parked_kept", "S3x2", 2, 15), ("causes_by_transposed", "S3x2", 3, 15), ("playout_counts_steps", "S3x2", 2, 15),
          ("outcomes_tracker_not_updated", "N10x2_x4", 1, 15)]


@pytest.mark.parametrize("kind,name,seed,after", FAULTS, ids=[f[0] for f in FAULTS])
def test_an_injected_silent_defect_is_caught(kind, name, seed, after):
    cfg = of.BY_NAME[name]
    ops = of.gen_ops(cfg, seed, cfg["n_ops"])
    bad = of.OracleAdapter(fault=(kind, after))
    with pytest.raises(of.Mismatch) as err:
        of.run(bad, cfg, ops)
    msg = str(err.value)
    assert bad.fault_at is not None and bad.fault_at >= after, "the defect was never injected"
    at = int(re.search(r"differs at op (\d+)", msg).group(1))
    assert bad.fault_at <= at <= len(ops), (bad.fault_at, at, msg)
    assert cfg["name"] in msg and f"seed {seed}" in msg and "first differing env" in msg
    # the replay the message names reproduces it; one op less does not reach it
    if at < len(ops):
        with pytest.raises(of.Mismatch):
            of.run(of.OracleAdapter(fault=(kind, after)), cfg, ops[:at + 1])


def test_a_guard_band_and_an_unselected_row_are_watched():
    """The whole-buffer comparison itself: a byte in a guard band, and a row of an env a masked reset did not select."""
    cfg = of.BY_NAME["S3x2"]
    ops = of.gen_ops(cfg, 2, cfg["n_ops"])     # (a seed whose sequence holds a masked reset with obs that leaves an env out)

    class Scribbler(of.OracleAdapter):
        def __init__(self, where):
            super().__init__()
            self.where = where

        def reset_mask(self, mask, want_obs, want_final, want_trunc):
            out = super().reset_mask(mask, want_obs, want_final, want_trunc)
            if want_obs and self.where == "guard":
                out["obs"][-1] = 0
            if want_obs and self.where == "row" and (mask == 0).any():
                e = int((mask == 0).argmax())
                out["obs"][of.GUARD + e * of.row_bytes(cfg)] = 0
            return out

    with pytest.raises(of.Mismatch, match="guard band of obs"):
        of.run(Scribbler("guard"), cfg, ops)
    with pytest.raises(of.Mismatch, match="untouched"):
        of.run(Scribbler("row"), cfg, ops)


# ---------------------------------------------------------------------------------------------- determinism
def test_the_generator_is_deterministic_and_pinned():
    cfg = of.BY_NAME["A10x2"]
    a, b = of.gen_ops(cfg, 2, cfg["n_ops"]), of.gen_ops(cfg, 2, cfg["n_ops"])
    assert a == b and repr(a) == repr(b)
    assert a != of.gen_ops(cfg, 3, cfg["n_ops"])
    assert hashlib.sha256(repr(a).encode()).hexdigest() == PINNED


PINNED = "efb132d3a0cbad70d2ab41fad2d04e09b7621b5dfc6d2989074cdb3f19855ba4"
