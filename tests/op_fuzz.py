"""Model-based differential test of every entry point on ONE handle, and of the state two handles hand each other: a
seeded random sequence of operations goes to a handle (and its twin) and to the CPU oracle side by side, and after every
operation everything the operation returns is compared and everything it must leave alone is checked.  Integer and byte
arithmetic throughout: every comparison is bit-exact.

What this is for: the state one kernel leaves in HBM for a DIFFERENT kernel to pick up (parked Philox draws, the
finished bit, the overflow ring's head, chunk 0 of the adversarial fruit list, the persistent kernel's 16-step batches,
the device-side episode totals), a state made on one record policy and continued on the other, a state the copy kernel
wrote (ring rewritten from position 0, parked draws zeroed, totals kept), and a state that changes hands between the
step kernels compiled for the handle's shape and the generic ones.

  gen_ops(cfg, seed, n_ops)  pure host: a list of plain-dict operations, every random choice made (bulk data such as
                             action tensors is named by a seed in the op and derived from it alone)
  run(adapter, cfg, ops)     drives an adapter and two Oracles; ops[:k] replays a failure up to the op where it appeared
  HipAdapter                 the library (msnake.MultiSnakeVecEnv and, for NULL outputs / strides, its C entry points)
  OracleAdapter              the same interface over further Oracles (no GPU needed); fault= injects one silent defect

The twin: the adapter owns a second handle of the same shape (num_envs, dim, n_snakes, n_fruits, rules, max_steps,
auto_reset, obs_scale) that is the neighbouring shard (env_id_base + num_envs) with another seed, the opposite record
policy where the rule set has two, and another envs_per_block (twin_cfg); it is reset once at open.  The driver keeps
a Model for each.  `fork` copies envs between the two with msnake_copy_envs (either direction; the identity, a
permutation, a sparse map with duplicates and negative entries, or one with entries >= num_envs, which the header
defines: untouched, errors + 1), then compares BOTH handles' states in full and both stats().  `swap` exchanges the
roles: everything after it, every older op kind included, runs on the handle the copy kernel last wrote, on its
record policy and launch shape.  `space` (msnake_space_actions) and `cells` (msnake_render_cells) change no state and
go anywhere; their outputs are compared with tests/space_play.py and tests/cells_play.py on the oracle's states.

The entry points added since are wired the same way.  Readers that change no state and go anywhere (READERS): `local`
(msnake_render_local), `rays` (msnake_render_rays), `territory`, `path`, `timed` (msnake_*_actions: a random subset of
their optional outputs, snake bits that may be 0, and greedy columns that drive the next step as `scripted` does),
`heads` (msnake_head_fields), `fates` (msnake_fate_actions; snake_env and adversarial), `export` (msnake_export_states:
the stride words_max, words_max + 3 or one word short of the longest state, whose row then stays untouched), `hash`
(msnake_hash_states, by the header's formula on the oracle's words: state_domain.header_hash).  `causes`
(msnake_death_causes with the main handle as `after` and the twin as `before`, on whatever the two hold), `playout`
(msnake_playout, by playout_play.np_playout with the handle's own seed, env_id_base and max_steps; the handle's blob and
stats() must be what they were) and `outcomes` (msnake_agent_outcomes: the adapter and the driver each own a tracker per
handle, compared whole after every call, and the result is computed from the tracker words, stale or not) move no
handle state either.  `sweep` is one op that calls every applicable reader once; gen_ops places one directly behind the
first op of each writer of state (SWEEP_AFTER).  `import` (msnake_import_states into the main handle) is the one new
writer: rows exported from the twin on the device, the same permuted, the handle's own with the draw counter edited,
or such rows with a few made to be refused for the six reasons of state_domain; a NULL, sparse or full mask; counts NULL,
given, or with entries below 0 and above the stride.  state_domain.accepts says what each env's status must be; an
accepted env is Model.install, anything else stays byte for byte, and the full blob and stats() are compared as `fork`
does.  It shares the pair class C with checkpoint_self and set_words.  Three blocks are placed by construction: arm ->
(copy into the twin) -> step -> (causes) -> outcomes, where the driver also holds the header's guarantee cause != 0 <=>
MSNAKE_AGENT_DIED; rollout -> playout -> import of its end words into the twin -> swap -> step; and a sparse copy with
duplicates -> import with edited counters -> BOARD and FULL hashes.

Entry points not fuzzed, host-only and tested elsewhere: msnake_state_blob_info, msnake_state_words_max (the GPU
adapter holds it against the header's formula), msnake_kernel_name and msnake_kernel_name_for_config (the GPU adapter
asks msnake_kernel_name once at open, as a precondition).

A plain helper module (like scripted_play), imported by tests/test_op_fuzz_host.py and tests/test_op_fuzz_gpu.py.

Every output buffer an adapter hands back is the WHOLE buffer: GUARD bytes of SENT, the payload, GUARD bytes of SENT,
pre-filled with SENT before the call.  The driver builds the same bytes from the oracle (rows an op must not write keep
SENT) and compares all of them, so outputs, untouched rows, surplus action columns and guard bands are one comparison.
"""
import ctypes
import struct

import numpy as np

import agents_play as ap
import causes_play as csp
import cells_play as cp
import fates_play as fp
import heads_play as hp
import local_play as lp
import path_play as pp
import playout_play as plp
import rays_play as rp
import scripted_play as sp
import space_play as spp
import state_domain as sd
import territory_play as tp
import timed_play as tmp

GUARD, SENT = 64, 0xA5
ROLLOUT_STEPS = (1, 2, 15, 16, 17, 31, 32, 33, 48)
INVALID_ACTIONS = (-1, 5, 7)      # as tools/gen_golden.py random_configs mixes them in
OBS_CAP = 400 << 20               # no single observation buffer above this many bytes
READERS = ("local", "rays", "territory", "path", "timed", "heads", "fates", "export", "hash")   # one entry point each, state unchanged
KINDS = ("step", "step_tape", "rollout", "reset_all", "reset_mask", "render", "scripted", "checkpoint_self", "set_words",
         "migrate", "stats", "space", "cells", "fork", "swap") + READERS + ("causes", "playout", "outcomes", "import", "sweep")
# change no state of a handle: go anywhere (outcomes moves its tracker, which only outcomes reads)
QUIET = ("render", "scripted", "stats", "space", "cells") + READERS + ("causes", "playout", "outcomes", "sweep")
SEARCH_KINDS = ("territory", "path", "timed", "heads", "fates", "playout", "causes", "sweep")   # a Python search per env
SWEEP_AFTER = ("fork", "import", "migrate", "rollout", "reset_mask", "set_long")    # the writers a sweep goes directly behind
PAIR_CLASS = {"step": "S", "step_tape": "S", "rollout": "R", "reset_mask": "K", "checkpoint_self": "C", "set_words": "C",
              "import": "C", "migrate": "M", "fork": "F"}   # (swap has no class of its own: it completes the F node in front of it)
LOCAL_RADII = ("1", "2", "5", "dim")
EXPORT_STRIDES = ("max", "max+3", "short")     # words_max, words_max + 3, the longest current count - 1
IMPORT_SOURCES = ("twin", "twin_perm", "self_ctr", "self_refused")
IMPORT_MASKS = ("null", "sparse", "all")
IMPORT_COUNTS = ("null", "given", "given_bad")
STATE_SKIPPED, STATE_OK = 255, 0               # MSNAKE_STATE_SKIPPED, MSNAKE_STATE_OK; the reasons are state_domain's R_*
HASH_WHAT = {"full": 0, "board": 1}            # MSNAKE_HASH_FULL, MSNAKE_HASH_BOARD
PLAYOUT_STEPS = (1, 2, 5, 8)
PLAYOUT_POLICY = {None: 0, "safe_greedy": 1, "hamiltonian": 2, "wary_greedy": 3}
PLAYOUT_OUTPUTS = ("steps", "end", "ret", "info", "words", "count")
AGENT_ARM, AGENT_DIED, AGENT_ENDED = 1, 4, 8   # MSNAKE_AGENT_*
PAIR_CLASSES = "SRKCMF"
FORK_MODES = ("identity", "perm", "sparse", "oob")
FORK_DIRS = ("main<-twin", "twin<-main")
SPEC_SHAPES = ((19, 3), (19, 2), (10, 1))      # boards x snakes the step kernels are compiled for (include/msnake.h)
RULE_NAMES = {0: "snake_env", 1: "new_world", 2: "adversarial"}


# ----------------------------------------------------------------------------------------------- configurations
BIG_N_OPS = 71   # what gen_ops fixes for the batch above 8 192 envs (spine, long-body block, quotas), nothing random on top


def _cfg(name, rules, dim, ns, n, max_steps, auto_reset, scale=1, nf=None, seed=1, base=0, rec="full", epb=0,
         store="auto", n_ops=126, seeds=(1, 2, 3)):
    return dict(name=name, rules=sp.RULES[rules], dim=dim, n_snakes=ns, n_fruits=ns if nf is None else nf, num_envs=n,
                max_steps=max_steps, auto_reset=bool(auto_reset), obs_scale=scale, seed=seed, env_id_base=base,
                tuning=dict(record_policy=rec, envs_per_block=epb, obs_store_policy=store), n_ops=n_ops, seeds=tuple(seeds))


# Between them (not as a cross product): the three rule sets; 1..3 snakes and 4 for new_world; boards 3x3 .. 19x19;
# max_steps 5..12; auto reset on and off; obs_scale 1 and 4; a start on the full and on the short record; batches of
# 1, 130, 257, 333, 777 envs; non-zero env_id_base and seeds with a non-zero high word; one batch above 8 192 envs with
# the launch shape the library picks itself (short record, 4 envs per workgroup) and a short sequence (the minimum that
# holds the quotas of gen_ops); two 19x19 starts on the step kernels compiled for the handle's shape (S10x1 is the third
# compiled shape), with env counts that are no multiple of the 8 envs per workgroup.
CONFIGS = [
    _cfg("S3x2_n1", "snake_env", 3, 2, 1, 5, 1, seed=7, rec="full", epb=1),
    _cfg("S3x2", "snake_env", 3, 2, 130, 6, 0, seed=11, base=5, rec="short", epb=8),
    _cfg("S19x3_x4", "snake_env", 19, 3, 130, 12, 1, scale=4, seed=(3 << 32) | 17, base=1 << 33, rec="short", epb=4),
    _cfg("S12x3", "snake_env", 12, 3, 200, 9, 0, seed=23, base=77, rec="full", epb=2),
    _cfg("S10x1", "snake_env", 10, 1, 777, 8, 1, seed=5, rec="full", epb=8, store="stream"),
    _cfg("A6x3", "adversarial", 6, 3, 333, 7, 0, seed=29, base=4096, rec="full", epb=4),
    _cfg("A10x2", "adversarial", 10, 2, 130, 10, 1, seed=(9 << 32) | 2, rec="short", epb=1),
    _cfg("A19x2_x4", "adversarial", 19, 2, 65, 12, 0, scale=4, seed=31, base=3, rec="short", epb=8, store="plain"),
    _cfg("N6x4", "new_world", 6, 4, 130, 8, 1, nf=9, seed=37, rec="auto", epb=0),
    _cfg("N10x2_x4", "new_world", 10, 2, 100, 10, 0, scale=4, nf=4, seed=(1 << 40) | 41, base=9, rec="auto", epb=2),
    _cfg("N19x3", "new_world", 19, 3, 257, 12, 1, nf=3, seed=43, base=(1 << 32) + 6, rec="auto", epb=8),
    _cfg("S19x3_big", "snake_env", 19, 3, 8201, 10, 1, seed=47, base=12, rec="auto", epb=0, n_ops=BIG_N_OPS, seeds=(1,)),
    _cfg("S19x3_spec", "snake_env", 19, 3, 130, 12, 1, seed=53, rec="full", epb=8, store="plain"),
    _cfg("S19x2_spec", "snake_env", 19, 2, 65, 12, 1, seed=(7 << 32) | 59, base=(1 << 34) + 21, rec="full", epb=8, store="plain"),
]
BY_NAME = {c["name"]: c for c in CONFIGS}


def cases():
    """(cfg, seed) of every run of the GPU file (and so of the host file)."""
    return [(c, s) for c in CONFIGS for s in c["seeds"]]


def twin_cfg(cfg):
    """The configuration of the twin handle: the same shape, the neighbouring shard, another seed, the opposite record
    policy where the rule set has two, another envs_per_block."""
    t = dict(cfg["tuning"])
    if cfg["rules"] != 1:
        t["record_policy"] = "short" if effective_record(cfg, t) == "full" else "full"
    t["envs_per_block"] = {0: 2, 1: 2, 2: 4, 4: 8, 8: 1}[t["envs_per_block"]]
    return dict(cfg, seed=cfg["seed"] ^ 0x5A5A5A5A, env_id_base=cfg["env_id_base"] + cfg["num_envs"], tuning=t)


def compiled_shape(cfg, tuning):
    """The handle of this tuning steps with the kernels compiled for its shape (as msnake_create decides it; the host
    file asks msnake_kernel_name_for_config for the configurations it counts this on)."""
    return (cfg["rules"] == 0 and cfg["obs_scale"] == 1 and cfg["auto_reset"] and (cfg["dim"], cfg["n_snakes"]) in SPEC_SHAPES
            and effective_record(cfg, tuning) == "full")


def effective_record(cfg, tuning):
    """The record a handle of this tuning runs on (msnake_capi.hip: new_world always full; auto = short above 8 192)."""
    if cfg["rules"] == 1:
        return "full"
    if tuning["record_policy"] == "auto":
        return "short" if cfg["num_envs"] > 8192 else "full"
    return tuning["record_policy"]


def long_body_allowed(cfg):
    return cfg["dim"] >= 10       # 100 cells: a body of 66..72 and room for the other snakes and the fruits


def applicable(cfg):
    """The op kinds gen_ops issues for this configuration: what the header refuses (move fates and death causes under
    new_world, playouts off snake_env, causes and outcomes on a handle that resets itself) is left out, and above 8 192
    envs the kinds whose reference is a Python search per env."""
    out = set(KINDS)
    if cfg["rules"] == 1:
        out -= {"fates", "causes"}
    if cfg["rules"] != 0:
        out -= {"playout"}
    if cfg["auto_reset"]:
        out -= {"causes", "outcomes"}
    if cfg["num_envs"] > 8192:
        out -= set(SEARCH_KINDS)
    return out


def domain_cfg(cfg):
    """The configuration as tests/state_domain.py reads it (rules by name)."""
    return dict(rules=RULE_NAMES[cfg["rules"]], dim=cfg["dim"], n_snakes=cfg["n_snakes"], n_fruits=cfg["n_fruits"],
                max_steps=cfg["max_steps"])


def words_max(cfg):
    """msnake_state_words_max as the header states it: 8 + 2 F + n_snakes (6 + 2 (cap - 2))."""
    d = domain_cfg(cfg)
    return 8 + 2 * (sd.fcap(d) if cfg["rules"] == 2 else cfg["n_fruits"]) + cfg["n_snakes"] * (6 + 2 * (sd.cap(d) - 2))


def row_bytes(cfg):
    views = cfg["n_snakes"] if cfg["rules"] == 1 else 3
    return ((cfg["dim"] + 2) * cfg["obs_scale"]) ** 2 * 3 * views


# ----------------------------------------------------------------------------------------------- the generator
def _euler(rng):
    """A closed walk over the six classes of state-changing ops that takes every ordered pair (A, B), A == B included,
    exactly once: 37 nodes (Hierholzer on the complete digraph with loops, edge order shuffled)."""
    k = len(PAIR_CLASSES)
    out_edges = {a: [PAIR_CLASSES[j] for j in rng.permutation(k)] for a in PAIR_CLASSES}
    stack, walk = [PAIR_CLASSES[int(rng.integers(0, k))]], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == k * k + 1
    return walk


class _Gen:
    def __init__(self, cfg, rng, seed=0):
        self.cfg, self.rng = cfg, rng
        self.tuning = dict(cfg["tuning"])                  # of the handle that is main right now
        self.twin_tuning = dict(twin_cfg(cfg)["tuning"])   # ... and of the other one; swap() exchanges them
        self.n_c = self.n_imp = 0
        self.n_ref = 3 * int(seed)       # where the refusal reasons start: over the seeds, every reason also where one row refuses

    def seed(self):
        return int(self.rng.integers(0, 1 << 31))

    def pick(self, seq, p=None):
        return seq[int(self.rng.choice(len(seq), p=p))]

    def stride(self):
        ns = self.cfg["n_snakes"]
        return ns if self.rng.random() < 0.5 else int(self.rng.integers(ns, 8))

    def step(self):
        return dict(kind="step", stride=self.stride(), obs=bool(self.rng.random() < 0.7), seed=self.seed())

    def _obs_fits(self, T):
        return T * self.cfg["num_envs"] * row_bytes(self.cfg) <= OBS_CAP

    def step_tape(self):
        T = int(self.rng.integers(1, 21))
        obs = "all" if self._obs_fits(T) and self.rng.random() < 0.7 else "none"
        return dict(kind="step_tape", n_steps=T, stride=self.stride(), obs=obs, seed=self.seed())

    def rollout(self):
        T = int(self.pick(ROLLOUT_STEPS))
        inplace = bool(self.rng.random() < 0.3)
        modes = ["last", "none"] if inplace or not self._obs_fits(T) else ["all", "all", "last", "none"]
        return dict(kind="rollout", n_steps=T, stride=self.stride(), inplace=inplace, obs=self.pick(modes), seed=self.seed())

    def reset_all(self):
        return dict(kind="reset_all")

    def reset_mask(self):
        r = self.rng
        return dict(kind="reset_mask", p_done=float(self.pick([0.0, 0.5, 1.0, 1.0])), p_mid=float(self.pick([0.0, 0.05, 0.3])),
                    p_fin=float(self.pick([0.0, 0.5, 1.0, 1.0])), obs=bool(r.random() < 0.6), final=bool(r.random() < 0.6),
                    trunc=bool(r.random() < 0.6), seed=self.seed())

    def render(self):
        return dict(kind="render")

    def scripted(self):
        ns, r = self.cfg["n_snakes"], self.rng
        pols = ["safe_greedy", "safe_greedy", None] + (["hamiltonian", "hamiltonian"] if self.cfg["dim"] % 2 == 0 else [])
        pol = self.pick(pols)
        bits = 0 if pol is None else int(r.integers(1, 1 << ns))
        return dict(kind="scripted", policy=pol, snakes=bits, stride=self.stride(),
                    safe=bool(pol is None or r.random() < 0.6), seed=self.seed())

    def checkpoint_self(self):
        return dict(kind="checkpoint_self")

    def set_words(self, edit=None):
        if edit is None:
            edit = self.pick(["ctr", "ctr", "none"])
        return dict(kind="set_words", count=int(self.rng.integers(1, 9)), edit=edit, k=int(self.rng.integers(1, 13)),
                    seed=self.seed())

    def migrate(self):
        cfg, old = self.cfg, self.tuning
        new = dict(old)
        if cfg["rules"] != 1:      # [N] has no short record: it migrates over envs_per_block (and the store policy) only
            new["record_policy"] = "full" if effective_record(cfg, old) == "short" else "short"
        new["envs_per_block"] = int(self.pick([e for e in (1, 2, 4, 8) if e != old["envs_per_block"]]))
        new["obs_store_policy"] = self.pick(["auto", "plain", "stream"])
        op = dict(kind="migrate", tuning=new, keep=bool(self.rng.random() < 0.3),
                  direction=effective_record(cfg, old) + ">" + effective_record(cfg, new))
        self.tuning = new
        return op

    def stats(self):
        return dict(kind="stats", reset=bool(self.rng.random() < 0.4))

    def space(self):
        ns, r = self.cfg["n_snakes"], self.rng
        bits = int(r.integers(0, 1 << ns))
        safe, space = bool(r.random() < 0.5), bool(r.random() < 0.7)
        if bits == 0 and not (safe or space):
            safe, space = bool(r.random() < 0.5), True
        return dict(kind="space", snakes=bits, stride=self.stride(), safe=safe, space=space, seed=self.seed())

    def cells(self):
        nv, r = cp.n_views(self.cfg["rules"], self.cfg["n_snakes"]), self.rng
        how = self.pick(["all", "one", "any", "table"])
        mask = {"all": (1 << nv) - 1, "one": 1 << int(r.integers(0, nv)), "any": int(r.integers(1, 1 << nv)), "table": 0}[how]
        return dict(kind="cells", views=mask, table=bool(mask == 0 or r.random() < 0.5))

    def _flags(self, names, p=0.6, need=True):
        """One random flag per optional output; with `need`, at least one of them is set."""
        out = {k: bool(self.rng.random() < p) for k in names}
        if need and not any(out.values()):
            out[names[int(self.rng.integers(0, len(names)))]] = True
        return out

    def _some_snakes(self):
        return int(self.rng.integers(1, 1 << self.cfg["n_snakes"]))

    def local(self):
        return dict(kind="local", radius=self.pick(LOCAL_RADII), snakes=self._some_snakes(), oriented=int(self.rng.integers(0, 2)),
                    heading=bool(self.rng.random() < 0.7))

    def rays(self):
        return dict(kind="rays", snakes=self._some_snakes(), oriented=int(self.rng.integers(0, 2)), heading=bool(self.rng.random() < 0.7))

    def _counted(self, kind, outs):
        bits = int(self.rng.integers(0, 1 << self.cfg["n_snakes"]))
        return dict(kind=kind, snakes=bits, stride=self.stride(), seed=self.seed(), **self._flags(("safe",) + outs, need=bits == 0))

    def territory(self):
        return self._counted("territory", ("counts",))

    def path(self):
        return self._counted("path", ("dist", "field"))

    def timed(self):
        return self._counted("timed", ("reach", "life"))

    def heads(self):
        return dict(kind="heads", snakes=self._some_snakes(), **self._flags(("dist", "owner", "counts")))

    def fates(self):
        bits = int(self.rng.integers(0, 1 << self.cfg["n_snakes"]))
        return dict(kind="fates", snakes=bits, stride=self.stride(), seed=self.seed(),
                    **self._flags(("fate", "by", "eat", "mask"), need=bits == 0))

    def export(self):
        words, count = self.pick([(True, True), (True, True), (True, False), (False, True)])
        return dict(kind="export", stride=self.pick(EXPORT_STRIDES), words=words, count=count)

    def hash(self):
        return dict(kind="hash", what=self.pick(("full", "board")))

    def causes(self):
        return dict(kind="causes", **self._flags(("cause", "by", "victims", "where")))

    def playout(self, outs=None):
        ns, r = self.cfg["n_snakes"], self.rng
        names = [None, "safe_greedy", "wary_greedy"] + (["hamiltonian"] if self.cfg["dim"] % 2 == 0 else [])
        first = int(r.integers(0, 1 << ns))
        return dict(kind="playout", n_steps=int(self.pick(PLAYOUT_STEPS)), policies=[self.pick(names) for _ in range(ns)], first=first,
                    stride=self.stride() if first else 0, seed=self.seed(), **(outs or self._flags(PLAYOUT_OUTPUTS, 0.5)))

    def outcomes(self):
        arm = bool(self.rng.random() < 0.3)
        return dict(kind="outcomes", arm=arm, **({} if arm else self._flags(("rew", "ate", "flags", "info"))))

    def import_(self, source=None, mask=None, count=None):
        """The first two the generator chooses freely are a plain one (every env taken) and one with a sparse mask; then
        anything.  A refusing import gives the counts (a row can only be too short by its count) and starts its reasons
        one further each time."""
        if source is None:
            self.n_imp += 1
            source = "twin" if self.n_imp <= 2 else self.pick(IMPORT_SOURCES)
            mask = {1: "null", 2: "sparse"}.get(self.n_imp)
        self.n_ref += source == "self_refused"
        count = "given" if source == "self_refused" else count or self.pick(IMPORT_COUNTS)
        return dict(kind="import", source=source, mask=mask or self.pick(IMPORT_MASKS), count=count, pad=int(self.pick((0, 0, 3))),
                    r0=self.n_ref, seed=self.seed())

    def sweep(self, behind):
        """Every applicable reader once, parameters seeded: what a freshly written state looks like to all of them."""
        return dict(kind="sweep", behind=behind, ops=[getattr(self, k)() for k in READERS if k in applicable(self.cfg)])

    def fork(self, form, mode):
        """One F node: fork(main<-twin), or fork(twin<-main) and the swap that makes the written handle the main one."""
        if form == "m":
            return [dict(kind="fork", dir="main<-twin", mode=mode, seed=self.seed())]
        return [dict(kind="fork", dir="twin<-main", mode=mode, seed=self.seed()), self.swap()]

    def swap(self):
        self.tuning, self.twin_tuning = self.twin_tuning, self.tuning
        return dict(kind="swap")

    def of_class(self, c, n_step):
        if c == "S":
            return self.step() if n_step[0] < 3 or self.rng.random() < 0.5 else self.step_tape()
        if c == "C":
            self.n_c += 1
            return (self.import_, self.checkpoint_self, self.set_words)[self.n_c % 3]()
        return {"R": self.rollout, "K": self.reset_mask, "M": self.migrate}[c]()


def gen_ops(cfg, seed, n_ops):
    """The op list of (cfg, seed).  Built so that the coverage conditions of tests/test_op_fuzz_host.py hold by
    construction where they can: a spine that takes every ordered pair of state-changing op classes (cut into segments
    that re-enter on the node they left, so no pair is lost), in which every F node leaves the ACTIVE handle freshly
    written by the copy kernel -- fork(main<-twin), or fork(twin<-main) and a swap; the first of them the latter, so the
    twin first receives played state; the index modes in turn; a stats() behind the first out-of-range fork --, a block
    `set_words(long body) -> fork(twin<-main, identity) + swap -> migrate -> checkpoint_self -> step` where the board
    allows a body over 64 cells, a block `(migrate onto the full record) -> step, rollout, step_tape with stride ==
    n_snakes -> step, rollout with a padded stride` where the start is on the step kernels compiled for the shape, at
    least three ops of every kind (one each of space and cells above 8 192 envs, where the NumPy flood fill costs
    seconds), migrations that flip the record policy of the handle they act on every time -- and random ops (weights
    below) for the rest, in the gaps.  Of the kinds added since: the three blocks of the module docstring, a block
    `import -> step, import -> rollout, import -> reset_mask` whose first import refuses rows, two ops of every
    applicable kind that no sweep holds, and a sweep directly behind the first op of each writer in SWEEP_AFTER (behind
    the swap, for a copy into the twin).  Above 8 192 envs the sequence stays minimal: no kind whose reference is a
    Python search per env (applicable()), no sweep, no import or hash block, one op of each remaining new kind."""
    rng = np.random.default_rng([0x6F70, int(seed), cfg["rules"], cfg["dim"], cfg["n_snakes"], cfg["num_envs"]])
    g = _Gen(cfg, rng, seed)
    walk = _euler(rng)
    cuts = sorted(int(x) for x in rng.choice(np.arange(3, len(walk) - 3), 2, replace=False))
    segments = [walk[:cuts[0] + 1], walk[cuts[0]:cuts[1] + 1], walk[cuts[1]:]]
    n_f = sum(seg.count("F") for seg in segments)
    forms = ["t"] + [("m", "t")[int(j) % 2] for j in rng.permutation(n_f - 1)]      # both directions, the first twin<-main
    modes = [FORK_MODES[int(j)] for j in rng.permutation(4)]
    modes = [modes[j % 4] for j in range(n_f)]                                      # every index mode, in turn
    first_oob = modes.index("oob")
    spec = compiled_shape(cfg, cfg["tuning"])
    few = cfg["num_envs"] > 8192
    app = applicable(cfg)
    n_sweeps = len(SWEEP_AFTER) - (not long_body_allowed(cfg)) if "sweep" in app else 0
    n_fixed = 1 + sum(len(s) for s in segments) + forms.count("t") + 1 + (6 if long_body_allowed(cfg) else 0) + (6 if spec else 0) + \
        (0 if few else 6) + (4 if 1 < cfg["num_envs"] and not few else 0) + (3 if "outcomes" in app else 0) + \
        (2 if "causes" in app else 0) + (5 if "playout" in app else 0) + n_sweeps
    quota = ["render"] * 3 + ["scripted"] * 3 + ["stats"] * 2 + ["reset_all"] * 2 + ["step_tape"] * 3 + ["set_words"] + \
            ["space"] * (1 if few else 3) + ["cells"] * (1 if few else 3)
    # the newer kinds: two of each where they apply (the sweeps add to that), one above 8 192 envs
    # (the five readers whose reference is a Python search per env run in every sweep, five or six times a case)
    quota += [k for k in READERS + ("causes", "playout", "outcomes") if k in app and not (k in SEARCH_KINDS and k in READERS)] * \
        (1 if few else 2)
    quota += ["playout"] * (6 if cfg["num_envs"] < 6 and "playout" in app else 0)    # one env: more playouts, to meet every end
    weights = dict(step=5, step_tape=2, rollout=4, reset_all=1, reset_mask=3, render=1, scripted=3, checkpoint_self=2,
                   set_words=2, migrate=2, stats=1, space=2, cells=2)
    if not cfg["auto_reset"]:     # finished envs step no further: reset them more often
        weights["reset_mask"] = 7
    assert n_ops >= n_fixed + len(quota), (cfg["name"], seed, n_ops, n_fixed + len(quota))
    names = list(weights)
    p = np.array([weights[k] for k in names], float)
    extra = quota + [names[int(i)] for i in rng.choice(len(names), n_ops - n_fixed - len(quota), p=p / p.sum())]
    extra = [extra[int(i)] for i in rng.permutation(len(extra))]
    quiet = [k for k in extra if k in QUIET]
    loud = [k for k in extra if k not in QUIET]                              # go into the gaps between segments
    gaps = [[], [], []]
    for k in loud:
        gaps[int(rng.integers(0, 3))].append(k)
    # the order the ops are MADE in is the order they run in (migrate and swap track the tunings they leave)
    plan, k_f = [], 0
    for seg, gap in zip(segments, gaps):
        for c in seg:
            if c == "F":
                plan.append(("fork", (forms[k_f], modes[k_f], k_f == first_oob)))
                k_f += 1
            else:
                plan.append(("class", c))
        plan += [("kind", k) for k in gap]
        if seg is segments[0] and long_body_allowed(cfg):
            plan += [("long", None)]
        if seg is segments[1] and spec:
            plan += [("spec", None)]
        if seg is segments[0] and cfg["num_envs"] > 1 and not few:
            plan += [("hashes", None)]
        if seg is segments[1] and "outcomes" in app:
            plan += [("agents", None)]
        if seg is segments[2]:
            plan += ([] if few else [("imports", None)]) + ([("playout", None)] if "playout" in app else [])
    for k in quiet:
        plan.insert(int(rng.integers(0, len(plan) + 1)), ("kind", k))
    ops, n_step = [dict(kind="reset_all", gen_seed=int(seed), cfg=cfg["name"])], [0]
    after_f = False                       # the S node behind an F node is a plain step (not a tape)
    unswept = [w for w in SWEEP_AFTER if w != "set_long" or long_body_allowed(cfg)] if n_sweeps else []

    def emit(new):
        """Append ops; the first op of each writer of SWEEP_AFTER gets a sweep directly behind it (behind the swap, for
        a copy into the twin)."""
        for op in new:
            prev = ops[-1]
            ops.append(op)
            tag = {"swap": "fork" if prev["kind"] == "fork" else None, "import": None if op.get("source") == "playout" else "import",
                   "set_words": "set_long" if op.get("edit") == "long" else None}.get(op["kind"], op["kind"])
            if op["kind"] == "fork" and op["dir"] == "twin<-main":
                tag = None            # the handle it wrote becomes main with the swap behind it
            if tag in unswept:
                unswept.remove(tag)
                ops.append(g.sweep(tag))

    for what, arg in plan:
        if what == "class":
            op = g.step() if arg == "S" and after_f else g.of_class(arg, n_step)
            n_step[0] += op["kind"] == "step"
            emit([op])
        elif what == "fork":
            emit(g.fork(arg[0], arg[1]) + ([dict(kind="stats", reset=False)] if arg[2] else []))
        elif what == "long":
            emit([g.set_words(edit="long")] + g.fork("t", "identity") + [g.migrate(), g.checkpoint_self(), g.step()])
        elif what == "spec":      # on the compiled kernels: three stepping ops that run them, two that fall back for the call
            ns = cfg["n_snakes"]
            emit([g.checkpoint_self() if compiled_shape(cfg, g.tuning) else g.migrate()])
            emit([dict(g.step(), stride=ns), dict(g.rollout(), stride=ns), dict(g.step_tape(), stride=ns),
                  dict(g.step(), stride=ns + 2), dict(g.rollout(), stride=ns + 1)])
        elif what == "agents":    # the tracker armed in front of one step; where causes apply, the twin holds that state too
            both = "causes" in app
            emit([dict(kind="outcomes", arm=True)] +
                 ([dict(kind="fork", dir="twin<-main", mode="identity", seed=g.seed())] if both else []) + [g.step()] +
                 ([dict(kind="causes", cause=True, by=True, victims=True, where=True, block=True)] if both else []) +
                 [dict(kind="outcomes", arm=False, rew=True, ate=True, flags=True, info=True, block=both)])
        elif what == "hashes":    # copies of one env that differ in the draw counter alone: equal BOARD, different FULL hashes
            emit([dict(kind="fork", dir="main<-twin", mode="sparse", seed=g.seed()),
                  g.import_("self_ctr", mask="all", count="null"), dict(kind="hash", what="board"), dict(kind="hash", what="full")])
        elif what == "imports":   # an import directly in front of each stepping writer; refusals, a permutation, an edited counter
            small = cfg["num_envs"] < 6      # one reason per refusing row: three such imports give three reasons
            emit([g.import_("self_refused", mask="all"), g.step(),
                  g.import_("self_refused", mask="all") if small else g.import_("twin_perm"), g.rollout(),
                  g.import_("self_refused", mask="all") if small else g.import_("self_ctr"), g.reset_mask()])
        elif what == "playout":   # the import continues the game where the playout ended
            emit([g.rollout(), g.playout(outs=dict(steps=True, end=True, ret=True, info=True, words=True, count=True)),
                  dict(kind="import", source="playout", mask="fits", count="given", pad=0, seed=g.seed()), g.swap(), g.step()])
        else:
            emit([getattr(g, "import_" if arg == "import" else arg)()])
        after_f = what == "fork" or (after_f and what == "kind" and arg in QUIET)
    assert not unswept and len(ops) == n_ops, (unswept, len(ops), n_ops)
    return ops


# ----------------------------------------------------------------------------------------------- shared pieces
def up(frames, k):
    """The fused WarpFrame: integer pixel replication of oracle frames [..., H, W, C] (always a copy)."""
    return frames.copy() if k == 1 else np.repeat(np.repeat(frames, k, axis=-3), k, axis=-2)


def guarded(payload):
    """payload (any dtype / shape) -> the whole buffer as bytes: GUARD x SENT, payload, GUARD x SENT."""
    g = np.full(GUARD, SENT, np.uint8)
    return np.concatenate([g, np.ascontiguousarray(payload).reshape(-1).view(np.uint8), g])


def sent_rows(n, stride):
    """int32 [n, stride] whose every byte is SENT: rows of canonical words as an untouched buffer holds them."""
    return np.full((n, 4 * stride), SENT, np.uint8).view(np.int32)


MASK_CODES = np.array([1, 2, 0x80, 0xFF], np.uint8)     # every non-zero byte selects


def import_mask(op, n):
    """The env mask of an import op: None, every env, or a seeded half with at least one env left out (and one taken,
    where there are two)."""
    if op["mask"] == "null":
        return None
    sel = np.ones(n, bool)
    if op["mask"] == "sparse":
        rs = np.random.default_rng([0x1A95, op["seed"]])
        sel = rs.random(n) < 0.5
        out = int(op["seed"]) % n
        sel[(out + 1) % n] = True
        sel[out] = False
    return np.where(sel, MASK_CODES[np.arange(n) % 4], 0).astype(np.uint8)


def import_order(op, n):
    """Which source row each row of the import holds: the identity, or a seeded permutation."""
    return np.random.default_rng([0x1309, op["seed"]]).permutation(n) if op["source"] == "twin_perm" else np.arange(n)


def import_bad_counts(op, n, stride):
    """{env: count} of the counts an op with count == "given_bad" replaces: below 0 and above the stride, in turn."""
    if op["count"] != "given_bad":
        return {}
    rs = np.random.default_rng([0xBADC, op["seed"]])
    envs = rs.choice(n, min(n, 3), replace=False)
    return {int(e): (-1, stride + 1, -(1 << 31))[j % 3] for j, e in enumerate(envs)}


def refuse(cfg, reason, row, counts, e):
    """Mutate row e (in place) so that state_domain.accepts refuses it for `reason`; heads stay inside the grid."""
    nfr, ns = int(row[6]), cfg["n_snakes"]
    k = 8 + 2 * max(nfr, 0)
    if reason == sd.R_SHORT:
        counts[e] -= 1
    elif reason == sd.R_SNAKES:
        row[7] = (ns + 1) | (int(row[7]) & 0x100)
    elif reason == sd.R_FRUITS:
        row[6] = -1 if cfg["rules"] == 2 else cfg["n_fruits"] + 1
    elif reason == sd.R_CELL:
        if nfr > 0:
            row[8] = cfg["dim"] + 1
        else:
            st = sd.St(row[:counts[e]])        # no fruit in the list (adversarial): the last piece of the first body there is
            s = next((j for j in range(ns) if st.snakes[j]["cells"]), None)
            if s is None:
                row[0] = -1                    # nothing has a cell: R_SCALAR instead
            else:
                row[st.snake_start(s) + 6 + 2 * (len(st.snakes[s]["cells"]) - 1)] = cfg["dim"] + 3
    elif reason == sd.R_LEN:
        row[k] = -1
    elif reason == sd.R_SCALAR:
        row[0] = -1


def import_edit(cfg, op, rows, counts):
    """What the "self_*" sources do to the handle's own exported rows, in place: every other env's draw counter moves on,
    and under "self_refused" a seeded few rows are made to be refused, the six reasons in turn from op["r0"]."""
    n = len(rows)
    for e in range(0, n, 2):
        ctr = ((int(rows[e, 1]) & 0xFFFFFFFF) | (int(rows[e, 2]) & 0xFFFFFFFF) << 32) + 1000 + e
        rows[e, 1], rows[e, 2] = np.array([ctr & 0xFFFFFFFF, (ctr >> 32) & 0xFFFFFFFF], np.uint32).view(np.int32)
    hit = {}
    if op["source"] == "self_refused":
        rs = np.random.default_rng([0x4EF, op["seed"]])
        for j, e in enumerate(sorted(int(x) for x in rs.choice(n, max(1, min(12, n // 4)), replace=False))):
            hit[e] = (op["r0"] + j) % 6 + 1
            refuse(cfg, hit[e], rows[e], counts, e)
    return hit


def import_rows(cfg, op, h, stride):
    """(rows int32 [n, stride], counts int32 [n] or None, mask uint8 [n] or None) of an import op, from the models of
    `h` (the driver or the oracle adapter: .m, .tw and, for the end words of the last playout, .play_end)."""
    n = cfg["num_envs"]
    if op["source"] == "playout":
        words, counts = h.play_end
        rows = sent_rows(n, stride)
        for e, w in enumerate(words):
            rows[e, :len(w)] = w
        counts = np.asarray(counts, np.int32).copy()
        return rows, counts, (counts <= stride).astype(np.uint8)
    src, order = (h.tw if op["source"].startswith("twin") else h.m).all_words(), import_order(op, n)
    rows, counts = np.zeros((n, stride), np.int32), np.zeros(n, np.int32)
    for e in range(n):
        w = src[order[e]]
        rows[e, :len(w)], counts[e] = w, len(w)
    if op["source"].startswith("self"):
        import_edit(cfg, op, rows, counts)
    for e, c in import_bad_counts(op, n, stride).items():
        counts[e] = c
    return rows, (None if op["count"] == "null" else counts), import_mask(op, n)


def import_apply(cfg, model, rows, counts, mask):
    """msnake_import_states on a Model: the status of every env by state_domain.accepts, accepted rows installed."""
    d, (n, stride) = domain_cfg(cfg), rows.shape
    status = np.full(n, STATE_SKIPPED, np.uint8)
    for e in range(n):
        if mask is not None and not mask[e]:
            continue
        c = stride if counts is None else int(counts[e])
        reason = sd.R_SHORT if c < 0 or c > stride else sd.accepts(d, rows[e, :c])
        status[e] = reason or STATE_OK
        if reason is None:
            model.install(e, rows[e, :sd.canonical_len(d, rows[e])])
    return status


def make_actions(cfg, seed, shape):
    """Seeded uniform actions 0..4 with ~2 % invalid codes, int32 of `shape` (.., num_envs, stride)."""
    rs = np.random.default_rng([0xAC7, int(seed)])
    a = rs.integers(0, 5, shape).astype(np.int32)
    bad = rs.random(shape) < 0.02
    a[bad] = np.array(INVALID_ACTIONS, np.int32)[rs.integers(0, 3, int(bad.sum()))]
    return a


def pack_blob(cfg, words):
    """include/msnake.h's state blob (version 2) from one int32 word array per env."""
    off = np.zeros(len(words) + 1, np.uint64)
    off[1:] = np.cumsum([len(w) for w in words])
    head = struct.pack("<IIiiiiiiQ", 0x5453534D, 2, len(words), cfg["dim"], cfg["n_snakes"], cfg["n_fruits"], cfg["rules"], 0,
                       int(off[-1]))
    return np.frombuffer(head + off.tobytes() + np.concatenate(words).astype(np.int32).tobytes(), np.uint8).copy()


def unpack_blob(blob):
    b = np.ascontiguousarray(blob, np.uint8).tobytes()
    magic, version, n = struct.unpack_from("<IIi", b, 0)
    assert magic == 0x5453534D and version == 2, (hex(magic), version)
    total, = struct.unpack_from("<Q", b, 32)
    off = np.frombuffer(b, np.uint64, n + 1, 40).astype(np.int64)
    words = np.frombuffer(b, np.int32, int(total), 40 + 8 * (n + 1))
    assert off[0] == 0 and off[-1] == total and len(b) == 40 + 8 * (n + 1) + 4 * total
    return [words[off[e]:off[e + 1]] for e in range(n)]


def make_oracle(cfg):
    from oracle.snake_oracle import Oracle
    return Oracle(cfg["num_envs"], dim=cfg["dim"], n_snakes=cfg["n_snakes"], n_fruits=cfg["n_fruits"], rules=cfg["rules"],
                  seed=cfg["seed"], env_id_base=cfg["env_id_base"], max_steps=cfg["max_steps"], auto_reset=cfg["auto_reset"])


_MEMO = {}     # (reference, configuration, an env's words) -> what the reference says of that state: Model._memo


class Totals:
    """msnake_get_stats as a model: an episode counts on the step it ends and, while its env stays finished, only once."""

    def __init__(self):
        self.episodes = self.ep_len_sum = self.ep_return_sum = self.env_steps = self.errors = 0

    def count(self, done, fin, er, el):
        new = (done != 0) & ~fin
        self.episodes += int(new.sum())
        self.ep_len_sum += int(el[new].astype(np.int64).sum())
        self.ep_return_sum += int(er[new].astype(np.int64).sum())

    def dict(self):
        return {"episodes": self.episodes, "ep_len_sum": self.ep_len_sum, "ep_return_sum": self.ep_return_sum,
                "env_steps": self.env_steps, "errors": self.errors}


class Model:
    """An Oracle behind the op interface (one per handle: cfg carries the handle's seed and env_id_base): payloads as the library must write them (SENT where it must not write), the
    finished bits and the episode totals -- all from the oracle's outputs alone."""

    def __init__(self, cfg, hook=None):
        self.cfg, self.n, self.ns = cfg, cfg["num_envs"], cfg["n_snakes"]
        self.ora = make_oracle(cfg)
        self.fin = np.zeros(self.n, bool)
        self.totals = Totals()
        self.threads = 8 if self.n >= 2000 else 1
        self.hook = hook                      # called after every single step with (done,) -- coverage counting
        self._buf = np.zeros(256, np.int32)
        self.last_done = np.zeros(self.n, np.uint8)

    def words(self, e):
        L, h = self.ora.L, self.ora.h
        k = L.orc_export_state(h, e, self._buf.ctypes.data, len(self._buf))
        if k > len(self._buf):
            self._buf = np.zeros(2 * k, np.int32)
            k = L.orc_export_state(h, e, self._buf.ctypes.data, len(self._buf))
        w = self._buf[:k].copy()
        if L.orc_finished(h, e):
            w[7] |= 0x100
        return w

    def install(self, e, words):
        w = np.ascontiguousarray(words, np.int32)
        rc = self.ora.L.orc_import_state(self.ora.h, e, w.ctypes.data, len(w))
        assert rc == 0, rc
        self.fin[e] = bool(w[7] & 0x100)

    def state(self, e):
        from oracle.snake_oracle import flat_to_state
        return flat_to_state(self.words(e))

    def reset_all(self):
        obs = self.ora.reset()
        self.fin[:] = False
        return {"obs": up(obs, self.cfg["obs_scale"])}

    def render(self):
        return {"obs": up(self.ora.render(), self.cfg["obs_scale"])}

    def step(self, act, want_obs=True):
        obs, rew, done, ns, er, el = self.ora.step(act, threads=self.threads, want_obs=want_obs)
        self.totals.count(done, self.fin, er, el)
        self.totals.env_steps += self.n
        if self.cfg["auto_reset"]:
            self.fin[done != 0] = False
        else:
            self.fin[done != 0] = True
        info = np.stack([er.view(np.int32), el, ns, done.astype(np.int32)], axis=1).astype(np.int32)
        out = {"rew": rew.copy(), "done": done.copy(), "info": info}
        if want_obs:
            out["obs"] = up(obs, self.cfg["obs_scale"])
        self.last_done = done.copy()
        if self.hook:
            self.hook(done)
        return out

    def tape(self, tape, obs_mode, inplace):
        T = len(tape)
        steps = [self.step(tape[t], obs_mode == "all" or (obs_mode == "last" and t == T - 1)) for t in range(T)]
        out = {k: steps[-1][k] if inplace else np.stack([s[k] for s in steps]) for k in ("rew", "done", "info")}
        if obs_mode == "all":
            out["obs"] = np.stack([s["obs"] for s in steps])
        elif obs_mode == "last":
            out["obs"] = steps[-1]["obs"]
        return out

    def reset_mask(self, mask, want_obs, want_final, want_trunc):
        shape = (self.n,) + self.ora.obs_shape
        obs = np.full(shape, SENT, np.uint8) if want_obs else None
        final = np.full(shape, SENT, np.uint8) if want_final else None
        trunc = np.full(self.n, SENT, np.uint8) if want_trunc else None
        self.ora.reset_envs(mask, obs=obs, final_obs=final, truncated=trunc)
        self.fin[np.asarray(mask) != 0] = False
        out = {}
        if want_obs:
            out["obs"] = up(obs, self.cfg["obs_scale"])
        if want_final:
            out["final"] = up(final, self.cfg["obs_scale"])
        if want_trunc:
            out["trunc"] = trunc
        return out

    def scripted(self, policy, bits, act, want_safe):
        """scripted_play's policies (eps = 0) and the NumPy safe mask on the oracle's canonical states."""
        dim, ns = self.cfg["dim"], self.ns
        states = [self.state(e) for e in range(self.n)]
        out = {}
        if policy is not None:
            pol = sp.POLICIES[policy]
            want = np.array([pol(st, dim, ns, None, 0.0) for st in states], np.int32).reshape(self.n, ns)
            act = act.copy()
            for s in range(ns):
                if bits >> s & 1:
                    act[:, s] = want[:, s]
            out["act"] = act
        if want_safe:
            out["safe"] = np.array([sp.np_safe_mask(st, dim, ns) for st in states], np.uint8).reshape(self.n, ns)
        return out

    def space(self, bits, act, want_safe, want_space):
        """space_play's counts and space_greedy (eps = 0), and the NumPy safe mask, on the oracle's canonical states."""
        dim, ns = self.cfg["dim"], self.ns
        states = [self.state(e) for e in range(self.n)]
        out = {}
        if bits:
            want = np.array([spp.space_greedy(st, dim, ns, None, 0.0) for st in states], np.int32).reshape(self.n, ns)
            act = act.copy()
            for s in range(ns):
                if bits >> s & 1:
                    act[:, s] = want[:, s]
            out["act"] = act
        if want_safe:
            out["safe"] = np.array([sp.np_safe_mask(st, dim, ns) for st in states], np.uint8).reshape(self.n, ns)
        if want_space:
            out["space"] = np.array([spp.np_space(st, dim, ns) for st in states]).astype(np.uint16).reshape(self.n, ns, 4)
        return out

    def cells(self, mask, want_table):
        """cells_play's planes of the selected views (ascending) and its table, on the oracle's canonical states; and
        the header's equivalence claim on every one of these states: decode_frame of the oracle's own frame gives the
        planes of every view."""
        dim, ns, rules = self.cfg["dim"], self.ns, self.cfg["rules"]
        nv = cp.n_views(rules, ns)
        states = [self.state(e) for e in range(self.n)]
        planes = np.stack([cp.np_cells(st, dim, ns, rules, list(range(nv))) for st in states])
        decoded = cp.decode_frame(self.ora.render(), list(range(nv)))
        if not np.array_equal(decoded, planes):
            e = int(np.flatnonzero((decoded != planes).reshape(self.n, -1).any(1))[0])
            raise Mismatch(f"op_fuzz: decode_frame(oracle frame) differs from np_cells in env {e}: state {states[e]}")
        out = {}
        views = [v for v in range(nv) if mask >> v & 1]
        if views:
            out["cells"] = np.ascontiguousarray(planes[:, views])
        if want_table:
            out["table"] = np.stack([cp.np_snake_rows(st, ns) for st in states]).astype(np.int32)
        return out

    # ---- the readers added since: every one on the oracle's canonical states, through the references of tests/*_play.py
    def states(self, words=None):
        from oracle.snake_oracle import flat_to_state
        out = [flat_to_state(w) for w in (self.all_words() if words is None else words)]
        for e in np.flatnonzero(self.fin):
            out[e]["finished"] = True
        return out

    def _memo(self, name, fn, states, words):
        """[fn(state) for every env], each looked up by the env's words first: the references are functions of the state
        alone, the oracle adapter's models hold the states of the driver's, and a sweep asks the same thing twice."""
        head, out = (name, self.cfg["rules"], self.cfg["dim"], self.ns, self.cfg["n_fruits"]), []
        if len(_MEMO) > 400000:
            _MEMO.clear()
        for st, w in zip(states, words):
            key = head + (w.tobytes(),)
            if key not in _MEMO:
                _MEMO[key] = fn(st)
            out.append(_MEMO[key])
        return out

    def _greedy(self, out, bits, act, name, policy, states, words):
        """Columns `bits` of the caller's action rows become the policy's (eps = 0); the others stay."""
        if bits:
            want = np.array(self._memo(name, policy, states, words), np.int32).reshape(self.n, self.ns)
            act = act.copy()
            for s in range(self.ns):
                if bits >> s & 1:
                    act[:, s] = want[:, s]
            out["act"] = act

    def _selected(self, mask):
        return [s for s in range(self.ns) if mask >> s & 1]

    def local(self, radius, mask, oriented, heading):
        win, head = lp.np_local_all(self.states(), self.cfg["dim"], self.ns, self.cfg["rules"], self._selected(mask), radius, oriented)
        return dict({"local": win}, **({"heading": head} if heading else {}))

    def rays(self, mask, oriented, heading):
        rays, head = rp.np_rays_all(self.states(), self.cfg["dim"], self.ns, self.cfg["rules"], self._selected(mask), oriented)
        return dict({"rays": rays}, **({"heading": head} if heading else {}))

    def _counted(self, bits, act, want, policy, outputs):
        dim, ns, words, out = self.cfg["dim"], self.ns, self.all_words(), {}
        states = self.states(words)
        self._greedy(out, bits, act, policy[0], policy[1], states, words)
        if want.get("safe"):
            out["safe"] = np.stack(self._memo("safe", lambda st: sp.np_safe_mask(st, dim, ns), states, words)).astype(np.uint8)
        for flag, (name, fn) in outputs.items():
            if want[flag]:
                out[name] = np.stack([np.asarray(x) for x in self._memo(name, fn, states, words)]).astype(np.uint16)
        return out

    def territory(self, bits, act, want):
        dim, ns = self.cfg["dim"], self.ns
        return self._counted(bits, act, want, ("territory_greedy", lambda st: tp.territory_greedy(st, dim, ns)),
                             {"counts": ("territory", lambda st: tp.territory_sets(st, dim, ns))})

    def path(self, bits, act, want):
        dim, ns = self.cfg["dim"], self.ns
        return self._counted(bits, act, want, ("path_greedy", lambda st: pp.path_greedy(st, dim, ns)),
                             {"dist": ("path", lambda st: pp.np_path(st, dim, ns)), "field": ("field", lambda st: pp.np_field(st, dim))})

    def timed(self, bits, act, want):
        dim, ns, never = self.cfg["dim"], self.ns, tmp.never_pops(self.cfg)
        return self._counted(bits, act, want, ("timed_greedy", lambda st: tmp.timed_greedy(st, dim, ns, never=never)),
                             {"reach": ("reach", lambda st: tmp.np_timed(st, dim, ns, never=never)),
                              "life": ("life", lambda st: tmp.np_life(st, dim, never))})

    def heads(self, mask, want):
        words = self.all_words()
        res = self._memo("heads", lambda st: hp.np_heads(st, self.cfg["dim"], self.ns), self.states(words), words)
        out = {}
        if want["dist"]:
            out["hdist"] = np.stack([r[0][self._selected(mask)] for r in res]).astype(np.uint16)
        if want["owner"]:
            out["owner"] = np.stack([r[1] for r in res]).astype(np.uint8)
        if want["counts"]:
            out["hcounts"] = np.stack([r[2] for r in res]).astype(np.uint16)
        return out

    def fates(self, bits, act, want):
        words, out = self.all_words(), {}
        res = self._memo("fates", lambda st: fp.expected(dict(dim=self.cfg["dim"], n_snakes=self.ns), [st]), self.states(words), words)
        ref = [np.concatenate([r[k] for r in res]) for k in range(5)]
        if bits:
            act = act.copy()
            for s in range(self.ns):
                if bits >> s & 1:
                    act[:, s] = ref[0][:, s]
            out["act"] = act
        for k, name in enumerate(("fate", "by", "eat", "mask")):
            if want[name]:
                out["f" + name] = ref[k + 1]
        return out

    def export(self, stride, want_words, want_count):
        words, out = self.all_words(), {}
        if want_words:
            out["words"] = sent_rows(self.n, stride)
            for e, w in enumerate(words):
                if len(w) <= stride:
                    out["words"][e, :len(w)] = w
        if want_count:
            out["count"] = np.array([len(w) for w in words], np.int32)
        return out

    def hash(self, what):
        return {"hash": np.array([sd.header_hash(w, board=what == "board") for w in self.all_words()], np.int64)}

    def causes(self, before, want):
        """self is `after`, the Model `before` the other handle: the header's formulas on whatever the two hold."""
        res = [csp.np_causes(b, a, self.cfg["dim"]) for b, a in zip(before.states(), self.states())]
        return {"c" + name: np.stack([r[k] for r in res]) for k, name in enumerate(("cause", "by", "victims", "where")) if want[name]}

    def playout(self, n_steps, policies, first_bits, first, want):
        ref = plp.np_playout(self.cfg, self.states(), policies, n_steps, first=first if first_bits else None,
                             first_snakes=self._selected(first_bits))
        out = {"p" + k: ref[k] for k in ("steps", "end", "ret", "info", "count") if want[k]}
        if want["words"]:
            out["pwords"] = sent_rows(self.n, words_max(self.cfg))
            for e, w in enumerate(ref["words"]):
                out["pwords"][e, :len(w)] = w
        return out, ref

    def outcomes(self, track, done, want):
        """msnake_agent_outcomes from the tracker words and the current state, whatever the tracker holds: (outputs, the
        tracker behind the call)."""
        rules, ns = self.cfg["rules"], self.ns
        res, new = [], track.copy()
        for e, now in enumerate(self.states()):
            rows = track[e]
            alive = [bool(a) for a in rows[:, ap.TR_ALIVE]]
            prev = dict(grow_to=[int(g) for g in rows[:, ap.GROW_TO]], alive=alive, snakes=[[0] if a else [] for a in alive])
            r = ap.np_outcomes(prev, now, done[e], rules, rows[:, ap.EP_FRUIT:ap.EP_RETURN + 1])
            res.append(r)
            new[e] = ap.track_rows(now, rules, r[4])
            if done[e]:
                new[e] = 0
                new[e, :, ap.GROW_TO], new[e, :, ap.TR_ALIVE] = 3, 1
        out = {"a" + name: np.stack([r[k] for r in res]) for k, name in enumerate(("rew", "ate", "flags", "info")) if want[name]}
        return out, new

    def armed(self):
        return np.stack([ap.track_rows(st, self.cfg["rules"], ap.zero_totals(self.ns)) for st in self.states()]).astype(np.int32)

    def all_words(self):
        return [self.words(e) for e in range(self.n)]

    def copy_from(self, src_words, idx):
        """msnake_copy_envs on the oracle: export from the source (all of it read first: `src_words`), import here.  The
        totals stay; an entry >= the source's env count leaves the env alone and counts one error."""
        for e, i in enumerate(range(self.n) if idx is None else [int(i) for i in idx]):
            if i >= len(src_words):
                self.totals.errors += 1
            elif i >= 0:
                self.install(e, src_words[i])


# ----------------------------------------------------------------------------------------------- adapters
class OracleAdapter:
    """The adapter interface over a second Oracle.  fault=(kind, min_op): one silent defect, applied to ONE env once, at
    the first suitable op with index >= min_op (self.fault_at then holds that index):
      "ctr_lag"      after a rollout, an env's draw counter is re-installed one lower
      "fruit_moved"  after a migrate, a fruit of one env lies on another free cell
      "fin_dropped"  a checkpoint_self drops the finished bit of one finished env
      "double_count" one finished episode is counted twice in the totals
      "fork_row_shifted"         a fork gives one destination env the state of source index + 1
      "fork_touched_unselected"  a fork changes the draw counter of an env whose index entry is negative
      "fork_totals_copied"       a fork makes the destination's episode total the source's
      "space_off_by_one"         one reachable-space count is one too high
      "cells_head_as_body"       one code 3 (own head) of a plane is 2 (own body)
      "local_shifted"            one window is off by one cell
      "rays_wrong_channel"       one ray reports its own-body distance as another snake's and the reverse
      "territory_off_by_one", "path_off_by_one", "timed_life_off_by_one"   one count / distance / lifetime is one too high
      "heads_owner_tie_as_owner" one tied cell of the owner map goes to snake 0
      "fates_tail_as_body"       one TAIL bit of a fate is reported as BODY
      "export_row_written_when_short"   a row that does not fit the stride is written up to the stride
      "hash_board_keeps_finished"       the BOARD hash of one finished env keeps bit 8 of word 7
      "import_refused_row_written"      an import changes the draw counter of an env whose row it refused
      "import_parked_kept"       an accepted env's next draw is the stale one: its draw counter lags by one
      "causes_by_transposed"     one env's `by` holds the relation from the killer's side
      "playout_counts_steps"     a playout adds its steps to the handle's env_steps
      "outcomes_tracker_not_updated"    one env's tracker rows stay as they were"""

    def __init__(self, fault=None):
        self.fault, self.fault_at, self.op_index = fault, None, -1

    def open(self, cfg):
        self.cfg, self.cfg_tw = cfg, twin_cfg(cfg)      # of the main model and of the twin; swap() exchanges them
        self.m, self.tw = Model(self.cfg), Model(self.cfg_tw)
        self.tw.reset_all()
        self.kept = []
        self.track, self.track_tw = (np.zeros((cfg["num_envs"], cfg["n_snakes"], 8), np.int32) for _ in range(2))
        self.play_end = None

    def _due(self, kind):
        return self.fault and self.fault_at is None and self.fault[0] == kind and self.op_index >= self.fault[1]

    def _wrap(self, out):
        return {k: guarded(v) for k, v in out.items()}

    def reset_all(self):
        return self._wrap(self.m.reset_all())

    def render(self):
        return self._wrap(self.m.render())

    def _after_steps(self, before):
        if self._due("double_count") and self.m.totals.episodes > before:
            self.m.totals.episodes += 1
            self.fault_at = self.op_index

    def step(self, act, want_obs):
        before = self.m.totals.episodes
        out = self._wrap(self.m.step(act, want_obs))
        self._after_steps(before)
        return out

    def tape(self, tape, persistent, obs_mode, inplace):
        before = self.m.totals.episodes
        out = self._wrap(self.m.tape(tape, obs_mode, inplace))
        self._after_steps(before)
        if persistent and self._due("ctr_lag"):
            e = self.cfg["num_envs"] // 2
            w = self.m.words(e)
            ctr = ((int(w[1]) & 0xFFFFFFFF) | (int(w[2]) & 0xFFFFFFFF) << 32) - 1
            w[1], w[2] = np.array([ctr & 0xFFFFFFFF, ctr >> 32], np.uint32).view(np.int32)
            self.m.install(e, w)
            self.fault_at = self.op_index
        return out

    def reset_mask(self, mask, want_obs, want_final, want_trunc):
        return self._wrap(self.m.reset_mask(mask, want_obs, want_final, want_trunc))

    def scripted(self, policy, bits, act, want_safe):
        return self._wrap(self.m.scripted(policy, bits, act, want_safe))

    def space(self, bits, act, want_safe, want_space):
        out = self.m.space(bits, act, want_safe, want_space)
        if want_space and self._due("space_off_by_one") and out["space"].any():
            at = np.flatnonzero(out["space"].reshape(-1))
            out["space"].reshape(-1)[at[len(at) // 2]] += 1
            self.fault_at = self.op_index
        return self._wrap(out)

    def cells(self, mask, want_table):
        out = self.m.cells(mask, want_table)
        if "cells" in out and self._due("cells_head_as_body") and (out["cells"] == 3).any():
            at = np.flatnonzero(out["cells"].reshape(-1) == 3)
            out["cells"].reshape(-1)[at[len(at) // 2]] = 2
            self.fault_at = self.op_index
        return self._wrap(out)

    def _bump(self, fault, arr, ok):
        """A due defect `fault`: the middle one of the entries of `arr` that `ok` marks is one too high."""
        if arr is not None and self._due(fault) and ok.any():
            at = np.flatnonzero(ok.reshape(-1))
            arr.reshape(-1)[at[len(at) // 2]] += 1
            self.fault_at = self.op_index

    def local(self, radius, mask, oriented, heading):
        out = self.m.local(radius, mask, oriented, heading)
        if self._due("local_shifted"):
            win = out["local"].reshape(-1, 2 * radius + 1, 2 * radius + 1)
            moved = [j for j in range(len(win)) if not np.array_equal(np.roll(win[j], 1, axis=1), win[j])]
            if moved:
                j = moved[len(moved) // 2]
                win[j] = np.roll(win[j], 1, axis=1)
                self.fault_at = self.op_index
        return self._wrap(out)

    def rays(self, mask, oriented, heading):
        out = self.m.rays(mask, oriented, heading)
        if self._due("rays_wrong_channel"):
            r = out["rays"].reshape(-1, 4)
            at = np.flatnonzero(r[:, rp.OWN] != r[:, rp.OTHER])
            if len(at):
                j = at[len(at) // 2]
                r[j, rp.OWN], r[j, rp.OTHER] = r[j, rp.OTHER], r[j, rp.OWN]
                self.fault_at = self.op_index
        return self._wrap(out)

    def territory(self, bits, act, want):
        out = self.m.territory(bits, act, want)
        self._bump("territory_off_by_one", out.get("territory"), out.get("territory", np.zeros(1)) != 0)
        return self._wrap(out)

    def path(self, bits, act, want):
        out = self.m.path(bits, act, want)
        self._bump("path_off_by_one", out.get("path"), out.get("path", np.zeros(1)) < pp.NONE - 1)
        return self._wrap(out)

    def timed(self, bits, act, want):
        out = self.m.timed(bits, act, want)
        self._bump("timed_life_off_by_one", out.get("life"), (out.get("life", np.zeros(1)) != 0) & (out.get("life", np.zeros(1)) < tmp.LIFE_CAP))
        return self._wrap(out)

    def heads(self, mask, want):
        out = self.m.heads(mask, want)
        if "owner" in out and self._due("heads_owner_tie_as_owner") and (out["owner"] == hp.OWNER_TIE).any():
            at = np.flatnonzero(out["owner"].reshape(-1) == hp.OWNER_TIE)
            out["owner"].reshape(-1)[at[len(at) // 2]] = 0
            self.fault_at = self.op_index
        return self._wrap(out)

    def fates(self, bits, act, want):
        out = self.m.fates(bits, act, want)
        if "ffate" in out and self._due("fates_tail_as_body") and (out["ffate"] & fp.TAIL).any():
            at = np.flatnonzero(out["ffate"].reshape(-1) & fp.TAIL)
            j = at[len(at) // 2]
            out["ffate"].reshape(-1)[j] = (int(out["ffate"].reshape(-1)[j]) & (0xFF ^ fp.TAIL)) | fp.BODY
            self.fault_at = self.op_index
        return self._wrap(out)

    def export(self, stride, want_words, want_count):
        out = self.m.export(stride, want_words, want_count)
        if want_words and self._due("export_row_written_when_short"):
            words = self.m.all_words()
            short = [e for e, w in enumerate(words) if len(w) > stride]
            if short:
                e = short[len(short) // 2]
                out["words"][e] = words[e][:stride]
                self.fault_at = self.op_index
        return self._wrap(out)

    def hash(self, what):
        out = self.m.hash(what)
        if what == "board" and self._due("hash_board_keeps_finished") and self.m.fin.any():
            e = int(np.flatnonzero(self.m.fin)[len(np.flatnonzero(self.m.fin)) // 2])
            out["hash"][e] = sd.header_hash(self.m.words(e), board=True, clear_finished=False)
            self.fault_at = self.op_index
        return self._wrap(out)

    def causes(self, want):
        out = self.m.causes(self.tw, want)
        if "cby" in out and self._due("causes_by_transposed"):
            by = out["cby"]
            t = np.zeros_like(by)           # bit k of by[s] -> bit s of by[k], in both nibbles
            for s in range(by.shape[1]):
                for k in range(by.shape[1]):
                    t[:, k] |= ((by[:, s] >> k & 1) << s) | ((by[:, s] >> (4 + k) & 1) << (4 + s))
            rows = np.flatnonzero((t != by).any(1))
            if len(rows):
                e = rows[len(rows) // 2]
                by[e] = t[e]
                self.fault_at = self.op_index
        return self._wrap(out)

    def playout(self, n_steps, policies, first_bits, first, want):
        out, ref = self.m.playout(n_steps, policies, first_bits, first, want)
        self.play_end = (ref["words"], ref["count"])
        if self._due("playout_counts_steps"):
            self.m.totals.env_steps += int(ref["steps"].sum()) or 1
            self.fault_at = self.op_index
        return self._wrap(out)

    def outcomes(self, arm, done, want):
        if arm:
            self.track = self.m.armed()
            return {}
        out, new = self.m.outcomes(self.track, done, want)
        if self._due("outcomes_tracker_not_updated") and not np.array_equal(new, self.track):
            e = int(np.flatnonzero((new != self.track).reshape(len(new), -1).any(1))[0])
            new[e] = self.track[e]
            self.fault_at = self.op_index
        self.track = new
        return self._wrap(out)

    def get_track(self):
        return guarded(self.track)

    def import_(self, op):
        """The rows as the driver builds them, from this adapter's own models."""
        into, stride = (self.tw, words_max(self.cfg)) if op["source"] == "playout" else (self.m, words_max(self.cfg) + op["pad"])
        rows, counts, mask = import_rows(self.cfg, op, self, stride)
        before = into.all_words()
        status = import_apply(self.cfg, into, rows, counts, mask)
        if self._due("import_refused_row_written") and ((status != STATE_OK) & (status != STATE_SKIPPED)).any():
            e = int(np.flatnonzero((status != STATE_OK) & (status != STATE_SKIPPED))[0])
            w = before[e].copy()
            w[1] ^= 1
            into.install(e, w)
            self.fault_at = self.op_index
        if self._due("import_parked_kept") and (status == STATE_OK).any():
            e = int(np.flatnonzero(status == STATE_OK)[0])
            w = into.words(e)
            ctr = ((int(w[1]) & 0xFFFFFFFF) | (int(w[2]) & 0xFFFFFFFF) << 32) - 1
            w[1], w[2] = np.array([ctr & 0xFFFFFFFF, (ctr >> 32) & 0xFFFFFFFF], np.uint32).view(np.int32)
            into.install(e, w)
            self.fault_at = self.op_index
        return self._wrap({"status": status})

    def fork(self, to_main, idx):
        dst, src = (self.m, self.tw) if to_main else (self.tw, self.m)
        words, n = src.all_words(), self.cfg["num_envs"]
        plain = np.arange(n) if idx is None else np.asarray(idx, np.int64)
        if self._due("fork_row_shifted"):
            ok = [e for e in range(n) if 0 <= plain[e] < n - 1 and not np.array_equal(words[plain[e]], words[plain[e] + 1])]
            if ok:
                plain = plain.copy()
                plain[ok[len(ok) // 2]] += 1
                self.fault_at = self.op_index
        dst.copy_from(words, plain)
        if idx is not None and self._due("fork_touched_unselected") and (plain < 0).any():
            e = int(np.flatnonzero(plain < 0)[0])
            w = dst.words(e)
            w[1] ^= 1
            dst.install(e, w)
            self.fault_at = self.op_index
        if self._due("fork_totals_copied") and dst.totals.episodes != src.totals.episodes:
            dst.totals.episodes = src.totals.episodes
            self.fault_at = self.op_index

    def swap(self):
        self.m, self.tw = self.tw, self.m
        self.cfg, self.cfg_tw = self.cfg_tw, self.cfg
        self.track, self.track_tw = self.track_tw, self.track

    def get_words(self, e):
        return self.m.words(e)

    def set_words(self, e, words):
        self.m.install(e, words)

    def get_blob(self, twin=False):
        m = self.tw if twin else self.m
        return pack_blob(self.cfg, m.all_words())

    def set_blob(self, blob, _migrating=False):
        words = [w.copy() for w in unpack_blob(blob)]
        if not _migrating and self._due("fin_dropped"):
            fin = [e for e, w in enumerate(words) if w[7] & 0x100]
            if fin:
                words[fin[len(fin) // 2]][7] &= 0xFF
                self.fault_at = self.op_index
        for e, w in enumerate(words):
            self.m.install(e, w)

    def migrate(self, tuning, keep, blob):
        if keep:
            self.kept.append(self.m.totals.dict())
        self.m = Model(self.cfg)
        self.m.reset_all()
        self.set_blob(blob, _migrating=True)
        if self._due("fruit_moved"):
            from oracle.snake_oracle import flat_to_state, state_to_flat
            dim = self.cfg["dim"]
            for e in range(self.cfg["num_envs"]):
                w = self.m.words(e)
                st = flat_to_state(w)
                used = {tuple(c) for b in st["snakes"] for c in b} | {tuple(f) for f in st["fruits"]}
                free = [(x, y) for x in range(dim) for y in range(dim) if (x, y) not in used]
                if st["fruits"] and free:
                    st["fruits"][0] = list(free[len(free) // 2])
                    st["finished"] = bool(w[7] & 0x100)
                    self.m.install(e, state_to_flat(st, self.cfg["n_snakes"]))
                    self.fault_at = self.op_index
                    break

    def stats(self, reset, twin=False):
        m = self.tw if twin else self.m
        out = m.totals.dict()
        if reset:
            m.totals = Totals()
        return out

    def kept_stats(self):
        return list(self.kept)

    def close(self):
        self.m = self.tw = None


class HipAdapter:
    """The library.  Handles come from msnake.MultiSnakeVecEnv; every stream-ordered call goes to the C entry point
    directly (NULL outputs, strides and guarded raw buffers have no face on the Python class), on one stream of the
    adapter's own that is current for everything it does."""

    def __init__(self):
        self.op_index = -1

    def open(self, cfg):
        import torch
        self.torch = torch
        self.cfg, self.cfg_tw = cfg, twin_cfg(cfg)      # of the main handle and of the twin; swap() exchanges them
        self.stream = torch.cuda.Stream()
        self.kept = []
        self.env = self._make(self.cfg, self.cfg["tuning"])
        self.twin = self._make(self.cfg_tw, self.cfg_tw["tuning"])
        for env, c in ((self.env, self.cfg), (self.twin, self.cfg_tw)):
            if compiled_shape(c, c["tuning"]):     # or the case would test the generic kernels twice, silently
                assert env.kernel_name().endswith(f", {c['dim']}>"), env.kernel_name()
        with torch.cuda.stream(self.stream):
            self.twin.reset_device()
            self.track, self.track_tw = (self._put(np.zeros((cfg["num_envs"], cfg["n_snakes"], 8), np.int32)) for _ in range(2))
        self.play_end = None

    def _make(self, c, tuning):
        import msnake
        with self.torch.cuda.stream(self.stream):
            return msnake.MultiSnakeVecEnv(c["num_envs"], dim=c["dim"], n_snakes=c["n_snakes"], n_fruits=c["n_fruits"],
                                           rules=c["rules"], seed=c["seed"], env_id_base=c["env_id_base"],
                                           max_steps=c["max_steps"], auto_reset=c["auto_reset"], obs_scale=c["obs_scale"],
                                           **tuning)

    def _s(self):
        return ctypes.c_void_p(self.stream.cuda_stream)

    def _new(self, nbytes):
        """A SENT-filled device buffer of nbytes + two guard bands; (tensor, pointer to the payload)."""
        t = self.torch.full((int(nbytes) + 2 * GUARD,), SENT, dtype=self.torch.uint8, device=self.env.device)
        return t, t.data_ptr() + GUARD

    def _put(self, arr):
        t = self.torch.from_numpy(guarded(arr)).to(self.env.device)
        return t, t.data_ptr() + GUARD

    def _call(self, name, *args):
        from msnake import _capi
        _capi.check(getattr(self.env._L, name)(self.env._h, *args), name)

    def _back(self, bufs):
        return {k: t.cpu().numpy() for k, (t, _) in bufs.items()}

    def _obs_call(self, name):
        with self.torch.cuda.stream(self.stream):
            bufs = {"obs": self._new(self.cfg["num_envs"] * row_bytes(self.cfg))}
            self._call(name, bufs["obs"][1], self._s())
            return self._back(bufs)

    def reset_all(self):
        return self._obs_call("msnake_reset")

    def render(self):
        return self._obs_call("msnake_render")

    def step(self, act, want_obs):
        n = self.cfg["num_envs"]
        with self.torch.cuda.stream(self.stream):
            a = self._put(act)
            bufs = {"rew": self._new(4 * n), "done": self._new(n), "info": self._new(16 * n)}
            if want_obs:
                bufs["obs"] = self._new(n * row_bytes(self.cfg))
            self._call("msnake_step", a[1], int(act.shape[1]), bufs["obs"][1] if want_obs else None, bufs["rew"][1],
                       bufs["done"][1], bufs["info"][1], self._s())
            return self._back(bufs)

    def tape(self, tape, persistent, obs_mode, inplace):
        n, T = self.cfg["num_envs"], int(tape.shape[0])
        rows = n * row_bytes(self.cfg)
        k = 1 if inplace else T
        with self.torch.cuda.stream(self.stream):
            a = self._put(tape)
            bufs = {"rew": self._new(4 * n * k), "done": self._new(n * k), "info": self._new(16 * n * k)}
            if obs_mode != "none":
                bufs["obs"] = self._new(rows * (T if obs_mode == "all" else 1))
            self._call("msnake_rollout_tape" if persistent else "msnake_step_tape", a[1], int(tape.shape[2]), T,
                       bufs["obs"][1] if obs_mode != "none" else None, rows if obs_mode == "all" else 0, bufs["rew"][1],
                       bufs["done"][1], bufs["info"][1], 0 if inplace else n, self._s())
            return self._back(bufs)

    def reset_mask(self, mask, want_obs, want_final, want_trunc):
        n = self.cfg["num_envs"]
        with self.torch.cuda.stream(self.stream):
            m = self._put(np.ascontiguousarray(mask, np.uint8))
            bufs = {}
            if want_obs:
                bufs["obs"] = self._new(n * row_bytes(self.cfg))
            if want_final:
                bufs["final"] = self._new(n * row_bytes(self.cfg))
            if want_trunc:
                bufs["trunc"] = self._new(n)
            ptr = lambda k: bufs[k][1] if k in bufs else None  # noqa: E731
            self._call("msnake_reset_envs", m[1], ptr("obs"), ptr("final"), ptr("trunc"), self._s())
            return self._back(bufs)

    def scripted(self, policy, bits, act, want_safe):
        from msnake import _capi
        n, ns = self.cfg["num_envs"], self.cfg["n_snakes"]
        with self.torch.cuda.stream(self.stream):
            bufs = {}
            if policy is not None:
                bufs["act"] = self._put(act)
            if want_safe:
                bufs["safe"] = self._new(n * ns)
            self._call("msnake_scripted_actions", _capi.SCRIPTED_POLICY[policy], bits,
                       bufs["act"][1] if policy is not None else None, int(act.shape[1]) if policy is not None else 0,
                       bufs["safe"][1] if want_safe else None, self._s())
            return self._back(bufs)

    def space(self, bits, act, want_safe, want_space):
        n, ns = self.cfg["num_envs"], self.cfg["n_snakes"]
        with self.torch.cuda.stream(self.stream):
            bufs = {}
            if bits:
                bufs["act"] = self._put(act)
            if want_safe:
                bufs["safe"] = self._new(n * ns)
            if want_space:
                bufs["space"] = self._new(2 * n * ns * 4)
            ptr = lambda k: bufs[k][1] if k in bufs else None  # noqa: E731
            self._call("msnake_space_actions", bits, ptr("act"), int(act.shape[1]) if bits else 0, ptr("safe"), ptr("space"),
                       self._s())
            return self._back(bufs)

    def cells(self, mask, want_table):
        n, ns, dim = self.cfg["num_envs"], self.cfg["n_snakes"], self.cfg["dim"]
        with self.torch.cuda.stream(self.stream):
            bufs = {}
            if mask:
                bufs["cells"] = self._new(n * bin(mask).count("1") * dim * dim)
            if want_table:
                bufs["table"] = self._new(4 * n * ns * 8)
            ptr = lambda k: bufs[k][1] if k in bufs else None  # noqa: E731
            self._call("msnake_render_cells", mask, ptr("cells"), ptr("table"), self._s())
            return self._back(bufs)

    def _outs(self, sizes):
        """name -> (tensor, payload pointer) for every output asked for (a size of None: not asked for, the call gets NULL)."""
        return {k: self._new(v) for k, v in sizes.items() if v is not None}

    def local(self, radius, mask, oriented, heading):
        n, p, w = self.cfg["num_envs"], bin(mask).count("1"), 2 * radius + 1
        with self.torch.cuda.stream(self.stream):
            bufs = self._outs({"local": n * p * w * w, "heading": n * p if heading else None})
            self._call("msnake_render_local", radius, mask, oriented, bufs["local"][1], bufs["heading"][1] if heading else None, self._s())
            return self._back(bufs)

    def rays(self, mask, oriented, heading):
        n, p = self.cfg["num_envs"], bin(mask).count("1")
        with self.torch.cuda.stream(self.stream):
            bufs = self._outs({"rays": n * p * 32, "heading": n * p if heading else None})
            self._call("msnake_render_rays", mask, oriented, bufs["rays"][1], bufs["heading"][1] if heading else None, self._s())
            return self._back(bufs)

    def _counted(self, entry, bits, act, sizes):
        """msnake_*_actions(h, snake_mask, actions, stride, <outputs in the order of `sizes`>, stream)."""
        with self.torch.cuda.stream(self.stream):
            bufs = self._outs(sizes)
            if bits:
                bufs["act"] = self._put(act)
            self._call(entry, bits, bufs["act"][1] if bits else None, int(act.shape[1]) if bits else 0,
                       *[bufs[k][1] if k in bufs else None for k in sizes], self._s())
            return self._back(bufs)

    def territory(self, bits, act, want):
        n, ns = self.cfg["num_envs"], self.cfg["n_snakes"]
        return self._counted("msnake_territory_actions", bits, act, {"safe": n * ns if want["safe"] else None,
                                                                      "territory": 8 * n * ns if want["counts"] else None})

    def path(self, bits, act, want):
        n, ns, d2 = self.cfg["num_envs"], self.cfg["n_snakes"], self.cfg["dim"] ** 2
        return self._counted("msnake_path_actions", bits, act, {"safe": n * ns if want["safe"] else None,
                                                                 "path": 8 * n * ns if want["dist"] else None,
                                                                 "field": 2 * n * d2 if want["field"] else None})

    def timed(self, bits, act, want):
        n, ns, d2 = self.cfg["num_envs"], self.cfg["n_snakes"], self.cfg["dim"] ** 2
        return self._counted("msnake_timed_actions", bits, act, {"safe": n * ns if want["safe"] else None,
                                                                  "reach": 8 * n * ns if want["reach"] else None,
                                                                  "life": 2 * n * d2 if want["life"] else None})

    def fates(self, bits, act, want):
        n, ns = self.cfg["num_envs"], self.cfg["n_snakes"]
        return self._counted("msnake_fate_actions", bits, act, {"f" + k: n * ns * (2 if k == "mask" else 5) if want[k] else None
                                                                 for k in ("fate", "by", "eat", "mask")})

    def heads(self, mask, want):
        n, ns, d2 = self.cfg["num_envs"], self.cfg["n_snakes"], self.cfg["dim"] ** 2
        with self.torch.cuda.stream(self.stream):
            bufs = self._outs({"hdist": 2 * n * bin(mask).count("1") * d2 if want["dist"] else None,
                               "owner": n * d2 if want["owner"] else None, "hcounts": 2 * n * ns if want["counts"] else None})
            self._call("msnake_head_fields", mask, *[bufs[k][1] if k in bufs else None for k in ("hdist", "owner", "hcounts")], self._s())
            return self._back(bufs)

    def export(self, stride, want_words, want_count):
        n = self.cfg["num_envs"]
        with self.torch.cuda.stream(self.stream):
            bufs = self._outs({"words": 4 * n * stride if want_words else None, "count": 4 * n if want_count else None})
            self._call("msnake_export_states", bufs["words"][1] if want_words else None, stride if want_words else 0,
                       bufs["count"][1] if want_count else None, self._s())
            return self._back(bufs)

    def hash(self, what):
        with self.torch.cuda.stream(self.stream):
            bufs = self._outs({"hash": 8 * self.cfg["num_envs"]})
            self._call("msnake_hash_states", HASH_WHAT[what], bufs["hash"][1], self._s())
            return self._back(bufs)

    def causes(self, want):
        from msnake import _capi
        n, ns = self.cfg["num_envs"], self.cfg["n_snakes"]
        with self.torch.cuda.stream(self.stream):
            bufs = self._outs({"c" + k: n * ns * (2 if k == "where" else 1) if want[k] else None for k in ("cause", "by", "victims", "where")})
            _capi.check(self.env._L.msnake_death_causes(self.env._h, self.twin._h, *[bufs["c" + k][1] if "c" + k in bufs else None
                                                                                      for k in ("cause", "by", "victims", "where")],
                                                        self._s()), "msnake_death_causes")
            return self._back(bufs)

    def playout(self, n_steps, policies, first_bits, first, want):
        n, ns, wm = self.cfg["num_envs"], self.cfg["n_snakes"], words_max(self.cfg)
        assert wm == self.env.state_words_max, (wm, self.env.state_words_max)
        pol = (ctypes.c_int32 * 4)(*([PLAYOUT_POLICY[p] for p in policies] + [0] * (4 - ns)))
        sizes = dict(psteps=4 * n, pend=n, pret=4 * n * ns, pinfo=16 * n * ns, pwords=4 * n * wm, pcount=4 * n)
        with self.torch.cuda.stream(self.stream):
            bufs = self._outs({k: v if want[k[1:]] else None for k, v in sizes.items()})
            f = self._put(first) if first_bits else None
            self._call("msnake_playout", pol, n_steps, f[1] if f else None, int(first.shape[1]) if f else 0, first_bits,
                       *[bufs[k][1] if k in bufs else None for k in ("psteps", "pend", "pret", "pinfo", "pwords")], wm if want["words"] else 0,
                       bufs["pcount"][1] if want["count"] else None, self._s())
            if want["words"] and want["count"]:
                self.play_end = (bufs["pwords"], bufs["pcount"])      # stay on the device for an import
            return self._back(bufs)

    def outcomes(self, arm, done, want):
        n, ns = self.cfg["num_envs"], self.cfg["n_snakes"]
        with self.torch.cuda.stream(self.stream):
            if arm:
                self._call("msnake_agent_outcomes", AGENT_ARM, self.track[1], None, None, None, None, None, self._s())
                return {}
            d = self._put(np.ascontiguousarray(done, np.uint8))
            bufs = self._outs({"arew": 4 * n * ns if want["rew"] else None, "aate": n * ns if want["ate"] else None,
                               "aflags": n * ns if want["flags"] else None, "ainfo": 16 * n * ns if want["info"] else None})
            self._call("msnake_agent_outcomes", 0, self.track[1], d[1], *[bufs[k][1] if k in bufs else None
                                                                            for k in ("arew", "aate", "aflags", "ainfo")], self._s())
            return self._back(bufs)

    def get_track(self):
        """The whole tracker of the main handle, guard bands included."""
        return self.track[0].cpu().numpy()

    def import_(self, op):
        """msnake_import_states.  The twin's rows go from its msnake_export_states to the import on the device (a
        permutation by index_select there), the end words of a playout stay where the playout wrote them; the handle's
        own rows are edited on the host in between."""
        from msnake import _capi
        torch, n, src = self.torch, self.cfg["num_envs"], op["source"]
        into, stride = (self.twin, words_max(self.cfg)) if src == "playout" else (self.env, words_max(self.cfg) + op["pad"])
        with torch.cuda.stream(self.stream):
            if src == "playout":
                (_, p_words), (t_count, p_count) = self.play_end
                count = t_count[GUARD:GUARD + 4 * n].view(torch.int32)
                mask = (count <= stride).to(torch.uint8)
                p_mask, keep = mask.data_ptr(), (mask,)
            else:
                words = torch.zeros((n, stride), dtype=torch.int32, device=self.env.device)
                count = torch.zeros(n, dtype=torch.int32, device=self.env.device)
                donor = self.twin if src.startswith("twin") else self.env
                _capi.check(donor._L.msnake_export_states(donor._h, words.data_ptr(), stride, count.data_ptr(), self._s()),
                            "msnake_export_states")
                if src == "twin_perm":
                    order = torch.from_numpy(import_order(op, n).astype(np.int64)).to(self.env.device)
                    words, count = words.index_select(0, order).contiguous(), count.index_select(0, order).contiguous()
                if src.startswith("self"):
                    rows, counts = words.cpu().numpy(), count.cpu().numpy()
                    import_edit(self.cfg, op, rows, counts)
                    words, count = torch.from_numpy(rows).to(self.env.device), torch.from_numpy(counts).to(self.env.device)
                for e, c in import_bad_counts(op, n, stride).items():
                    count[e] = c
                m = import_mask(op, n)
                mask = None if m is None else torch.from_numpy(m).to(self.env.device)
                p_words, p_count = words.data_ptr(), None if op["count"] == "null" else count.data_ptr()
                p_mask, keep = None if mask is None else mask.data_ptr(), (words, count, mask)
            bufs = self._outs({"status": n})
            _capi.check(into._L.msnake_import_states(into._h, p_mask, p_words, stride, p_count, bufs["status"][1], self._s()),
                        "msnake_import_states")
            out = self._back(bufs)      # (synchronises: `keep` outlives the launch)
            del keep
            return out

    def fork(self, to_main, idx):
        from msnake import _capi
        dst, src = (self.env, self.twin) if to_main else (self.twin, self.env)
        with self.torch.cuda.stream(self.stream):
            t = None if idx is None else self.torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dst.device)
            _capi.check(dst._L.msnake_copy_envs(dst._h, src._h, None if t is None else t.data_ptr(), self._s()), "msnake_copy_envs")

    def swap(self):
        self.env, self.twin = self.twin, self.env
        self.cfg, self.cfg_tw = self.cfg_tw, self.cfg
        self.track, self.track_tw = self.track_tw, self.track

    def get_words(self, e):
        return self.env.get_state_words(e)

    def set_words(self, e, words):
        self.env.set_state_words(e, words)

    def get_blob(self, twin=False):
        return (self.twin if twin else self.env).get_state_all()

    def set_blob(self, blob):
        self.env.set_state_all(blob)

    def migrate(self, tuning, keep, blob):
        if keep:
            self.kept.append(self.env)
        else:
            self.env.close()
        self.env = self._make(self.cfg, tuning)
        with self.torch.cuda.stream(self.stream):
            self.env.reset_device()        # a fresh handle is reset, then takes the blob (as a checkpoint restore does)
        self.env.set_state_all(blob)

    def stats(self, reset, twin=False):
        return (self.twin if twin else self.env).stats(reset=reset)

    def kept_stats(self):
        return [e.stats() for e in self.kept]

    def close(self):
        self.stream.synchronize()
        for e in self.kept + [self.env, self.twin]:
            e.close()
        self.kept = []


# ----------------------------------------------------------------------------------------------- the driver
class Mismatch(AssertionError):
    pass


def new_cov():
    return dict(kinds={k: 0 for k in KINDS}, migrate_dirs={}, pairs=set(), stepping=0, with_end=0, with_respawn=0,
                rollout_cross16_end=0, wraps=0, long_migrate=0, long_checkpoint=0, fin_across=0, resets_of_finished=0,
                episodes=0, env_steps=0, fork_dirs={d: 0 for d in FORK_DIRS}, fork_modes={m: 0 for m in FORK_MODES},
                fork_dst_finished=0, fork_src_finished=0, fork_src_long=0, stats_saw_errors=0,
                after_fork={"step": 0, "rollout": 0, "reset_mask": 0}, compiled_steps=0, fallback_steps=0,
                to_generic=0, to_compiled=0, reader_on=set(), sweep_after={w: 0 for w in SWEEP_AFTER}, import_status=set(),
                import_after={"step": 0, "rollout": 0, "reset_mask": 0}, import_onto_finished=0, import_long=0,
                playout_ends=set(), playout_blocks=0, causes_blocks=0, causes_nonzero=0, outcomes_armed_died=0,
                outcomes_armed_ended=0, outcomes_stale=0, export_short=0, board_twins=0)


def max_body(words):
    """The longest body of an env's canonical words."""
    k, out = 8 + 2 * int(words[6]), 0
    for _ in range(int(words[7]) & 0xFF):
        out = max(out, int(words[k]))
        k += 6 + 2 * int(words[k])
    return out


class _Driver:
    def __init__(self, adapter, cfg, count):
        self.a, self.cfg, self.count = adapter, cfg, count
        self.n, self.ns = cfg["num_envs"], cfg["n_snakes"]
        self.m = Model(cfg, hook=self._on_step if count else None)             # of the handle that is main right now
        self.tw = Model(twin_cfg(cfg), hook=self._on_step if count else None)  # ... and of the other one
        self.tw.reset_all()
        self.tuning, self.tuning_tw = dict(cfg["tuning"]), dict(twin_cfg(cfg)["tuning"])
        self.prev_kind = None
        self.cov = new_cov()
        self.touched = []                 # envs set_words installed into (most recent last): always in the sample
        self.pending = None               # actions a scripted op filled, for the next step
        self.kept = []
        self.gen_seed = None
        self.prev_class = None
        self.watch = list(range(min(self.n, 128)))   # envs whose draw counter / fruit count is read around every step (coverage)
        self.seen_r = np.zeros(self.n, bool)
        self.seen_c = np.zeros(self.n, bool)
        self.ctr_of, self.ctr_of_tw = {}, {}     # (per handle, like seen_r / seen_c below: they follow a swap)
        self.track, self.track_tw = (np.zeros((self.n, self.ns, 8), np.int32) for _ in range(2))   # the trackers of msnake_agent_outcomes
        self.version, self.track_ver, self.last_loud = 0, None, None    # ops that moved the main handle; when the tracker was written
        self.play_end = self.block_cause = None

    # ---- failure message
    def fail(self, i, op, what, env=None, detail=""):
        c = {k: v for k, v in self.cfg.items() if k not in ("n_ops", "seeds")}
        raise Mismatch(f"op_fuzz: {what} differs at op {i} {op!r}; first differing env {env}; cfg {c}; seed {self.gen_seed}; "
                       f"replay with run(adapter, cfg, gen_ops(cfg, seed, n_ops)[:{i + 1}]) {detail}")

    def eq(self, i, op, got, want, per_env):
        """got: name -> whole buffer (bytes) from the adapter; want: name -> payload from the model; per_env: name ->
        bytes per env row (the first differing env is derived from it)."""
        if set(got) != set(want):
            self.fail(i, op, f"the set of outputs {sorted(got)} vs {sorted(want)}")
        for k in sorted(want):
            w = guarded(want[k])
            g = np.asarray(got[k]).reshape(-1)
            if g.shape != w.shape:
                self.fail(i, op, f"size of {k} ({g.shape} vs {w.shape})")
            if not np.array_equal(g, w):
                at = int(np.flatnonzero(g != w)[0])
                if at < GUARD or at >= len(w) - GUARD:
                    self.fail(i, op, f"guard band of {k} (byte {at - GUARD} of the payload)")
                row = (at - GUARD) // per_env[k]
                self.fail(i, op, k, env=row % self.n, detail=f"(row {row}, byte {(at - GUARD) % per_env[k]}: got {int(g[at])}, "
                          f"want {int(w[at])}; 0x{SENT:X} = untouched)")

    def _sizes(self, stride=0):
        rb = row_bytes(self.cfg)
        return {"obs": rb, "final": rb, "trunc": 1, "rew": 4, "done": 1, "info": 16, "act": 4 * max(stride, 1), "safe": self.ns,
                "space": 8 * self.ns, "cells": 1, "table": 32 * self.ns}

    # ---- coverage hooks (count=True only; numbers of the oracle alone)
    def _ctr(self, e):
        w = self.m.words(e)
        return (int(w[1]) & 0xFFFFFFFF) | (int(w[2]) & 0xFFFFFFFF) << 32

    def _ctr_nf(self, e):
        w = self.m.words(e)
        return (int(w[1]), int(w[2]), int(w[6]))

    def _on_step(self, done):
        ctr = [self._ctr_nf(e) for e in self.watch]
        if any(c != p and not done[e] for e, c, p in zip(self.watch, ctr, self._watch_ctr)):
            self._respawn = True
        self._watch_ctr = ctr
        if done.any():
            self._ended = True

    def _begin_stepping(self):
        self._respawn = self._ended = False
        if self.count:
            self._watch_ctr = [self._ctr_nf(e) for e in self.watch]

    def _end_stepping(self, op):
        cov = self.cov
        cov["stepping"] += 1
        if compiled_shape(self.cfg, self.tuning):     # stride == n_snakes runs compiled, a padded one the generic fallback
            cov["compiled_steps" if self._stride == self.ns else "fallback_steps"] += 1
        if self.prev_kind == "fork" and op["kind"] in cov["after_fork"]:
            cov["after_fork"][op["kind"]] += 1
        if self.prev_kind == "import" and op["kind"] in cov["import_after"]:
            cov["import_after"][op["kind"]] += 1
        cov["with_end"] += self._ended
        cov["with_respawn"] += self._respawn
        if op["kind"] == "rollout" and op["n_steps"] > 16 and self._ended:
            cov["rollout_cross16_end"] += 1

    # ---- ops
    def op_reset_all(self, i, op):
        self.eq(i, op, self.a.reset_all(), self.m.reset_all(), self._sizes())

    def op_render(self, i, op):
        self.eq(i, op, self.a.render(), self.m.render(), self._sizes())

    def op_step(self, i, op):
        if self.pending is not None:
            act, self.pending = self.pending, None
        else:
            act = make_actions(self.cfg, op["seed"], (self.n, op["stride"]))
        self._stride = int(act.shape[1])
        self._begin_stepping()
        want = self.m.step(act, op["obs"])
        self.eq(i, op, self.a.step(act, op["obs"]), want, self._sizes())
        self._end_stepping(op)

    def _tape(self, i, op, persistent):
        tape = make_actions(self.cfg, op["seed"], (op["n_steps"], self.n, op["stride"]))
        inplace = op.get("inplace", False)
        fin_before = self.m.fin.copy()
        self._stride = op["stride"]
        self._begin_stepping()
        want = self.m.tape(tape, op["obs"], inplace)
        self.eq(i, op, self.a.tape(tape, persistent, op["obs"], inplace), want, self._sizes())
        self._end_stepping(op)
        if persistent:
            self.seen_r |= fin_before & self.m.fin

    def op_step_tape(self, i, op):
        self._tape(i, op, False)

    def op_rollout(self, i, op):
        self._tape(i, op, True)

    def op_reset_mask(self, i, op):
        rs = np.random.default_rng([0x3A5C, op["seed"]])
        fin = self.m.fin
        mask = ((self.m.last_done != 0) & (rs.random(self.n) < op["p_done"])) | (~fin & (rs.random(self.n) < op["p_mid"])) | \
               (fin & (rs.random(self.n) < op["p_fin"]))
        mask = np.where(mask, np.array([1, 2, 0x80, 0xFF], np.uint8)[np.arange(self.n) % 4], 0).astype(np.uint8)
        self.cov["resets_of_finished"] += int((fin & (mask != 0)).sum())
        self.cov["after_fork"]["reset_mask"] += self.prev_kind == "fork"
        self.cov["import_after"]["reset_mask"] += self.prev_kind == "import"
        want = self.m.reset_mask(mask, op["obs"], op["final"], op["trunc"])
        self.eq(i, op, self.a.reset_mask(mask, op["obs"], op["final"], op["trunc"]), want, self._sizes())

    def op_scripted(self, i, op):
        act = make_actions(self.cfg, op["seed"], (self.n, op["stride"]))
        want = self.m.scripted(op["policy"], op["snakes"], act, op["safe"])
        self.eq(i, op, self.a.scripted(op["policy"], op["snakes"], act, op["safe"]), want, self._sizes(op["stride"]))
        if op["policy"] is not None:
            self.pending = want["act"]

    def op_space(self, i, op):
        act = make_actions(self.cfg, op["seed"], (self.n, op["stride"]))
        want = self.m.space(op["snakes"], act, op["safe"], op["space"])
        self.eq(i, op, self.a.space(op["snakes"], act, op["safe"], op["space"]), want, self._sizes(op["stride"]))
        if op["snakes"]:
            self.pending = want["act"]

    def op_cells(self, i, op):
        sizes = dict(self._sizes(), cells=bin(op["views"]).count("1") * self.cfg["dim"] ** 2)
        self.eq(i, op, self.a.cells(op["views"], op["table"]), self.m.cells(op["views"], op["table"]), sizes)

    # ---- the readers added since, the tracker, the playout
    def _reader(self, kind):
        t = self.tuning
        self.cov["reader_on"].add((kind, effective_record(self.cfg, t), bool(compiled_shape(self.cfg, t)), t["envs_per_block"]))

    def _act(self, op):
        return make_actions(self.cfg, op["seed"], (self.n, op["stride"]))

    def op_local(self, i, op):
        self._reader("local")
        r = self.cfg["dim"] if op["radius"] == "dim" else int(op["radius"])
        p = bin(op["snakes"]).count("1")
        self.eq(i, op, self.a.local(r, op["snakes"], op["oriented"], op["heading"]),
                self.m.local(r, op["snakes"], op["oriented"], op["heading"]), {"local": p * (2 * r + 1) ** 2, "heading": p})

    def op_rays(self, i, op):
        self._reader("rays")
        p = bin(op["snakes"]).count("1")
        self.eq(i, op, self.a.rays(op["snakes"], op["oriented"], op["heading"]), self.m.rays(op["snakes"], op["oriented"], op["heading"]),
                {"rays": 32 * p, "heading": p})

    def _counted(self, i, op, kind, extra):
        self._reader(kind)
        act = self._act(op)
        want = getattr(self.m, kind)(op["snakes"], act, op)
        self.eq(i, op, getattr(self.a, kind)(op["snakes"], act, op), want, dict(self._sizes(op["stride"]), **extra))
        if op["snakes"]:
            self.pending = want["act"]

    def op_territory(self, i, op):
        self._counted(i, op, "territory", {"territory": 8 * self.ns})

    def op_path(self, i, op):
        self._counted(i, op, "path", {"path": 8 * self.ns, "field": 2 * self.cfg["dim"] ** 2})

    def op_timed(self, i, op):
        self._counted(i, op, "timed", {"reach": 8 * self.ns, "life": 2 * self.cfg["dim"] ** 2})

    def op_fates(self, i, op):
        self._counted(i, op, "fates", {"ffate": 5 * self.ns, "fby": 5 * self.ns, "feat": 5 * self.ns, "fmask": 2 * self.ns})

    def op_heads(self, i, op):
        self._reader("heads")
        d2 = self.cfg["dim"] ** 2
        self.eq(i, op, self.a.heads(op["snakes"], op), self.m.heads(op["snakes"], op),
                {"hdist": 2 * bin(op["snakes"]).count("1") * d2, "owner": d2, "hcounts": 2 * self.ns})

    def op_export(self, i, op):
        self._reader("export")
        longest = max(len(w) for w in self.m.all_words())
        stride = {"max": words_max(self.cfg), "max+3": words_max(self.cfg) + 3, "short": longest - 1}[op["stride"]]
        self.cov["export_short"] += bool(op["words"] and longest > stride)
        self.eq(i, op, self.a.export(stride, op["words"], op["count"]), self.m.export(stride, op["words"], op["count"]),
                {"words": 4 * stride, "count": 4})

    def op_hash(self, i, op):
        self._reader("hash")
        self.eq(i, op, self.a.hash(op["what"]), self.m.hash(op["what"]), {"hash": 8})
        if self.count and not self.cov["board_twins"]:
            full = {}
            for w in self.m.all_words():
                full.setdefault(sd.header_hash(w, board=True), set()).add(sd.header_hash(w))
            self.cov["board_twins"] += any(len(v) > 1 for v in full.values())

    def op_causes(self, i, op):
        self._reader("causes")
        want = self.m.causes(self.tw, op)
        self.eq(i, op, self.a.causes(op), want, {"ccause": self.ns, "cby": self.ns, "cvictims": self.ns, "cwhere": 2 * self.ns})
        if op.get("block"):
            self.cov["causes_blocks"] += 1
            self.cov["causes_nonzero"] += bool(want["ccause"].any())
            self.block_cause = want["ccause"] != 0

    def op_playout(self, i, op):
        self._reader("playout")
        first = self._act(op) if op["first"] else None
        blob, stats = self.a.get_blob(), self.a.stats(False)
        want, ref = self.m.playout(op["n_steps"], op["policies"], op["first"], first, op)
        if op["words"] and op["count"]:
            self.play_end = (ref["words"], ref["count"])
        self.cov["playout_ends"] |= {int(x) for x in ref["end"]}
        ns, wm = self.ns, words_max(self.cfg)
        self.eq(i, op, self.a.playout(op["n_steps"], op["policies"], op["first"], first, op), want,
                {"psteps": 4, "pend": 1, "pret": 4 * ns, "pinfo": 16 * ns, "pwords": 4 * wm, "pcount": 4})
        # the handle is only read: record, rings, parked draws, counters and totals are what they were
        if not np.array_equal(self.a.get_blob(), blob):
            self.fail(i, op, "the handle's state blob before and after the playout")
        if self.a.stats(False) != stats or stats != self.m.totals.dict():
            self.fail(i, op, f"stats() around the playout ({stats}, {self.a.stats(False)}, model {self.m.totals.dict()})")

    def op_outcomes(self, i, op):
        self._reader("outcomes")
        if op["arm"]:
            self.a.outcomes(True, None, op)
            self.track = self.m.armed()
        else:
            # armed: the tracker was written at the state in front of ONE msnake_step, the only thing that has moved the
            # handle since; anything else is a stale tracker, for which the header defines the result all the same
            armed = self.track_ver is not None and self.version == self.track_ver + 1 and self.last_loud == "step"
            done = self.m.last_done
            full, self.track = self.m.outcomes(self.track, done, dict(rew=True, ate=True, flags=True, info=True))
            self.eq(i, op, self.a.outcomes(False, done, op), {k: v for k, v in full.items() if op[k[1:]]},
                    {"arew": 4 * self.ns, "aate": self.ns, "aflags": self.ns, "ainfo": 16 * self.ns})
            died = (full["aflags"] & AGENT_DIED) != 0
            cov = self.cov
            cov["outcomes_armed_died"] += bool(armed and died.any())
            cov["outcomes_armed_ended"] += bool(armed and (full["aflags"] & AGENT_ENDED).any())
            cov["outcomes_stale"] += not armed
            if op.get("block"):      # the header's guarantee for a pair one step apart: cause != 0 <=> MSNAKE_AGENT_DIED
                if not armed:
                    self.fail(i, op, "the causes block (driver error: its tracker is not armed)")
                if not np.array_equal(self.block_cause, died):
                    e = int(np.flatnonzero((self.block_cause != died).any(1))[0])
                    self.fail(i, op, "cause != 0 <=> AGENT_DIED (the header's guarantee, on the oracle's own states)", env=e)
        self.track_ver = self.version
        got = np.asarray(self.a.get_track()).reshape(-1)
        if not np.array_equal(got, guarded(self.track)):
            at = int(np.flatnonzero(got != guarded(self.track))[0]) - GUARD
            self.fail(i, op, "the tracker behind the call", env=at // (32 * self.ns), detail=f"(byte {at} of the tracker)")

    def op_sweep(self, i, op):
        self.cov["sweep_after"][op["behind"]] += self.prev_kind == {"set_long": "set_words"}.get(op["behind"], op["behind"])
        for sub in op["ops"]:
            getattr(self, "op_" + sub["kind"])(i, sub)
            self.cov["kinds"][sub["kind"]] += 1

    def op_import(self, i, op):
        into, stride = (self.tw, words_max(self.cfg)) if op["source"] == "playout" else (self.m, words_max(self.cfg) + op["pad"])
        rows, counts, mask = import_rows(self.cfg, op, self, stride)
        before, fin = into.all_words(), into.fin.copy()
        status = import_apply(self.cfg, into, rows, counts, mask)
        after = into.all_words()
        for e in np.flatnonzero(status != STATE_OK):
            if not np.array_equal(after[e], before[e]):
                self.fail(i, op, "the model's own import (driver error)", env=int(e))
        ok = status == STATE_OK
        cov = self.cov
        cov["import_status"] |= {int(x) for x in status}
        cov["import_onto_finished"] += int((fin & ok).any())
        cov["import_long"] += int(any(max_body(after[e]) > 64 for e in np.flatnonzero(ok)))
        cov["playout_blocks"] += op["source"] == "playout"
        self.eq(i, op, self.a.import_(op), {"status": status}, {"status": 1})
        twin = op["source"] == "playout"
        self._words_fail(i, op, "the handle the import wrote", self.a.get_blob(twin=twin), after)
        for tw, m in ((False, self.m), (True, self.tw)):
            got = self.a.stats(False, twin=tw)
            if got != m.totals.dict():
                self.fail(i, op, f"stats() of the {'twin' if tw else 'main'} handle after the import ({got} vs {m.totals.dict()})")
        c = self.ctr_of_tw if twin else self.ctr_of
        for e in np.flatnonzero(ok):
            c.pop(int(e), None)
        if not twin:
            self.seen_r[ok] = False
            self.seen_c[ok] = False

    def _fork_index(self, op):
        """None (the identity), a permutation, a random map with duplicates, unused sources and at least n / 8 negative
        entries, or such a map with a few entries >= num_envs."""
        n, mode = self.n, op["mode"]
        rs = np.random.default_rng([0xF02C, op["seed"]])
        if mode == "identity":
            return None
        if mode == "perm":
            return rs.permutation(n).astype(np.int32)
        idx = rs.integers(-1, n, n).astype(np.int64)
        idx[rs.choice(n, min(n, max(2, n // 8)) if n > 1 else int(rs.integers(0, 2)), replace=False)] = -1
        if mode == "oob":
            at = rs.choice(n, min(n, 3), replace=False)
            idx[at] = np.array([n, n + 1, 2**31 - 1], np.int64)[:len(at)]
        return idx.astype(np.int32)

    def _words_fail(self, i, op, what, got_blob, want):
        got = unpack_blob(got_blob)
        if len(got) != len(want):
            self.fail(i, op, f"num_envs of the blob of {what} ({len(got)})")
        for e, (g, w) in enumerate(zip(got, want)):
            if not np.array_equal(g, w):
                self.fail(i, op, f"state of {what} after the copy", env=e, detail=f"got words {list(g)[:40]} want {list(w)[:40]}")

    def op_fork(self, i, op):
        to_main = op["dir"] == "main<-twin"
        dst, src = (self.m, self.tw) if to_main else (self.tw, self.m)
        idx = self._fork_index(op)
        s0, d0 = src.all_words(), dst.all_words()
        plain = np.arange(self.n) if idx is None else idx.astype(np.int64)
        sel = (plain >= 0) & (plain < self.n)
        cov = self.cov
        cov["fork_dirs"][op["dir"]] += 1
        cov["fork_modes"][op["mode"]] += 1
        cov["fork_dst_finished"] += int((dst.fin & sel).any())
        cov["fork_src_finished"] += int(src.fin[plain[sel]].any())
        cov["fork_src_long"] += int(any(max_body(s0[j]) > 64 for j in set(plain[sel].tolist())))
        # the header's three statements, from the words of BEFORE the call: selected destination envs hold the source's,
        # the others (negative and out-of-range entries) their own, and the source is unchanged
        want = [s0[j] if ok else d0[e] for e, (j, ok) in enumerate(zip(plain.tolist(), sel.tolist()))]
        dst.copy_from(s0, plain)
        for e, w in enumerate(dst.all_words()):
            if not np.array_equal(w, want[e]):
                self.fail(i, op, "the model's own copy (driver error)", env=e)
        self.a.fork(to_main, idx)
        self._words_fail(i, op, "the destination (" + ("main" if to_main else "twin") + ")", self.a.get_blob(twin=not to_main), want)
        self._words_fail(i, op, "the source (" + ("twin" if to_main else "main") + ")", self.a.get_blob(twin=to_main), s0)
        for twin, m in ((False, self.m), (True, self.tw)):
            got = self.a.stats(False, twin=twin)
            if got != m.totals.dict():
                self.fail(i, op, f"stats() of the {'twin' if twin else 'main'} handle after the copy ({got} vs {m.totals.dict()})")
        # coverage bookkeeping follows the states: what was watched on a source env is watched on its copies
        c_dst, c_src = (self.ctr_of, self.ctr_of_tw) if to_main else (self.ctr_of_tw, self.ctr_of)
        moved = {e: int(j) for e, (j, ok) in enumerate(zip(plain.tolist(), sel.tolist())) if ok}
        new = {e: c_src[j] for e, j in moved.items() if j in c_src}
        for e in moved:
            c_dst.pop(e, None)
        c_dst.update(new)
        if to_main:
            self.seen_r[sel] = False
            self.seen_c[sel] = False

    def op_swap(self, i, op):
        self.a.swap()
        was = compiled_shape(self.cfg, self.tuning)
        self.m, self.tw = self.tw, self.m
        self.tuning, self.tuning_tw = self.tuning_tw, self.tuning
        self.ctr_of, self.ctr_of_tw = self.ctr_of_tw, self.ctr_of
        self.track, self.track_tw, self.track_ver = self.track_tw, self.track, None
        self.seen_r[:] = False
        self.seen_c[:] = False
        self._hand_over(was)

    def _hand_over(self, was):
        now = compiled_shape(self.cfg, self.tuning)
        self.cov["to_generic"] += was and not now
        self.cov["to_compiled"] += now and not was

    def _check_blob(self, i, op, blob):
        words = unpack_blob(blob)
        if len(words) != self.n:
            self.fail(i, op, f"num_envs of the blob ({len(words)})")
        for e in range(self.n):
            if not np.array_equal(words[e], self.m.words(e)):
                self._state_fail(i, op, e, words[e], "state blob")

    def op_checkpoint_self(self, i, op):
        blob = self.a.get_blob()
        self._check_blob(i, op, blob)
        self.a.set_blob(blob)
        self._check_blob(i, op, self.a.get_blob())     # every env, finished bits included, as the restore left them
        self.seen_c |= self.m.fin
        self.cov["long_checkpoint"] += self._long_touched()

    def op_migrate(self, i, op):
        got = self.a.stats(False)
        if got != self.m.totals.dict():
            self.fail(i, op, f"stats() before the migration ({got} vs {self.m.totals.dict()})")
        blob = self.a.get_blob()
        self._check_blob(i, op, blob)
        if op["keep"]:
            self.kept.append(self.m.totals.dict())
        self.a.migrate(op["tuning"], op["keep"], blob)
        self._check_blob(i, op, self.a.get_blob())
        self.m.totals = Totals()
        was = compiled_shape(self.cfg, self.tuning)
        self.tuning = dict(op["tuning"])
        self._hand_over(was)
        d = op["direction"]
        self.cov["migrate_dirs"][d] = self.cov["migrate_dirs"].get(d, 0) + 1
        self.cov["long_migrate"] += self._long_touched()

    def op_stats(self, i, op):
        got, want = self.a.stats(op["reset"]), self.m.totals.dict()
        if got != want:
            self.fail(i, op, f"stats() ({got} vs the model {want})")
        self.cov["stats_saw_errors"] += want["errors"] > 0
        if op["reset"]:
            self.cov["episodes"] += want["episodes"]
            self.cov["env_steps"] += want["env_steps"]
            self.m.totals = Totals()

    def _long_touched(self):
        return int(any(max(len(b) for b in self.m.state(e)["snakes"]) > 64 for e in self.touched[-16:]))

    def _long_state(self, e, st, rs):
        """The env's state with snake 0 laid along a boustrophedon path as a body of 66..72 cells, head last on the path."""
        dim, ns = self.cfg["dim"], self.ns
        L = int(rs.integers(66, 73))
        path = []
        for y in range(dim):
            path += [(x, y) for x in (range(dim) if y % 2 == 0 else range(dim - 1, -1, -1))]
        body = [list(c) for c in reversed(path[:L])]
        free = path[L + 2:]
        n_fr = min(len(st["fruits"]), len(free) - (ns - 1))
        pick = [free[int(j)] for j in rs.choice(len(free), (ns - 1) + n_fr, replace=False)]
        st = dict(st)
        st["snakes"] = [body] + [[list(pick[s])] for s in range(ns - 1)]
        st["vels"] = [[body[0][0] - body[1][0], body[0][1] - body[1][1]]] + [[1, 0]] * (ns - 1)
        st["grow_to"] = [L + int(rs.integers(0, 3))] + [1] * (ns - 1)
        st["alive"], st["in_dead"] = [True] * ns, [False] * ns
        st["fruits"] = [list(pick[ns - 1 + f]) for f in range(n_fr)]
        st["t"], st["ep_len"], st["ep_return"] = 1, 1, 0.0
        return st

    def op_set_words(self, i, op):
        from oracle.snake_oracle import state_to_flat
        rs = np.random.default_rng([0x5E7, op["seed"]])
        envs = sorted(int(e) for e in rs.choice(self.n, min(self.n, op["count"]), replace=False))
        for j, e in enumerate(envs):
            got, want = self.a.get_words(e), self.m.words(e)
            if not np.array_equal(got, want):
                self._state_fail(i, op, e, got, "get_state before set_words")
            edit = op["edit"] if j % 2 == 0 else "none"    # every other env: its own words go back in unchanged
            if edit != "none":
                st = self.m.state(e)
                if edit == "ctr":
                    st["ctr"] = (1 << 32) - (op["k"] + j)    # the wrap comes a few draws later
                else:
                    st = self._long_state(e, st, rs)
                st["finished"] = bool(want[7] & 0x100) and edit == "ctr"
                want = state_to_flat(st, self.ns)
            self.m.install(e, want)
            self.a.set_words(e, want)
            self.ctr_of[e] = self._ctr(e)
            if e in self.touched:
                self.touched.remove(e)
            self.touched.append(e)

    # ---- state checks
    def _state_fail(self, i, op, e, got, what):
        from oracle.snake_oracle import flat_finished, flat_to_state
        try:
            g = (flat_to_state(got), flat_finished(got))
        except Exception:  # noqa: BLE001
            g = list(got)
        self.fail(i, op, what, env=e, detail=f"got {g} want {(self.m.state(e), bool(self.m.fin[e]))}")

    def check_states(self, i, op, every=False):
        if every:
            envs = range(self.n)
        else:
            rs = np.random.default_rng([0x57A7E, i])
            envs = sorted(set(int(e) for e in rs.choice(self.n, min(self.n, 8), replace=False)) | set(self.touched[-16:]))
        for e in envs:
            want = self.m.words(e)
            if bool(want[7] & 0x100) != bool(self.m.fin[e]):
                self.fail(i, op, "the model's own finished bit (driver error)", env=e)
            got = self.a.get_words(e)
            if not np.array_equal(got, want):
                self._state_fail(i, op, e, got, "canonical state / finished bit")
        for e in list(self.ctr_of):        # 2^32 wraps of the counters set_words moved close to it
            now = self._ctr(e)
            if self.ctr_of[e] < (1 << 32) <= now:
                self.cov["wraps"] += 1
            self.ctr_of[e] = now

    def play(self, ops):
        self.gen_seed = ops[0].get("gen_seed") if ops else None
        self.a.open(self.cfg)
        i, op = -1, None
        for i, op in enumerate(ops):
            self.a.op_index = i
            kind = op["kind"]
            getattr(self, "op_" + kind)(i, op)
            self.cov["kinds"][kind] += 1
            cls = PAIR_CLASS.get(kind)
            if cls:
                if self.prev_class:
                    self.cov["pairs"].add(self.prev_class + cls)
                self.prev_class = cls
            elif kind == "reset_all":
                self.prev_class = None
            if kind not in QUIET + ("swap",):   # (what the next stepping op follows)
                self.prev_kind = kind
            if kind not in QUIET and not (kind == "fork" and op["dir"] == "twin<-main") and op.get("source") != "playout":
                self.version, self.last_loud = self.version + 1, kind
            self.seen_r &= self.m.fin
            self.seen_c &= self.m.fin
            self.cov["fin_across"] = max(self.cov["fin_across"], int((self.seen_r & self.seen_c).sum()))
            self.check_states(i, op)
        end = dict(kind="end of sequence")
        self.a.op_index = len(ops)
        self.check_states(len(ops), end, every=True)
        got, want = self.a.stats(False), self.m.totals.dict()
        if got != want:
            self.fail(len(ops), end, f"stats() ({got} vs the model {want})")
        self.cov["episodes"] += want["episodes"]
        self.cov["env_steps"] += want["env_steps"]
        self._words_fail(len(ops), end, "the twin", self.a.get_blob(twin=True), self.tw.all_words())
        got, want = self.a.stats(False, twin=True), self.tw.totals.dict()
        if got != want:
            self.fail(len(ops), end, f"stats() of the twin ({got} vs the model {want})")
        got = self.a.kept_stats()
        if got != self.kept:
            self.fail(len(ops), end, f"stats() of the handles kept open after a migration ({got} vs {self.kept})")


def run(adapter, cfg, ops, count=True):
    """Drive `adapter` (its handle and the twin) and two Oracles through `ops` side by side (ops[:k] of a generated list is as good as the list).
    Raises Mismatch (an AssertionError) at the first difference; returns the coverage counters (count=False skips the
    ones that cost per-step reads of the oracle)."""
    d = _Driver(adapter, cfg, count)
    try:
        d.play(ops)
    finally:
        try:
            adapter.close()
        except Exception:  # noqa: BLE001  (a failed open leaves nothing to close)
            pass
    return d.cov
