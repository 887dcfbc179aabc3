"""The masked reset as export / reset / import on the CPU oracle, and the truncation flag read off canonical words: what
reset_envs is pinned to by tests/test_oracle_reset_envs.py and, on the device, by tests/test_reset_envs_gpu.py."""
from state_domain import export


def raw_words(ora, e):
    """orc_export_state: the oracle's own words, without the vec layer's `finished` bit."""
    return export(ora, e, finished_bit=False)


def cut_by_time(words, rules, max_steps):
    """The truncation flag of a FINISHED episode from its canonical words: t >= max_steps and the rule set's own end
    condition does not hold ([S]/[A]: the main snake is dead = its body is empty; [N]: its alive bit, done = alive)."""
    k = 8 + 2 * int(words[6])  # snake 0: len, v0, v1, grow_to, alive, in_dead
    ended = bool(words[k + 4]) if rules == "new_world" else int(words[k]) == 0
    return int(words[0]) >= max_steps and not ended


def emulated_masked_reset(ora, mask):
    """The masked reset as the GPU tests emulated it before orc_reset_envs existed: the unselected envs' words are exported,
    every env is reset, and the saved words are imported again; then every row is re-rendered.  (The import drops the
    oracle's `finished`, which its export does not carry: callers of this helper keep that bit themselves.)"""
    keep = {e: raw_words(ora, e) for e in range(ora.num_envs) if not mask[e]}
    ora.reset()
    for e, w in keep.items():
        assert ora.L.orc_import_state(ora.h, e, w.ctypes.data, len(w)) == 0
    return ora.render().copy()
