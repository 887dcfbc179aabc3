"""The oracle against the reference beyond the tapes: configurations and action streams drawn at random (fixed seeds),
every observation byte, reward, done, num_snakes, episode return / length and the full state after every step.  The
reference's side is tests/golden/random_configs.npz, recorded by tools/gen_golden.py (gen_random_configs) running the
reference itself the way the tapes are recorded (source text by path, gym stubbed in memory, the Philox shim injected
as np_random): the actions it chose from the reference's state, the scalars it returned for them, and its observations
and states as one BLAKE2b-256 per configuration with a 32-bit tag after every step (golden_util.feed_step)."""
import hashlib
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, feed_step

FIXTURE = os.path.join(GOLDEN, "random_configs.npz")


def _load():
    with np.load(FIXTURE) as z:
        return json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}


META, REC = _load()


@pytest.mark.parametrize("case", list(enumerate(META["configs"])),
                         ids=lambda ic: f"{['S', 'N', 'A'][ic[1]['rules']]}-{ic[1]['dim']}x{ic[1]['n_snakes']}x"
                                        f"{ic[1]['n_fruits']}-ar{int(ic[1]['auto_reset'])}-eps{ic[1]['eps']}")
def test_oracle_equals_the_running_reference(case):
    from oracle.snake_oracle import Oracle
    i, cfg = case
    ref = {k: v[i] for k, v in REC.items()}
    rules, E, ns = cfg["rules"], cfg["num_envs"], cfg["n_snakes"]
    ora = Oracle(E, dim=cfg["dim"], n_snakes=ns, n_fruits=cfg["n_fruits"], rules=rules, seed=cfg["seed"],
                 env_id_base=cfg["env_id_base"], auto_reset=cfg["auto_reset"])
    h = hashlib.blake2b(digest_size=32)
    states = lambda: [ora.get_state(e) for e in range(E)]  # noqa: E731
    nr = 0
    assert feed_step(h, ora.reset(), states(), rules) == ref["reset_tag"][nr], "reset observation or state"
    for t in range(META["steps"]):
        # eps-greedy walk towards the nearest fruit (eats, long bodies, collisions), with invalid action codes mixed in
        o_obs, o_rew, o_done, o_ns, o_er, o_el = ora.step(ref["actions"][t, :E, :ns].astype(np.int32))
        assert np.array_equal(o_rew, ref["reward"][t, :E]) and np.array_equal(o_done, ref["done"][t, :E]), t
        assert np.array_equal(o_ns, ref["num_snakes"][t, :E]) and np.array_equal(o_er, ref["ep_return"][t, :E]), t
        assert np.array_equal(o_el, ref["ep_len"][t, :E]), t
        assert feed_step(h, o_obs, states(), rules) == ref["tag"][t], f"observation or state differs at step {t}"
        if not cfg["auto_reset"] and t % 25 == 24:  # a bare gym loop resets by hand
            nr += 1
            assert feed_step(h, ora.reset(), states(), rules) == ref["reset_tag"][nr], f"reset after step {t}"
    assert not ref["reset_tag"][nr + 1:].any()
    assert h.digest() == ref["digest"].tobytes(), "observations or states differ from the reference's"
