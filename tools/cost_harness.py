"""The timing harness the *_cost.py tools share: a played-in handle, legs captured into HIP graphs and replayed between
events, median / min / max, the check that a leg only read the state, and the JSON on disk.  Each tool keeps its own
legs, arguments and sanity assertions."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def played_env(n, play_steps, masked_reset=False, **kw):
    """(env, acts): a 19x19x3 snake_env handle of n envs (kw changes the constructor's arguments), reset and then
    `play_steps` steps into safe_greedy play; with masked_reset every step is followed by a reset of the done envs (for
    a handle without auto reset).  acts is the int32 [n, n_snakes] buffer the play wrote its actions to."""
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(n, **dict(dict(dim=19, n_snakes=3, rules="snake_env", seed=0), **kw))
    acts = torch.ones((n, env.n_snakes), dtype=torch.int32, device=env.device)
    env.reset_device()
    play(env, acts, play_steps, masked_reset)
    return env, acts


def play(env, acts, steps, masked_reset=False):
    for _ in range(steps):
        _, _, done, _ = env.step_device(env.scripted_actions_device("safe_greedy", out=acts))
        if masked_reset:
            env.reset_device(mask=done)


def timed(fn, calls):
    """HIP-event time of fn() in us per call, fn being `calls` calls."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls


def graph_legs(legs, calls, rounds, restore=None, eager=False):
    """legs: name -> fn.  Every leg is warmed up on a side stream and `calls` back-to-back calls of it are captured into
    one HIP graph; then, `rounds` times, the graphs are replayed in turn.  restore(), if given, runs once behind the
    captures and before every measurement (a leg that moves the state).  eager: each leg is also timed as `calls` calls
    through the Python wrapper.  Returns name -> {"graph_us": [us per call, one per round]} (and "call_us" likewise)."""
    import torch
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in legs.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on a side stream, as graph capture wants
            fn(), fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                fn()
        graphs[name] = g
    restore = restore or (lambda: None)
    times = {k: {"graph_us": [], **({"call_us": []} if eager else {})} for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            restore()
            times[name]["graph_us"].append(timed(graphs[name].replay, calls))
            if eager:
                restore()
                times[name]["call_us"].append(timed(lambda: [fn() for _ in range(calls)], calls))
    restore()
    return times


def med(v):
    return [round(sorted(v)[len(v) // 2], 3), round(min(v), 3), round(max(v), 3)]


def assert_unchanged(env, blob):
    """The handle's state blob is the one taken before the legs, and no kernel reported an error."""
    assert env.get_state_all().tobytes() == bytes(blob) and env.stats()["errors"] == 0


def write_json(res, out):
    """Prints the result; out, if not None, also receives it (its directory is made)."""
    text = json.dumps(res, indent=1)
    if out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    print(text)
