"""Multi-GPU: envs shard by global id, one process per GPU, no data-path collective.

The reference's only parallelism is env-level data parallelism (one SubprocVecEnv worker per
env, src/baselines/common/vec_env/subproc_vec_env.py:31-50; per-env seed = seed + rank,
src/utils.py:39).  Here rank r of W owns the contiguous global env ids shard_range(N, r, W); the
Philox subsequence is the GLOBAL id, so trajectories are identical for every W.  The single
collective is an all-gather of the fixed 4 x int64 episode-statistics record per logging interval
(the epinfobuf aggregation of src/ppo_multi_agent.py:288,331,366-390), RCCL over xGMI on GPUs
(backend "nccl"), gloo on CPU in the tests.
"""


def shard_range(total_envs, rank, world):
    """(first global env id, count) of `rank`'s contiguous shard; counts differ by at most 1."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"bad rank/world {rank}/{world}")
    base, rem = divmod(int(total_envs), world)
    start = rank * base + min(rank, rem)
    return start, base + (1 if rank < rem else 0)


STAT_KEYS = ("episodes", "ep_len_sum", "ep_return_sum", "env_steps")


def gather_stats(local, device=None, group=None):
    """all-gather the per-rank record; returns (list of per-rank dicts, totals dict).

    `local` is MultiSnakeVecEnv.stats() (or any dict with STAT_KEYS).  Without an initialised
    process group this is the single-rank identity."""
    import torch
    import torch.distributed as dist

    live = dist.is_available() and dist.is_initialized()
    backend = str(dist.get_backend(group)) if live else "none"
    if device is None:
        # RCCL ("nccl") moves device tensors only; gloo moves host tensors
        on_gpu = live and "nccl" in backend and torch.cuda.is_available()
        device = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rec = torch.tensor([int(local[k]) for k in STAT_KEYS], dtype=torch.int64, device=device)
    if live:
        world = dist.get_world_size(group)
        out = [torch.zeros_like(rec) for _ in range(world)]
        dist.all_gather(out, rec, group=group)
    else:
        out = [rec]
    per_rank = [dict(zip(STAT_KEYS, (int(x) for x in o.tolist()))) for o in out]
    total = {k: sum(r[k] for r in per_rank) for k in STAT_KEYS}
    total["mean_ep_return"] = total["ep_return_sum"] / max(1, total["episodes"])
    total["mean_ep_len"] = total["ep_len_sum"] / max(1, total["episodes"])
    # where the gathered records lived and what moved them (logging; "cuda:N" + "nccl" = RCCL)
    total["record_device"], total["backend"] = str(out[0].device), backend
    return per_rank, total


_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _i64(x):
    """The 64 bits of x as the int64 that holds them."""
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def _mix64_i64(z):
    """The splitmix64 finaliser on a torch int64 tensor holding 64-bit patterns (products wrap; shifts made logical)."""
    z = (z ^ ((z >> 30) & ((1 << 34) - 1))) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ ((z >> 27) & ((1 << 37) - 1))) * _i64(0x94D049BB133111EB)
    return z ^ ((z >> 31) & ((1 << 33) - 1))


def fingerprint(hashes, env_id_base=0):
    """One order-independent 64-bit number (a Python int in [0, 2^64)) for the per-env hashes of a shard whose first
    env has the global id `env_id_base`: sum_e mix64(hash_e + (env_id_base + e) * 0x9E3779B97F4A7C15) mod 2^64.

    `hashes` is the int64 [n] tensor of MultiSnakeVecEnv.hash_states_device(), on any device; the sum is formed there.
    The fingerprints of the shards of a run add up (mod 2^64) to the fingerprint of the unsharded run, however the envs
    are split, and swapping the hashes of two envs changes it."""
    import torch

    if not isinstance(hashes, torch.Tensor) or hashes.dtype != torch.int64 or hashes.dim() != 1:
        raise ValueError("hashes must be a 1-d int64 tensor (hash_states_device())")
    if isinstance(env_id_base, bool) or not isinstance(env_id_base, int) or env_id_base < 0:
        raise ValueError(f"env_id_base must be a non-negative int, got {env_id_base!r}")
    ids = torch.arange(hashes.shape[0], dtype=torch.int64, device=hashes.device) + _i64(env_id_base)
    return int(_mix64_i64(hashes + ids * _i64(_GOLDEN)).sum().item()) & _M64


def all_fingerprint(env, what="full", device=None, group=None):
    """The fingerprint of a sharded run, the same on every rank and equal to the unsharded run's: every rank forms
    fingerprint(env.hash_states_device(what), env's env_id_base) and the ranks' numbers -- 8 bytes each -- are gathered
    like gather_stats' record and summed mod 2^64.  Without an initialised process group: the single-rank identity."""
    import torch
    import torch.distributed as dist

    local = fingerprint(env.hash_states_device(what), int(env.cfg.env_id_base))
    if not (dist.is_available() and dist.is_initialized()):
        return local
    if device is None:
        on_gpu = "nccl" in str(dist.get_backend(group)) and torch.cuda.is_available()
        device = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    rec = torch.tensor([_i64(local)], dtype=torch.int64, device=device)
    out = [torch.zeros_like(rec) for _ in range(dist.get_world_size(group))]
    dist.all_gather(out, rec, group=group)
    return sum(int(o.item()) for o in out) & _M64


def make_sharded(total_envs, rank=None, world=None, device=None, **kw):
    """MultiSnakeVecEnv for this rank's shard of `total_envs` global envs (env ids stay global).

    rank / world default to torchrun's RANK / WORLD_SIZE; the device defaults to cuda:LOCAL_RANK
    (one process per GPU), so a rank that never called torch.cuda.set_device still lands on its own
    card.  The handle and every buffer of the env live on that device."""
    import os
    from .vec_env import MultiSnakeVecEnv

    rank = int(os.environ.get("RANK", "0")) if rank is None else rank
    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else world
    if device is None:
        device = f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}"
    start, count = shard_range(total_envs, rank, world)
    return MultiSnakeVecEnv(count, env_id_base=start, device=device, **kw)
