"""Diagnostic: device time of copy_envs() (pgx_copy_envs, docs/SPEC.md S19), HIP events on the engine's stream, BASELINE
configs[1] and [2] in one process.  The work: B/8 roots (envs 0, 8, 16, ...) are branched into the 7 other slots of their
group of 8, so 7B/8 pairs per call.  on_target="restart", so that the component tables (12 of the 13 H W map bytes) are
part of the state.  Per configuration, with equal maps (one shared map) and with distinct maps (a random map per env):
    (a)  copy_envs() with no distance-field cache allocated
    (b)  copy_envs(cache=True) with the cache allocated
    (c)  copy_envs(cache=False) with the cache allocated, and (c') the cost_to_go() that follows it
next to
    (s)  save_state() + load_state() of the whole batch, the only route without copy_envs (host clock around both and a
         synchronise: both calls sync the host themselves)
    (m)  one device-to-device copy of as many bytes as (a) / (b) / (c) move, in the same process: the bandwidth
         yardstick; the achieved fraction is (m) / (x)
With distinct maps every repetition first restores the state from a snapshot, outside the timed window: after one copy
the maps of a pair are equal and a second copy would skip them.  The last block times (a) with equal maps at configs[2]'s
shape on 64 x 64 and on 256 x 256 maps: a branch inside one map must not scale with H W.
docs/EXPERIMENTS.md records the numbers.  Needs a GPU.

    python tools/time_copy_envs.py [--reps N] [--warmup N] [--configs 1,2] [--no-big]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0]


def pair_bytes(S, A, r, same_map, cache):
    """Bytes one pair moves (each read once and written once), from the shapes: (state, map, cache rows)."""
    state = 4 * 4 * A + A + 4 + 16 + 4 * A                    # pos, tgt, pos0, tgt0, active, elapsed, macc, tcount
    bmw = (S + 2 * r) * ((S + 2 * r + 31) // 32)
    maps = 0 if same_map else S * S + 4 * bmw + 12 * S * S    # map_u8, obst, comp_begin / _len / _cells
    cell = 2 if S * S <= 65536 else 4
    rows = (4 * A + 4 * S * ((S + 31) // 32) + A * S * S * cell) if cache else 0
    return state, maps, rows


def make(B, S, A, r, shared):
    one = (np.random.default_rng(S).random((S, S)) < 0.2).astype(np.uint8).tolist() if shared else None
    gc = GridConfig(size=S, map=one, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                    on_target="restart", max_episode_steps=10**6)
    env = VecPogema(gc, batch=B)
    env.reset(seed=0)
    return env


def pairs(B, dev):
    dst = torch.tensor([b for b in range(B) if b % 8], dtype=torch.int32, device=dev)
    return (dst // 8 * 8).to(torch.int32), dst


def timed_copy(env, src, dst, reps, warmup, restore, cache, then=None):
    """Median / min us of copy_envs over `reps` (and of `then`, called right after it); `restore` runs before each one."""
    t_copy, t_then = [], []
    for i in range(warmup + reps):
        if restore is not None:
            restore()
        torch.cuda.synchronize()
        us = event_us(lambda: env.copy_envs(src, dst, cache=cache, validate=False))
        us2 = event_us(then) if then is not None else 0.0
        if i >= warmup:
            t_copy.append(us)
            t_then.append(us2)
    return median(t_copy), median(t_then)


def memcpy_us(nbytes, reps, warmup, dev):
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    t = [event_us(lambda: b.copy_(a)) for _ in range(warmup + reps)][warmup:]
    return median(t)


def report(name, t, nbytes, m):
    print(f"  {name:44s} {t[0]:9.1f} ({t[1]:9.1f}) us   {nbytes / 1e6:9.2f} MB moved   same bytes by one device copy "
          f"{m[0]:8.1f} us: {100 * m[0] / t[0]:5.1f} % of it", flush=True)


def run_config(c, args):
    B, S, A, r = CONFIGS[c]
    for shared in (True, False):
        env = make(B, S, A, r, shared)
        dev = env.device
        src, dst = pairs(B, dev)
        n = dst.numel()
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}, {'equal maps' if shared else 'distinct maps'}, {n} pairs, "
              f"{args.reps} reps after {args.warmup} warm-up, median (min):", flush=True)
        snap = env.save_state()
        restore = None if shared else (lambda: env.load_state(snap))
        # (s) the route without copy_envs
        t = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.load_state(env.save_state())
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e6)
        s = median(t[args.warmup:])
        print(f"  {'(s) save_state() + load_state(), host clock':44s} {s[0]:9.1f} ({s[1]:9.1f}) us   "
              f"{2 * snap['engine'].numel() / 1e6:9.2f} MB moved", flush=True)
        state, maps, _ = pair_bytes(S, A, r, shared, False)
        # (a) no cache allocated
        assert env.cost_to_go_builds == 0
        ta, _ = timed_copy(env, src, dst, args.reps, args.warmup, restore, True)
        nb = n * (state + maps)
        report("(a) copy_envs(), no cache allocated", ta, nb, memcpy_us(nb, args.reps, args.warmup, dev))
        print(f"      (s) / (a) = {s[0] / ta[0]:.1f}", flush=True)
        # (b), (c) with the cache
        if restore is not None:
            restore()
        env.cost_to_go()
        rows = pair_bytes(S, A, r, shared, True)[2]
        tb, _ = timed_copy(env, src, dst, args.reps, args.warmup, restore, True)
        nb = n * (state + maps + rows)
        report("(b) copy_envs(cache=True), cache allocated", tb, nb, memcpy_us(nb, args.reps, args.warmup, dev))
        window = torch.empty((B, A, 2 * r + 1, 2 * r + 1), dtype=torch.int32, device=dev)

        def sync_cache():  # the destinations' own state and their own fields again, outside the timed window
            env.load_state(snap)
            env.cost_to_go(out=window)

        tc, tq = timed_copy(env, src, dst, args.reps, args.warmup, sync_cache, False, lambda: env.cost_to_go(out=window))
        nb = n * (state + maps)
        report("(c) copy_envs(cache=False), cache allocated", tc, nb, memcpy_us(nb, args.reps, args.warmup, dev))
        print(f"  {'(c_) the cost_to_go() after (c)':44s} {tq[0]:9.1f} ({tq[1]:9.1f}) us   (c) + (c_) = {tc[0] + tq[0]:.1f} us "
              f"against (b) = {tb[0]:.1f} us", flush=True)
        st = env.get_state()
        assert torch.equal(st["agents_xy"][dst.long()], st["agents_xy"][src.long()])
        env.close()
        del snap, env
        torch.cuda.empty_cache()


def run_big(args):
    B, _, A, r = CONFIGS[2]
    print(f"equal maps, no cache, configs[2]'s shape (B={B}, A={A}) on two map sizes: does a branch scale with H W?", flush=True)
    for S in (64, 256):
        env = make(B, S, A, r, True)
        src, dst = pairs(B, env.device)
        t, _ = timed_copy(env, src, dst, args.reps, args.warmup, None, True)
        state, maps, _ = pair_bytes(S, A, r, True, False)
        full = pair_bytes(S, A, r, False, False)[1]
        print(f"  {S:4d} x {S:<4d} {t[0]:9.1f} ({t[1]:9.1f}) us   {dst.numel() * (state + maps) / 1e6:9.2f} MB moved "
              f"({dst.numel() * full / 1e6:9.2f} MB of map rows skipped)", flush=True)
        env.close()
        del env
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--no-big", action="store_true", help="skip the 64 x 64 against 256 x 256 block")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_copy_envs.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",") if x):
        run_config(c, args)
    if not args.no_big:
        run_big(args)


if __name__ == "__main__":
    main()
