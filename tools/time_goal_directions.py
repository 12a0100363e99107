"""Diagnostic: device time of goal_directions() (pgx_goal_directions) in its three formats next to cost_to_go() of the same
shape, HIP events, BASELINE configs[1] and [2].  Per configuration a fresh env: the first call allocates the cache and
builds every field, then the state stays put, so that every timed call is the steady-state one (no stale field: the
refresh launches compare tags and the gather runs).  The four calls alternate inside each repetition, so that drift of
the machine hits them alike.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/time_goal_directions.py [--reps N] [--configs 1,2]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="1,2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_goal_directions.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        w = 2 * r + 1
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        outs = {"cost_to_go": torch.empty((B, A, w, w), dtype=torch.int32, device="cuda"),
                "float32": torch.empty((B, A, 4, w, w), dtype=torch.float32, device="cuda"),
                "uint8": torch.empty((B, A, 4, w, w), dtype=torch.uint8, device="cuda"),
                "bits": torch.empty((B, A, w, w), dtype=torch.uint8, device="cuda")}
        calls = {"cost_to_go": lambda: env.cost_to_go(out=outs["cost_to_go"])}
        for fmt in ("float32", "uint8", "bits"):
            calls[fmt] = lambda fmt=fmt: env.goal_directions(format=fmt, out=outs[fmt])
        calls["bits"]()                           # the fresh cache: allocated here, every field built
        torch.cuda.synchronize()
        b0 = env.cost_to_go_builds
        assert b0 == B * A
        for fn in calls.values():                 # warm-up of every kernel the window uses
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(event_us(fn))
        assert env.cost_to_go_builds == b0, "the timed calls built fields"
        # the planes and the windows describe the same fields
        ctg = outs["cost_to_go"]
        assert torch.equal(outs["bits"] != 0, ctg > 0)
        assert torch.equal(outs["float32"], outs["uint8"].to(torch.float32))
        env.close()
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}, {args.reps} reps, median (min) us per call:", flush=True)
        for k, v in times.items():
            v.sort()
            med = v[len(v) // 2]
            nbytes = outs[k].numel() * outs[k].element_size()
            print(f"  {k:11s} {med:9.1f} ({v[0]:9.1f}) us   writes {nbytes / 1e6:9.2f} MB = {nbytes / med / 1e3:8.1f} GB/s   "
                  f"{med / sorted(times['cost_to_go'])[len(v) // 2]:5.2f} x cost_to_go", flush=True)


if __name__ == "__main__":
    main()
