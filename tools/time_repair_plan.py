"""Diagnostic: device time of repair_plan() (pgx_repair_plan, docs/SPEC.md S29) for K = 8, 16 and 31 on a warm
distance-field cache, given whca_plan(K)'s own paths, with all, half, an eighth and none of the agents asked for, next to
whca_plan(K) on the same state and a plain fill of the output bytes.  The expectation to test: the prologue plus (share
replanned) x the serial loop of whca_plan.  HIP events; BASELINE configs[1] and [2] after a reset.  The calls alternate
inside each repetition, so that drift of the machine hits them alike.  docs/EXPERIMENTS.md records the numbers.  Needs a
GPU; fails without one.

    python tools/time_repair_plan.py [--reps N] [--configs 1,2] [--horizons 8,16,31]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius
MASKS = {"all": 1, "half": 2, "eighth": 8, "none": 0}  # every n-th agent is asked for


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def timed(calls, reps, title):
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            times[k].append(event_us(fn))
    print(title, flush=True)
    med_whca = sorted(times["whca_plan"])[reps // 2]
    for k, v in times.items():
        v.sort()
        med = v[len(v) // 2]
        print(f"  {k:14s} {med:10.1f} ({v[0]:10.1f}) us   this / whca_plan = {med / med_whca:6.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--horizons", default="8,16,31")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_repair_plan.py needs a GPU")
    for c in (int(v) for v in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        index = torch.arange(A, device="cuda").expand(B, A)
        masks = {k: ((index % n == 0) if n else torch.zeros_like(index, dtype=torch.bool)).contiguous() for k, n in MASKS.items()}
        for K in (int(v) for v in args.horizons.split(",")):
            outs = (torch.empty((K, B, A), dtype=torch.int64, device="cuda"), torch.empty((K, B, A, 2), dtype=torch.int32, device="cuda"),
                    *(torch.empty((B, A), dtype=torch.int32, device="cuda") for _ in range(3)))
            fill = torch.empty(sum(t.numel() * t.element_size() for t in outs), dtype=torch.uint8, device="cuda")
            _, given, _, failed = env.whca_plan(K)
            builds = env.cost_to_go_builds
            calls = {"whca_plan": lambda: env.whca_plan(K, out=outs[:4])}
            served = {}
            for k, mask in masks.items():
                calls[f"repair {k}"] = lambda mask=mask: env.repair_plan(given, replan=mask, out=outs)
                served[k] = int(env.repair_plan(given, replan=mask)[4].sum())
            calls["fill"] = lambda: fill.zero_()
            timed(calls, args.reps,
                  f"configs[{c}] B={B} {S}x{S} A={A} K={K} after a reset, {args.reps} reps, {int(failed.sum())} failed in the given "
                  f"plan, agents served: {served}, writes {fill.numel() / 1e6:.2f} MB, median (min) us per call:")
            assert env.cost_to_go_builds == builds, "a timed call built fields: the cache was not warm"
        env.close()


if __name__ == "__main__":
    main()
