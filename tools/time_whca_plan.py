"""Diagnostic: device time of whca_plan(K) (pgx_whca_plan, docs/SPEC.md S28) for K = 8, 16 and 31 on a warm distance-field
cache, next to three yardsticks on the same state and for the same K: pibt_plan(K), the planner it competes with;
cost_to_go(), one read of the same field windows; and a plain fill of the output bytes.  HIP events; BASELINE configs[1]
and [2], each after a reset and after 32 planner-driven steps.  Per configuration a fresh env; the state stays put while
calls are timed.  The calls alternate inside each repetition, so that drift of the machine hits them alike.
docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/time_whca_plan.py [--reps N] [--configs 1,2] [--horizons 8,16,31] [--once]
`--once`: one call of each kind per state and nothing else (for a kernel trace).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def timed(calls, reps, title):
    for _ in range(3):                        # warm-up of every kernel the window uses
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
        print(f"  {k:12s} {med:10.1f} ({v[0]:10.1f}) us   whca_plan / this = {med_whca / med:8.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--horizons", default="8,16,31")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_whca_plan.py needs a GPU")
    for c in (int(v) for v in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        policy = PibtPolicy(env)
        window = torch.empty((B, A, 2 * r + 1, 2 * r + 1), dtype=torch.int32, device="cuda")
        for phase in ("after a reset", "after 32 planner-driven steps"):
            if phase != "after a reset":
                for _ in range(32):
                    out = env.step(policy.act()[0])
                    policy.update(out[1], out[4]["episode_done"])
            prio = policy.priority.clone()
            builds = None
            for K in (int(v) for v in args.horizons.split(",")):
                outs = (torch.empty((K, B, A), dtype=torch.int64, device="cuda"), torch.empty((K, B, A, 2), dtype=torch.int32, device="cuda"),
                        torch.empty((B, A), dtype=torch.int32, device="cuda"), torch.empty((B, A), dtype=torch.int32, device="cuda"))
                fill = torch.empty(sum(t.numel() * t.element_size() for t in outs), dtype=torch.uint8, device="cuda")
                calls = {"whca_plan": lambda: env.whca_plan(K, priority=prio, out=outs),
                         "pibt_plan": lambda: env.pibt_plan(K, priority=prio, out=outs),
                         "cost_to_go": lambda: env.cost_to_go(out=window),
                         "fill": lambda: fill.zero_()}
                if args.once:
                    for fn in calls.values():
                        fn()
                    torch.cuda.synchronize()
                    continue
                _, _, arrival, failed = env.whca_plan(K, priority=prio)
                active = env.get_state()["is_active"]
                builds = env.cost_to_go_builds if builds is None else builds
                timed(calls, args.reps,
                      f"configs[{c}] B={B} {S}x{S} A={A} K={K} {phase}, {args.reps} reps, {int(active.sum())} planned agents, "
                      f"{int(failed.sum())} failed, {int((arrival >= 0).sum())} arrive, writes {fill.numel() / 1e6:.2f} MB, "
                      f"median (min) us per call:")
                assert env.cost_to_go_builds == builds, "a timed call built fields: the cache was not warm"
        env.close()


if __name__ == "__main__":
    main()
