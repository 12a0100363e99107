"""Diagnostic: device time of pibt_actions(swap=True) (pgx_pibt_swap_actions, docs/SPEC.md S23) next to pibt_actions() --
the yardstick: the same planner without the swap rule, on the same build and the same states.  HIP events, BASELINE
configs[1] and [2], lifelong (`restart`) envs under `soft`.  Two states per configuration: after a reset, and after 32
steps driven by the plain planner with PibtPolicy's priorities, when agents have met in corridors and the swap rule has
partners to find.  The distance-field cache is warm in every timed call (the first call of each state builds the stale
fields and is not timed), and the two calls alternate inside each repetition, so that drift of the machine hits them
alike.  Both calls are two launches, the cache refresh (which finds nothing to build) and the planner's kernel;
`--once` makes a few calls of each kind on the second state and nothing else, for a kernel trace that shows the two
kernels alone.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/time_pibt_swap.py [--reps N] [--configs 1,2] [--once]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius
STEPS = 32


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pibt_swap.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   on_target="restart", max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        policy = PibtPolicy(env)
        out = {k: (torch.empty((B, A), dtype=torch.int64, device=env.device),
                   torch.empty((B, A, 2), dtype=torch.int32, device=env.device)) for k in ("plain", "swap")}
        calls = {"plain": lambda: env.pibt_actions(priority=policy.priority, out=out["plain"]),
                 "swap": lambda: env.pibt_actions(priority=policy.priority, out=out["swap"], swap=True)}
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}, {args.reps} reps, median (min) us per call:", flush=True)
        for state in ("after reset", f"after {STEPS} steps"):
            if state != "after reset":
                for _ in range(STEPS):
                    actions, _ = policy.act()
                    _, rewards, _, _, infos = env.step(actions, compute_obs=False)
                    policy.update(rewards, infos["episode_done"])
            for fn in calls.values():             # builds the stale fields, warms both kernels up
                fn()
                fn()
            torch.cuda.synchronize()
            if args.once:
                continue
            b0 = env.cost_to_go_builds
            times = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, fn in calls.items():
                    times[k].append(event_us(fn))
            assert env.cost_to_go_builds == b0, "the timed calls built fields"
            differ = float((out["plain"][0] != out["swap"][0]).any(dim=1).float().mean())
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            for k, v in times.items():
                print(f"  {state:15s} {k:5s} {med[k]:9.1f} ({min(v):9.1f}) us", flush=True)
            print(f"  {state:15s} swap / plain = {med['swap'] / med['plain']:.2f}; the answers differ in "
                  f"{100 * differ:.1f} % of the envs", flush=True)
        env.close()


if __name__ == "__main__":
    main()
