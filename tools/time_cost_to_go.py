"""Diagnostic: device time of cost_to_go() (pgx_cost_to_go) next to step() of the same shape, HIP events, BASELINE
configs[1] and [2].  Per configuration: the steady-state call (no stale field), the call right after reset(seed) (every
field stale), and a lifelong (on_target="restart") run driven by expert_actions() with the fields built per step.
docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/time_cost_to_go.py [--reps N] [--configs 1,2] [--lifelong-steps N]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius
HBM_BYTES_PER_S = 8e12


def timed(fn, reps, before=None):
    """Median device time of fn() in microseconds, one event pair per call (`before` runs outside the events)."""
    times = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--lifelong-steps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cost_to_go.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        w = 2 * r + 1
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        acts = torch.zeros((B, A), dtype=torch.int64, device="cuda")  # noop: the state stays put
        out = torch.empty((B, A, w, w), dtype=torch.int32, device="cuda")
        env.cost_to_go(out=out)                   # allocates the cache, builds every field
        env.step(acts)
        torch.cuda.synchronize()
        step_us = timed(lambda: env.step(acts), args.reps)
        b0 = env.cost_to_go_builds
        steady_us = timed(lambda: env.cost_to_go(out=out), args.reps)
        assert env.cost_to_go_builds == b0, "the steady-state calls built fields"
        seeds = iter(range(1, 10**6))
        stale_us = timed(lambda: env.cost_to_go(out=out), max(3, args.reps // 4), before=lambda: env.reset(seed=next(seeds)))
        # byte model of the steady-state call: the output stream + W row segments of W cells per agent
        cell = 2 if S * S <= 65536 else 4
        model = B * A * w * w * 4 + B * A * w * w * cell
        frac = model / (steady_us * 1e-6) / HBM_BYTES_PER_S
        env.close()

        life = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                    on_target="restart", max_episode_steps=10**6), batch=B)
        life.reset(seed=0)
        life.cost_to_go(out=out)
        torch.cuda.synchronize()
        built0, times = life.cost_to_go_builds, []
        for _ in range(args.lifelong_steps):
            a, _ = life.expert_actions()
            life.step(a)
            times.append(timed(lambda: life.cost_to_go(out=out), 1))
        per_step = (life.cost_to_go_builds - built0) / args.lifelong_steps
        times.sort()
        life.close()
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}: step {step_us:8.1f} us | cost_to_go steady {steady_us:8.1f} us "
              f"({steady_us / step_us:.2f} x step, byte model {model / 1e6:.1f} MB = {100 * frac:.1f} % of 8 TB/s) | "
              f"after reset {stale_us:9.1f} us | lifelong: {per_step:.1f} builds/step, call median "
              f"{times[len(times) // 2]:8.1f} us", flush=True)


if __name__ == "__main__":
    main()
