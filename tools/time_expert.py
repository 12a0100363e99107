"""Diagnostic: device time of expert_actions() (pgx_expert_actions) next to step() of the same shape, HIP events,
BASELINE configs[1], [2] and [4].  One line per configuration; docs/EXPERIMENTS.md records the numbers.

    python tools/time_expert.py [--reps N] [--configs 1,2,4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5), 4: (4096, 256, 256, 7)}  # batch, size, agents, obs_radius


def timed(fn, reps):
    """Median device time of fn() in microseconds, one event pair per call."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="1,2,4")
    args = ap.parse_args()
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        acts = torch.zeros((B, A), dtype=torch.int64, device="cuda")  # noop: the state (and the searches) stay put
        out_a = torch.empty((B, A), dtype=torch.int64, device="cuda")
        out_d = torch.empty((B, A), dtype=torch.int32, device="cuda")
        step_us, _ = timed(lambda: env.step(acts), args.reps)
        reps = max(3, args.reps // 4) if c == 4 else args.reps
        ex_us, ex_min = timed(lambda: env.expert_actions(out=(out_a, out_d)), reps)
        exo_us, _ = timed(lambda: env.expert_actions(agents_as_obstacles=True, out=(out_a, out_d)), reps)
        d = out_d[out_d >= 0].float()
        print(f"configs[{c}] B={B} {S}x{S} A={A}: step {step_us:9.1f} us | expert {ex_us:10.1f} us (min {ex_min:.1f}, "
              f"{ex_us / step_us:6.1f} x step) | agents_as_obstacles {exo_us:10.1f} us | mean distance "
              f"{float(d.mean()) if d.numel() else 0.0:.1f}", flush=True)
        env.close()


if __name__ == "__main__":
    main()
