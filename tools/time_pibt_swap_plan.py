"""Diagnostic: device time of pibt_plan(K, swap=True) (pgx_pibt_swap_plan, docs/SPEC.md S27) next to its two yardsticks on
the same build and the same states: pibt_plan(K), the plain lookahead, and what the swap plan replaces -- K eager
iterations of pibt_actions(swap=True), step() and PibtPolicy's priority update.  HIP events, BASELINE configs[1] and
[2], lifelong (`restart`) envs under `soft`, K = 8 and 32.  Two states per configuration: after a reset, and after 32
steps driven by the plain planner with PibtPolicy's priorities, when agents have met in corridors and the swap rule has
partners to find.  The distance-field cache is warm in every timed plan (the first call of each state builds the stale
fields and is not timed), and the plans alternate inside each repetition, so that drift of the machine hits them alike;
one pibt_actions(swap=True) call is timed with them, to set a plan's cost per step against it.  The eager loops come
last in each state, because they move it: their time includes the fields a lifelong env rebuilds after an arrival,
which a plan does not see; `--loops 0` leaves them out.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails
without one.

    python tools/time_pibt_swap_plan.py [--reps N] [--loops N] [--configs 1,2]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius
STEPS = 32
HORIZONS = (8, 32)


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def drive(env, policy, steps):
    for _ in range(steps):
        actions, _ = policy.act()
        _, rewards, _, _, infos = env.step(actions, compute_obs=False)
        policy.update(rewards, infos["episode_done"])


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--configs", default="1,2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pibt_swap_plan.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   on_target="restart", max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        policy = PibtPolicy(env)
        dev = env.device
        outs = {K: tuple((torch.empty((K, B, A), dtype=torch.int64, device=dev), torch.empty((K, B, A, 2), dtype=torch.int32, device=dev),
                          torch.empty((B, A), dtype=torch.int32, device=dev), torch.empty((B, A), dtype=torch.int32, device=dev))
                         for _ in range(2)) for K in HORIZONS}
        one = (torch.empty((B, A), dtype=torch.int64, device=dev), torch.empty((B, A, 2), dtype=torch.int32, device=dev))
        calls = {"pibt_actions(swap=True)": lambda: env.pibt_actions(priority=policy.priority, out=one, swap=True)}
        for K in HORIZONS:
            calls[f"pibt_plan({K}, swap=True)"] = lambda K=K: env.pibt_plan(K, priority=policy.priority, out=outs[K][0], swap=True)
            calls[f"pibt_plan({K})"] = lambda K=K: env.pibt_plan(K, priority=policy.priority, out=outs[K][1])
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}, {args.reps} reps, median (min) us per call:", flush=True)
        for state in ("after reset", f"after {STEPS} steps"):
            if state != "after reset":
                env.reset(seed=0)
                policy.reset()
                drive(env, policy, STEPS)
            for fn in calls.values():             # builds the stale fields, warms the kernels up
                fn()
                fn()
            torch.cuda.synchronize()
            b0 = env.cost_to_go_builds
            times = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, fn in calls.items():
                    times[k].append(event_us(fn))
            assert env.cost_to_go_builds == b0, "the timed calls built fields"
            med = {k: median(v) for k, v in times.items()}
            for k, v in times.items():
                print(f"  {state:15s} {k:26s} {med[k]:10.1f} ({min(v):10.1f}) us", flush=True)
            single = med["pibt_actions(swap=True)"]
            for K in HORIZONS:
                swap, plain = med[f"pibt_plan({K}, swap=True)"], med[f"pibt_plan({K})"]
                differ = float((outs[K][0][0] != outs[K][1][0]).any(dim=2).any(dim=0).float().mean())
                print(f"  {state:15s} K={K}: swap / plain = {swap / plain:.2f}; {swap / K:.1f} us per step of the swap plan "
                      f"against {single:.1f} us for one pibt_actions(swap=True); the plans differ in {100 * differ:.1f} % of "
                      f"the envs", flush=True)
            # what the plan replaces: K eager iterations with the swap rule (they move the state: last)
            if not args.loops:
                continue
            eager = PibtPolicy(env, swap=True)
            eager.priority.copy_(policy.priority)
            drive(env, eager, 2)
            torch.cuda.synchronize()
            for K in HORIZONS:
                loop = [event_us(lambda: drive(env, eager, K)) for _ in range(args.loops)]
                print(f"  {state:15s} {K} x (pibt_actions(swap=True) + step() + update()): {median(loop):10.1f} "
                      f"({min(loop):10.1f}) us, {median(loop) / K:.1f} us per step; pibt_plan({K}, swap=True) + rollout() "
                      f"replaces it", flush=True)
        env.close()


if __name__ == "__main__":
    main()
