"""Diagnostic: solve rate of examples/whca_rollout.py's receding-horizon loop (whca_plan(K), rollout of the first steps,
growing priorities, replan) against examples/planned_rollout.py's plan (PibtPolicy.plan(16) + rollout(), with and without
the swap rule) on the 80 instances of the swap rule's solve-rate measurement (tests/pibt_swap_cases.py: solve_suite --
12 x 12, density 0.35, 8 agents), 150 steps, `soft`, under on_target "nothing" (solved = all agents on their targets at
once, the measurement's rule) and "finish".  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/whca_solve_rate.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tests", "examples"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pibt_swap_cases import solve_suite  # noqa: E402
from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402
from whca_rollout import FirstEpisode, whca_episode  # noqa: E402

STEPS = 150


def main():
    if not torch.cuda.is_available():
        raise SystemExit("whca_solve_rate.py needs a GPU")
    suite = list(solve_suite())
    obstacles, agents, targets = (np.stack([inst[k] for inst in suite]) for k in range(3))
    for on_target in ("nothing", "finish"):
        gc = GridConfig(map=obstacles[0].tolist(), num_agents=agents.shape[1], obs_radius=5, seed=0, collision_system="soft",
                        on_target=on_target, max_episode_steps=STEPS + 1)
        env = VecPogema(gc, batch=len(suite), auto_reset=False)
        for horizon, execute in ((16, 8), (16, 1), (31, 8)):
            env.reset_from_state(obstacles, agents, targets)
            first, failed, plans = whca_episode(env, STEPS, horizon, execute)
            print(f"{on_target} whca K={horizon} execute={execute}: solved (CSR) {int(first.csr.sum())} of {len(suite)}, "
                  f"ISR {float(first.isr.mean()):.4f}, seen {int(first.seen.sum())}, failed searches {failed}, plans {plans}",
                  flush=True)
        for swap in (False, True):
            env.reset_from_state(obstacles, agents, targets)
            policy = PibtPolicy(env)
            first = FirstEpisode(env)
            for t0 in range(0, STEPS, 16):
                actions, _, _ = policy.plan(min(16, STEPS - t0), swap=swap)
                out = env.rollout(actions, obs_slots=0)
                first.add(out)
                policy.priority[out["episode_done"].any(dim=0)] = 0
            print(f"{on_target} pibt_plan(16, swap={swap}): solved (CSR) {int(first.csr.sum())} of {len(suite)}, "
                  f"ISR {float(first.isr.mean()):.4f}, seen {int(first.seen.sum())}", flush=True)
        env.close()


if __name__ == "__main__":
    main()
