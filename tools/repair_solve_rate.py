"""Diagnostic: examples/lns_repair.py's loop (whca_plan(16) once, then repair_plan() -- failed searches with their
neighbourhood, and after every 8 steps only the agents whose path is stale or ends off their target) against
examples/whca_rollout.py's loop (whca_plan(16) for everybody every 8 steps) on the 80 instances of the swap rule's
solve-rate measurement (tests/pibt_swap_cases.py: solve_suite -- 12 x 12, density 0.35, 8 agents), 150 steps, `soft`,
under on_target "nothing" (solved = all agents on their targets at once) and "finish".  Reports the solve rate and the
number of agent searches both loops made.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/repair_solve_rate.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tests", "examples"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lns_repair import repair_episode  # noqa: E402
from pibt_swap_cases import solve_suite  # noqa: E402
from pogema_amd import GridConfig, VecPogema  # noqa: E402
from whca_rollout import FirstEpisode  # noqa: E402

STEPS, HORIZON, EXECUTE = 150, 16, 8


def whca_episode_counted(env, steps, horizon, execute):
    """examples/whca_rollout.py's whca_episode, which also counts the agents it serves."""
    prio = torch.zeros((env.batch, env.num_agents), dtype=torch.int32, device=env.device)
    first = FirstEpisode(env)
    searches = 0
    for t0 in range(0, steps, execute):
        searches += int(env.get_state()["is_active"].sum())
        actions = env.whca_plan(horizon, priority=prio)[0]
        n = min(execute, horizon, steps - t0)
        out = env.rollout(actions[:n], obs_slots=0)
        first.add(out)
        st = env.get_state()
        zero = (st["agents_xy"] == st["targets_xy"]).all(dim=-1) | ~st["is_active"].bool() | out["episode_done"].any(dim=0).view(-1, 1)
        prio = torch.where(zero, torch.zeros_like(prio), prio + n)
    return first, searches


def main():
    if not torch.cuda.is_available():
        raise SystemExit("repair_solve_rate.py needs a GPU")
    suite = list(solve_suite())
    obstacles, agents, targets = (np.stack([inst[k] for inst in suite]) for k in range(3))
    for on_target in ("nothing", "finish"):
        gc = GridConfig(map=obstacles[0].tolist(), num_agents=agents.shape[1], obs_radius=5, seed=0, collision_system="soft",
                        on_target=on_target, max_episode_steps=STEPS + 1)
        env = VecPogema(gc, batch=len(suite), auto_reset=False)
        env.reset_from_state(obstacles, agents, targets)
        first, searches, conflicts = repair_episode(env, STEPS, HORIZON, EXECUTE, log=lambda *a: None)
        print(f"{on_target} repair loop K={HORIZON} execute={EXECUTE}: solved (CSR) {int(first.csr.sum())} of {len(suite)}, "
              f"ISR {float(first.isr.mean()):.4f}, seen {int(first.seen.sum())}, agent searches {searches}, conflicts left in "
              f"the windows run {conflicts}", flush=True)
        env.reset_from_state(obstacles, agents, targets)
        first, searches = whca_episode_counted(env, STEPS, HORIZON, EXECUTE)
        print(f"{on_target} whca_plan every {EXECUTE} steps K={HORIZON}: solved (CSR) {int(first.csr.sum())} of {len(suite)}, "
              f"ISR {float(first.isr.mean()):.4f}, seen {int(first.seen.sum())}, agent searches {searches}", flush=True)
        env.close()


if __name__ == "__main__":
    main()
