"""Diagnostic: device time of blocking() (pgx_blocking) at inflation 10 and 1 and with blockers="on_target", next to
three yardsticks on the same process, GPU and state: goal_paths(planes=False) -- a cache refresh plus one walk per agent;
visible_agents() -- what finding the pairs costs; and a forced rebuild of every distance field -- cost_to_go() after
set_targets() on every agent, what one unbounded search per agent costs.  HIP events, BASELINE configs[1] and [2], after
a reset and after 32 steps driven by pibt_actions() (on_target="restart", so that every agent stays active).  Per
repetition the calls alternate, so that drift of the machine hits them alike; the two rebuilds of a repetition (to
rolled targets and back) leave the cache as the other calls found it, so every other timed call is the steady-state one.
Also reports, from a host recount with tests/blocking_reference.py on the first envs, the share of eligible pairs the
filter dismisses and the searches that remain.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/time_blocking.py [--reps N] [--configs 1,2] [--recount-envs E]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from blocking_reference import CUT_OFF, DETOUR, blocking_reference, searched_pairs  # noqa: E402
from pogema_amd import GridConfig, VecPogema, _lib  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def recount(env, inflation, envs):
    """Eligible pairs, the filter's share and the blocked pairs of the first `envs` envs, on the host."""
    st = env.get_state()
    maps = torch.empty((env.batch, env.height, env.width), dtype=torch.uint8, device=env.device)
    _lib.check(env._lib.pgx_get_map(env._handle, maps.data_ptr(), env._stream()))
    maps, xy, tg = maps[:envs].cpu().numpy(), st["agents_xy"][:envs].cpu().numpy(), st["targets_xy"][:envs].cpu().numpy()
    kinds = {}
    want = blocking_reference(maps, xy, tg, st["is_active"][:envs].cpu().numpy(), env.obs_radius, inflation, kinds=kinds)
    got = env.blocking(inflation=inflation)
    assert np.array_equal(got[0][:envs].cpu().numpy(), want[0]) and np.array_equal(got[1][:envs].cpu().numpy(), want[1]), \
        "blocking() differs from the reference"
    dismissed, searched = searched_pairs(maps, xy, tg, kinds)
    blocked = sum(v in (CUT_OFF, DETOUR) for v in kinds.values())
    return len(kinds), len(dismissed), len(searched), blocked


def measure(env, reps, label):
    B, A = env.batch, env.num_agents
    dev = env.device
    count = torch.empty((B, A), dtype=torch.int32, device=dev)
    blocked_by = torch.empty((B, A), dtype=torch.int32, device=dev)
    subgoal = torch.empty((B, A, 2), dtype=torch.int8, device=dev)
    length = torch.empty((B, A), dtype=torch.int32, device=dev)
    nb = tuple(t.to(dev) for t in (torch.empty((B, A, 13), dtype=torch.int32), torch.empty((B, A, 13, 2), dtype=torch.int8),
                                   torch.empty((B, A), dtype=torch.int32)))
    window = torch.empty((B, A, env.window, env.window), dtype=torch.int32, device=dev)
    targets = env.get_state()["targets_xy"].clone()
    rolled = targets.roll(1, dims=1)          # every agent gets its neighbour's target: every field is stale
    changed = float((rolled != targets).any(-1).float().mean())
    calls = {
        "blocking inflation 10": lambda: env.blocking(10, out=(count, blocked_by)),
        "blocking inflation 1": lambda: env.blocking(1, out=(count, blocked_by)),
        "blocking on_target": lambda: env.blocking(10, "on_target", out=(count, blocked_by)),
        "goal_paths no planes": lambda: env.goal_paths(planes=False, out=(subgoal, length)),
        "visible_agents k=13": lambda: env.visible_agents(13, out=nb),
    }
    for fn in calls.values():                 # warm-up of every kernel the window uses; the first one fills the cache
        fn()
    env.set_targets(rolled)
    env.cost_to_go(out=window)
    env.set_targets(targets)
    env.cost_to_go(out=window)
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    times["rebuild every field"] = []
    for _ in range(reps):
        for tg in (rolled, targets):
            env.set_targets(tg)
            b0 = env.cost_to_go_builds
            times["rebuild every field"].append(event_us(lambda: env.cost_to_go(out=window)))
            built = env.cost_to_go_builds - b0
        b0 = env.cost_to_go_builds
        for k, fn in calls.items():
            times[k].append(event_us(fn))
        assert env.cost_to_go_builds == b0, "a steady-state call built fields"
    print(f"  {label}: {reps} reps ({2 * reps} rebuilds of {built} fields, {changed:.0%} of the agents' targets differ), "
          f"median [p10 .. p90] (min) us per call:", flush=True)
    med_b = float(np.median(times["blocking inflation 10"]))
    for k, v in times.items():
        v = np.sort(np.array(v))
        print(f"    {k:24s} {np.median(v):9.1f} [{np.percentile(v, 10):9.1f} .. {np.percentile(v, 90):9.1f}] ({v[0]:9.1f}) us"
              f"   this / blocking(10) = {np.median(v) / med_b:6.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--recount-envs", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_blocking.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   on_target="restart", max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}", flush=True)
        for label, steps in (("after reset", 0), ("after 32 planner-driven steps", 32)):
            for _ in range(steps):
                env.step(env.pibt_actions()[0])
            for inflation in (10, 1):
                pairs, dismissed, searched, blocked = recount(env, inflation, min(args.recount_envs, B))
                print(f"  {label}, inflation {inflation}, first {min(args.recount_envs, B)} envs on the host: {pairs} eligible "
                      f"pairs, the filter dismisses {dismissed} ({dismissed / max(pairs, 1):.1%}), {searched} searches, "
                      f"{blocked} blocked pairs", flush=True)
            measure(env, args.reps, label)
        env.close()


if __name__ == "__main__":
    main()
