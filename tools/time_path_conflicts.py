"""Diagnostic: device time of path_conflicts() (pgx_path_conflicts) on given forecast cells with K = 3 and K = 8, next to
three yardsticks on the same state: the torch all-pairs composition of the same four outputs (a [K, B, A, A] mask per
kind: what a user runs without the query), agent_forecasts(K, planes=False) as the cost of producing the paths, and a
plain fill of the output bytes.  HIP events; BASELINE configs[1] and [2], each after a reset and after 32 planner-driven
steps, and 1024 agents per env (one env per workgroup) after a reset; at configs[1] also a 32-step pibt_plan()'s path_xy.
Per configuration a fresh env; the state stays put while calls are timed.  The calls alternate inside each repetition,
so that drift of the machine hits them alike.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/time_path_conflicts.py [--reps N] [--configs 1,2,3] [--steps 3,8]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5), 3: (256, 64, 1024, 5)}  # batch, size, agents, obs_radius
KINDS = ("vertex", "edge", "follow")


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def composition(env, paths, vanish):
    """path_conflicts(paths, kinds=KINDS) out of get_state() and torch: docs/SPEC.md S26 stated over all pairs."""
    B, A, Wd = env.batch, env.num_agents, env.width
    st = env.get_state()
    steps = paths.permute(2, 0, 1, 3) if paths.dtype == torch.int16 else paths               # [K, B, A, 2]
    pos = torch.cat((st["agents_xy"].unsqueeze(0), steps.to(torch.int32)))                  # [K + 1, B, A, 2]
    K = pos.shape[0] - 1
    x, y = pos[..., 0], pos[..., 1]
    part = (x >= 0) & (x < env.height) & (y >= 0) & (y < Wd) & st["is_active"].bool().unsqueeze(0)
    if vanish:
        on = (pos == st["targets_xy"].unsqueeze(0)).all(-1)
        before = torch.zeros_like(on)
        before[1:] = on.cumsum(0)[:-1] > 0
        part &= ~before
    key = x * Wd + y
    now, was, p_now, p_was = key[1:], key[:-1], part[1:], part[:-1]
    other = ~torch.eye(A, dtype=torch.bool, device=pos.device)
    both_now = p_now.unsqueeze(3) & p_now.unsqueeze(2) & other
    both = both_now & p_was.unsqueeze(3) & p_was.unsqueeze(2)
    moved = now != was
    vertex = both_now & (now.unsqueeze(3) == now.unsqueeze(2))
    into = both & (now.unsqueeze(3) == was.unsqueeze(2)) & moved.unsqueeze(3)
    edge = into & (was.unsqueeze(3) == now.unsqueeze(2))
    follow = into & moved.unsqueeze(2) & ~edge
    any_kind = vertex | edge | follow                                                        # [K, B, A, A]
    bits = vertex.to(torch.uint8) | edge.to(torch.uint8) * 2 | follow.to(torch.uint8) * 4
    count = any_kind.sum((0, 3), dtype=torch.int32)
    per_step = any_kind.any(3)
    has = per_step.any(0)
    h0 = per_step.to(torch.uint8).argmax(0)                                                  # [B, A]
    idx = h0.view(1, B, A, 1).expand(1, B, A, A)
    row = any_kind.gather(0, idx)[0]
    first = torch.where(has, h0 + 1, -1).to(torch.int32)
    partner = torch.where(has, row.to(torch.uint8).argmax(-1), -1).to(torch.int32)
    at = bits.gather(0, idx)[0]                                                              # [B, A, A]: the first step's bits
    kind = sum(((at & bit) != 0).any(-1).to(torch.uint8) * bit for bit in (1, 2, 4))
    return first, partner, kind, count


def timed(calls, nbytes, reps, title):
    for fn in calls.values():                 # warm-up of every kernel the window uses
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            times[k].append(event_us(fn))
    print(title, flush=True)
    med_comp = sorted(times["composition"])[reps // 2]
    for k, v in times.items():
        v.sort()
        med = v[len(v) // 2]
        print(f"  {k:22s} {med:10.1f} ({v[0]:10.1f}) us   writes {nbytes[k] / 1e6:8.2f} MB   composition / this = {med_comp / med:8.2f}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="1,2,3")
    ap.add_argument("--steps", default="3,8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_path_conflicts.py needs a GPU")
    for c in (int(v) for v in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.1 if c == 3 else 0.3, seed=0,
                                   collision_system="soft", max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        policy = PibtPolicy(env)
        outs = (torch.empty((B, A), dtype=torch.int32, device="cuda"), torch.empty((B, A), dtype=torch.int32, device="cuda"),
                torch.empty((B, A), dtype=torch.uint8, device="cuda"), torch.empty((B, A), dtype=torch.int32, device="cuda"))
        out_bytes = 13 * B * A
        fill = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
        for phase in ("after a reset",) if c == 3 else ("after a reset", "after 32 planner-driven steps"):
            if phase != "after a reset":
                for _ in range(32):
                    out = env.step(policy.act()[0])
                    policy.update(out[1], out[4]["episode_done"])
            for K in (int(v) for v in args.steps.split(",")):
                if c == 3 and K != 3:
                    continue
                cells = env.agent_forecasts(K, planes=False)[1]
                vanish = env.grid_config.on_target == "finish"
                want = env.path_conflicts(cells, kinds=KINDS)
                for got, ref, name in zip(composition(env, cells, vanish), want, ("first_step", "partner", "kind", "count")):
                    assert torch.equal(got, ref), f"the composition's {name} differs from path_conflicts()"
                calls = {"path_conflicts": lambda: env.path_conflicts(cells, kinds=KINDS, out=outs),
                         "composition": lambda: composition(env, cells, vanish),
                         "forecasts no planes": lambda: env.agent_forecasts(K, planes=False, out=(cells,)),
                         "fill": lambda: fill.zero_()}
                nbytes = {"path_conflicts": out_bytes, "composition": out_bytes, "forecasts no planes": 2 * cells.numel(),
                          "fill": out_bytes}
                conflicts = float(want[3].float().mean())
                timed(calls, nbytes, args.reps,
                      f"configs[{c}] B={B} {S}x{S} A={A} K={K} {phase}, {args.reps} reps, {conflicts:.3f} conflicts per agent, "
                      f"median (min) us per call:")
            if c == 1 and phase == "after a reset":
                path_xy = env.pibt_plan(32)[1]
                want = env.path_conflicts(path_xy, kinds=KINDS)
                for got, ref in zip(composition(env, path_xy, vanish), want):
                    assert torch.equal(got, ref)
                calls = {"path_conflicts": lambda: env.path_conflicts(path_xy, kinds=KINDS, out=outs),
                         "composition": lambda: composition(env, path_xy, vanish),
                         "pibt_plan(32)": lambda: env.pibt_plan(32),
                         "fill": lambda: fill.zero_()}
                nbytes = {"path_conflicts": out_bytes, "composition": out_bytes, "pibt_plan(32)": 0, "fill": out_bytes}
                timed(calls, nbytes, args.reps, f"configs[1] pibt_plan(32).path_xy, K=32, {args.reps} reps, median (min) us per call:")
        env.close()


if __name__ == "__main__":
    main()
