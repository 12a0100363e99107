"""Diagnostic: device time of agent_forecasts() (pgx_agent_forecasts) with K = 3 as uint8 and float32 planes and
without planes, next to three yardsticks on the same state: the torch composition of the same result (goal_directions(
"bits"), K rounds of gather and compare for the cells, a pairwise visibility test and one scatter for the planes: what a
user runs without the query), goal_paths(planes=False) as the cost of one walk per agent over the same fields, and a
plain fill of the same bytes.  HIP events, BASELINE configs[1] and [2].  Per configuration a fresh env: the first call
allocates the cache and builds every field, then the state stays put, so that every timed call is the steady-state
one.  The calls alternate inside each repetition, so that drift of the machine hits them alike.  docs/EXPERIMENTS.md
records the numbers.  Needs a GPU; fails without one.

    python tools/time_agent_forecasts.py [--reps N] [--configs 1,2] [--steps 3]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


class Composition:
    """agent_forecasts(K, "uint8") out of get_state(), goal_directions("bits") and torch, for K <= obs_radius + 1 (the
    walk stays inside the agent's own window of masks, which are exact up to its edge): per step one gather of the mask
    under every agent's cursor and the compare that picks the move; then the pairwise visibility test, the forecast
    cells relative to every observer and one scatter."""

    def __init__(self, env, K):
        B, A, w = env.batch, env.num_agents, env.window
        assert K <= env.obs_radius + 1
        dev = env.device
        self.env, self.K = env, K
        self.bits = torch.empty((B, A, w, w), dtype=torch.uint8, device=dev)
        delta = torch.zeros((16, 2), dtype=torch.int64, device=dev)     # by the mask's lowest bit: the move's (du, dv)
        for low, d in ((1, (-1, 0)), (2, (1, 0)), (4, (0, -1)), (8, (0, 1))):
            delta[low] = torch.tensor(d)
        self.delta = delta
        self.other = ~torch.eye(A, dtype=torch.bool, device=dev)
        self.planes = torch.empty((B, A, K, w, w), dtype=torch.uint8, device=dev)

    def __call__(self):
        env, K = self.env, self.K
        B, A, w, r = env.batch, env.num_agents, env.window, env.obs_radius
        st = env.get_state()
        pos, active = st["agents_xy"].long(), st["is_active"].bool()
        flat = env.goal_directions(format="bits", out=self.bits).view(B * A, w * w).long()
        u = torch.full((B * A,), r, dtype=torch.int64, device=flat.device)
        v = u.clone()
        cells = []
        for _ in range(K):
            m = flat.gather(1, (u * w + v).unsqueeze(1)).squeeze(1)
            d = self.delta[m & -m]
            u, v = u + d[:, 0], v + d[:, 1]
            cells.append(pos + torch.stack((u - r, v - r), -1).view(B, A, 2))
        cells = torch.stack(cells, 2)                                             # [B, A, K, 2]
        cells = torch.where(active.view(B, A, 1, 1), cells, torch.full_like(cells, -1))
        off = pos.view(B, 1, A, 2) - pos.view(B, A, 1, 2)                         # [b, i, j]: j seen from i
        seen = (off.abs() <= r).all(-1) & active.view(B, A, 1) & active.view(B, 1, A) & self.other
        rel = cells.view(B, 1, A, K, 2) - pos.view(B, A, 1, 1, 2) + r             # [b, i, j, s]: window cell of q_j(s)
        inside = ((rel >= 0) & (rel < w)).all(-1) & seen.unsqueeze(-1)
        b, i, _, s = torch.nonzero(inside, as_tuple=True)
        uv = rel[inside]
        planes = self.planes.zero_()
        planes[b, i, s, uv[:, 0], uv[:, 1]] = 1
        return planes, cells.to(torch.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_agent_forecasts.py needs a GPU")
    K = args.steps
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        w = 2 * r + 1
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        planes = {"float32": torch.empty((B, A, K, w, w), dtype=torch.float32, device="cuda"),
                  "uint8": torch.empty((B, A, K, w, w), dtype=torch.uint8, device="cuda")}
        cells = torch.empty((B, A, K, 2), dtype=torch.int16, device="cuda")
        subgoal = torch.empty((B, A, 2), dtype=torch.int8, device="cuda")
        length = torch.empty((B, A), dtype=torch.int32, device="cuda")
        compose = Composition(env, K)
        calls, nbytes = {}, {}
        for fmt in ("uint8", "float32"):
            calls[f"forecasts {fmt}"] = lambda fmt=fmt: env.agent_forecasts(K, fmt, out=(planes[fmt], cells))
            nbytes[f"forecasts {fmt}"] = planes[fmt].numel() * planes[fmt].element_size() + 2 * cells.numel()
        calls["forecasts no planes"] = lambda: env.agent_forecasts(K, planes=False, out=(cells,))
        nbytes["forecasts no planes"] = 2 * cells.numel()
        calls["composition"] = compose
        nbytes["composition"] = planes["uint8"].numel() + 2 * cells.numel()
        calls["paths no planes"] = lambda: env.goal_paths(planes=False, out=(subgoal, length))
        nbytes["paths no planes"] = subgoal.numel() + 4 * length.numel()
        for fmt in ("uint8", "float32"):
            calls[f"fill {fmt}"] = lambda fmt=fmt: planes[fmt].zero_()
            nbytes[f"fill {fmt}"] = planes[fmt].numel() * planes[fmt].element_size()
        calls["paths no planes"]()                # the fresh cache: allocated here, every field built
        torch.cuda.synchronize()
        b0 = env.cost_to_go_builds
        assert b0 == B * A
        # the composition states the same result as the query
        want = env.agent_forecasts(K, "uint8")
        for got, ref, name in zip(compose(), want, ("planes", "cells")):
            assert torch.equal(got, ref), f"the composition's {name} differ from agent_forecasts({K})"
        assert torch.equal(env.agent_forecasts(K, "float32")[0], want[0].to(torch.float32))
        marked = float(want[0].float().sum((-1, -2, -3)).mean())
        for fn in calls.values():                 # warm-up of every kernel the window uses
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(event_us(fn))
        assert env.cost_to_go_builds == b0, "the timed calls built fields"
        env.close()
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r} K={K}, {args.reps} reps, {marked:.2f} cells marked per agent, "
              f"median (min) us per call:", flush=True)
        med_comp = sorted(times["composition"])[args.reps // 2]
        for k, v in times.items():
            v.sort()
            med = v[len(v) // 2]
            print(f"  {k:20s} {med:9.1f} ({v[0]:9.1f}) us   writes {nbytes[k] / 1e6:9.2f} MB = {nbytes[k] / med / 1e3:8.1f} GB/s   "
                  f"composition / this = {med_comp / med:6.2f}", flush=True)


if __name__ == "__main__":
    main()
