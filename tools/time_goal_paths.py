"""Diagnostic: device time of goal_paths() (pgx_goal_paths) in its three formats and without planes, next to
goal_directions("bits") of the same shape (the yardstick: a window of the same fields read per agent, one byte out per
cell, as goal_paths("uint8") writes), to the torch composition of the same result with steps = 2r (goal_directions("bits") plus 2r rounds
of gather, compare and scatter: what a user runs without the query) and to a plain fill of the same bytes.  HIP events,
BASELINE configs[1] and [2].  Per configuration a fresh env: the first call allocates the cache and builds every field,
then the state stays put, so that every timed call is the steady-state one.  The calls alternate inside each
repetition, so that drift of the machine hits them alike.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails
without one.

    python tools/time_goal_paths.py [--reps N] [--configs 1,2]
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
    """goal_paths(steps=2r, format="uint8") out of goal_directions("bits") and torch: per path step one gather of the
    mask under every agent's cursor, the compares that pick the move and keep it inside the window, and one scatter of
    the mark."""

    def __init__(self, env):
        B, A, w = env.batch, env.num_agents, env.window
        dev = env.device
        self.env, self.w, self.r, self.n = env, w, env.obs_radius, B * A
        self.bits = torch.empty((B, A, w, w), dtype=torch.uint8, device=dev)
        delta = torch.zeros((16, 2), dtype=torch.int64, device=dev)     # by the mask's lowest bit: the move's (du, dv)
        for low, d in ((1, (-1, 0)), (2, (1, 0)), (4, (0, -1)), (8, (0, 1))):
            delta[low] = torch.tensor(d)
        self.delta = delta
        self.planes = torch.empty((B * A, w * w), dtype=torch.uint8, device=dev)

    def __call__(self):
        w, r = self.w, self.r
        flat = self.env.goal_directions(format="bits", out=self.bits).view(self.n, w * w)
        u = torch.full((self.n,), r, dtype=torch.int64, device=flat.device)
        v = u.clone()
        length = torch.zeros_like(u)
        alive = torch.ones_like(u, dtype=torch.bool)
        planes = self.planes.zero_()
        for _ in range(2 * r):
            m = flat.gather(1, (u * w + v).unsqueeze(1)).squeeze(1).to(torch.int64)
            d = self.delta[m & -m]
            nu, nv = u + d[:, 0], v + d[:, 1]
            alive = alive & (m != 0) & (nu >= 0) & (nu < w) & (nv >= 0) & (nv < w)
            u, v = torch.where(alive, nu, u), torch.where(alive, nv, v)
            at = (u * w + v).unsqueeze(1)        # (an agent that has stopped rewrites the cell under its cursor as it is)
            planes.scatter_(1, at, torch.where(alive.unsqueeze(1), 1, planes.gather(1, at)).to(torch.uint8))
            length += alive
        shape = self.bits.shape[:2]
        return (planes.view(self.bits.shape), torch.stack((u - r, v - r), -1).to(torch.int8).view(shape + (2,)),
                length.to(torch.int32).view(shape))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="1,2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_goal_paths.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        w = 2 * r + 1
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        planes = {"float32": torch.empty((B, A, w, w), dtype=torch.float32, device="cuda"),
                  "uint8": torch.empty((B, A, w, w), dtype=torch.uint8, device="cuda"),
                  "rows": torch.empty((B, A, w), dtype=torch.int32, device="cuda")}
        subgoal = torch.empty((B, A, 2), dtype=torch.int8, device="cuda")
        length = torch.empty((B, A), dtype=torch.int32, device="cuda")
        bits = torch.empty((B, A, w, w), dtype=torch.uint8, device="cuda")
        compose = Composition(env)
        small = subgoal.numel() + 4 * length.numel()
        calls, nbytes = {}, {}
        for fmt in ("float32", "uint8", "rows"):
            calls[f"paths {fmt}"] = lambda fmt=fmt: env.goal_paths(format=fmt, out=(planes[fmt], subgoal, length))
            nbytes[f"paths {fmt}"] = planes[fmt].numel() * planes[fmt].element_size() + small
        calls["paths no planes"] = lambda: env.goal_paths(planes=False, out=(subgoal, length))
        nbytes["paths no planes"] = small
        calls["directions bits"] = lambda: env.goal_directions(format="bits", out=bits)
        nbytes["directions bits"] = bits.numel()
        calls["composition 2r"] = compose
        nbytes["composition 2r"] = bits.numel() + small
        for fmt in ("float32", "uint8"):
            calls[f"fill {fmt}"] = lambda fmt=fmt: planes[fmt].zero_()
            nbytes[f"fill {fmt}"] = planes[fmt].numel() * planes[fmt].element_size()
        calls["directions bits"]()                # the fresh cache: allocated here, every field built
        torch.cuda.synchronize()
        b0 = env.cost_to_go_builds
        assert b0 == B * A
        # the composition states the same result as the capped query
        want = env.goal_paths(steps=2 * r, format="uint8")
        for got, ref, name in zip(compose(), want, ("planes", "subgoal", "length")):
            assert torch.equal(got, ref), f"the composition's {name} differ from goal_paths(steps=2r)"
        for fn in calls.values():                 # warm-up of every kernel the window uses
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(event_us(fn))
        assert env.cost_to_go_builds == b0, "the timed calls built fields"
        u8 = env.goal_paths(format="uint8")
        assert torch.equal(env.goal_paths(format="float32")[0], u8[0].to(torch.float32))
        mean_len = float(u8[2].float().mean())
        env.close()
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}, {args.reps} reps, mean length {mean_len:.2f}, "
              f"median (min) us per call:", flush=True)
        med_comp = sorted(times["composition 2r"])[args.reps // 2]
        for k, v in times.items():
            v.sort()
            med = v[len(v) // 2]
            print(f"  {k:16s} {med:9.1f} ({v[0]:9.1f}) us   writes {nbytes[k] / 1e6:9.2f} MB = {nbytes[k] / med / 1e3:8.1f} GB/s   "
                  f"composition / this = {med_comp / med:6.2f}", flush=True)


if __name__ == "__main__":
    main()
