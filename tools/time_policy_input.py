"""Diagnostic: device time of policy_input() (pgx_policy_input, docs/SPEC.md S18) next to the composition it replaces,
observe() + goal_directions() + torch.cat, HIP events, BASELINE configs[1] and [2] in one process.  Per configuration:
    (a)  policy_input() with the default 7 channels, float32
    (b)  torch.cat((observe(), goal_directions()), 2), float32 -- the same tensor
    (c)  policy_input(dtype=torch.bfloat16) and (b) followed by .to(torch.bfloat16)
    (d)  policy_input() with all 8 channels, float32
A step(compute_obs=False) of random actions runs between the repetitions, outside the timed windows, so that the state
moves (on_target="nothing": no target changes, hence no field is rebuilt inside a window).  The calls alternate inside
each repetition, so that drift of the machine hits them alike; medians and minima over the repetitions.  The margin of
the (a) / (b) comparison is (b)'s own min-to-median spread.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU.

    python tools/time_policy_input.py [--reps N] [--warmup N] [--configs 1,2]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius
ALL8 = ("obstacles", "agents", "target", "other_goals", "up", "down", "left", "right")
HBM_PEAK = 8.0e12  # bytes / s
KA, KB, KC = "a policy_input f32 x7", "b observe+directions+cat", "c policy_input bf16 x7"
KC2, KD = "c' (b) + .to(bf16)", "d policy_input f32 x8"


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="1,2")
    args = ap.parse_args()
    if args.reps < 50:
        raise SystemExit("--reps must be at least 50")
    if not torch.cuda.is_available():
        raise SystemExit("time_policy_input.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        w = 2 * r + 1
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                                   on_target="nothing", max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        dev = env.device
        x7 = torch.empty((B, A, 7, w, w), dtype=torch.float32, device=dev)
        x7h = torch.empty((B, A, 7, w, w), dtype=torch.bfloat16, device=dev)
        x8 = torch.empty((B, A, 8, w, w), dtype=torch.float32, device=dev)
        obs = torch.empty((B, A, 3, w, w), dtype=torch.float32, device=dev)
        planes = torch.empty((B, A, 4, w, w), dtype=torch.float32, device=dev)
        cat = torch.empty_like(x7)
        cath = torch.empty_like(x7h)

        def compose():
            torch.cat((env.observe(out=obs), env.goal_directions(out=planes)), 2, out=cat)

        def compose_bf16():
            compose()
            cath.copy_(cat)                      # .to(torch.bfloat16) into a buffer that exists: no allocation is timed

        calls = {KA: lambda: env.policy_input(out=x7),
                 KB: compose,
                 KC: lambda: env.policy_input(dtype=torch.bfloat16, out=x7h),
                 KC2: compose_bf16,
                 KD: lambda: env.policy_input(channels=ALL8, out=x8)}
        nbytes = {KA: x7.numel() * 4, KB: x7.numel() * 4,
                  KC: x7h.numel() * 2, KC2: x7h.numel() * 2,
                  KD: x8.numel() * 4}
        gen = torch.Generator(device=dev)
        gen.manual_seed(c)

        def move():
            env.step(torch.randint(0, 5, (B, A), generator=gen, device=dev), compute_obs=False)

        calls[KA]()          # the fresh cache: allocated here, every field built
        torch.cuda.synchronize()
        b0 = env.cost_to_go_builds
        for _ in range(args.warmup):              # warm-up of every kernel the windows use
            move()
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            move()
            torch.cuda.synchronize()
            for k, fn in calls.items():
                times[k].append(event_us(fn))
        assert env.cost_to_go_builds == b0, "the timed calls built fields"
        # the last repetition's results describe one state: the new call equals the composition
        assert torch.equal(x7, cat) and torch.equal(x7h, cath) and torch.equal(x7h, x7.to(torch.bfloat16))
        assert torch.equal(x8[:, :, (0, 1, 2, 4, 5, 6, 7)], x7)
        env.close()
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}, {args.reps} reps after {args.warmup} warm-up rounds, "
              f"median (min) us per call:", flush=True)
        med = {}
        for k, v in times.items():
            v.sort()
            med[k] = v[len(v) // 2]
            print(f"  {k:26s} {med[k]:9.1f} ({v[0]:9.1f}) us   result {nbytes[k] / 1e6:9.2f} MB = "
                  f"{nbytes[k] / med[k] / 1e3:8.1f} GB/s of result", flush=True)
        a, b = med[KA], med[KB]
        spread = b - times[KB][0]
        rate = nbytes[KA] / (a * 1e-6)
        print(f"  (b) / (a) = {b / a:.2f}   (c') / (c) = {med[KC2] / med[KC]:.2f}   "
              f"margin: (b)'s min-to-median spread {spread:.1f} us; (a) is {'faster' if a + spread < b else 'NOT faster'} "
              f"than (b) beyond it", flush=True)
        print(f"  store rate of (a): {rate / 1e9:.1f} GB/s = {100 * rate / HBM_PEAK:.1f} % of 8 TB/s", flush=True)


if __name__ == "__main__":
    main()
