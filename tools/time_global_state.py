"""Diagnostic: device time of global_state() (pgx_global_state, docs/SPEC.md S20) next to the torch composition it
replaces and to a plain device fill of the same bytes, HIP events, BASELINE configs[1], [2] and [4] in one process.  Per
configuration, for the default three planes in float32:
    (a)  global_state(out=...)
    (b)  the torch composition of the same tensor: pgx_get_map into a uint8 buffer, get_state(), the flat cell indices of
         agents and targets, two scatters into uint8 planes and the cast into the float32 result
    (c)  out.fill_(1.0): the store stream of the same bytes with nothing else to do
    (d)  global_state() with all five channels, float32 (the id instance of the kernel)
collision_system="priority" and on_target="nothing": no ghosts and every agent active for good, so (b) -- which knows no
ghost and scatters every agent's is_active, all ones -- equals (a) and the run asserts it.  A step(compute_obs=False) of
random actions runs between the repetitions, outside the timed windows, so that the state moves.  The calls alternate
inside each repetition, so that drift of the machine hits them alike; medians and minima over the repetitions.
docs/EXPERIMENTS.md records the numbers.  Needs a GPU.

    python tools/time_global_state.py [--reps N] [--warmup N] [--configs 1,2,4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema, _lib  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5), 4: (4096, 256, 256, 7)}  # batch, size, agents, obs_radius
ALL5 = ("obstacles", "agents", "targets", "agent_ids", "target_ids")
HBM_PEAK = 8.0e12  # bytes / s
KA, KB, KC, KD = "a global_state f32 x3", "b torch composition", "c fill of the same bytes", "d global_state f32 x5"


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
    ap.add_argument("--configs", default="1,2,4")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("time_global_state.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="priority",
                                   on_target="nothing", max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        dev = env.device
        x3 = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
        x5 = torch.empty((B, 5, S, S), dtype=torch.float32, device=dev)
        comp = torch.empty_like(x3)
        filled = torch.empty_like(x3)
        maps = torch.empty((B, S, S), dtype=torch.uint8, device=dev)
        marks = torch.empty((B, 2, S * S), dtype=torch.uint8, device=dev)

        def compose():
            _lib.check(env._lib.pgx_get_map(env._handle, maps.data_ptr(), env._stream()))
            st = env.get_state()
            act = st["is_active"].to(torch.uint8)
            axy, txy = st["agents_xy"].long(), st["targets_xy"].long()
            marks.zero_()
            marks[:, 0].scatter_(1, axy[..., 0] * S + axy[..., 1], act)
            marks[:, 1].scatter_(1, txy[..., 0] * S + txy[..., 1], act)
            comp[:, 0].copy_(maps)
            comp[:, 1:].copy_(marks.view(B, 2, S, S))

        calls = {KA: lambda: env.global_state(out=x3),
                 KB: compose,
                 KC: lambda: filled.fill_(1.0),
                 KD: lambda: env.global_state(channels=ALL5, out=x5)}
        nbytes = {KA: x3.numel() * 4, KB: x3.numel() * 4, KC: x3.numel() * 4, KD: x5.numel() * 4}
        gen = torch.Generator(device=dev)
        gen.manual_seed(c)

        def move():
            env.step(torch.randint(0, 5, (B, A), generator=gen, device=dev), compute_obs=False)

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
        # the last repetition's results describe one state: the new call equals the composition
        assert torch.equal(x3, comp), "global_state() differs from the torch composition"
        assert torch.equal(x5[:, :3], x3) and torch.equal(x5[:, 3:] != 0, x3[:, 1:] != 0)
        assert env.cost_to_go_builds == 0
        env.close()
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}, {args.reps} reps after {args.warmup} warm-up rounds, "
              f"median (min) us per call:", flush=True)
        med = {}
        for k, v in times.items():
            v.sort()
            med[k] = v[len(v) // 2]
            print(f"  {k:26s} {med[k]:9.1f} ({v[0]:9.1f}) us   result {nbytes[k] / 1e6:9.2f} MB = "
                  f"{nbytes[k] / med[k] / 1e3:8.1f} GB/s of result", flush=True)
        a, b, f = med[KA], med[KB], med[KC]
        spread = b - times[KB][0]
        print(f"  (b) / (a) = {b / a:.2f}   (a) / (c) = {a / f:.2f}   margin: (b)'s min-to-median spread {spread:.1f} us; "
              f"(a) is {'faster' if a + spread < b else 'NOT faster'} than (b) beyond it", flush=True)
        print(f"  store rate of (a): {nbytes[KA] / (a * 1e-6) / 1e9:.1f} GB/s = "
              f"{100 * nbytes[KA] / (a * 1e-6) / HBM_PEAK:.1f} % of 8 TB/s", flush=True)
        del x3, x5, comp, filled, maps, marks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
