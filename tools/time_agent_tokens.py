"""Diagnostic: device time of agent_tokens() (pgx_agent_tokens, docs/SPEC.md S21) next to the torch composition it
replaces and to a plain device fill of the same bytes, HIP events, BASELINE configs[1] and [2] in one process.  Per
configuration, with slots=13 and length=256:
    (a)  agent_tokens(history=..., length=256, out=...)
    (b)  the torch composition of the same tensor from the four queries S21 is written in: cost_to_go(),
         visible_agents(k=12), goal_directions("bits") and get_state(), then the gathers, clamps, cats and wheres
    (c)  out.fill_(64): the store stream of the same bytes with nothing else to do
on_target="nothing": the targets stay, so that no call of a timed window builds a distance field -- (a) and (b) both
refresh the cache and find it valid.  A step(compute_obs=False) of random actions runs between the repetitions, outside
the timed windows, so that the state moves; the history is a random int8 tensor.  The calls alternate inside each
repetition, so that drift of the machine hits them alike; medians and minima over the repetitions.  The run asserts that
(a) equals (b) on the last state.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU.

    python tools/time_agent_tokens.py [--reps N] [--warmup N] [--configs 1,2]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5)}  # batch, size, agents, obs_radius
SLOTS, LENGTH = 13, 256
HBM_PEAK = 8.0e12  # bytes / s
KA, KB, KC = "a agent_tokens", "b torch composition", "c fill of the same bytes"


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def compose(env, history, out):
    """S21 in torch, from the four queries, into `out`."""
    B, A, W, r = env.batch, env.num_agents, env.window, env.obs_radius
    dev = env.device
    ctg = env.cost_to_go()
    own = ctg[:, :, r, r]
    st = env.get_state()
    xy, tg = st["agents_xy"], st["targets_xy"]
    m = env.goal_directions("bits")[:, :, r, r].to(torch.int32)
    index, offset, _ = env.visible_agents(k=SLOTS - 1)
    win = ctg.view(B, A, W * W)
    blocked = (win == -1) | (own == -1).unsqueeze(-1)
    wtok = torch.where(blocked, 41, (win - own.unsqueeze(-1)).clamp(-20, 20) + 20)
    j = torch.cat((torch.arange(A, device=dev, dtype=torch.int32).view(1, A, 1).expand(B, A, 1), index), 2)
    off = torch.cat((torch.zeros((B, A, 1, 2), dtype=torch.int32, device=dev), offset.to(torch.int32)), 2)
    present = j >= 0
    jj = j.clamp(min=0).long()
    b = torch.arange(B, device=dev).view(B, 1, 1)
    goal = (tg[b, jj] - xy.unsqueeze(2)).clamp(-20, 20) + 20
    h = history.to(torch.int32)
    ht = torch.where((h >= 0) & (h <= 4), 43 + h, 42)
    slot = torch.cat((off + 20, goal, ht[b, jj], (48 + m[b, jj]).unsqueeze(-1)), -1)
    slot = torch.where(present.unsqueeze(-1), slot, 64)
    l0 = W * W + 10 * SLOTS
    out[:, :, :W * W] = wtok
    out[:, :, W * W:l0] = slot.view(B, A, 10 * SLOTS)
    out[:, :, l0:] = 64
    out.masked_fill_(~st["is_active"].bool().unsqueeze(-1), 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="1,2")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("time_agent_tokens.py needs a GPU")
    for c in (int(x) for x in args.configs.split(",")):
        B, S, A, r = CONFIGS[c]
        env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="priority",
                                   on_target="nothing", max_episode_steps=10**6), batch=B)
        env.reset(seed=0)
        dev = env.device
        gen = torch.Generator(device=dev)
        gen.manual_seed(c)
        history = torch.randint(-1, 5, (B, A, 5), generator=gen, device=dev).to(torch.int8)
        fused = torch.empty((B, A, LENGTH), dtype=torch.uint8, device=dev)
        comp = torch.empty_like(fused)
        filled = torch.empty_like(fused)
        calls = {KA: lambda: env.agent_tokens(slots=SLOTS, history=history, length=LENGTH, out=fused),
                 KB: lambda: compose(env, history, comp),
                 KC: lambda: filled.fill_(64)}
        nbytes = fused.numel()

        def move():
            env.step(torch.randint(0, 5, (B, A), generator=gen, device=dev), compute_obs=False)

        for _ in range(args.warmup):              # warm-up of every kernel the windows use; the first builds the fields
            move()
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        built = env.cost_to_go_builds
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            move()
            torch.cuda.synchronize()
            for k, fn in calls.items():
                times[k].append(event_us(fn))
        # the last repetition's results describe one state: the new call equals the composition
        assert torch.equal(fused, comp), "agent_tokens() differs from the torch composition"
        assert env.cost_to_go_builds == built, "a timed window built distance fields"
        env.close()
        print(f"configs[{c}] B={B} {S}x{S} A={A} r={r} slots={SLOTS} length={LENGTH}, {args.reps} reps after "
              f"{args.warmup} warm-up rounds, median (min .. max) us per call:", flush=True)
        med = {}
        for k, v in times.items():
            v.sort()
            med[k] = v[len(v) // 2]
            print(f"  {k:26s} {med[k]:9.1f} ({v[0]:9.1f} .. {v[-1]:9.1f}) us   result {nbytes / 1e6:8.2f} MB = "
                  f"{nbytes / med[k] / 1e3:8.1f} GB/s of result", flush=True)
        a, b, f = med[KA], med[KB], med[KC]
        spread = b - times[KB][0]
        print(f"  (b) / (a) = {b / a:.2f}   (a) / (c) = {a / f:.2f}   margin: (b)'s min-to-median spread {spread:.1f} us; "
              f"(a) is {'faster' if a + spread < b else 'NOT faster'} than (b) beyond it", flush=True)
        print(f"  store rate of (a): {nbytes / (a * 1e-6) / 1e9:.1f} GB/s = "
              f"{100 * nbytes / (a * 1e-6) / HBM_PEAK:.2f} % of 8 TB/s", flush=True)
        del fused, comp, filled, history
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
