"""Diagnostic: device time of visible_agents() (pgx_visible_agents) next to step() of the same shape and next to the
torch formulation it replaces -- get_state(), a [B, A, A] broadcast compare and a top-k on the packed key -- with HIP
events, median after warm-up, for the BASELINE configs[1..4] shapes and K = 8, 13, 32.  One child process per shape.  The
torch formulation only runs where its intermediates fit into the free device memory; its result is compared with the
engine's before it is timed.  docs/EXPERIMENTS.md records the numbers.  Needs a GPU; fails without one.

    python tools/time_visible_agents.py [--reps N] [--configs 1,2,3,4] [--ks 8,13,32]
    python tools/time_visible_agents.py --child 2      # one shape in this very process (what a profiler should wrap)
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {1: (1024, 16, 8, 5), 2: (8192, 64, 64, 5), 3: (8192, 32, 16, 5), 4: (4096, 256, 256, 7)}  # batch, size, agents, r
# bytes the torch formulation holds per (env, i, j) pair at its peak: d int32 x 2, |d| temporaries, the squared distance,
# the key and its masked copy (int32 each), three bool masks
TORCH_BYTES_PER_PAIR = 8 + 8 + 4 + 4 + 4 + 3


def timed(fn, reps, warmup=3):
    """Median device time of fn() in microseconds, one event pair per call."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2]


def torch_formulation(env, k):
    """What a caller does without the entry point: (index, offset, count) of docs/SPEC.md S12 from get_state()."""
    import torch
    r, A = env.obs_radius, env.num_agents
    st = env.get_state()
    xy, act = st["agents_xy"], st["is_active"]
    d = xy[:, None, :, :] - xy[:, :, None, :]                       # [B, i, j, 2] = xy_j - xy_i
    dx, dy = d[..., 0], d[..., 1]
    j = torch.arange(A, dtype=torch.int32, device=xy.device)
    vis = (dx.abs() <= r) & (dy.abs() <= r) & act[:, None, :] & act[:, :, None] & (j[None, :, None] != j[None, None, :])
    key = ((dx * dx + dy * dy) << 20) | ((dx + r) << 15) | ((dy + r) << 10) | j
    empty = torch.iinfo(torch.int32).max
    key = torch.where(vis, key, empty)
    vals = torch.topk(key, min(k, A), dim=2, largest=False, sorted=True).values
    if k > A:
        vals = torch.nn.functional.pad(vals, (0, k - A), value=empty)
    none = vals == empty
    index = torch.where(none, -1, vals & 1023)
    off = torch.stack((((vals >> 15) & 31) - r, ((vals >> 10) & 31) - r), dim=-1)
    offset = torch.where(none[..., None], 0, off).to(torch.int8)
    return index, offset, vis.sum(dim=2, dtype=torch.int32)


def child(c, reps, ks):
    import torch
    from pogema_amd import GridConfig, VecPogema
    if not torch.cuda.is_available():
        raise SystemExit("time_visible_agents.py needs a GPU")
    B, S, A, r = CONFIGS[c]
    reps = min(reps, 5) if c == 4 else reps
    env = VecPogema(GridConfig(size=S, num_agents=A, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                               max_episode_steps=10**6), batch=B)
    env.reset(seed=0)
    acts = torch.zeros((B, A), dtype=torch.int64, device="cuda")     # noop: the state stays put
    env.step(acts)
    step_us = timed(lambda: env.step(acts), reps)
    count = env.visible_agents(k=1)[2]
    print(f"configs[{c}] B={B} {S}x{S} A={A} r={r}: step {step_us:.1f} us; visible agents per agent: mean "
          f"{count.float().mean().item():.2f}, max {int(count.max())}", flush=True)
    need = B * A * A * TORCH_BYTES_PER_PAIR
    for k in ks:
        out = (torch.empty((B, A, k), dtype=torch.int32, device="cuda"), torch.empty((B, A, k, 2), dtype=torch.int8, device="cuda"),
               torch.empty((B, A), dtype=torch.int32, device="cuda"))
        call_us = timed(lambda: env.visible_agents(k=k, out=out), reps)
        moved = B * A * (5 + 6 * k + 4)
        free = torch.cuda.mem_get_info()[0]
        if need > free // 2:
            torch_txt = f"does not fit ({need / 1e9:.1f} GB of intermediates, {free / 1e9:.1f} GB free)"
        else:
            ref = torch_formulation(env, k)
            same = all(torch.equal(x, y) for x, y in zip(out, ref))
            del ref
            torch_us = timed(lambda: torch_formulation(env, k), reps)
            torch_txt = f"{torch_us:10.1f} us ({torch_us / call_us:.0f} x the call, {'equal' if same else 'DIFFERENT'} result)"
        print(f"  K={k:2d}: visible_agents {call_us:8.1f} us = {100 * call_us / step_us:5.1f} % of step "
              f"({moved / 1e6:.1f} MB moved) | torch formulation {torch_txt}", flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per number (5 at configs[4])")
    ap.add_argument("--configs", default="1,2,3,4")
    ap.add_argument("--ks", default="8,13,32")
    ap.add_argument("--child", type=int, default=0, help="run this one shape in this process instead of one child process per shape")
    args = ap.parse_args()
    ks = [int(x) for x in args.ks.split(",")]
    if args.child:
        return child(args.child, args.reps, ks)
    for c in (int(x) for x in args.configs.split(",")):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(c), "--reps", str(args.reps),
                             "--ks", args.ks], timeout=600).returncode
        if rc != 0:
            raise SystemExit(f"configs[{c}] failed with status {rc}")


if __name__ == "__main__":
    main()
