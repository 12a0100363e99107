"""Diagnostic: cost of the map pool path (docs/EXPERIMENTS.md "Map pools").

  reset(seed) at the configs[2] shape (8192 envs x 64x64, 64 agents): a pool of 256 Bernoulli(0.3) maps against random
  maps of the same density (per-env obstacles + labelling), wall time per call, median of 5;
  pool install (set_map_pool: copy, labelling, capacity check, one sync);
  device time per step of step() + regenerate (auto_reset='regenerate', max_episode_steps=16, uniform random actions):
  pool vs one shared map vs random maps, CUDA events over 128 steps after 32 warm-up steps.
Run under `timeout`; prints one line per figure."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402

B, S, A, R, DENSITY, M = 8192, 64, 64, 5, 0.3, 256
POOL = (np.random.default_rng(0).random((M, S, S)) < DENSITY).astype(np.uint8)


def timed_resets(env, n=5):
    env.reset(seed=0)
    torch.cuda.synchronize()
    t = []
    for i in range(n):
        t0 = time.perf_counter()
        env.reset(seed=i + 1)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return statistics.median(t) * 1e3


def step_regen_us(env, steps=128, warmup=32):
    env.reset(seed=1)
    out = (torch.empty(env.obs_shape, dtype=torch.float32, device="cuda"),
           torch.empty((B, A), dtype=torch.float32, device="cuda"), torch.empty((B, A), dtype=torch.bool, device="cuda"),
           torch.empty((B, A), dtype=torch.bool, device="cuda"), torch.empty((B, A), dtype=torch.bool, device="cuda"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.randint(0, 5, (warmup + steps, B, A), generator=gen, device="cuda", dtype=torch.int8)
    for t in range(warmup):
        env.step(acts[t], out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(warmup, warmup + steps):
        env.step(acts[t], out=out)
    b.record()
    b.synchronize()
    fails = env.regenerate_failures()
    return a.elapsed_time(b) * 1e3 / steps, fails


def main():
    base = dict(num_agents=A, obs_radius=R, density=DENSITY, seed=0)
    env = VecPogema(GridConfig(size=S, **base), batch=B)
    print(f"reset(seed) random maps      {timed_resets(env):8.2f} ms  (configs[2]: {B} x {S}x{S}, {A} agents)", flush=True)
    env.close()
    env = VecPogema(GridConfig(size=S, **base), batch=B)  # constructed without a pool: set_map_pool timed on its own
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env.set_map_pool(POOL)
    torch.cuda.synchronize()
    print(f"set_map_pool({M} maps)         {(time.perf_counter() - t0) * 1e3:8.2f} ms  (upload + labelling + capacity check)",
          flush=True)
    t0 = time.perf_counter()
    env.set_map_pool(POOL[::-1].copy())
    torch.cuda.synchronize()
    print(f"set_map_pool again, same size {(time.perf_counter() - t0) * 1e3:8.2f} ms", flush=True)
    print(f"reset(seed) pool of {M} maps  {timed_resets(env):8.2f} ms", flush=True)
    env.close()
    rows = [("pool", dict(map_pool=POOL), GridConfig(**base, max_episode_steps=16)),
            ("shared map", {}, GridConfig(map=POOL[0].tolist(), num_agents=A, obs_radius=R, seed=0, max_episode_steps=16)),
            ("random maps", {}, GridConfig(size=S, **base, max_episode_steps=16))]
    for name, kw, gc in rows:
        env = VecPogema(gc, batch=B, auto_reset="regenerate", **kw)
        us, fails = step_regen_us(env)
        print(f"step()+regenerate {name:12s} {us:8.1f} us/step device time (max_episode_steps=16; failures {fails})",
              flush=True)
        env.close()


if __name__ == "__main__":
    main()
