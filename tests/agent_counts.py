"""Agent counts between 257 and 1023, the range in which every kernel's lane layout changes shape and which the
layouts of the other suites step over: the counts, their maps and batches, the integer formulas of the kernels restated in
Python, and the hand-built states the CPU file (tests/test_agent_counts.py) and the GPU file
(tests/test_agent_counts_gpu.py) share.  Nothing here needs a GPU.  Test infrastructure only."""
from __future__ import annotations

import contextlib
import ctypes as C
import zlib

import numpy as np

from util import generate_instances, random_actions

MAX_LANES = 1024          # lanes of the PIBT-family workgroup above 256 agents (T in pgx_pibt.hip, pgx_outcomes.hip)
NB_THREADS = 256          # lanes of a neighbour-list workgroup (pgx_neighbours.hip)

AGENT_COUNTS = (
    257,    # one agent more than four waves: 5 waves, the last holds one lane; the first count with epb = 3 and with a second
            # neighbour chunk, which holds ONE row; the first count that needs a 9th closure round
    320,    # exactly 5 full waves; epb = 3 with 64 idle tail lanes
    341,    # the last count with epb = 3 (3 * 341 = 1023 lanes, one idle); 6 waves, the last ragged
    342,    # the first count with epb = 2 (3 * 342 > 1024): 340 idle tail lanes
    511,    # 8 waves, one lane short of full; the reservation set (1024 words) two words above 2A
    512,    # exactly 8 full waves; the last count with epb = 2, no idle lane; the reservation set exactly 2A words; the last
            # count with 9 closure rounds; two FULL neighbour chunks
    513,    # the first count with epb = 1, log2n = 11 and a 10th closure round; 9 waves, the last holds one lane; a third
            # neighbour chunk of one row
    640,    # exactly 10 full waves
    769,    # 13 waves, the last holds one lane; a fourth neighbour chunk of one row
    960,    # exactly 15 full waves
    961,    # 16 waves as at 1024, the last holds one lane
    1023,   # 16 waves, one lane short of 1024; a last neighbour chunk of 255 rows; one idle lane in the workgroup
)

# count -> (height, width, batch, obs_radius).  Half of the maps have both sides <= 64 (the small cost-to-go layout), the
# other half one side above 64 (the large one); density 0.1 throughout.  The batch leaves the last PIBT-family workgroup
# partly filled wherever a workgroup holds more than one env: 5 = 3 + 2 where epb = 3, 3 = 2 + 1 where epb = 2, and 2 where
# epb = 1.  obs_radius is the largest of RADII the engine's LDS budget admits (README.md "Limits").
RADII = (1, 5, 15)
DENSITY = 0.1
CASES = {
    257: (40, 40, 5, 15),
    320: (48, 80, 5, 15),
    341: (48, 80, 5, 15),
    342: (48, 48, 3, 15),
    511: (80, 48, 3, 5),
    512: (56, 56, 3, 5),
    513: (56, 56, 2, 5),
    640: (56, 80, 2, 5),
    769: (64, 80, 2, 5),
    960: (80, 64, 2, 5),
    961: (64, 64, 2, 5),
    1023: (64, 64, 2, 5),
}

PAIRINGS = (("soft", "finish"), ("priority", "restart"), ("block_both", "nothing"))
# the counts that additionally run the other observation formats, the forced large-map layout and the other soft rules
EXTRA_COUNTS = (257, 512, 513, 1023)
# the rows tests/test_visible_agents_gpu.py's LAYOUTS gets: (agents, map side, batch) of the square maps above
LAYOUT_ROWS = tuple((a, CASES[a][0], CASES[a][2]) for a in (257, 342, 512, 513, 1023))


# ---- the kernels' integer formulas ------------------------------------------------------------------------------------
def waves(A):
    """Waves per environment of step_kernel / rollout_kernel."""
    return (A + 63) // 64


def last_wave_lanes(A):
    return A - 64 * (waves(A) - 1)


def closure_rounds(A):
    """Pointer-doubling rounds of the step resolver and of outcomes_kernel: ceil(log2 A)."""
    rounds = 1
    while (1 << rounds) < A:
        rounds += 1
    return rounds


def pibt_geometry(A, batch):
    """(lanes, epb, log2n, workgroups, envs in the last workgroup) of pibt / shield / pibt_horizon / outcomes kernels."""
    T = 256 if A <= 256 else MAX_LANES
    epb = min(64, T // A)
    log2n = 1
    while (1 << log2n) < 2 * A:
        log2n += 1
    grid = (batch + epb - 1) // epb
    return T, epb, log2n, grid, batch - epb * (grid - 1)


def neighbour_chunk_rows(A):
    """Rows of each of the ceil(A / 256) workgroups visible_agents_kernel gives an env of more than 256 agents."""
    chunks = (A + NB_THREADS - 1) // NB_THREADS
    return [min(NB_THREADS, A - NB_THREADS * c) for c in range(chunks)]


def env_first_lanes(A, batch):
    """Lane at which each env of the first PIBT-family workgroup starts."""
    _, epb, _, _, _ = pibt_geometry(A, batch)
    return [e * A for e in range(min(epb, batch))]


# ---- what the engine admits ---------------------------------------------------------------------------------------------
def config_accepted(A, H, W, batch, r):
    """pgx_check_config on the launch shape (no device needed)."""
    from pogema_amd import _lib
    lib = _lib.load()
    cfg = _lib.PgxConfig(batch=batch, height=H, width=W, num_agents=A, obs_radius=r, collision_system=0, on_target=0,
                         max_episode_steps=64, auto_reset=1, obs_dtype=0, seed=0, env_index_base=0, random_outside=0,
                         outside_density=DENSITY, soft_vertex_rule=0, coop_reward=0, bad_action=0, lifelong_rng=0,
                         soft_occupancy=0, abi_version=_lib.PGX_ABI_VERSION)
    return lib.pgx_check_config(C.byref(cfg)) == 0


def largest_radius(A, H, W, batch, radii=RADII):
    ok = [r for r in radii if config_accepted(A, H, W, batch, r)]
    assert ok, (A, H, W)
    return max(ok)


def radii_accepted(agents, size, batch, radii=RADII):
    """The members of `radii` the engine admits for a square map (the lane-layout suites)."""
    return tuple(r for r in radii if config_accepted(agents, size, size, batch, r))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def seed_of(text):
    return zlib.crc32(text.encode()) % (2 ** 31)


def count_instance(A):
    """(obstacles, agents, targets, actions [8, B, A], obs_radius) of one count: the host generator's instance."""
    H, W, B, r = CASES[A]
    seed = seed_of(f"agent_counts/{A}")
    obstacles, agents, targets = generate_instances(B, H, W, A, DENSITY, seed)
    return obstacles, agents, targets, random_actions(8, B, A, seed + 1), r


def pairing_of(A):
    return PAIRINGS[AGENT_COUNTS.index(A) % 3]


def corridor_orders(A):
    rng = np.random.default_rng(A)
    return {"ascending": np.arange(A), "descending": np.arange(A)[::-1].copy(), "shuffled": rng.permutation(A)}


def corridor_actions(A):
    right = np.full((1, 1, A), 4, np.int64)
    return np.concatenate([right, right, random_actions(4, 1, A, 5), right])


def ring_case(A, order):
    """A agents on the A cells of a square ring, all stepping forward: (obstacles, agents, targets, first actions)."""
    n = A // 4 + 1  # a square ring with side n holds 4(n-1) = A cells
    ring = [(0, j) for j in range(n - 1)] + [(i, n - 1) for i in range(n - 1)] + \
           [(n - 1, j) for j in range(n - 1, 0, -1)] + [(i, 0) for i in range(n - 1, 0, -1)]
    assert len(ring) == A
    obstacles = np.ones((1, n, n), np.uint8)
    for c in ring:
        obstacles[0][c] = 0
    step_to = {(0, 1): 4, (1, 0): 2, (0, -1): 3, (-1, 0): 1}
    agents = np.zeros((1, A, 2), np.int32)
    acts = np.zeros((1, 1, A), np.int64)
    for k in range(A):
        cur, nxt = ring[k], ring[(k + 1) % A]
        agents[0, order[k]] = cur
        acts[0, 0, order[k]] = step_to[(nxt[0] - cur[0], nxt[1] - cur[1])]
    return obstacles, agents, agents.copy(), acts


END_VARIANTS = ("all", "first_idles", "last_idles", "middle_idles")


def idler_of(A, variant):
    """The agent that stays behind in step 1 (None: nobody)."""
    return {"all": None, "first_idles": 0, "last_idles": A - 1, "middle_idles": 64 * (waves(A) // 2) + 7}[variant]


def episode_end_case(A, variant):
    """Every agent one move above its own target on an open 64-wide map, all cells disjoint: agent k stands on
    (2 (k // 64), k % 64) and wants the cell below it.  Step 1: all move down but the variant's idler; step 2: all move
    down (the idler arrives); step 3: random.  Returns (obstacles, agents, targets, actions [3, 1, A])."""
    rows = 2 * ((A + 63) // 64)
    obstacles = np.zeros((1, rows, 64), np.uint8)
    k = np.arange(A)
    agents = np.stack([2 * (k // 64), k % 64], axis=1).astype(np.int32)[None]
    targets = agents.copy()
    targets[0, :, 0] += 1
    down = np.full((1, 1, A), 2, np.int64)
    first = down.copy()
    idler = idler_of(A, variant)
    if idler is not None:
        first[0, 0, idler] = 0
    return obstacles, agents, targets, np.concatenate([first, down, random_actions(1, 1, A, A)])


def crowd_case(A):
    """A agents packed shoulder to shoulder into one half of a small open map (from the top row down, from the left column,
    from the bottom row up, from the right column, by env), in random index order, their targets a random permutation of
    cells: pushes, inheritance chains that run through the whole pack, and branches that fail because an agent inside the
    pack has no free cell around it.  341 agents on 26 x 26 = 676 cells, 512 on 32 x 32 = 1024; the batch leaves the last
    workgroup partly filled (3 + 1 envs, 2 + 1 envs).  Returns (obstacles, agents, targets)."""
    side, batch = {341: (26, 4), 512: (32, 3)}[A]
    rng = np.random.default_rng(A)
    obstacles = np.zeros((batch, side, side), np.uint8)
    cells = np.stack(np.divmod(np.arange(side * side), side), axis=1).astype(np.int32)
    agents, targets = [], []
    for b in range(batch):
        block = cells[:A] if b % 2 == 0 else cells[:, ::-1][:A]
        if b >= 2:
            block = side - 1 - block
        agents.append(block[rng.permutation(A)])
        targets.append(cells[rng.permutation(len(cells))[:A]])
    return obstacles, np.stack(agents), np.stack(targets)


@contextlib.contextmanager
def shared_fields(obstacles, targets):
    """The planners' references ask `bfs_from` for one distance field per distinct target and call; inside this block they
    get tests/pibt_plan_reference.py's memo instead, filled for all `targets` of every map by its vectorised search (the
    same distances: pibt_plan_reference relies on it)."""
    import pibt_plan_reference
    import pibt_reference
    import shield_reference
    for b in range(len(obstacles)):
        pibt_plan_reference._prefill(np.asarray(obstacles[b]) != 0, np.asarray(targets[b]).reshape(-1, 2))
    saved = pibt_reference.bfs_from, shield_reference.bfs_from
    pibt_reference.bfs_from = shield_reference.bfs_from = pibt_plan_reference._bfs_memo
    try:
        yield
    finally:
        pibt_reference.bfs_from, shield_reference.bfs_from = saved


# ---- the slot-based queries: states shared by the CPU and the GPU file -----------------------------------------------------
# (agents, name) -> (height, width, batch, obs_radius): one map with both sides <= 64 and one with a side above 64 each
QUERY_CASES = {
    (257, "small"): (24, 24, 2, 2), (257, "large"): (8, 72, 2, 3),
    (513, "small"): (40, 40, 2, 2), (513, "large"): (20, 80, 1, 3),
    (1023, "small"): (52, 52, 1, 2), (1023, "large"): (32, 80, 1, 2),
}
QUERY_TARGETS = 12        # distinct targets per env: the references run one search per distinct target


def query_script(A, name):
    """The instance of a QUERY_CASES row with the agents sharing QUERY_TARGETS targets, and the four action arrays that
    follow the reset: mostly the reference expert's actions on the C oracle's state, some random (util.mixed_actions on
    the CPU).  Returns (obstacles, agents, targets, actions [4, B, A], states), states = the oracle's get_state() plus its
    observation `obs` after the reset and after the four steps, under collision_system "priority" and on_target
    "finish"."""
    from expert_reference import expert_reference
    from oracle.c_oracle import COracle
    H, W, B, r = QUERY_CASES[(A, name)]
    seed = seed_of(f"agent_counts/queries/{A}/{name}")
    obstacles, agents, targets = generate_instances(B, H, W, A, DENSITY, seed)
    targets = np.ascontiguousarray(targets[:, np.arange(A) % QUERY_TARGETS])
    rng = np.random.default_rng(seed)
    env = COracle(B, H, W, A, r, "priority", "finish", 64, False, seed=seed)
    env.reset(obstacles, agents, targets)
    states = [dict(env.get_state(), obs=env.observe())]
    actions = np.zeros((4, B, A), np.int64)
    for t in range(4):
        st = env.get_state()
        expert, _ = expert_reference(obstacles, st["agents_xy"], st["targets_xy"], st["is_active"].astype(bool))
        rnd = rng.integers(0, 5, size=(B, A))
        actions[t] = np.where(rng.random((B, A)) < 0.8, expert, rnd)
        env.step(actions[t])
    states.append(dict(env.get_state(), obs=env.observe()))
    env.close()
    return obstacles, agents, targets, actions, states
