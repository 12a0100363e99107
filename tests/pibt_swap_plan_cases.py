"""The states the GPU suite of the multi-step planner with the swap operation installs (docs/SPEC.md S27) and what the
reference must report on them at least, shared by the CPU file (tests/test_pibt_swap_plan.py) and the GPU file
(tests/test_pibt_swap_plan_gpu.py).  What counts here is what the rule does at steps h >= 1 of a lookahead ("late"): step
0 is the one-step kernel's ground.  Nothing here needs a GPU.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from pibt_swap_cases import layout_case, layout_radii, solve_suite
from pibt_swap_plan_reference import late, pibt_swap_plan_reference

# agents -> (recipe of solve_suite, K): layout_case's head-on pairs swap at step 0 and have then arrived, so the small
# layouts take corridor-heavy random instances (8 x 8 or 12 x 12 at density 0.35, agents and targets two permutations of
# one component) in which agents meet inside the lookahead
SUITES = {2: (dict(n=24, size=8, density=0.35, agents=2, seed=2, min_cells=20), 12),
          3: (dict(n=24, size=8, density=0.35, agents=3, seed=3, min_cells=20), 12),
          8: (dict(n=24, size=12, density=0.35, agents=8, seed=8, min_cells=20), 12),
          16: (dict(n=24, size=12, density=0.35, agents=16, seed=16, min_cells=32), 12)}
MAX_BATCH = 24          # the reference is a Python recursion per env and step


def horizon_of(agents):
    """K of a layout's case: 12 on the suites, 6 on layout_case's states up to 256 agents, 3 above."""
    return SUITES[agents][1] if agents in SUITES else 6 if agents <= 256 else 3


def _full_range(agents, shape):
    full = np.iinfo(np.int32)
    return np.random.default_rng(1000 * agents + 27).integers(full.min, full.max + 1, size=shape).astype(np.int32)


def plan_case(agents, size, batch):
    """The states of one lane layout (a row of test_visible_agents_gpu.LAYOUTS): a list of
    (obstacles [B, H, W], agents [B, A, 2], targets [B, A, 2], priority int32 [B, A], map size, obs_radius, K).
    The priority is random over the whole int32 range; every state is planned under it and under None."""
    if agents in SUITES:
        recipe, K = SUITES[agents]
        obstacles, pos, tgt = (np.stack(v) for v in zip(*solve_suite(**recipe)))
        return [(obstacles.astype(np.uint8), pos, tgt, _full_range(agents, pos.shape[:2]), recipe["size"], 2, K)]
    r = layout_radii(agents)[0]
    obstacles, pos, tgt, _ = layout_case(agents, size, min(batch, MAX_BATCH), r)
    return [(obstacles, pos, tgt, _full_range(agents, pos.shape[:2]), size, r, horizon_of(agents))]


def add_counts(total, counters):
    """Adds a plan reference's per-step counters [K, B] to `total`: late counts by name, step 0's under "first"."""
    first = total.setdefault("first", {})
    for name in ("reversed", "usual", "clear", "pulled"):
        total[name] = total.get(name, 0) + late(counters, name)
        first[name] = first.get(name, 0) + int(np.asarray(counters[name])[0].sum())
    return total


def case_counts(agents, size, batch):
    """What the reference alone reports on plan_case's states under on_target = "finish", summed over the states and
    the two priority forms (the case's, None)."""
    total = {}
    for obstacles, pos, tgt, prio, _, _, K in plan_case(agents, size, batch):
        for p in (prio, None):
            out = pibt_swap_plan_reference(obstacles, pos, tgt, np.ones(pos.shape[:2], dtype=bool), K, p)
            add_counts(total, out[5])
    return total


# agents -> the late counts the reference reports at least on plan_case(agents, ...), summed over the states and their two
# priority forms, under `finish`.  Up to 200 agents these are the counts tests/pibt_swap_plan_reference.py reports (the
# CPU file recounts them); the larger layouts were counted once -- late reversed / clear / pulled: 257: 12 / 1 / 6,
# 342: 11 / 0 / 9, 512: 26 / 2 / 21, 513: 7 / 0 / 6, 1023: 22 / 0 / 15, 1024: 45 / 1 / 30 -- and are held to one late
# reversal.  One agent has no partner: nothing is ever reversed.  Step 0 of the suites (2 to 16 agents) reverses at most
# one list, step 0 of layout_case's states dozens: both grounds are covered.
LATE_MIN = {1: {},
            2: {"reversed": 4, "pulled": 4}, 3: {"reversed": 3, "pulled": 3}, 8: {"reversed": 12, "pulled": 12},
            16: {"reversed": 59, "pulled": 37},
            33: {"reversed": 13, "clear": 2, "pulled": 8}, 64: {"reversed": 16, "clear": 3, "pulled": 11},
            65: {"reversed": 15, "clear": 6, "pulled": 8}, 200: {"reversed": 27, "clear": 2, "pulled": 21},
            **{a: {"reversed": 1} for a in (257, 342, 512, 513, 1023, 1024)}}


def meets(total, agents):
    """The names of LATE_MIN[agents] whose count in `total` (add_counts) is too low."""
    return [name for name, least in LATE_MIN[agents].items() if total.get(name, 0) < least]


# ---- corridor states for the agreement with the step-by-step policy: solve_suite instances (12 x 12, 8 agents) in which
# the reference reverses lists at steps h >= 1, under `finish` and under `nothing`
AGREE = dict(n=24, size=12, density=0.35, agents=8, seed=8, min_cells=20, K=12)


def agreement_case():
    c = dict(AGREE)
    c.pop("K")
    obstacles, pos, tgt = (np.stack(v) for v in zip(*solve_suite(**c)))
    return obstacles.astype(np.uint8), pos, tgt
