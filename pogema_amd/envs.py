"""Single-environment, list-per-agent view of the engine: the reference's native calling convention
(upstream `pogema/envs.py` + `pogema/integrations/make_pogema.py`: `pogema_v0(grid_config)`;
SURVEY.md section 8b "what the reference exposes").

    env = pogema_v0(GridConfig(num_agents=2, size=8))
    obs, infos = env.reset()
    obs, rewards, terminated, truncated, infos = env.step([0, 3])

`obs[i]` is a float32 numpy array (3, 2r+1, 2r+1); rewards floats; terminated/truncated bools; infos
dicts with 'is_active'.  Everything is computed by the HIP engine with batch = 1 (this view exists
for API compatibility and tests, not for throughput -- use `VecPogema` for that).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._lib import DEFAULT_GLOBAL_CHANNELS as _DEFAULT_GLOBAL_CHANNELS
from ._lib import DEFAULT_POLICY_CHANNELS as _DEFAULT_POLICY_CHANNELS
from .grid_config import GridConfig
from .vec_env import VecPogema

try:  # gymnasium is optional (not installed in the build image)
    import gymnasium  # type: ignore
    _Box, _Discrete = gymnasium.spaces.Box, gymnasium.spaces.Discrete
except Exception:  # pragma: no cover - exercised only where gymnasium is missing
    class _Box:  # minimal duck-typed stand-ins
        def __init__(self, low, high, shape, dtype=np.float32):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype

        def contains(self, x):
            x = np.asarray(x)
            return x.shape == self.shape and (x >= self.low).all() and (x <= self.high).all()

    class _Discrete:
        def __init__(self, n):
            self.n = n
            self._rng = np.random.default_rng()

        def sample(self):
            return int(self._rng.integers(self.n))

        def contains(self, x):
            return 0 <= int(x) < self.n


class Pogema:
    def __init__(self, grid_config: Optional[GridConfig] = None, device="cuda:0", auto_reset=None, semantics=None):
        self.grid_config = grid_config if grid_config is not None else GridConfig(num_agents=2)
        self._vec = VecPogema(self.grid_config, batch=1, device=device, auto_reset=auto_reset, semantics=semantics)
        full = 2 * self.grid_config.obs_radius + 1
        self.observation_space = _Box(0.0, 1.0, shape=(3, full, full), dtype=np.float32)
        self.action_space = _Discrete(len(self.grid_config.MOVES))
        # `GridConfig.persistent` (upstream PersistentWrapper): one engine snapshot per step, `step_back()` restores
        self._history = [] if self.grid_config.persistent else None

    def get_num_agents(self):
        return self.grid_config.num_agents

    def sample_actions(self):
        return [self.action_space.sample() for _ in range(self.get_num_agents())]

    def _obs_list(self, obs):
        if isinstance(obs, dict):  # POMAPF / MAPF: one dict per agent, as the reference returns
            host = {k: v[0].cpu().numpy() for k, v in obs.items()}
            n = self.get_num_agents()
            per_agent = []
            for i in range(n):
                d = {k: (host[k] if k == "global_obstacles" else host[k][i]) for k in host}
                for k in ("xy", "target_xy", "global_xy", "global_target_xy"):
                    if k in d:
                        d[k] = tuple(int(c) for c in d[k])
                per_agent.append(d)
            return per_agent
        host = obs[0].cpu().numpy()
        return [host[i] for i in range(host.shape[0])]

    def reset(self, seed: Optional[int] = None, return_info: bool = True, options=None):
        if self._history is not None:
            self._history.clear()
        obs, infos = self._vec.reset(seed=seed)
        active = infos["is_active"][0].cpu().numpy()
        out = self._obs_list(obs)
        if return_info:
            return out, [{"is_active": bool(a)} for a in active]
        return out

    def _packed_io(self):
        """One device buffer for every per-step output (+ a pinned host mirror) and a pinned staging buffer for the
        actions: a step of this single-env view then costs one H2D copy, one kernel launch and ONE D2H copy instead
        of six small synchronous copies (135 -> ~45 us per step on an MI355X box)."""
        if getattr(self, "_io", None) is not None:
            return self._io
        import torch
        vec = self._vec
        A, W = vec.num_agents, vec.window
        n_obs = A * 3 * W * W * 4
        off = {"obs": 0, "rewards": n_obs, "metrics": n_obs + 4 * A}
        off["terminated"] = off["metrics"] + 4 * 6
        off["truncated"] = off["terminated"] + A
        off["is_active"] = off["truncated"] + A
        off["episode_done"] = off["is_active"] + A
        total = off["episode_done"] + 1
        dev = torch.zeros(total, dtype=torch.uint8, device=vec.device)
        host = torch.zeros(total, dtype=torch.uint8).pin_memory()
        hnp = host.numpy()
        views = {
            "obs": hnp[:n_obs].view(np.float32).reshape(A, 3, W, W),
            "rewards": hnp[off["rewards"]:off["rewards"] + 4 * A].view(np.float32),
            "metrics": hnp[off["metrics"]:off["metrics"] + 24].view(np.float32),
            "terminated": hnp[off["terminated"]:off["terminated"] + A], "truncated": hnp[off["truncated"]:off["truncated"] + A],
            "is_active": hnp[off["is_active"]:off["is_active"] + A], "episode_done": hnp[off["episode_done"]:],
        }
        act_host = torch.zeros(A, dtype=torch.int64).pin_memory()
        act_dev = torch.zeros(A, dtype=torch.int64, device=vec.device)
        base = dev.data_ptr()
        ptr = {k: base + v for k, v in off.items()}
        from . import _lib
        _lib.check(vec._lib.pgx_set_metrics_buffers(vec._handle, ptr["metrics"], ptr["episode_done"]))
        self._io = dict(dev=dev, host=host, views=views, act_host=act_host, act_np=act_host.numpy(), act_dev=act_dev, ptr=ptr)
        return self._io

    def step_back(self) -> bool:
        """Undo the last step (`PersistentWrapper.step_back`); needs GridConfig(persistent=True)."""
        if self._history is None:
            raise RuntimeError("step_back needs GridConfig(persistent=True)")
        if not self._history:
            return False
        self._vec.load_state(self._history.pop())
        return True

    def _refuse_bad_actions(self, action):
        """Semantics(bad_action='flag'): the reference indexes MOVES[action] for every ACTIVE agent before anything
        moves, so an out-of-range action raises IndexError with the state untouched.  The actions of this API are host
        values: check them here, BEFORE the engine steps (the is_active flags are fetched only when something is out
        of range).  Python's negative wrap-around (MOVES[-1]) is not reproduced: negative actions are refused."""
        acts = np.asarray(action).reshape(-1)
        out_of_range = (acts < 0) | (acts >= len(self.grid_config.MOVES))
        if out_of_range.any():
            active = self._vec.get_state()["is_active"][0].cpu().numpy().astype(bool)
            bad = int((out_of_range & active).sum())
            if bad:
                raise IndexError(f"{bad} action(s) of active agents were outside 0..{len(self.grid_config.MOVES) - 1}")

    def step(self, action):
        assert len(action) == self.get_num_agents()
        if self._vec.semantics.bad_action == "flag":
            self._refuse_bad_actions(action)
        if self._history is not None:
            self._history.append(self._vec.save_state())
        import torch
        from . import _lib
        vec = self._vec
        if vec.observation_type != "default":  # dict observations: the general (multi-copy) route
            return self._step_general(action)
        io = self._packed_io()
        io["act_np"][:] = action
        io["act_dev"].copy_(io["act_host"], non_blocking=True)
        p = io["ptr"]
        _lib.check(vec._lib.pgx_step(vec._handle, io["act_dev"].data_ptr(), 2, p["obs"], p["rewards"], p["terminated"],
                                     p["truncated"], p["is_active"], vec._stream()))
        io["host"].copy_(io["dev"], non_blocking=True)
        torch.cuda.current_stream(vec.device).synchronize()
        if vec.semantics.bad_action == "flag":  # the reference's IndexError on MOVES[action]
            bad = int(vec._lib.pgx_bad_action_count(vec._handle, vec._stream()))
            if bad < 0:
                _lib.check(bad)
            if bad:  # unreachable after _refuse_bad_actions; kept as the engine's own verdict
                raise IndexError(f"{bad} action(s) of active agents were outside 0..{len(self.grid_config.MOVES) - 1}")
        v = io["views"]
        obs = v["obs"].copy()
        info_list = [{"is_active": bool(a)} for a in v["is_active"]]
        if v["episode_done"][0]:  # metric wrappers: infos[0]['metrics'] on the step that ends the episode
            info_list[0]["metrics"] = self._metrics_dict(v["metrics"])
        return ([obs[i] for i in range(obs.shape[0])], [float(x) for x in v["rewards"]],
                [bool(x) for x in v["terminated"]], [bool(x) for x in v["truncated"]], info_list)

    def expert_actions(self, agents_as_obstacles: bool = False):
        """The shortest-path expert's action for every agent (VecPogema.expert_actions), as a list for step()."""
        actions, _ = self._vec.expert_actions(agents_as_obstacles=agents_as_obstacles)
        return [int(a) for a in actions[0].cpu().numpy()]

    def cost_to_go(self):
        """The cost-to-go window of every agent (VecPogema.cost_to_go) as a list of int32 (W, W) numpy arrays."""
        w = self._vec.cost_to_go()[0].cpu().numpy()
        return [w[i] for i in range(w.shape[0])]

    def goal_directions(self):
        """The direction-to-goal planes of every agent (VecPogema.goal_directions) as a list of uint8 (4, W, W) numpy
        arrays."""
        d = self._vec.goal_directions(format="uint8")[0].cpu().numpy()
        return [d[i] for i in range(d.shape[0])]

    def goal_paths(self, steps=None):
        """The path to the goal of every agent (VecPogema.goal_paths) as a list of (plane uint8 (W, W), (dx, dy), length)
        tuples: the marked window cells, the sub-goal's offset and the number of marked cells."""
        planes, subgoal, length = (t[0].cpu().numpy() for t in self._vec.goal_paths(steps=steps, format="uint8"))
        return [(planes[i], (int(subgoal[i][0]), int(subgoal[i][1])), int(length[i])) for i in range(planes.shape[0])]

    def agent_forecasts(self, steps=3):
        """Where the agents each agent sees will be after 1..`steps` steps (VecPogema.agent_forecasts) as a list of
        (planes uint8 (K, W, W), cells) tuples: the agent's forecast planes and its own forecast cells as K (x, y) tuples."""
        planes, cells = (t[0].cpu().numpy() for t in self._vec.agent_forecasts(steps=steps, format="uint8"))
        return [(planes[i], [(int(x), int(y)) for x, y in cells[i]]) for i in range(planes.shape[0])]

    def path_conflicts(self, paths=None, steps=3, kinds=("vertex", "edge"), arrived=None):
        """Where K-step paths collide (VecPogema.path_conflicts) as a list of (first_step, partner, kinds, count) per
        agent: ints, and the kinds of the first conflict as a tuple of names of pogema_amd.CONFLICT_KINDS.  `paths`: a
        tensor as VecPogema.path_conflicts takes it (batch 1), or None for the agents' forecasts over `steps` steps."""
        from ._lib import CONFLICT_KINDS
        first, partner, kind, count = (t[0].cpu().numpy() for t in
                                       self._vec.path_conflicts(paths=paths, steps=steps, kinds=kinds, arrived=arrived))
        return [(int(first[i]), int(partner[i]), tuple(n for n, b in CONFLICT_KINDS.items() if int(kind[i]) & b), int(count[i]))
                for i in range(first.shape[0])]

    def blocking(self, inflation=10, blockers="all"):
        """Which agents stand in the way of others (VecPogema.blocking) as two lists of ints: count[i], the number of
        agents that agent i blocks, and blocked_by[j], the number of agents that block agent j."""
        count, blocked_by = (t[0].cpu().numpy() for t in self._vec.blocking(inflation=inflation, blockers=blockers))
        return [int(c) for c in count], [int(c) for c in blocked_by]

    def policy_input(self, channels=_DEFAULT_POLICY_CHANNELS):
        """The network's input planes of every agent (VecPogema.policy_input) as a list of uint8 (C, W, W) numpy
        arrays, plane c the channel channels[c]."""
        import torch
        x = self._vec.policy_input(channels=channels, dtype=torch.uint8)[0].cpu().numpy()
        return [x[i] for i in range(x.shape[0])]

    def global_state(self, channels=_DEFAULT_GLOBAL_CHANNELS, dtype=np.uint8):
        """The whole-map planes a centralised critic reads (VecPogema.global_state) as one numpy array (C, H, W) of
        `dtype` (float32, float16 or uint8), plane c the channel channels[c]."""
        import torch
        table = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16, np.dtype(np.uint8): torch.uint8}
        try:
            key = np.dtype(dtype)
        except TypeError:
            key = None
        if key not in table:
            raise ValueError(f"dtype must be one of numpy float32, float16, uint8, got {dtype!r}")
        return self._vec.global_state(channels=channels, dtype=table[key])[0].cpu().numpy()

    def agent_tokens(self, slots: int = 13, history=None, length=None):
        """The token observations of every agent (VecPogema.agent_tokens) as one numpy uint8 array (agents, length).
        `history`: five recorded actions per agent, most recent first, as an integer array (agents, 5), None = nothing
        recorded."""
        import torch
        vec = self._vec
        if history is not None:
            history = torch.as_tensor(np.asarray(history, dtype=np.int8)[None], device=vec.device)
        return vec.agent_tokens(slots=slots, history=history, length=length)[0].cpu().numpy()

    def visible_agents(self, k: int = 13):
        """The agents each agent sees in its window (VecPogema.visible_agents): per agent a list of (j, dx, dy) tuples,
        nearest first, truncated to `k`."""
        index, offset, _ = (t[0].cpu().numpy() for t in self._vec.visible_agents(k=k))
        return [[(int(j), int(d[0]), int(d[1])) for j, d in zip(index[i], offset[i]) if j >= 0]
                for i in range(index.shape[0])]

    def pibt_actions(self, priority=None, swap=False):
        """The cooperative planner's action for every agent (VecPogema.pibt_actions), as a list for step().  `priority`:
        one integer per agent, None = all equal.  `swap=True`: the planner with the swap operation (docs/SPEC.md S23)."""
        import torch
        vec = self._vec
        if priority is not None:
            priority = torch.as_tensor(np.asarray(priority, dtype=np.int64)[None], device=vec.device)
        actions, _ = vec.pibt_actions(priority=priority, swap=swap)
        return [int(a) for a in actions[0].cpu().numpy()]

    def pibt_plan(self, horizon, priority=None, swap=False):
        """The cooperative planner's actions for the next `horizon` steps (VecPogema.pibt_plan), as one list per step
        for step().  `priority`: one integer per agent for the first step, None = all equal; they grow inside the
        lookahead.  `swap=True`: every step plans with the swap operation (docs/SPEC.md S27)."""
        import torch
        vec = self._vec
        if priority is not None:
            priority = torch.as_tensor(np.asarray(priority, dtype=np.int64)[None], device=vec.device)
        actions = vec.pibt_plan(horizon, priority=priority, swap=swap)[0]
        return [[int(a) for a in row] for row in actions[:, 0].cpu().numpy()]

    def whca_plan(self, horizon, priority=None):
        """Windowed cooperative A* paths for the next `horizon` steps (VecPogema.whca_plan), as one list of actions per
        step for step().  `priority`: one integer per agent, None = all equal; an agent the planner could not serve
        stays on its cell (VecPogema.whca_plan reports which)."""
        import torch
        vec = self._vec
        if priority is not None:
            priority = torch.as_tensor(np.asarray(priority, dtype=np.int64)[None], device=vec.device)
        actions = vec.whca_plan(horizon, priority=priority)[0]
        return [[int(a) for a in row] for row in actions[:, 0].cpu().numpy()]

    def repair_plan(self, paths, replan=None, priority=None):
        """A plan repaired (VecPogema.repair_plan), as one list of actions per step for step().  `paths`: nested lists
        [K][agents][2], the cell after each step; `replan`: one truth value per agent, None = only the agents whose
        given path cannot be walked are replanned; `priority`: one integer per agent, None = all equal."""
        import torch
        vec = self._vec
        paths = torch.as_tensor(np.asarray(paths, dtype=np.int32)[:, None], device=vec.device).contiguous()
        if replan is not None:
            replan = torch.as_tensor(np.asarray(replan, dtype=bool)[None], device=vec.device)
        if priority is not None:
            priority = torch.as_tensor(np.asarray(priority, dtype=np.int64)[None], device=vec.device)
        actions = vec.repair_plan(paths, replan=replan, priority=priority)[0]
        return [[int(a) for a in row] for row in actions[:, 0].cpu().numpy()]

    def shield_actions(self, scores, priority=None):
        """A policy's action scores made jointly collision-free (VecPogema.shield_actions), as a list for step().
        `scores`: array-like [agents, 5], one score per agent and action, higher is better; `priority`: one integer per
        agent, None = all equal."""
        import torch
        vec = self._vec
        scores = torch.as_tensor(np.asarray(scores, dtype=np.float32)[None], device=vec.device)
        if priority is not None:
            priority = torch.as_tensor(np.asarray(priority, dtype=np.int64)[None], device=vec.device)
        actions, _, _ = vec.shield_actions(scores, priority=priority)
        return [int(a) for a in actions[0].cpu().numpy()]

    def move_outcomes(self, actions):
        """What the move phase of step(actions) would do to every agent (VecPogema.move_outcomes): per agent a dict
        with `next_xy` (row, col), `outcome` (a name of pogema_amd.OUTCOMES) and `blocker` (an agent index or None)."""
        from ._lib import OUTCOMES
        next_xy, outcome, blocker, _ = (t[0].cpu().numpy() for t in
                                        self._vec.move_outcomes(np.asarray(actions, dtype=np.int64)[None]))
        return [{"next_xy": (int(next_xy[i, 0]), int(next_xy[i, 1])), "outcome": OUTCOMES[int(outcome[i])],
                 "blocker": int(blocker[i]) if blocker[i] >= 0 else None} for i in range(outcome.shape[0])]

    def _metrics_dict(self, values):
        from ._lib import METRIC_NAMES
        metrics = {k: float(x) for k, x in zip(METRIC_NAMES, values)}
        if self.grid_config.on_target == "restart":
            return {"avg_throughput": metrics["avg_throughput"]}
        metrics.pop("avg_throughput")
        return metrics

    def _step_general(self, action):
        obs, rewards, terminated, truncated, infos = self._vec.step(np.asarray(action, dtype=np.int64)[None])
        info_list = [{"is_active": bool(v)} for v in infos["is_active"][0].cpu().numpy()]
        if bool(infos["episode_done"][0]):
            info_list[0]["metrics"] = self._metrics_dict(infos["metrics"][0].cpu().numpy())
        return (self._obs_list(obs), [float(v) for v in rewards[0].cpu().numpy()],
                [bool(v) for v in terminated[0].cpu().numpy()], [bool(v) for v in truncated[0].cpu().numpy()],
                info_list)

    # ---- state accessors in the style of `Grid.get_agents_xy` etc. (unpadded coordinates) ----------
    def get_agents_xy(self):
        return [tuple(int(c) for c in p) for p in self._vec.get_state()["agents_xy"][0].cpu().numpy()]

    def get_targets_xy(self):
        return [tuple(int(c) for c in p) for p in self._vec.get_state()["targets_xy"][0].cpu().numpy()]

    def get_obstacles(self):
        """Unpadded obstacle map (`Grid.get_obstacles(ignore_borders=True)`), int array [H, W]."""
        return self._vec._initial[0][0].cpu().numpy().astype(np.int64)

    def get_agents_xy_relative(self):
        """Agent cells relative to their start cells (`Grid.get_agents_xy_relative`)."""
        start = self._vec._initial[1][0].cpu().numpy()
        return [(int(x - sx), int(y - sy)) for (x, y), (sx, sy) in zip(self.get_agents_xy(), start)]

    def get_targets_xy_relative(self):
        start = self._vec._initial[1][0].cpu().numpy()
        return [(int(x - sx), int(y - sy)) for (x, y), (sx, sy) in zip(self.get_targets_xy(), start)]

    def get_state(self):
        """`Grid.get_state`-style export: obstacles, agents, targets, active flags (unpadded coordinates)."""
        st = self._vec.get_state()
        return {"obstacles": self.get_obstacles(), "agents_xy": self.get_agents_xy(), "targets_xy": self.get_targets_xy(),
                "is_active": [bool(v) for v in st["is_active"][0].cpu().numpy()], "elapsed": int(st["elapsed"][0])}

    def render(self, mode: str = "ansi"):
        """Text rendering of the current state (upstream `pogema/utils.py: render_grid`, console view): '#' obstacle,
        '.' free, lowercase letter = agent, the same letter in uppercase = its target ('*' agent standing on its own
        target; hidden/finished agents are not drawn).  Returns the string (and prints it when mode == 'human')."""
        obstacles = self.get_obstacles()
        st = self.get_state()
        rows = [["#" if v else "." for v in row] for row in obstacles]
        names = "abcdefghijklmnopqrstuvwxyz"
        for i, (tx, ty) in enumerate(st["targets_xy"]):
            rows[tx][ty] = names[i % 26].upper()
        for i, ((x, y), active) in enumerate(zip(st["agents_xy"], st["is_active"])):
            if active:
                rows[x][y] = "*" if (x, y) == tuple(st["targets_xy"][i]) else names[i % 26]
        text = "\n".join("".join(r) for r in rows)
        if mode == "human":
            print(text)
        return text

    def close(self):
        self._vec.close()


class PogemaParallel:
    """PettingZoo-parallel-style dict view (agent names 'player_i'); thin adapter over `Pogema`."""

    def __init__(self, grid_config: Optional[GridConfig] = None, device="cuda:0"):
        self._env = Pogema(grid_config, device=device)
        self.possible_agents = [f"player_{i}" for i in range(self._env.get_num_agents())]
        self.agents = list(self.possible_agents)

    def observation_space(self, agent):
        return self._env.observation_space

    def action_space(self, agent):
        return self._env.action_space

    def reset(self, seed=None, options=None):
        obs, infos = self._env.reset(seed=seed)
        self.agents = list(self.possible_agents)
        return dict(zip(self.possible_agents, obs)), dict(zip(self.possible_agents, infos))

    def step(self, actions: dict):
        acts = [int(actions.get(name, 0)) for name in self.possible_agents]
        obs, rew, term, trunc, infos = self._env.step(acts)
        names = self.possible_agents
        self.agents = [n for n, t, tr in zip(names, term, trunc) if not (t or tr)]
        return (dict(zip(names, obs)), dict(zip(names, rew)), dict(zip(names, term)), dict(zip(names, trunc)),
                dict(zip(names, infos)))


class PogemaSampleFactory(Pogema):
    """`integration='SampleFactory'` view (upstream `pogema/integrations/sample_factory.py`: AutoResetWrapper over
    IsMultiAgentWrapper over MetricsForwardingWrapper): multi-agent lists, auto-reset inside `step()` (done by the
    engine), `is_multiagent` / `num_agents` attributes, episode metrics copied to `infos[i]['episode_extra_stats']`."""

    is_multiagent = True

    def __init__(self, grid_config: Optional[GridConfig] = None, device="cuda:0"):
        super().__init__(grid_config, device=device, auto_reset=True)

    @property
    def num_agents(self):
        return self.get_num_agents()

    def step(self, action):
        obs, rewards, terminated, truncated, infos = super().step(action)
        for info in infos:
            if "metrics" in info:
                info["episode_extra_stats"] = dict(info["metrics"])
        return obs, rewards, terminated, truncated, infos


class PogemaSingleAgent:
    """`integration='gymnasium'` view for `num_agents == 1` (upstream `SingleAgentWrapper`): plain gymnasium
    signature with scalar reward / flags and one observation array."""

    def __init__(self, grid_config: Optional[GridConfig] = None, device="cuda:0"):
        self._env = Pogema(grid_config, device=device)
        if self._env.get_num_agents() != 1:
            raise ValueError("integration='gymnasium' is the single-agent view: num_agents must be 1")
        self.observation_space, self.action_space = self._env.observation_space, self._env.action_space
        self.grid_config = self._env.grid_config

    def reset(self, seed: Optional[int] = None, options=None):
        obs, infos = self._env.reset(seed=seed)
        return obs[0], infos[0]

    def step(self, action):
        obs, rew, term, trunc, infos = self._env.step([int(action)])
        return obs[0], rew[0], term[0], trunc[0], infos[0]

    def close(self):
        self._env.close()


def pogema_v0(grid_config: Optional[GridConfig] = None, device="cuda:0", semantics=None):
    """Factory with the reference's name: dispatches on `GridConfig.integration`.  `semantics`
    (pogema_amd.Semantics) selects the variants of the low-confidence recollections; default: PGX_SEMANTICS or the
    recalled behaviour."""
    gc = grid_config if grid_config is not None else GridConfig(num_agents=2)
    if gc.integration is None:
        return Pogema(gc, device=device, semantics=semantics)
    if gc.integration == "gymnasium":
        return PogemaSingleAgent(gc, device=device)
    if gc.integration == "PettingZoo":
        return PogemaParallel(gc, device=device)
    if gc.integration == "SampleFactory":
        return PogemaSampleFactory(gc, device=device)
    raise NotImplementedError(f"integration={gc.integration!r} is outside the hot-path scope of this build")
