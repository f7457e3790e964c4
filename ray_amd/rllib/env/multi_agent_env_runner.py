"""Multi-agent EnvRunner (reference: rllib/env/multi_agent_env_runner.py,
rllib/env/multi_agent_episode.py).

Steps ``num_envs_per_env_runner`` MultiAgentEnvs; each acting agent is routed to an
RLModule through ``policy_mapping_fn(agent_id, episode_id)`` (evaluated once per agent per
episode), and all agents that share a module are batched into one forward pass.

The output keeps the time-major [T, B] layout the HIP GAE kernel consumes: every
(env, agent, module) triple seen in the fragment is one column of its module's batch.
A column is that agent's OWN timeline -- row k is its k-th completed action -- right-
aligned in the T rows; the leading rows are padding with ``terminateds = 1`` (the GAE /
V-trace recursions never cross them) and ``loss_mask = 0`` (the learners drop them), so
advantages of the real rows are exact.

Credit assignment (reference: MultiAgentEpisode's per-agent reward buffers): an action is
a *pending* row until its outcome is known -- rewards paid to the agent in later steps
(turn-based games pay the mover after the opponent's reply) accumulate into it, and it
is completed when the agent is asked to act again (or is in the very next observation
dict: simultaneous-move envs complete every row in the step it was taken) or when the
agent's episode ends. A pending row carries over to the next fragment; the column's
bootstrap observation is the state the agent acts on next, i.e. that pending row's obs.
Agents act only when they receive an observation, so turn-based envs (one mover per
step) and simultaneous-move envs share this runner."""


from __future__ import annotations

import time
from collections import defaultdict

import numpy as np
import torch

from ray_amd.rllib.core.rl_module import RLModule
from ray_amd.rllib.env.envs import make_env

DEFAULT_MODULE_ID = "default_policy"


def _default_mapping(agent_id, episode=None, **kw):
    return DEFAULT_MODULE_ID


class MultiAgentEnvRunner:
    def __init__(self, config: dict, worker_index: int = 0):
        torch.set_num_threads(int(config.get("num_cpus_per_env_runner", 1) or 1))
        self.config = config
        self.worker_index = worker_index
        n = int(config.get("num_envs_per_env_runner", 1))
        seed = config.get("seed")
        self.envs = []
        for i in range(n):
            ec = dict(config.get("env_config") or {})
            ec.setdefault("seed", (seed or 0) * 1000 + worker_index * 100 + i)
            self.envs.append(make_env(config["env"], ec))
        self.mapping_fn = config.get("policy_mapping_fn") or _default_mapping
        self.specs = config["_module_specs"]
        self.module_kind = config.get("module_kind", "actor_critic")
        self.modules = {mid: self._make_module(os_, as_, mid).eval()
                        for mid, (os_, as_) in self.specs.items()}
        self.obs, self.alive, self.agent_module, self.pending = [], [], [], []
        self.ep_ret = np.zeros(n)
        self.ep_len = np.zeros(n, dtype=np.int64)
        self.ep_agent_ret = [defaultdict(float) for _ in range(n)]
        self._ep_counter = 0
        self.ep_ids = [None] * n
        for i, e in enumerate(self.envs):
            o, _ = e.reset(seed=None if seed is None else seed * 1000 + worker_index * 100 + i)
            self._start_episode(i, o)
        self.done_returns, self.done_lengths = [], []
        self.done_module_returns = defaultdict(list)
        self.weights_version = -1
        self.total_steps = 0

    def _start_episode(self, i, obs):
        if len(self.obs) <= i:
            self.obs.append(None)
            self.alive.append(None)
            self.agent_module.append(None)
            self.pending.append(None)
        self._ep_counter += 1
        self.ep_ids[i] = f"{self.worker_index}-{i}-{self._ep_counter}"
        self.obs[i] = dict(obs)
        # turn-based envs show only the first mover at reset: every agent of the env is
        # alive until it is done (or the episode is)
        ids = self.envs[i].get_agent_ids() if hasattr(self.envs[i], "get_agent_ids") else ()
        self.alive[i] = set(ids) | set(obs)
        self.agent_module[i] = {}
        self.pending[i] = {}  # agent -> its last action awaiting its outcome

    def _make_module(self, os_, as_, mid=None):
        if self.module_kind == "q":  # multi-agent DQN: epsilon-greedy over Q-values
            from ray_amd.rllib.core.rl_module import QModule, q_model_config

            return QModule(os_, as_, q_model_config(self.config))
        if self.module_kind == "sac":  # multi-agent SAC: the squashed-Gaussian actor
            from ray_amd.rllib.core.rl_module import SquashedGaussianPolicy

            return SquashedGaussianPolicy(os_, as_, self.config.get("policy_model_config")
                                          or self.config.get("model"))
        from ray_amd.rllib.core.rl_module.rl_module import build_module

        return build_module(self.config, os_, as_, mid)

    def _act(self, mod, x, explore, epsilon, as_):
        """(actions, logp, dist inputs) for a stacked observation batch."""
        if self.module_kind == "q":
            if getattr(mod, "noisy", False):  # noisy nets explore through parameter noise
                mod.set_explore(explore)
                mod.reset_noise()
            q = mod(x).float()
            a = q.argmax(-1).numpy()
            if explore and epsilon:
                rnd = np.random.random(len(a)) < epsilon
                a = np.where(rnd, np.random.randint(0, as_.n, len(a)), a)
            return a, np.zeros(len(a), np.float32), q.numpy()
        if self.module_kind == "sac":
            a, lp = mod(x.float(), explore)
            a, lp = a.float().numpy(), lp.float().numpy()
            return a, lp, np.zeros((len(a), 1), np.float32)
        di = mod.forward_inference(x)["action_dist_inputs"]
        a, lp = mod.sample_actions(di, explore)
        return a.cpu().numpy(), lp.cpu().numpy(), di.float().cpu().numpy()

    def _module_of(self, i, aid):
        m = self.agent_module[i].get(aid)
        if m is None:
            m = self.mapping_fn(aid, self.ep_ids[i])
            if m not in self.modules:
                raise ValueError(f"policy_mapping_fn mapped agent {aid!r} to unknown module "
                                 f"{m!r}; known: {sorted(self.modules)}")
            self.agent_module[i][aid] = m
        return m

    # ---------------------------------------------------------------- weights
    def set_weights(self, weights, version: int = 0):
        if version is not None and version == self.weights_version:
            return
        for mid, w in weights.items():
            if mid in self.modules:
                self.modules[mid].load_state_dict(
                    {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v))
                     for k, v in w.items()})
        self.weights_version = version

    def get_weights(self):
        return {mid: {k: v.detach().cpu() for k, v in m.state_dict().items()}
                for mid, m in self.modules.items()}

    # ---------------------------------------------------------------- module set
    def add_module(self, module_id, spaces, weights=None):
        """A module added mid-training (Algorithm.add_module): built here for inference,
        with ``weights`` when given."""
        os_, as_ = spaces
        self.specs = dict(self.specs)
        self.specs[module_id] = (os_, as_)
        m = self._make_module(os_, as_, module_id).eval()
        if weights is not None:
            m.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()})
        self.modules[module_id] = m
        return True

    def remove_module(self, module_id):
        """Drop a module; agents of episodes in progress that acted with it are re-mapped
        on their next step (their unfinished rows of the removed module are dropped)."""
        self.modules.pop(module_id, None)
        self.specs = {k: v for k, v in self.specs.items() if k != module_id}
        for i in range(len(self.envs)):
            for aid, m in list(self.agent_module[i].items()):
                if m == module_id:
                    del self.agent_module[i][aid]
            for aid, row in list(self.pending[i].items()):
                if row["module"] == module_id:
                    del self.pending[i][aid]
        return True

    def set_mapping_fn(self, fn):
        """New agent -> module mapping; episodes in progress keep their agents' modules
        (the mapping is evaluated once per agent per episode)."""
        self.mapping_fn = fn
        return True

    def apply(self, fn_blob):
        """Run ``fn(env_runner)`` here (Algorithm.env_runner_group.foreach_env_runner)."""
        import cloudpickle

        return cloudpickle.loads(fn_blob)(self)

    def ping(self):
        return self.worker_index

    # ---------------------------------------------------------------- sampling
    def _complete(self, cols, i, aid, terminated=False, truncated=False, next_obs=None):
        """Move agent `aid`'s pending row (env i) into its column; `next_obs` is the state
        the agent acts on next (kept for the Q-learning transition)."""
        row = self.pending[i].pop(aid, None)
        if row is None:
            return
        row["next_obs"] = row["obs"] if next_obs is None else next_obs
        row["terminateds"] = 1.0 if terminated else 0.0
        row["truncateds"] = 1.0 if truncated else 0.0
        cols.setdefault((i, aid, row["module"]), []).append(row)

    def sample_with_meta(self, num_timesteps: int | None = None, explore: bool = True):
        """(batch, meta) as two objects (see SingleAgentEnvRunner.sample_with_meta)."""
        b = self.sample(num_timesteps, explore, with_metrics=True)
        meta = {"env_steps": b["env_steps"], "_metrics": b.pop("_metrics"),
                "weights_version": b.get("weights_version")}
        return b, meta

    def sample(self, num_timesteps: int | None = None, explore: bool = True,
               epsilon: float | None = None, with_metrics: bool = False):
        T = int(num_timesteps or self.config.get("rollout_fragment_length", 50))
        boot_trunc = bool(self.config.get("bootstrap_truncated"))
        cols: dict = {}   # (env, agent, module) -> completed rows, in order
        t0 = time.perf_counter()
        for _t in range(T):
            groups = defaultdict(list)
            for i in range(len(self.envs)):
                for aid in sorted(self.obs[i], key=str):
                    if aid in self.alive[i]:
                        groups[self._module_of(i, aid)].append((i, aid))
            actions = [{} for _ in self.envs]
            for mid, items in groups.items():
                mod = self.modules[mid]
                x = torch.from_numpy(np.stack([self.obs[i][aid] for i, aid in items]))
                as_ = self.specs[mid][1]
                with torch.no_grad():
                    a, lp, di = self._act(mod, x, explore, epsilon, as_)
                for j, (i, aid) in enumerate(items):
                    # acting again: the previous row is final
                    self._complete(cols, i, aid, next_obs=self.obs[i][aid])
                    self.pending[i][aid] = {"module": mid, "obs": self.obs[i][aid],
                                            "actions": a[j], "action_logp": lp[j],
                                            "action_dist_inputs": di[j], "rewards": 0.0}
                    aj = a[j]
                    actions[i][aid] = int(aj) if hasattr(as_, "n") else \
                        np.clip(aj, as_.low, as_.high)
            for i, env in enumerate(self.envs):
                o, r, te, tr, _ = env.step(actions[i])
                all_term, all_trunc = bool(te.get("__all__")), bool(tr.get("__all__"))
                for aid, rv in r.items():
                    self.ep_ret[i] += rv
                    self.ep_agent_ret[i][aid] += rv
                    row = self.pending[i].get(aid)
                    if row is not None:
                        row["rewards"] += float(rv)
                for aid in list(self.alive[i]):
                    a_te = bool(te.get(aid)) or all_term
                    a_tr = bool(tr.get(aid)) or all_trunc
                    if a_te or a_tr:
                        self._complete(cols, i, aid, terminated=a_te or not boot_trunc,
                                       truncated=a_tr, next_obs=o.get(aid))
                        self.alive[i].discard(aid)
                self.ep_len[i] += 1
                if all_term or all_trunc or not self.alive[i]:
                    for aid in list(self.pending[i]):
                        self._complete(cols, i, aid, terminated=True)
                    self.done_returns.append(float(self.ep_ret[i]))
                    self.done_lengths.append(int(self.ep_len[i]))
                    for aid, rv in self.ep_agent_ret[i].items():
                        self.done_module_returns[self.agent_module[i].get(aid, "?")].append(rv)
                    self.ep_ret[i], self.ep_len[i] = 0.0, 0
                    self.ep_agent_ret[i] = defaultdict(float)
                    o, _ = env.reset()
                    self._start_episode(i, o)
                else:
                    self.obs[i] = {aid: ob for aid, ob in o.items() if aid in self.alive[i]}
                    for aid in self.obs[i]:  # asked to act next step: its reward is in
                        self._complete(cols, i, aid, next_obs=self.obs[i][aid])
        env_steps = T * len(self.envs)
        self.total_steps += env_steps
        modules = {}
        for mid in self.modules:
            keys = sorted((k for k in cols if k[2] == mid), key=lambda k: (k[0], str(k[1])))
            if not keys:
                continue
            B = len(keys)
            os_, as_ = self.specs[mid]
            discrete = hasattr(as_, "n")
            b = {"obs": np.zeros((T, B) + tuple(os_.shape), dtype=os_.dtype),
                 "actions": np.zeros((T, B) if discrete else (T, B) + tuple(as_.shape),
                                     dtype=np.int64 if discrete else np.float32),
                 "rewards": np.zeros((T, B), np.float32),
                 "terminateds": np.ones((T, B), np.float32),  # padding cuts the recursion
                 "truncateds": np.zeros((T, B), np.float32),
                 "action_logp": np.zeros((T, B), np.float32),
                 "loss_mask": np.zeros((T, B), np.float32)}
            ndi = len(cols[keys[0]][0]["action_dist_inputs"])
            b["action_dist_inputs"] = np.zeros((T, B, ndi), np.float32)
            fields = ["obs", "actions", "rewards", "terminateds", "truncateds", "action_logp",
                      "action_dist_inputs"]
            if self.module_kind in ("q", "sac"):
                b["next_obs"] = np.zeros_like(b["obs"])
                fields.append("next_obs")
            boot = np.zeros((B,) + tuple(os_.shape), dtype=os_.dtype)
            for j, k in enumerate(keys):
                rows = cols[k]
                s0 = T - len(rows)  # right-aligned: the last real row meets the bootstrap
                for f in fields:
                    b[f][s0:, j] = np.stack([np.asarray(rw[f]) for rw in rows])
                b["loss_mask"][s0:, j] = 1.0
                i, aid, m = k
                nxt = self.pending[i].get(aid)
                if nxt is not None and nxt["module"] == m:
                    boot[j] = nxt["obs"]
                elif aid in self.obs[i] and self.agent_module[i].get(aid) == m:
                    boot[j] = self.obs[i][aid]
            b["bootstrap_obs"] = boot
            b["env_steps"] = env_steps
            b["agent_steps"] = int(b["loss_mask"].sum())
            modules[mid] = b
        out = {"modules": modules, "env_steps": env_steps,
               "agent_steps": sum(b["agent_steps"] for b in modules.values()),
               "sample_time_s": time.perf_counter() - t0,
               "weights_version": self.weights_version}
        if with_metrics:
            out["_metrics"] = self.get_metrics()
        return out

    def get_metrics(self):
        out = {"episode_returns": self.done_returns, "episode_lengths": self.done_lengths,
               "module_episode_returns": dict(self.done_module_returns),
               "num_env_steps": self.total_steps}
        self.done_returns, self.done_lengths = [], []
        self.done_module_returns = defaultdict(list)
        return out

    def stop(self):
        for e in self.envs:
            e.close()
