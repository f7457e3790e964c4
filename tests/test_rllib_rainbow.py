"""Rainbow DQN pieces on the CPU: the config keys, the categorical (C51) projection
against hand-computed values, the distributional / noisy QModule, NoisyLinear, the
learner's C51 loss on a fixed batch, and the tuned example end to end."""

import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ray_amd.ops import reference as ref
from ray_amd.rllib.algorithms.dqn import DQNConfig, DQNLearner
from ray_amd.rllib.env import make_env

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(REPO, "ray_amd", "rllib", "tuned_examples", "dqn", "cartpole-rainbow.yaml")
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------ config
def test_config_accepts_rainbow_keys_and_they_reach_the_learner():
    cfg = DQNConfig().training(num_atoms=51, v_min=-5, v_max=5, noisy=True, sigma0=0.4)
    assert cfg.validate()
    env = make_env("CartPole-v1", {})
    lr = DQNLearner(cfg.to_dict(), env.observation_space, env.action_space, device=CPU)
    for k, v in dict(num_atoms=51, v_min=-5, v_max=5, noisy=True, sigma0=0.4).items():
        assert lr.config[k] == v
    q = lr.module["q"]
    assert q.num_atoms == 51 and q.noisy and (q.v_min, q.v_max) == (-5.0, 5.0)
    assert q.adv.sigma0 == 0.4
    assert torch.equal(q.support, torch.linspace(-5, 5, 51))


def test_config_rejects_bad_support():
    with pytest.raises(ValueError):
        DQNConfig().training(num_atoms=0).validate()
    with pytest.raises(ValueError):
        DQNConfig().training(num_atoms=51, v_min=3.0, v_max=3.0).validate()
    with pytest.raises(ValueError):
        DQNConfig().training(num_atoms=51, v_min=4.0, v_max=-4.0).validate()


def test_noisy_turns_the_default_epsilon_schedule_off():
    assert DQNConfig().epsilon_schedule() == [(0, 1.0), (10000, 0.05)]
    assert DQNConfig().training(noisy=True).epsilon_schedule() == [(0, 0.0)]
    kept = DQNConfig().training(noisy=True, epsilon=[(0, 0.5), (100, 0.1)])
    assert kept.epsilon_schedule() == [(0, 0.5), (100, 0.1)]


# -------------------------------------------------------------------------- projection
def test_c51_project_by_hand():
    # support z = [-2, -1, 0, 1, 2] (dz = 1), float64
    p = torch.tensor([[0.10, 0.20, 0.40, 0.20, 0.10],   # interior: shift by 0.5, gamma 0.5
                      [0.10, 0.20, 0.40, 0.20, 0.10],   # terminated, r = 1: exactly on an atom
                      [0.30, 0.10, 0.20, 0.15, 0.25],   # r above v_max
                      [0.30, 0.10, 0.20, 0.15, 0.25],   # r below v_min
                      [0.05, 0.05, 0.05, 0.05, 0.80],   # terminated, r = 0.25
                      [0.80, 0.05, 0.05, 0.05, 0.05]],  # the same row with another p
                     dtype=torch.float64)
    r = torch.tensor([0.5, 1.0, 25.0, -25.0, 0.25, 0.25], dtype=torch.float64)
    disc = torch.tensor([0.5, 0.9, 0.9, 0.9, 0.9, 0.9], dtype=torch.float64)
    term = torch.tensor([0.0, 1.0, 0.0, 0.0, 1.0, 1.0], dtype=torch.float64)
    m = ref.c51_project(p, r, disc, term, -2.0, 2.0).numpy()
    # row 0: Tz = 0.5 + 0.5 z = [-0.5, 0, 0.5, 1, 1.5] -> b = [1.5, 2, 2.5, 3, 3.5]
    want0 = np.zeros(5)
    want0[1] += 0.10 * 0.5
    want0[2] += 0.10 * 0.5 + 0.20 + 0.40 * 0.5
    want0[3] += 0.40 * 0.5 + 0.20 + 0.10 * 0.5
    want0[4] += 0.10 * 0.5
    np.testing.assert_allclose(m[0], want0, atol=1e-15)
    # row 1: every atom lands exactly on z = 1 (index 3): all mass there, none lost
    np.testing.assert_allclose(m[1], [0, 0, 0, 1.0, 0], atol=1e-15)
    np.testing.assert_allclose(m[2], [0, 0, 0, 0, 1.0], atol=1e-15)
    np.testing.assert_allclose(m[3], [1.0, 0, 0, 0, 0], atol=1e-15)
    # rows 4, 5: terminated -> b = 2.25 for every atom, whatever p is
    np.testing.assert_allclose(m[4], [0, 0, 0.75, 0.25, 0], atol=1e-15)
    np.testing.assert_allclose(m[5], m[4], atol=1e-15)
    np.testing.assert_allclose(m.sum(-1), np.ones(6), atol=1e-12)


def test_c51_project_rows_sum_to_one_and_match_the_hat_function_form():
    g = torch.Generator().manual_seed(3)
    B, K = 64, 51
    p = torch.softmax(torch.randn(B, K, generator=g, dtype=torch.float64), -1)
    r = 4 * torch.randn(B, generator=g, dtype=torch.float64)
    r[::3] = 0.0
    term = (torch.rand(B, generator=g) < 0.3).double()
    disc = torch.full((B,), 0.99, dtype=torch.float64)
    m = ref.c51_project(p, r, disc, term, -10.0, 10.0)
    assert (m.sum(-1) - 1).abs().max() < 1e-12
    z = torch.linspace(-10, 10, K, dtype=torch.float64)
    b = ((r[:, None] + disc[:, None] * (1 - term[:, None]) * z).clamp(-10, 10) + 10) / 0.4
    i = torch.arange(K, dtype=torch.float64)
    hat = (1 - (b[:, :, None] - i).abs()).clamp(min=0)  # [B, j, i]
    assert ((p[:, :, None] * hat).sum(1) - m).abs().max() < 1e-12


def test_c51_loss_reference_gradient_and_selection():
    g = torch.Generator().manual_seed(4)
    B, A, K = 9, 3, 11
    logits = torch.randn(B, A, K, generator=g, dtype=torch.float64, requires_grad=True)
    nxt_on = torch.randn(B, A, K, generator=g, dtype=torch.float64)
    nxt_tg = torch.randn(B, A, K, generator=g, dtype=torch.float64)
    act = torch.randint(0, A, (B,), generator=g)
    r = torch.randn(B, generator=g, dtype=torch.float64)
    disc = torch.full((B,), 0.9, dtype=torch.float64)
    term = torch.zeros(B, dtype=torch.float64)
    w = torch.rand(B, generator=g, dtype=torch.float64) + 0.2
    loss, ce, na, m = ref.c51_loss(logits, act, nxt_on, nxt_tg, r, disc, term, w, -3.0, 3.0)
    z = torch.linspace(-3, 3, K, dtype=torch.float64)
    assert torch.equal(na, (torch.softmax(nxt_on, -1) * z).sum(-1).argmax(-1))
    na_t = ref.c51_loss(logits, act, None, nxt_tg, r, disc, term, w, -3.0, 3.0)[2]
    assert torch.equal(na_t, (torch.softmax(nxt_tg, -1) * z).sum(-1).argmax(-1))
    assert torch.allclose(loss, (ce * w).mean())
    loss.backward()
    rows = torch.arange(B)
    want = torch.zeros_like(logits)
    want[rows, act] = (w / B)[:, None] * (torch.softmax(logits.detach(), -1)[rows, act] - m)
    assert torch.allclose(logits.grad, want, atol=1e-14)


# ----------------------------------------------------------------------------- modules
def test_qmodule_distributional_and_default_layout():
    from ray_amd.rllib.core.rl_module import QModule

    env = make_env("CartPole-v1", {})
    torch.manual_seed(0)
    obs = torch.randn(5, 4)
    q = QModule(env.observation_space, env.action_space,
                {"fcnet_hiddens": [32], "num_atoms": 51, "v_min": -5.0, "v_max": 5.0})
    d = q.forward_dist(obs)
    assert d.shape == (5, 2, 51)
    want = (torch.softmax(d, -1) * q.support).sum(-1)
    assert torch.allclose(q(obs), want) and q(obs).shape == (5, 2)
    # dueling per atom: the advantage stream has zero mean over actions at every atom
    h = q.encoder(obs)
    assert torch.allclose(d.mean(1), q.val(h), atol=1e-6)
    nd = QModule(env.observation_space, env.action_space,
                 {"fcnet_hiddens": [32], "num_atoms": 51, "dueling": False})
    assert nd.val is None and nd.forward_dist(obs).shape == (5, 2, 51)
    # defaults: exactly today's parameters and outputs
    torch.manual_seed(1)
    q0 = QModule(env.observation_space, env.action_space, {"fcnet_hiddens": [32]})
    assert set(q0.state_dict()) == {"encoder.net.0.weight", "encoder.net.0.bias", "adv.weight",
                                    "adv.bias", "val.weight", "val.bias"}
    assert q0.adv.weight.shape == (2, 32) and q0.val.weight.shape == (1, 32)
    h = q0.encoder(obs)
    a = q0.adv(h)
    assert torch.equal(q0(obs), q0.val(h) + a - a.mean(-1, keepdim=True))


def test_noisy_linear():
    from ray_amd.rllib.algorithms.dqn.torch.torch_noisy_linear import NoisyLinear
    from ray_amd.rllib.core.rl_module import NoisyLinear as NL2

    assert NoisyLinear is NL2
    torch.manual_seed(0)
    lin = NoisyLinear(16, 8, sigma0=0.4)
    assert set(dict(lin.named_parameters())) == {"weight_mu", "weight_sigma", "bias_mu",
                                                 "bias_sigma"}
    assert set(lin.state_dict()) == {"weight_mu", "weight_sigma", "bias_mu", "bias_sigma"}
    assert torch.allclose(lin.weight_sigma, torch.full((8, 16), 0.4 / math.sqrt(16)))
    assert torch.allclose(lin.bias_sigma, torch.full((8,), 0.4 / math.sqrt(16)))
    x = torch.randn(5, 16)
    lin.eval()
    assert torch.equal(lin(x), F.linear(x, lin.weight_mu, lin.bias_mu))
    lin.train()
    y1, y1b = lin(x), lin(x)
    assert torch.equal(y1, y1b)  # the noise is fixed between resets
    assert not torch.allclose(y1, F.linear(x, lin.weight_mu, lin.bias_mu))
    lin.reset_noise()
    assert not torch.allclose(lin(x), y1)
    # factorised noise: f(e_out) f(e_in)^T with f(x) = sign(x) sqrt|x|
    w = lin.weight_mu + lin.weight_sigma * torch.outer(lin.eps_out, lin.eps_in)
    assert torch.allclose(lin(x), F.linear(x, w, lin.bias_mu + lin.bias_sigma * lin.eps_out))
    # exploring eval forwards (env runners) are noisy too
    lin.eval()
    lin.explore = True
    assert torch.equal(lin(x), F.linear(x, w, lin.bias_mu + lin.bias_sigma * lin.eps_out))


def test_noisy_qmodule_uses_noisy_layers_everywhere():
    from ray_amd.rllib.core.rl_module import NoisyLinear, QModule

    env = make_env("CartPole-v1", {})
    torch.manual_seed(0)
    q = QModule(env.observation_space, env.action_space,
                {"fcnet_hiddens": [32, 32], "num_atoms": 51, "noisy": True, "sigma0": 0.4})
    assert isinstance(q.adv, NoisyLinear) and isinstance(q.val, NoisyLinear)
    assert all(isinstance(m, NoisyLinear) for m in list(q.encoder.net)[0::2])
    obs = torch.randn(3, 4)
    q.eval()
    y = q(obs)
    assert torch.equal(y, q(obs))
    q.set_explore(True)
    y1 = q(obs)
    q.reset_noise()
    assert not torch.allclose(q(obs), y1)
    q.set_explore(False)
    assert torch.equal(q(obs), y)


# ----------------------------------------------------------------------------- learner
def _terminal_batch(n=64, seed=0):
    rng = np.random.default_rng(seed)
    return {"obs": rng.standard_normal((n, 4)).astype(np.float32),
            "next_obs": rng.standard_normal((n, 4)).astype(np.float32),
            "actions": rng.integers(0, 2, n),
            "rewards": (3 * rng.standard_normal(n)).astype(np.float32),
            "terminateds": np.ones(n, np.float32)}


def test_learner_c51_loss_falls_on_a_fixed_batch():
    """All rows terminated: the projected target is the reward's two neighbouring atoms
    (entropy <= ln 2), whatever the networks say, so the cross-entropy can fall from
    ln 51 (near-uniform initial logits) to below half of it."""
    env = make_env("CartPole-v1", {})
    cfg = DQNConfig().training(num_atoms=51).to_dict()
    cfg["seed"] = 0
    lr = DQNLearner(cfg, env.observation_space, env.action_space, device=CPU)
    batch = _terminal_batch()

    def mean_ce():
        b = lr._convert_batch(batch)
        lr.compute_loss_for_module(module_id=lr.module_id, config=lr.config, batch=b,
                                   fwd_out=lr.forward_train(b))
        return float(lr._td.mean())

    first = mean_ce()
    assert abs(first - math.log(51)) < 0.05 * math.log(51), first
    for i in range(600):
        res = lr.update_from_batch(batch)
        if i == 0:  # the first update reports the cross-entropy before its step
            assert res["td_error"].shape == (64,) and (res["td_error"] >= 0).all()
            assert abs(float(res["td_error"].mean()) - first) < 1e-5
    last = mean_ce()
    print(f"mean CE: before {first:.4f}, after 600 updates {last:.4f}")
    assert last < 0.5 * first, (first, last)


def test_learner_c51_matches_reference_loss_and_noisy_sigmas_travel():
    env = make_env("CartPole-v1", {})
    cfg = DQNConfig().training(num_atoms=51, noisy=True, double_q=False).to_dict()
    cfg["seed"] = 0
    lr = DQNLearner(cfg, env.observation_space, env.action_space, device=CPU)
    w = lr.get_weights()
    assert "adv.weight_sigma" in w and "encoder.net.0.weight_sigma" in w and "support" in w
    assert not any("eps" in k for k in w)
    b = lr._convert_batch(_terminal_batch(16, 1))
    out = lr.forward_train(b)
    assert out["next_online"] is None and out["logits"].shape == (16, 2, 51)
    assert out["logits"].requires_grad and not out["next_target"].requires_grad
    lr2 = DQNLearner(cfg, env.observation_space, env.action_space, device=CPU)
    lr2.set_weights(w)
    assert all(torch.equal(v, lr2.get_weights()[k]) for k, v in w.items())


# ------------------------------------------------------------------------ tuned example
def test_tuned_example_trains_on_cartpole():
    import yaml

    import ray_amd as ray
    from ray_amd.rllib.scripts import _load_experiments

    exps = _load_experiments(YAML)
    (name, spec), = exps.items()
    assert spec["run"] == "DQN" and spec["env"] == "CartPole-v1"
    c = spec["config"]
    assert c["num_atoms"] == 51 and c["noisy"] is True and c["n_step"] == 3
    assert c["double_q"] and c["dueling"] and "Prioritized" in c["replay_buffer_config"]["type"]
    assert yaml.safe_load(open(YAML))[name] == spec
    cfg = DQNConfig().update_from_dict(dict(c, env=spec["env"], seed=0, num_gpus_per_learner=0,
                                            num_steps_sampled_before_learning_starts=40))
    ray.init(num_cpus=2)
    try:
        algo = cfg.build()
        try:
            losses = []
            for _ in range(30):
                res = algo.train()
                assert res["learners"]["epsilon"] == 0.0  # noisy nets: no epsilon-greedy
                if "loss" in res["learners"]:
                    losses.append(res["learners"]["loss"])
            assert len(losses) >= 15 and np.isfinite(losses).all()
            assert algo.local_runner.module.noisy and algo.local_runner.module.num_atoms == 51
            mb = algo.buffer.sample(cfg.train_batch_size, beta=0.4)
            out = algo.learner_group.update_from_batch(mb)
            assert np.isfinite(out["loss"])
            assert out["td_error"].shape == (cfg.train_batch_size,)
            assert (out["td_error"] >= 0).all()
        finally:
            algo.stop()
    finally:
        ray.shutdown()
