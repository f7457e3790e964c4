"""The fused C51 projection-loss kernel (ops/csrc/c51.hip) against the float64 plain-torch
reference (floor/ceil + scatter_add form), its autograd wrapper, run-to-run determinism,
the K > 64 fallback, and the GPU DQN learner's distributional path (GPU only)."""

import numpy as np
import pytest
import torch

from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

V_MIN, V_MAX = -10.0, 10.0
ATOL = RTOL = 1e-3  # fp32 kernels against float64, as test_gae / test_vtrace


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _inputs(B, A, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = {"logits": 2 * torch.randn(B, A, K, generator=g),
         "actions": torch.randint(0, A, (B,), generator=g),
         "next_online": 2 * torch.randn(B, A, K, generator=g),
         "next_target": 2 * torch.randn(B, A, K, generator=g)}
    r = 4 * torch.randn(B, generator=g)
    r[::3] = 0.0          # targets landing exactly on atoms when the row is terminated
    r[1::11] = 25.0       # above the support
    r[2::13] = -25.0      # below it
    disc = torch.full((B,), 0.99)
    disc[::5] = 0.99 ** 3
    x.update(rewards=r, discounts=disc,
             terminateds=(torch.rand(B, generator=g) < 0.3).float(),
             weights=0.2 + 0.8 * torch.rand(B, generator=g))
    return x


_ORDER = ("logits", "actions", "next_online", "next_target", "rewards", "discounts",
          "terminateds", "weights")


def _args(x, dev=None, double=False):
    out = []
    for k in _ORDER:
        t = x[k]
        if t is not None:
            if double and t.is_floating_point():
                t = t.double()
            if dev is not None:
                t = t.to(dev)
        out.append(t)
    return out


def _reference(x):
    """float64 reference on the CPU + the rows whose greedy next action is well defined."""
    a = _args(x, double=True)
    a[0] = a[0].clone().requires_grad_()
    loss, ce, na, m = ref.c51_loss(*a, V_MIN, V_MAX)
    loss.backward()
    sel = a[3] if a[2] is None else a[2]
    K = sel.shape[-1]
    z = torch.linspace(V_MIN, V_MAX, K, dtype=torch.float64)
    q = (torch.softmax(sel, -1) * z).sum(-1)
    if q.shape[1] > 1:
        top = q.topk(2, -1).values
        keep = (top[:, 0] - top[:, 1]) >= 1e-3
    else:
        keep = torch.ones(q.shape[0], dtype=torch.bool)
    return loss.detach(), ce, na, m, a[0].grad, keep


@pytest.mark.parametrize("mode", ["double_q", "target_select", "no_weights"])
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("A", [1, 2, 6, 18])
@pytest.mark.parametrize("K", [2, 51, 64])
def test_c51_loss_vs_float64_reference(cuda_device, K, A, B, mode):
    x = _inputs(B, A, K, seed=K * 1000 + A * 10 + B)
    if mode == "target_select":
        x["next_online"] = None
    if mode == "no_weights":
        x["weights"] = None
    loss_r, ce_r, na_r, m_r, g_r, keep = _reference(x)
    loss, ce, na, dlogits, m = rf.c51_loss_forward(*_args(x, cuda_device), V_MIN, V_MAX,
                                                   with_target=True)
    assert na.dtype == torch.int32 and dlogits.shape == (B, A, K) and m.shape == (B, K)
    loss, ce, na, dlogits, m = (t.cpu() for t in (loss, ce, na, dlogits, m))
    # rows whose top-two expected-Q gap is below 1e-3 may pick either action
    dropped = int((~keep).sum())
    print(f"K={K} A={A} B={B} {mode}: {dropped} near-tie rows left out")
    assert dropped <= 0.02 * B
    assert torch.equal(na.long()[keep], na_r[keep])
    rows = torch.arange(B)
    act = x["actions"]
    torch.testing.assert_close(ce.double()[keep], ce_r[keep], atol=ATOL, rtol=RTOL)
    torch.testing.assert_close((B * dlogits.double())[rows, act][keep],
                               (B * g_r)[rows, act][keep], atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(m.double()[keep], m_r[keep], atol=1e-4, rtol=0)
    assert (m.sum(-1) - 1).abs().max() < 1e-5
    off = torch.ones(B, A, dtype=torch.bool)
    off[rows, act] = False
    assert (dlogits[off] == 0).all()
    assert dlogits[rows, act].sum(-1).abs().max() < 1e-6
    if dropped == 0:
        torch.testing.assert_close(loss.double(), loss_r, atol=ATOL, rtol=RTOL)
    w = x["weights"] if x["weights"] is not None else torch.ones(B)
    torch.testing.assert_close(loss.double(), (ce.double() * w.double()).sum() / B,
                               atol=1e-5, rtol=1e-5)


def test_c51_loss_autograd(cuda_device):
    x = _inputs(37, 6, 51, seed=5)
    _, ce_r, na_r, _, g_r, keep = _reference(x)
    a = _args(x, cuda_device)
    a[0] = a[0].clone().requires_grad_()
    loss, ce, na = rf.c51_loss(*a, v_min=V_MIN, v_max=V_MAX)
    assert not ce.requires_grad and loss.requires_grad
    (3.0 * loss).backward()
    assert a[0].grad is not None and a[0].grad.shape == (37, 6, 51)
    assert keep.all()
    torch.testing.assert_close(37 * a[0].grad.cpu().double(), 37 * 3.0 * g_r, atol=ATOL,
                               rtol=RTOL)
    torch.testing.assert_close(ce.cpu().double(), ce_r, atol=ATOL, rtol=RTOL)
    assert torch.equal(na.cpu().long(), na_r)


def test_c51_loss_is_bit_reproducible(cuda_device):
    a = _args(_inputs(257, 6, 51, seed=6), cuda_device)
    o1 = rf.c51_loss_forward(*a, V_MIN, V_MAX, with_target=True)
    o2 = rf.c51_loss_forward(*a, V_MIN, V_MAX, with_target=True)
    for t1, t2 in zip(o1, o2):
        assert torch.equal(t1, t2)
    assert torch.equal(rf.c51_loss(*a, v_min=V_MIN, v_max=V_MAX)[0], o1[0])


def test_c51_loss_wide_support_uses_the_reference(cuda_device):
    x = _inputs(9, 3, 65, seed=7)
    a = _args(x, cuda_device)
    a[0] = a[0].clone().requires_grad_()
    loss, ce, na = rf.c51_loss(*a, v_min=V_MIN, v_max=V_MAX)
    want = ref.c51_loss(*_args(x, cuda_device), V_MIN, V_MAX)
    # the same torch ops on the same fp32 inputs (scatter_add_ may add in another order)
    torch.testing.assert_close(loss.detach(), want[0], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(ce, want[1], atol=1e-5, rtol=1e-5)
    assert na.dtype == torch.int64 and torch.equal(na, want[2])
    loss.backward()
    assert a[0].grad is not None


def test_dqn_learner_c51_gpu_matches_cpu(cuda_device):
    from ray_amd.rllib.algorithms.dqn import DQNConfig, DQNLearner
    from ray_amd.rllib.env import make_env

    env = make_env("CartPole-v1", {})
    cfg = DQNConfig().training(num_atoms=51, model={"fcnet_hiddens": [64]}).to_dict()
    cfg["seed"] = 0
    cpu = DQNLearner(cfg, env.observation_space, env.action_space, device=torch.device("cpu"))
    gpu = DQNLearner(cfg, env.observation_space, env.action_space, device=cuda_device)
    w0 = {k: v.clone() for k, v in cpu.get_weights().items()}
    gpu.set_weights(w0)
    rng = np.random.default_rng(0)
    n = 32
    batch = {"obs": rng.standard_normal((n, 4)).astype(np.float32),
             "next_obs": rng.standard_normal((n, 4)).astype(np.float32),
             "actions": rng.integers(0, 2, n),
             "rewards": (3 * rng.standard_normal(n)).astype(np.float32),
             "terminateds": (rng.random(n) < 0.3).astype(np.float32),
             "weights": rng.uniform(0.2, 1.0, n).astype(np.float32)}
    rc, rg = cpu.update_from_batch(batch), gpu.update_from_batch(batch)
    assert rg["td_error"].shape == (n,)
    np.testing.assert_allclose(rg["td_error"], rc["td_error"], atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(rg["loss"], rc["loss"], atol=ATOL, rtol=RTOL)
    # both took one Adam step from the same weights: a first step moves a weight by at
    # most lr, so the two results are within 2 lr even where a tiny gradient's sign differs
    wc, wg = cpu.get_weights(), gpu.get_weights()
    assert any(not torch.equal(wc[k], w0[k]) for k in wc)
    for k in wc:
        torch.testing.assert_close(wg[k], wc[k], atol=2.2 * cfg["lr"], rtol=0)
