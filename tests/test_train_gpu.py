"""GPU tests for the headline training path: fused LM-head cross-entropy, fp32 flat
gradients (incl. gradient accumulation) and GPT-2 run as a Ray Train TorchTrainer job."""

import pytest
import torch

from ray_amd.ops import _lib
from ray_amd.ops import functional as rf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.parametrize("N,C,V,Vp,chunk", [(4096, 128, 1000, 1024, 1000),
                                            (2048, 768, 50257, 50304, 8192),
                                            (12388, 768, 50257, 50304, 4096)])
def test_lm_head_cross_entropy(cuda_device, N, C, V, Vp, chunk):
    """Chunked fused LM head + CE vs fp32 logits/log_softmax/nll (loss and both grads)."""
    torch.manual_seed(21)
    h = (torch.randn(N, C, device=cuda_device) * 0.5).bfloat16().requires_grad_()
    w = (torch.randn(Vp, C, device=cuda_device) * 0.05).bfloat16()
    w[V:] = 0
    w.requires_grad_()
    t = torch.randint(0, V, (N,), device=cuda_device)
    t[::7] = -100
    loss = rf.lm_head_cross_entropy(h, w, t, V, chunk=chunk)
    hr, wr = h.detach().float().requires_grad_(), w.detach().float().requires_grad_()
    logits = hr @ wr.t()
    lr_ = torch.nn.functional.cross_entropy(logits[:, :V], t, ignore_index=-100)
    assert abs(float(loss) - float(lr_)) < 2e-3 * abs(float(lr_))
    (loss * 1.5).backward()
    (lr_ * 1.5).backward()
    assert _rel(h.grad, hr.grad) < 2e-2
    assert _rel(w.grad[:V], wr.grad[:V]) < 2e-2
    assert float(w.grad[V:].float().abs().max()) == 0.0


def _tiny_cfg():
    from ray_amd.models.gpt2 import GPT2Config

    return GPT2Config(vocab_size=1000, padded_vocab=1024, n_positions=256, n_embd=128,
                      n_layer=2, n_head=2)


def test_flat_fp32_grads_match_autograd(cuda_device):
    """Every GPT-2 parameter gradient lands in the fp32 flat buffer through a direct sink
    (no .grad tensors), and matches fp32-compute autograd."""
    import copy

    from ray_amd.models.gpt2 import GPT2
    from ray_amd.parallel.flat import FlatParams

    torch.manual_seed(22)
    ref_m = GPT2(_tiny_cfg()).to(cuda_device)  # fp32 compute, plain PyTorch ops
    m = copy.deepcopy(ref_m).bfloat16()
    flat = FlatParams(m)  # fp32 gradient buffer (default)
    assert flat.g.dtype == torch.float32
    idx = torch.randint(0, 1000, (4, 256), device=cuda_device)
    tgt = torch.randint(0, 1000, (4, 256), device=cuda_device)
    m(idx, tgt).backward()
    ref_m(idx, tgt).backward()
    for (n, pr), p in zip(ref_m.named_parameters(), m.parameters()):
        assert p.grad is None, n  # nothing went through AccumulateGrad
        assert _rel(p._ra_grad, pr.grad) < 3e-2, n


@pytest.mark.parametrize("chunk", [None, 256])
def test_side_stream_wgrads_match_main_stream(cuda_device, monkeypatch, chunk):
    """Weight gradients on the wgrad side stream (the tied LM head's dW and its scaled
    accumulation into the flat sink, ordered before the embedding's scatter by an event)
    give the gradients of the all-main-stream path, for 2 micro-batches accumulated into
    one flat buffer. chunk=256: the LM head in 4 sequential chunks of the 1024 tokens."""
    import copy

    from ray_amd.models.gpt2 import GPT2
    from ray_amd.parallel.flat import FlatParams

    torch.manual_seed(23)
    base = GPT2(_tiny_cfg()).to(cuda_device).bfloat16()
    idx = torch.randint(0, 1000, (2, 4, 256), device=cuda_device)
    tgt = torch.randint(0, 1000, (2, 4, 256), device=cuda_device)
    grads = []
    for side in (False, True):
        monkeypatch.setattr(rf, "_WGRAD_STREAM", side)
        m = copy.deepcopy(base)
        if chunk:
            m.lm_head_chunk = chunk
        flat = FlatParams(m)
        for i in range(2):
            (m(idx[i], tgt[i]) * (0.5 + i)).backward()
        rf.join_side_streams()
        torch.cuda.synchronize()
        grads.append(flat.g.clone())
    assert _rel(grads[1], grads[0]) < 1e-5


def test_flat_fp32_grad_accum_exact(cuda_device):
    """grad_accum=4 into the fp32 flat buffer equals the fp64 sum of the four
    micro-batch gradients to ~1e-6 (bf16 accumulation is orders of magnitude worse)."""
    import copy

    from ray_amd.models.gpt2 import GPT2
    from ray_amd.parallel.flat import FlatParams

    torch.manual_seed(23)
    base = GPT2(_tiny_cfg()).to(cuda_device).bfloat16()
    batches = [(torch.randint(0, 1000, (2, 256), device=cuda_device),
                torch.randint(0, 1000, (2, 256), device=cuda_device)) for _ in range(4)]
    m1 = copy.deepcopy(base)
    f1 = FlatParams(m1)
    parts = []
    for x, y in batches:
        f1.zero_grad()
        m1(x, y).backward()
        parts.append(f1.g.double().clone())
    want = sum(parts)
    m2 = copy.deepcopy(base)
    f2 = FlatParams(m2)
    for x, y in batches:
        m2(x, y).backward()
    err32 = _rel(f2.g, want)
    assert err32 < 1e-5, err32
    m3 = copy.deepcopy(base)
    f3 = FlatParams(m3, grad_dtype=torch.bfloat16)
    for x, y in batches:
        m3(x, y).backward()
    err16 = _rel(f3.g, want)
    assert err16 > 10 * err32, (err16, err32)
    assert err16 < 2e-2


def test_gpt2_trainer_fp32_vs_bf16_grads(cuda_device):
    from ray_amd.train.gpt2_step import GPT2Trainer

    losses = {}
    for gd in (torch.float32, torch.bfloat16):
        tr = GPT2Trainer(_tiny_cfg(), 4, 128, cuda_device, lr=3e-3, warmup_steps=2,
                         total_steps=30, grad_dtype=gd, grad_accum=2)
        x, y = tr.synthetic_batch()
        first = None
        for _ in range(20):
            loss = float(tr.step([(x, y), (x, y)]))
            first = first or loss
        assert loss < first * 0.8, (gd, first, loss)
        losses[gd] = loss
    assert abs(losses[torch.float32] - losses[torch.bfloat16]) < 0.1 * losses[torch.float32]


def test_torchtrainer_gpt2_one_gpu(cuda_device, tmp_path):
    """The headline launcher end to end: ray_amd.init -> TorchTrainer(1 GPU worker) ->
    GPT-2 (tiny) on the flat-DDP path -> train.report, RCCL group of size 1."""
    import ray_amd as ray
    from ray_amd.train import RunConfig, ScalingConfig
    from ray_amd.train.examples.gpt2 import train_func
    from ray_amd.train.torch import TorchTrainer

    ray.init(num_cpus=4, num_gpus=1)
    try:
        cfg = dict(model="tiny", micro_batch=4, seq_len=128, steps=5, warmup=2,
                   tunableop="off")
        res = TorchTrainer(train_func, train_loop_config=cfg,
                           scaling_config=ScalingConfig(num_workers=1, use_gpu=True),
                           run_config=RunConfig(name="t_gpt2", storage_path=str(tmp_path))).fit()
        m = res.metrics
        assert m["device"].startswith("cuda")
        assert m["rccl_world_size"] == 1 and m["dist_backend"] == "nccl"
        assert m["tokens_per_sec"] > 0 and m["loss"] == m["loss"]
        assert m["grad_dtype"] == "fp32"
    finally:
        ray.shutdown()


def test_torchtrainer_gpt2_two_workers_one_gpu_gloo(cuda_device, tmp_path):
    """The world > 1 GPU path on a one-GPU box: two Train workers share the GPU
    (0.5 each) and join a gloo group (RCCL refuses two ranks on one device), so the flat
    DDP bucket hooks, the initial broadcast, the 1/world gradient scale and the
    per-rank step timing all run with world size 2 on HIP tensors."""
    import ray_amd as ray
    from ray_amd.train import RunConfig, ScalingConfig
    from ray_amd.train.examples.gpt2 import train_func
    from ray_amd.train.torch import TorchConfig, TorchTrainer

    ray.init(num_cpus=4, num_gpus=1)
    try:
        cfg = dict(model="tiny", micro_batch=4, seq_len=128, steps=4, warmup=2,
                   tunableop="off", bucket_mb=0.25)
        res = TorchTrainer(train_func, train_loop_config=cfg,
                           torch_config=TorchConfig(backend="gloo"),
                           scaling_config=ScalingConfig(num_workers=2, use_gpu=True,
                                                        resources_per_worker={"GPU": 0.5}),
                           run_config=RunConfig(name="t_gpt2_w2",
                                                storage_path=str(tmp_path))).fit()
        m = res.metrics
        assert m["device"].startswith("cuda")
        assert m["rccl_world_size"] == 2 and m["dist_backend"] == "gloo"
        assert m["ranks_in_sync"] is True
        assert len(m["per_rank_ms_per_step"]) == 2
        assert m["loss"] == m["loss"] and m["tokens_per_sec"] > 0
    finally:
        ray.shutdown()


def test_lt_choice_name_reports_kernels(cuda_device):
    """ops/lt.py names the hipBLASLt kernel a wgrad shape runs (the ragged LM-head dW of
    N = 12388 / chunk 4096 included) and is_streamk() recognises Tensile's StreamK tag."""
    from ray_amd.ops import lt

    for M, N, K in ((100, 50304, 768), (4096, 768, 768)):
        dy = torch.randn(M, N, device=cuda_device).bfloat16()
        x = torch.randn(M, K, device=cuda_device).bfloat16()
        out = torch.zeros(N, K, device=cuda_device)
        lt.wgrad_accum(dy, x, out, beta=0.0)
        assert _rel(out, dy.float().t() @ x.float()) < 1e-5
        name = lt.wgrad_choice_name(M, N, K)
        assert name.startswith(("Cijk", "Custom")), name
    assert lt.is_streamk("Cijk_..._SK3_SKXCCM8_...") and not lt.is_streamk("Cijk_MT256_SN_LDSB0")


def test_flat_ddp_world1_hooks_comm_stream(cuda_device):
    """FlatDDP(always_hook=True) on a world-1 RCCL group: every bucket is launched exactly
    once from the comm stream during backward, gradients are unchanged by the (identity)
    all-reduce, and a second step reuses the per-bucket events."""
    import copy
    import os

    import torch.distributed as dist

    from ray_amd.models.gpt2 import GPT2
    from ray_amd.parallel.flat import FlatDDP, FlatParams

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        dist.init_process_group("nccl", rank=0, world_size=1)
    torch.manual_seed(5)
    a = GPT2(_tiny_cfg()).to(cuda_device).bfloat16()
    b = copy.deepcopy(a)
    fa, fb = FlatParams(a), FlatParams(b)
    ddp = FlatDDP(fb, bucket_mb=0.1, always_hook=True)
    assert ddp.enabled and ddp._comm is not None and len(ddp.buckets) > 3
    idx = torch.randint(0, 1000, (4, 256), device=cuda_device)
    for step in range(2):
        fa.zero_grad()
        fb.zero_grad()
        a(idx, idx).backward()
        b(idx, idx).backward()
        # launched from the hooks while backward ran (not by finish())
        assert ddp.launched == (step + 1) * len(ddp.buckets)
        ddp.finish()
        torch.cuda.synchronize()
        assert _rel(fb.g, fa.g) < 1e-6


def test_dgrad_transposed_weight_copy(cuda_device, monkeypatch):
    """RAY_AMD_DGRAD_WT: dX from the transposed bf16 weight copy equals dY @ W, and the copy
    follows in-place weight updates (autograd's version counter) and optimizer steps (the
    weights epoch) instead of serving a stale transpose."""
    torch.manual_seed(5)
    x = torch.randn(512, 256, device=cuda_device).bfloat16().requires_grad_()
    w = (torch.randn(384, 256, device=cuda_device) * 0.05).bfloat16().requires_grad_()
    b = torch.zeros(384, device=cuda_device).bfloat16().requires_grad_()
    g = torch.randn(512, 384, device=cuda_device).bfloat16()

    def dx():
        x.grad = None
        rf.linear(x, w, b).backward(g)
        torch.cuda.synchronize()
        return x.grad.float()

    monkeypatch.setattr(rf, "_DGRAD_WT", False)
    ref = dx()
    monkeypatch.setattr(rf, "_DGRAD_WT", True)
    assert (dx() - ref).abs().max().item() <= 1e-2 * ref.abs().max().item()
    with torch.no_grad():
        w.mul_(0.5)  # in-place update: version counter moves
    assert (dx() - 0.5 * ref).abs().max().item() <= 1e-2 * ref.abs().max().item()
    wt_before = w._ra_wt[0].clone()
    rf.bump_weights_epoch()  # what FlatAdamW.step does after its in-place kernel
    dx()
    assert torch.equal(w._ra_wt[0], wt_before)  # refreshed from unchanged weights
    assert torch.equal(w._ra_wt[0], w.detach().t().contiguous())


def test_adamw_wt_matches_plain_adamw_and_refreshes_transposes(cuda_device):
    """ra_adamw_flat_wt (AdamW + the W^T copies of the linear weights in one pass) updates
    p32/m/v/p16 exactly like the plain flat AdamW kernel and leaves every W^T view equal to
    the transpose of its updated bf16 weight; ragged weight shapes included."""
    from ray_amd.parallel.flat import FlatAdamW, FlatParams

    def make():
        torch.manual_seed(21)
        m = torch.nn.Module()
        m.a_w = torch.nn.Parameter(torch.randn(2304, 768, device=cuda_device))
        m.b_w = torch.nn.Parameter(torch.randn(200, 132, device=cuda_device))  # ragged tiles
        m.c_w = torch.nn.Parameter(torch.randn(768, 3072, device=cuda_device))
        m.d = torch.nn.Parameter(torch.randn(1000, device=cuda_device))  # 1-D tail
        return m.bfloat16()

    mods = [make(), make()]
    fps = [FlatParams(mods[0], transpose=lambda n, p: n.endswith("_w")), FlatParams(mods[1])]
    assert fps[0].pt16 is not None and fps[1].pt16 is None
    assert fps[0].names == fps[1].names  # same layout: the _w weights were first anyway
    opts = [FlatAdamW(fp, lr=1e-2, weight_decay=0.1, max_grad_norm=1.0, zero_grad=True)
            for fp in fps]
    for step in range(3):
        torch.manual_seed(100 + step)
        grad = torch.randn(fps[0].numel, device=cuda_device)
        for fp, opt in zip(fps, opts):
            fp.g.copy_(grad)
            opt.step()
        torch.cuda.synchronize()
        # compare the parameters' own elements (the alignment padding between the tiled
        # weights is not part of any tile)
        for (name, prm), off in zip(fps[0].order, fps[0].offsets):
            k = prm.numel()
            # p16: the two kernels may contract the update differently (FMA), so a p32 value
            # a few ulps apart can round to the neighbouring bf16 (1 bf16 ulp ~ 2^-8 relative)
            for a, b, tol in ((fps[0].p32, fps[1].p32, 1e-6), (fps[0].p16, fps[1].p16, 4e-3),
                              (opts[0].m, opts[1].m, 1e-6), (opts[0].v, opts[1].v, 1e-6)):
                x, y = a[off:off + k].float(), b[off:off + k].float()
                assert (x - y).abs().max().item() <= tol * y.abs().max().item() + 1e-12, name
            assert float(fps[0].g[off:off + k].abs().max()) == 0.0  # zeroed in the same pass
        for name in ("a_w", "b_w", "c_w"):
            p = getattr(mods[0], name)
            assert torch.equal(p._ra_wt_view, p.detach().t()), name
            assert rf._transposed_weight(p)[0].data_ptr() == p._ra_wt_view.data_ptr()


def test_gpt2_graph_replay_matches_eager_then_eager_after_replay(cuda_device):
    """graphed steps reproduce the eager loss trajectory, and an eager step
    after replays (transposed weights, epoch-keyed caches) continues it."""
    from ray_amd.models.gpt2 import GPT2Config
    from ray_amd.train.gpt2_step import GPT2Trainer

    cfg = GPT2Config.tiny()
    gen = torch.Generator(device=cuda_device).manual_seed(3)
    ids = torch.randint(0, cfg.vocab_size, (6, 4, 129), device=cuda_device, generator=gen)
    batches = [[(b[:, :-1].contiguous(), b[:, 1:].contiguous())] for b in ids]

    def trainer():
        return GPT2Trainer(cfg, 4, 128, cuda_device, lr=3e-3, warmup_steps=1, seed=7)

    # eager: b0, b0 (the graph run's two warm-up steps), then b1 .. b5
    ta = trainer()
    eager = [float(ta.step(b)) for b in [batches[0], batches[0]] + batches[1:]]
    # graphed: enable_graph runs the two eager warm-up steps on b0, replays b1 .. b4, then
    # one eager step on b5 after the replays
    tb = trainer()
    assert tb.enable_graph(batches[0], warm=2)
    graphed = [float(tb.step(b)) for b in batches[1:5]]
    tb._graph = None
    graphed.append(float(tb.step(batches[5])))
    torch.cuda.synchronize()
    for a, b in zip(eager[2:], graphed):
        assert abs(a - b) <= 2e-3 * abs(a), (eager, graphed)


def test_bench_stream_autotune_reports_and_restores(cuda_device, monkeypatch):
    """run_steps times 2 side-stream and 2 single-stream warmup steps and runs the timed
    steps in the faster mode; the choice is reported, and training stays correct."""
    from ray_amd.ops import functional as rf
    from ray_amd.train.examples.gpt2 import run_steps

    monkeypatch.setenv("RAY_AMD_STREAM_AUTOTUNE", "1")
    monkeypatch.setattr(rf, "_WGRAD_STREAM", True)
    r = run_steps({"model": "tiny", "micro_batch": 4, "seq_len": 128, "steps": 3,
                   "warmup": 5, "tunableop": "off"}, cuda_device, 0, 1)
    ab = r["wgrad_stream_autotune"]
    assert ab is not None and ab["chosen"] in ("side", "serial")
    assert ab["side_stream_ms"] > 0 and ab["serial_ms"] > 0
    assert rf._WGRAD_STREAM == (ab["chosen"] == "side")
    assert r["ms_per_step"] > 0 and r["loss"] == r["loss"]  # finite


def test_gpt2_small_bench_path_grads_match_fp32_autograd(cuda_device):
    """The composed default bench path at the real GPT-2-small shapes (C 768, 12 layers,
    T 1024, vocab 50257 padded to 50304), B = 2: bf16 compute through the HIP kernels, the
    weight gradients on the side stream (split-K wgrad kernel, fused bias gradients), the
    LM head's dW with S = 3 splits, the input gradients from the W^T copies, LayerNorm
    column sums by atomics into the fp32 sinks, the fused embedding backward — every slice
    of the fp32 flat gradient vs fp32 autograd of the same weights."""
    from ray_amd.models.gpt2 import GPT2, GPT2Config
    from ray_amd.train.gpt2_step import GPT2Trainer

    torch.manual_seed(24)
    cfg = GPT2Config.small()
    tr = GPT2Trainer(cfg, 2, 1024, cuda_device, lm_head_chunk=65536)
    ref = GPT2(cfg).to(cuda_device)  # fp32 compute, plain PyTorch ops
    ref.load_state_dict({k: v.float() for k, v in tr.model.state_dict().items()})
    x, y = tr.synthetic_batch()
    loss = tr.model(x, y)
    loss.backward()
    rf.join_side_streams()
    lref = ref(x, y)
    lref.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(lref)) < 1e-2 * abs(float(lref))
    worst = []
    for (n, pr), p in zip(ref.named_parameters(), tr.model.parameters()):
        g = getattr(p, "_ra_grad", None)
        assert g is not None and p.grad is None, n  # landed in the flat sink
        r = _rel(g, pr.grad)
        worst.append((r, n))
        assert r < 5e-2, (n, r)
    # the side-stream wgrad kernel was on this path (not an eager fallback)
    assert rf._WGRAD_STREAM
    print("max rel err", max(worst))


@pytest.mark.parametrize("model,B,T,chunk", [("tiny", 4, 128, 8192), ("small", 8, 1024, 4096)])
def test_gpt2_training_steps_repeat_bitwise(cuda_device, model, B, T, chunk):
    """Two trainers built from the same seed and fed the same batches end with the same bits
    in loss, fp32 master weights and both AdamW moments: no kernel of the step sums in an
    order that changes from run to run (duplicate token ids, LayerNorm and bias gradients
    included). AdamW's normalised update would turn a last-bit difference in a gradient
    into a visible weight difference within two steps. 'small' is the benchmark's model at a
    smaller batch: the D = 768 LayerNorm backward, the weight-gradient side stream and a
    chunked LM head; one token fills a fifth of its batch (many chunks of the embedding
    backward)."""
    from ray_amd.models.gpt2 import GPT2Config
    from ray_amd.train.gpt2_step import GPT2Trainer

    def run():
        tr = GPT2Trainer(getattr(GPT2Config, model)(), B, T, cuda_device, total_steps=3, seed=7,
                         lm_head_chunk=chunk)
        gen = torch.Generator(device=cuda_device)
        gen.manual_seed(11)
        x, y = tr.synthetic_batch(gen)
        x[:, :T // 5] = x[0, 0]
        losses = [float(tr.step([(x, y)])) for _ in range(3)]
        torch.cuda.synchronize(cuda_device)
        out = losses, tr.flat.p32.clone(), tr.opt.m.clone(), tr.opt.v.clone()
        del tr
        return out

    a, b = run(), run()
    assert a[0] == b[0]
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)
