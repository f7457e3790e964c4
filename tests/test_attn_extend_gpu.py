"""The HIP extend-attention kernel (ops/csrc/attn_extend.hip, ``rf.attn_extend``) and the
cache-to-cache copy (ops/csrc/kv_slots.hip, ``rf.kv_copy``) against the plain-torch
references, then ``GPT2.extend_into`` and the engine's shared prefixes and chunked prefill
on the GPU in bf16.

Inputs are randn rounded to bf16, built on the CPU; the caches hold NaN past each row's
cached positions, so masking by multiplying with zero, or loading a row past the end into the
MFMA, fails. Error measure and bound of the cache-attention tests (test_attn_decode_gpu.py):
|a - b| / |b| < 1e-2 against the fp32 reference, overall and per active row."""

import dataclasses
import functools
import itertools

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

D = 64
REL = 1e-2
S = 5
TMAX = 328  # not a multiple of the 64-key tile


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _is_active(slot, base, n, Tn, n_slots=S, Tmax=TMAX):
    return 0 <= slot < n_slots and base >= 0 and 1 <= n <= Tn and base + n <= Tmax


@functools.lru_cache(maxsize=None)
def _case(rows, H, Tn, seed=0, n_slots=S, Tmax=TMAX):
    """``rows``: ((slot, base, n_new), ...). bf16 tensors on the CPU, the caches NaN from each
    active row's ``base`` on (and random elsewhere), the fp32 reference output and the
    expected caches after the call. Computed once, never modified."""
    g = torch.Generator().manual_seed(seed + 1000 * H + Tn)
    Bn = len(rows)
    qkv = torch.randn(Bn, Tn, 3, H, D, generator=g).bfloat16()
    kc = torch.randn(n_slots, H, Tmax, D, generator=g).bfloat16()
    vc = torch.randn(n_slots, H, Tmax, D, generator=g).bfloat16()
    active = [b for b, r in enumerate(rows) if _is_active(*r, Tn, n_slots, Tmax)]
    assert len({rows[b][0] for b in active}) == len(active)  # distinct slots
    for b in active:
        s, base, _ = rows[b]
        kc[s, :, base:] = float("nan")
        vc[s, :, base:] = float("nan")
    vecs = tuple(torch.tensor([r[i] for r in rows], dtype=torch.int32) for i in range(3))
    kf, vf = kc.float(), vc.float()
    want = ref.attn_extend(qkv.float(), kf, vf, *vecs)
    # the caches after the call, from the bf16 originals (fp32 may change a NaN's bits)
    k_after, v_after = kc.clone(), vc.clone()
    for b in active:
        s, base, n = rows[b]
        k_after[s, :, base: base + n] = qkv[b, :n, 1].transpose(0, 1)
        v_after[s, :, base: base + n] = qkv[b, :n, 2].transpose(0, 1)
    assert torch.equal(k_after.float().nan_to_num(7.0), kf.nan_to_num(7.0))  # the reference agrees
    return qkv, kc, vc, vecs, want, k_after, v_after, tuple(active)


def _run(case, dev):
    qkv, kc, vc, vecs, want = case[:5]
    kd, vd = kc.to(dev), vc.to(dev)
    out = rf.attn_extend(qkv.to(dev), kd, vd, *(t.to(dev) for t in vecs))
    assert out.shape == want.shape and out.dtype == torch.bfloat16
    return out.cpu(), kd.cpu(), vd.cpu()


def _check(case, rows, got, tag):
    qkv, kc, vc, vecs, want, k_after, v_after, active = case
    out, kd, vd = got
    assert torch.isfinite(out.float()).all(), tag
    err = _rel(out, want)
    print(f"{tag} rel err {err:.2e}")
    assert err < REL, tag
    for b, (s, base, n) in enumerate(rows):
        if b not in active:
            assert (out[b] == 0).all(), (tag, b)
            continue
        assert _rel(out[b, :n], want[b, :n]) < REL, (tag, b, base, n)
        assert (out[b, n:] == 0).all(), (tag, b)  # the padding queries
        if base == 0:  # query 0 has one key: its output is the new v itself
            assert torch.equal(_bits(out[b, 0]), _bits(qkv[b, 0, 2])), (tag, b)
    # the appended rows bitwise, every other cache element unchanged, the NaNs included
    assert torch.equal(_bits(kd), _bits(k_after)), tag
    assert torch.equal(_bits(vd), _bits(v_after)), tag


BASES = (0, 1, 63, 64, 65, 127, 128, 129, 200)
NEWS = (1, 31, 32, 33, 64, 127, 128)
GRID = [(base, n) for n in NEWS for base in BASES if base + n <= TMAX]
assert len(GRID) == 63 and (200, 128) in GRID and 200 + 128 == TMAX  # the exact-fit row


def _grid_calls():
    """The (base, n_new) grid as ragged calls of five active rows in permuted slots, each
    with two rows naming slots outside the cache and one more inactive row of another kind
    that names a slot an active row uses."""
    perms = list(itertools.permutations(range(S)))
    calls = []
    for c, i in enumerate(range(0, len(GRID), S)):
        part = GRID[i: i + S]
        perm = perms[(17 * c + 5) % len(perms)]
        rows = [(perm[j], base, n) for j, (base, n) in enumerate(part)]
        Tn = max(n for _, n in part)
        bad = [(perm[0], -1, 1), (perm[1], 3, 0), (perm[2], 3, Tn + 1),
               (perm[3], TMAX - Tn + 1, Tn)][c % 4]  # base -1, n 0, n > Tn, one past Tmax
        rows = rows[:2] + [(-1, 5, 1)] + rows[2:] + [(S, 5, 1), bad]
        calls.append((tuple(rows), Tn))
    return calls


@pytest.mark.parametrize("H", [1, 3])
def test_base_by_n_new_grid(cuda_device, H):
    for rows, Tn in _grid_calls():
        case = _case(rows, H, Tn)
        assert len(case[7]) == min(S, len(rows) - 3)
        _check(case, rows, _run(case, cuda_device), f"grid H={H} Tn={Tn} rows={rows}")


@pytest.mark.parametrize("H", [1, 3])
def test_tall_call_and_single_rows(cuda_device, H):
    # Tn = 129: a second query block of one row; beside it a short row and an exact fit
    rows = ((3, 70, 129), (0, 5, 2), (4, TMAX - 129, 129), (1, 0, 1))
    case = _case(rows, H, 129)
    _check(case, rows, _run(case, cuda_device), f"tall H={H}")
    for base, n in ((0, 1), (0, 128), (64, 64), (TMAX - 1, 1), (200, 128), (199, 129)):
        rows = ((2, base, n),)
        case = _case(rows, H, n)
        _check(case, rows, _run(case, cuda_device), f"single H={H} base={base} n={n}")


@pytest.mark.parametrize("base,n", [(129, 100), (65, 33), (0, 128), (200, 128), (63, 1)])
def test_batch_mate_independence(cuda_device, base, n):
    """A row's bits depend on its own base, n_new and data only: alone with Tn = n_new in
    one slot, and inside a wider, taller call in another slot."""
    H = 3
    alone = _case(((1, base, n),), H, n, seed=7)
    qkv, kc, vc = alone[0], alone[1], alone[2]
    out_a, k_a, v_a = _run(alone, cuda_device)
    _check(alone, ((1, base, n),), (out_a, k_a, v_a), f"alone base={base} n={n}")
    Tn = n + 37
    rows = ((0, 17, min(Tn, 150)), (4, 2, 9), (3, base, n), (-1, 0, 1), (2, 300, 20))
    wide = _case(rows, H, Tn, seed=8)
    wq, wk, wv = wide[0].clone(), wide[1].clone(), wide[2].clone()
    wq[2, :n] = qkv[0]  # the same new tokens, the same cached row, in slot 3
    wk[3], wv[3] = kc[1], vc[1]
    vecs = [t.to(cuda_device) for t in wide[3]]
    runs = []
    for _ in range(2):
        kd, vd = wk.to(cuda_device), wv.to(cuda_device)
        out = rf.attn_extend(wq.to(cuda_device), kd, vd, *vecs)
        runs.append((out.cpu(), kd.cpu(), vd.cpu()))
    for x, y in zip(*runs):  # the same call twice: the same bits
        assert torch.equal(_bits(x), _bits(y))
    out_w, k_w, v_w = runs[0]
    assert torch.equal(_bits(out_w[2, :n]), _bits(out_a[0]))
    assert (out_w[2, n:] == 0).all()
    assert torch.equal(_bits(k_w[3]), _bits(k_a[1])) and torch.equal(_bits(v_w[3]), _bits(v_a[1]))


def test_attn_extend_argument_checks(cuda_device):
    rows = ((0, 3, 4), (1, 0, 2))
    qkv, kc, vc, vecs = (_case(rows, 2, 4)[i] for i in range(4))
    qkv, kc, vc = qkv.to(cuda_device), kc.to(cuda_device), vc.to(cuda_device)
    sl, ba, nn = (t.to(cuda_device) for t in vecs)
    with pytest.raises(ValueError):
        rf.attn_extend(qkv, kc, vc, sl.long(), ba, nn)
    with pytest.raises(ValueError):
        rf.attn_extend(qkv, kc, vc, sl.cpu(), ba, nn)
    with pytest.raises(ValueError):
        rf.attn_extend(qkv, kc.transpose(0, 1).contiguous().transpose(0, 1), vc, sl, ba, nn)
    with pytest.raises(RuntimeError):
        rf.attn_extend(qkv.clone().requires_grad_(), kc, vc, sl, ba, nn)


# ------------------------------------------------------------------ kv_copy
def _rand_bits(shape, g):
    """bf16 of random bit patterns: every kind of value, NaNs of every payload included."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32) \
        .to(torch.int16).view(torch.bfloat16)


def test_kv_copy_bitwise(cuda_device):
    L, H, P, NS, Tsrc, Tdst = 2, 3, 4, 9, 80, 72
    g = torch.Generator().manual_seed(3)
    sk, sv = (_rand_bits((L, P, H, Tsrc, D), g).to(cuda_device) for _ in range(2))
    dk0, dv0 = (_rand_bits((L, NS, H, Tdst, D), g).to(cuda_device) for _ in range(2))
    #                    lens 0, 1, 7, 8, 9, 64, Tmax = min(Tsrc, Tdst) | skipped rows
    src = [0, 1, 2, 3, 0, 1, 2, -1, P, 3, 3]
    dst = [8, 3, 0, 5, 1, 7, 2, 4, 4, NS, 6]
    lens = [0, 1, 7, 8, 9, 64, Tdst, 5, 5, 5, Tdst + 1]
    vecs = [torch.tensor(x, dtype=torch.int32, device=cuda_device) for x in (src, dst, lens)]
    wk, wv = dk0.clone(), dv0.clone()
    ref.kv_copy(sk, sv, wk, wv, *vecs)
    dk, dv = dk0.clone(), dv0.clone()
    assert rf.kv_copy(sk, sv, dk, dv, *vecs) is None
    assert torch.equal(_bits(dk), _bits(wk)) and torch.equal(_bits(dv), _bits(wv))
    # ... and the reference wrote what the table says, and only that
    for c, c0, s_ in ((wk, dk0, sk), (wv, dv0, sv)):
        for row in range(NS):
            n = lens[dst.index(row)] if row in dst[:7] else 0
            assert torch.equal(_bits(c[:, row, :, n:]), _bits(c0[:, row, :, n:])), row
            if n:
                assert torch.equal(_bits(c[:, row, :, :n]),
                                   _bits(s_[:, src[dst.index(row)], :, :n])), row
    # the other direction: the destination is the longer cache
    back_k, back_v = sk.clone(), sv.clone()
    want_k = sk.clone()
    want_k[:, 2, :, :Tdst] = dk0[:, 5]
    one = [torch.tensor([x], dtype=torch.int32, device=cuda_device) for x in (5, 2, Tdst)]
    rf.kv_copy(dk0, dv0, back_k, back_v, *one)
    assert torch.equal(_bits(back_k), _bits(want_k))
    with pytest.raises(ValueError):
        rf.kv_copy(sk, sv, dk, dv, vecs[0].long(), vecs[1], vecs[2])
    with pytest.raises(ValueError):
        rf.kv_copy(sk, sv, dk.transpose(0, 1), dv.transpose(0, 1), *vecs)


# ------------------------------------------------------------------ model
def _cfg():
    return dataclasses.replace(GPT2Config.tiny(), n_embd=128, n_head=2, n_positions=256,
                               init_std=0.2)


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(0)
    return GPT2(_cfg()).eval().to(dev, torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _prompt150():
    g = torch.Generator().manual_seed(9)
    return torch.randint(0, 512, (150,), generator=g).tolist()


@functools.lru_cache(maxsize=None)
def _yardstick(dev):
    """The whole prompt through the same model in fp32 on the CPU (the reference path), and
    the bf16 whole-prompt ``prefill_into`` on the GPU. Computed once."""
    model = _model(dev)
    prompt = _prompt150()
    m32 = GPT2(_cfg()).eval()
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    c32 = KVCache(_cfg(), 1, 160)
    want = m32.prefill_into(torch.tensor([prompt]), [150], c32, torch.zeros(1, dtype=torch.int32))
    cache = KVCache(_cfg(), 3, 160, dev, torch.bfloat16)
    slot = torch.tensor([1], dtype=torch.int32, device=dev)
    whole = model.prefill_into(torch.tensor([prompt], device=dev), [150], cache, slot)
    return want, whole.float().cpu()


@pytest.mark.parametrize("cut", [1, 77, 128])
def test_extend_into_against_whole_prompt(cuda_device, cut):
    """prefill_into(first part) + extend_into(rest) against prefill_into(whole prompt): both
    are bf16 roundings of one computation in another order, so against the fp32 model the
    split path may err at most twice as much (one more rounding of the attention output per
    layer; a wrong mask or position errs by orders of magnitude more)."""
    model, prompt = _model(cuda_device), _prompt150()
    want, whole = _yardstick(cuda_device)
    cache = KVCache(_cfg(), 3, 160, cuda_device, torch.bfloat16)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    slot = torch.tensor([2], dtype=torch.int32, device=cuda_device)
    model.prefill_into(torch.tensor([prompt[:cut]], device=cuda_device), [cut], cache, slot)
    cache.lens.fill_(rf.SLOT_INACTIVE)
    got = model.extend_into(torch.tensor([prompt[cut:]], device=cuda_device), [150 - cut], cache,
                            slot, torch.tensor([cut], dtype=torch.int32, device=cuda_device))
    assert cache.lens.tolist() == [rf.SLOT_INACTIVE, rf.SLOT_INACTIVE, 150]
    assert torch.isfinite(cache.k[:, 2, :, :150].float()).all()
    assert torch.isnan(cache.k[:, 2, :, 150:].float()).all()
    e_whole, e_split = _rel(whole, want), _rel(got.float().cpu(), want)
    print(f"cut {cut}: whole-prompt rel err {e_whole:.3e}, split rel err {e_split:.3e}")
    assert e_split <= 2 * e_whole


# ------------------------------------------------------------------ engine
# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, continues the prefix)
MIX = [(1, 24, 0.0, None, None, 3, True), (150, 9, 0.8, 5, None, 11, False),
       (17, 16, 1.3, 50, 0.9, 2, True), (70, 3, 0.8, None, 0.9, 7, True),
       (9, 20, 1.3, None, None, -4, False), (130, 12, 0.0, 5, None, 0, True)]
EOS = 7


def _drive(model, graph):
    g = torch.Generator().manual_seed(5)
    prefix = torch.randint(0, 512, (70,), generator=g).tolist()
    prompts = [torch.randint(0, 512, (m[0],), generator=g).tolist() for m in MIX]
    kw = {} if graph else {"graph": False}
    eng = GPT2Engine(model, slots=3, max_len=256, poll_every=2, prefix_slots=1, prefill_chunk=64,
                     eos_token_id=EOS, **kw)
    assert (eng._graph is not None) == graph
    pid = eng.add_prefix(prefix)
    rids = [eng.submit(p, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                       prefix=pid if m[6] else None) for p, m in zip(prompts, MIX)]
    got = eng.run()
    assert not eng.has_work() and eng.num_filling == 0
    return [got[r] for r in rids]


def test_engine_prefix_and_chunks_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    graphed, eager, again = _drive(model, True), _drive(model, False), _drive(model, True)
    assert graphed == eager and graphed == again
    for toks, m in zip(graphed, MIX):
        assert EOS not in toks[:-1]
        assert len(toks) == m[1] or (toks[-1] == EOS and len(toks) < m[1])
