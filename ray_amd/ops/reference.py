"""Plain-PyTorch fp32 reference implementations of every HIP kernel.

Used (a) by the numerics tests as ground truth and (b) as the CPU path, so the
whole framework runs on CPU-only hosts. GPU tensors never route here: see
``ray_amd.ops.functional``.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def layer_norm(x, weight, bias, eps=1e-5):
    return F.layer_norm(x.float(), (x.shape[-1],), weight.float(), bias.float(), eps).to(x.dtype)


def gelu_tanh(u):
    return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u.pow(3))))


def bias_gelu(h, bias):
    return gelu_tanh(h.float() + bias.float()).to(h.dtype)


def bias_residual(h, bias, res):
    out = res.float() + h.float()
    if bias is not None:
        out = out + bias.float()
    return out.to(h.dtype)


def cross_entropy(logits, targets, vocab_size=None, ignore_index=-100):
    V = vocab_size or logits.shape[-1]
    lf = logits[..., :V].float().reshape(-1, V)
    return F.cross_entropy(lf, targets.reshape(-1), ignore_index=ignore_index)


def attn_decode(qkv_new, k_cache, v_cache, lens, scale=None):
    """Single-query attention over a K/V cache (ops/csrc/attn_decode.hip semantics).

    ``qkv_new`` [B, 3, H, D] is the new token's packed q/k/v, the caches are
    [B, H, Tmax, D], ``lens`` [B] the cached positions per row. A row with
    0 <= lens[b] < Tmax gets k/v written IN PLACE at position lens[b] and attends over
    0..lens[b]; any other row is inactive (cache untouched, zero output). Positions past
    lens[b] are masked out whatever they hold (NaN included). fp32 math, no host sync."""
    B, _, H, D = qkv_new.shape
    Tmax = k_cache.shape[2]
    if scale is None:
        scale = D ** -0.5
    q, k, v = qkv_new.unbind(1)
    lens = lens.long()
    active = (lens >= 0) & (lens < Tmax)
    idx = lens.clamp(0, Tmax - 1).view(B, 1, 1, 1).expand(B, H, 1, D)
    act = active.view(B, 1, 1, 1)
    for cache, new in ((k_cache, k), (v_cache, v)):
        cache.scatter_(2, idx, torch.where(act, new.unsqueeze(2).to(cache.dtype),
                                           cache.gather(2, idx)))
    t = torch.arange(Tmax, device=lens.device)
    keep = ((t.view(1, 1, Tmax) <= lens.view(B, 1, 1)) & active.view(B, 1, 1)).expand(B, H, Tmax)
    s = (q.float().unsqueeze(2) @ k_cache.float().transpose(-1, -2)).squeeze(2) * scale
    p = torch.softmax(s.masked_fill(~keep, float("-inf")), -1)
    p = torch.where(keep, p, torch.zeros_like(p))  # inactive rows: softmax of all -inf
    vf = torch.where(keep.unsqueeze(-1), v_cache.float(), torch.zeros((), device=s.device))
    return (p.unsqueeze(2) @ vf).squeeze(2).to(qkv_new.dtype)


SLOT_INACTIVE = -(1 << 30)  # ops/csrc/kv_slots.hip kSlotInactive: an idle slot's cache.lens


def kv_insert(qkv, k_cache, v_cache, slots, lens):
    """Moves a prefill's K/V into slots of a wider cache (ops/csrc/kv_slots.hip semantics).

    ``qkv`` [Bn, Tp, 3, H, D] is one layer's packed c_attn output for the right-padded
    prompts, the caches are [S, H, Tmax, D], ``slots`` and ``lens`` integer [Bn]. For every
    row b with 0 <= slots[b] < S, t in [0, min(lens[b], Tp, Tmax)) and every h,
    ``k_cache[slots[b], h, t] = qkv[b, t, 1, h]`` and the same for V with index 2, IN PLACE;
    every other element keeps its bits. Two rows naming one slot are the caller's error.
    No host sync."""
    Bn, Tp, _, H, D = qkv.shape
    S, Tmax = k_cache.shape[0], k_cache.shape[2]
    dev = qkv.device
    n = min(Tp, Tmax)
    slots = slots.long()
    valid = (slots >= 0) & (slots < S)
    # which prompt row feeds each slot (Bn: none); skipped rows land in a spare entry
    row = torch.full((S + 1,), Bn, dtype=torch.long, device=dev)
    row.scatter_(0, torch.where(valid, slots, S), torch.arange(Bn, device=dev))
    row = row[:S]
    fed = row < Bn
    row = row.clamp(max=Bn - 1)
    t = torch.arange(n, device=dev)
    take = (fed.view(S, 1) & (t.view(1, n) < lens.long()[row].view(S, 1))).view(S, 1, n, 1)
    for cache, which in ((k_cache, 1), (v_cache, 2)):
        new = qkv[row, :n, which].transpose(1, 2).to(cache.dtype)  # [S, H, n, D]
        cache[:, :, :n] = torch.where(take, new, cache[:, :, :n])


def _slot_rows(slots, valid, S, Bn):
    """Which of the Bn rows feeds each of S slots: ``(row [S], fed [S])``; the rows that are
    not ``valid`` land in a spare entry. No host sync."""
    dev = slots.device
    row = torch.full((S + 1,), Bn, dtype=torch.long, device=dev)
    row.scatter_(0, torch.where(valid, slots, S), torch.arange(Bn, device=dev))
    row = row[:S]
    return row.clamp(max=Bn - 1), row < Bn


def attn_extend(qkv_new, k_cache, v_cache, slots, base, n_new, scale=None):
    """Several new tokens for rows that already hold cached positions
    (ops/csrc/attn_extend.hip semantics): the single definition of them.

    ``qkv_new`` [Bn, Tn, 3, H, D] is the packed q/k/v of the right-padded new tokens, the
    caches are [S, H, Tmax, D], ``slots``, ``base`` and ``n_new`` integer [Bn]. Row b is
    ACTIVE when 0 <= slots[b] < S, base[b] >= 0, 1 <= n_new[b] <= Tn and base[b] + n_new[b]
    <= Tmax. For an active row, ``k_cache[slots[b], h, base[b] + i] = qkv_new[b, i, 1, h]``
    for i < n_new[b] (V: index 2), IN PLACE and bitwise, and ``out[b, i]`` is the softmax
    attention of ``qkv_new[b, i, 0]`` over keys 0 .. base[b] + i of that cache row;
    ``out[b, i]`` for i >= n_new[b] is zero. An inactive row writes nothing and gets zero
    output; every other cache element keeps its bits. Positions past a row's end are masked
    out whatever they hold (NaN included). Slots are distinct among the active rows (two
    active rows naming one slot are the caller's error). Returns [Bn, Tn, H, D] in
    ``qkv_new``'s dtype. fp32 math, no host sync."""
    Bn, Tn, _, H, D = qkv_new.shape
    S, Tmax = k_cache.shape[0], k_cache.shape[2]
    dev = qkv_new.device
    if scale is None:
        scale = D ** -0.5
    slots, base, n = slots.long(), base.long(), n_new.long()
    active = (slots >= 0) & (slots < S) & (base >= 0) & (n >= 1) & (n <= Tn) & (base + n <= Tmax)
    n = torch.where(active, n, torch.zeros_like(n))
    base = torch.where(active, base, torch.zeros_like(base))
    # append, seen from the cache: position t of the slot fed by row b takes new token t - base
    row, fed = _slot_rows(slots, active, S, Bn)
    t = torch.arange(Tmax, device=dev).view(1, Tmax)
    rb, rn = base[row].view(S, 1), n[row].view(S, 1)
    take = (fed.view(S, 1) & (t >= rb) & (t < rb + rn)).view(S, 1, Tmax, 1)
    src = (t - rb).clamp(0, Tn - 1)  # [S, Tmax]
    for cache, which in ((k_cache, 1), (v_cache, 2)):
        new = qkv_new[row.view(S, 1), src, which].transpose(1, 2).to(cache.dtype)  # [S,H,Tmax,D]
        cache.copy_(torch.where(take, new, cache))
    # attention over each row's slot
    sl = slots.clamp(0, S - 1)
    i = torch.arange(Tn, device=dev).view(1, Tn, 1)
    tt = t.view(1, 1, Tmax)
    keep = ((i < n.view(Bn, 1, 1)) & (tt <= base.view(Bn, 1, 1) + i)).unsqueeze(1)  # [Bn,1,Tn,Tmax]
    q = qkv_new[:, :, 0].float().transpose(1, 2)  # [Bn, H, Tn, D]
    s = (q @ k_cache[sl].float().transpose(-1, -2)) * scale
    p = torch.softmax(s.masked_fill(~keep, float("-inf")), -1)
    p = torch.where(keep, p, torch.zeros_like(p))  # padding and inactive rows: all -inf
    valid = (tt < (base + n).view(Bn, 1, 1)).view(Bn, 1, Tmax, 1)
    vf = torch.where(valid, v_cache[sl].float(), torch.zeros((), device=dev))
    return (p @ vf).transpose(1, 2).to(qkv_new.dtype)


def kv_copy(src_k, src_v, dst_k, dst_v, src_rows, dst_rows, lens):
    """Copies cached rows from one cache to another, all layers (ops/csrc/kv_slots.hip
    semantics): ``src_k``, ``src_v`` [L, P, H, Tsrc, D], ``dst_k``, ``dst_v`` [L, S, H, Tdst,
    D], ``src_rows``, ``dst_rows``, ``lens`` integer [Bn]. For every b with 0 <= src_rows[b]
    < P, 0 <= dst_rows[b] < S and 0 <= lens[b] <= min(Tsrc, Tdst):
    ``dst[l, dst_rows[b], h, t] = src[l, src_rows[b], h, t]`` for t < lens[b], IN PLACE and
    bitwise; any other b is skipped and every other element keeps its bits. Two rows naming
    one destination are the caller's error. No host sync."""
    P, Tsrc = src_k.shape[1], src_k.shape[3]
    S, Tdst = dst_k.shape[1], dst_k.shape[3]
    Bn = src_rows.shape[0]
    n = min(Tsrc, Tdst)
    sr, dr, ln = src_rows.long(), dst_rows.long(), lens.long()
    valid = (sr >= 0) & (sr < P) & (dr >= 0) & (dr < S) & (ln >= 0) & (ln <= n)
    row, fed = _slot_rows(dr, valid, S, Bn)
    t = torch.arange(n, device=dst_k.device)
    take = (fed.view(S, 1) & (t.view(1, n) < ln[row].view(S, 1))).view(1, S, 1, n, 1)
    from_row = sr[row].clamp(0, P - 1)
    for src, dst in ((src_k, dst_k), (src_v, dst_v)):
        new = src[:, from_row, :, :n].to(dst.dtype)  # [L, S, H, n, D]
        dst[:, :, :, :n] = torch.where(take, new, dst[:, :, :, :n])


def slot_advance(tok, lens, n_out, max_new, active, out, eos_token_id=None):
    """The continuous-batching engine's bookkeeping after the sampler
    (ops/csrc/kv_slots.hip semantics), everything IN PLACE: ``tok`` int64 [S], ``lens``,
    ``n_out``, ``max_new`` int32 [S], ``active`` uint8 [S], ``out`` int64 [S, cap].

    An active slot with 0 <= n_out[s] < cap stores ``out[s, n_out[s]] = tok[s]``, adds 1
    to ``n_out[s]`` and becomes inactive if ``n_out[s] >= max_new[s]`` or ``tok[s]`` is
    ``eos_token_id``; an active slot with any other ``n_out[s]`` becomes inactive without
    a write. Every slot that is inactive after that gets ``lens[s] = SLOT_INACTIVE``.
    No host sync."""
    cap = out.shape[1]
    n = n_out.long()
    ok = active.bool() & (n >= 0) & (n < cap)
    col = n.clamp(0, cap - 1).unsqueeze(1)
    out.scatter_(1, col, torch.where(ok.unsqueeze(1), tok.unsqueeze(1), out.gather(1, col)))
    n = n + ok
    n_out.copy_(n)
    stay = ok & (n < max_new)
    if eos_token_id is not None and int(eos_token_id) >= 0:
        stay = stay & (tok != int(eos_token_id))
    active.copy_(stay)
    lens.masked_fill_(~stay, SLOT_INACTIVE)


def spec_draft(tok0, hist, lens, n_out, max_new, active, k, ngram_min, ngram_max, win, n_win):
    """Prompt-lookup (n-gram) drafts of a speculative step (ops/csrc/spec.hip semantics): the
    single definition of them, as plain loops. ``tok0`` int64 [S] is the token just sampled
    for position ``p = lens[s]``, ``hist`` int32 [S, cap] the request's tokens by absolute
    position (only ``[0, p)`` is read), ``lens`` / ``n_out`` / ``max_new`` int32 [S],
    ``active`` uint8 [S]; ``win`` int64 [S, k + 1] and ``n_win`` int32 [S] are written IN PLACE.

    An inactive slot, or one with ``p`` outside ``[0, cap)``, gets ``n_win = 0`` and keeps
    its ``win`` row. Otherwise ``win[s, 0] = tok0[s]``; with ``seq = hist[s, :p] + [tok0]``,
    ``L = p + 1`` and ``room = min(max_new - n_out, cap - p)``: for ``n = ngram_max`` down to
    ``ngram_min`` with ``n <= L - 1``, the largest ``j`` with ``j + n <= L - 1`` and
    ``seq[j : j+n] == seq[L-n : L]`` is looked for, and the first ``n`` with a match wins.
    Then ``nd = min(k, room - 1)`` and draft i (1-based) is ``seq[q]``, ``q = j + n + i - 1``,
    if ``q < L``, else draft ``q - L + 1``: the continuation runs on into the drafts. Without
    a match ``nd = 0``. ``n_win = 1 + max(nd, 0)``. Reads the host."""
    cap = hist.shape[1]
    rows = zip(tok0.tolist(), lens.tolist(), n_out.tolist(), max_new.tolist(), active.tolist())
    for s, (t0, p, n_o, mx, act) in enumerate(rows):
        if not act or not 0 <= p < cap:
            n_win[s] = 0
            continue
        seq = hist[s, :p].tolist() + [t0]
        L = p + 1
        start = None  # j + n of the winning match
        for n in range(ngram_max, ngram_min - 1, -1):
            if n > L - 1:
                continue
            suffix = seq[L - n:]
            for j in range(L - 1 - n, -1, -1):
                if seq[j: j + n] == suffix:
                    start = j + n
                    break
            if start is not None:
                break
        nd = 0
        if start is not None:
            nd = max(min(k, min(mx - n_o, cap - p) - 1), 0)
            for i in range(nd):
                seq.append(seq[start + i])
        win[s, : 1 + nd] = torch.tensor(seq[p:], dtype=win.dtype)
        n_win[s] = 1 + nd
    return win, n_win


def spec_accept(win, n_win, cand, logits_win, lens, n_out, max_new, active, out, hist, buf,
                n_drafted, n_accepted, eos_token_id=None):
    """Acceptance of a speculative step (ops/csrc/spec.hip semantics): the single definition,
    as a plain loop, everything IN PLACE. ``win`` / ``cand`` int64 [S, k + 1] (``cand[s, i]``:
    the sampler's token for position ``p + 1 + i``, from the logits after ``win[s, i]``),
    ``n_win`` int32 [S], ``logits_win`` [S, k + 1, Vp], ``lens`` / ``n_out`` / ``max_new`` /
    ``n_drafted`` / ``n_accepted`` int32 [S], ``active`` uint8 [S], ``out`` int64 [S, cap],
    ``hist`` int32 [S, cap], ``buf`` [S, Vp].

    An active slot with ``1 <= n_win <= k + 1``, ``0 <= n_out < cap`` and ``0 <= p = lens[s]
    < cap``: ``a`` is the largest ``i <= n_win - 1`` with ``win[s, j] == cand[s, j-1]`` for all
    ``1 <= j <= i``. The tokens ``win[s, 0..a]`` are emitted, cut after the first
    ``eos_token_id`` (which is emitted) and at ``max(1, min(max_new - n_out, cap - n_out,
    cap - p))``: ``m >= 1`` tokens, stored at ``out[s, n_out ..]`` and ``hist[s, p ..]``;
    ``n_out += m``, ``lens += m``, ``n_drafted += n_win - 1``, ``n_accepted += m - 1``. The
    slot becomes inactive on EOS or when ``n_out >= max_new``; if it stays active,
    ``buf[s] = logits_win[s, m-1]`` bitwise (the logits at the new ``lens[s]``). An active
    slot with any other ``n_win`` / ``n_out`` / ``lens`` becomes inactive without a write.
    Every slot that is inactive after that gets ``lens[s] = SLOT_INACTIVE``. Reads the host."""
    W, cap = win.shape[1], out.shape[1]
    eos = -1 if eos_token_id is None else int(eos_token_id)
    for s in range(win.shape[0]):
        act = bool(active[s])
        if act:
            nw, n, p, mx = int(n_win[s]), int(n_out[s]), int(lens[s]), int(max_new[s])
            if not (1 <= nw <= W and 0 <= n < cap and 0 <= p < cap):
                act = False
            else:
                w, c = win[s].tolist(), cand[s].tolist()
                a = 0
                while a + 1 < nw and w[a + 1] == c[a]:
                    a += 1
                toks = w[: min(a + 1, max(1, min(mx - n, cap - n, cap - p)))]
                hit = eos >= 0 and eos in toks
                if hit:
                    toks = toks[: toks.index(eos) + 1]
                m = len(toks)
                out[s, n: n + m] = torch.tensor(toks, dtype=out.dtype)
                hist[s, p: p + m] = torch.tensor(toks, dtype=torch.int64).to(hist.dtype)
                n_out[s] = n + m
                lens[s] = p + m
                n_drafted[s] += nw - 1
                n_accepted[s] += m - 1
                if hit or n + m >= mx:
                    act = False
                else:
                    buf[s] = logits_win[s, m - 1]
            if not act:
                active[s] = 0
        if not act:
            lens[s] = SLOT_INACTIVE


def _lora_rows(y, x, a_stack, b_stack, idx):
    """The views and the per-row adapter choice both LoRA forms share: ``(y3, x3, A, B, ic,
    ok)`` with A, B the rows' adapters (a clamped id for the rows that have none)."""
    Bn, NA = idx.shape[0], a_stack.shape[0]
    i = idx.long()
    ok = ((i >= 0) & (i < NA)).view(Bn, 1, 1)
    ic = i.clamp(0, NA - 1)
    return (y.view(Bn, -1, y.shape[-1]), x.reshape(Bn, -1, x.shape[-1]),
            a_stack.index_select(0, ic), b_stack.index_select(0, ic), ic, ok)


def lora_add(y, x, a_stack, b_stack, scale, idx):
    """Per-row low-rank adapters (ops/csrc/lora.hip semantics): the single definition of
    them. ``x`` [Bn, T, Din] or [Bn, Din], ``y`` [Bn, T, Dout] or [Bn, Dout] written IN
    PLACE, ``a_stack`` [n_adapters, R, Din], ``b_stack`` [n_adapters, Dout, R], ``scale``
    [n_adapters], ``idx`` integer [Bn].

    For every row b with 0 <= idx[b] < n_adapters, a = idx[b], and every token i:
    ``t = sum_k x[b,i,k] * a_stack[a,:,k]`` in fp32, rounded ONCE to the input dtype (not at
    all for fp32 inputs), then ``y[b,i,:] = (float(y[b,i,:]) + scale[a] * sum_r t[r] *
    b_stack[a,:,r])`` rounded to y's dtype. Every other row keeps its bytes. No host sync."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    y3, x3, A, B, ic, ok = _lora_rows(y, x, a_stack, b_stack, idx)
    t = x3.to(ct) @ A.to(ct).transpose(1, 2)
    t = t.to(x.dtype).to(ct)
    d = t @ B.to(ct).transpose(1, 2)
    new = (y3.to(ct) + scale.to(ct)[ic].view(-1, 1, 1) * d).to(y.dtype)
    y3.copy_(torch.where(ok, new, y3))


def lora_add_bmm(y, x, a_stack, b_stack, scale, idx):
    """``lora_add`` as the usual torch composition: ``index_select`` of the stacks by the
    clamped ids, two ``bmm`` in the tensors' own dtype, rows without an adapter masked out.
    Same contract and no host sync, but the sums' order is the GEMM library's. The baseline
    ``scripts/lora_bench.py`` measures the HIP kernel against."""
    y3, x3, A, B, ic, ok = _lora_rows(y, x, a_stack, b_stack, idx)
    d = torch.bmm(torch.bmm(x3, A.transpose(1, 2)), B.transpose(1, 2))
    new = (y3.float() + scale[ic].view(-1, 1, 1) * d.float()).to(y.dtype)
    y3.copy_(torch.where(ok, new, y3))


_MASK64 = (1 << 64) - 1


def _i64(c):
    """The 64-bit constant ``c`` as the int64 with the same bits."""
    c &= _MASK64
    return c - (1 << 64) if c >> 63 else c


def _lsr(z, n):
    """Logical shift right of int64 bit patterns."""
    return (z >> n) & ((1 << (64 - n)) - 1)


def sample_uniform(seeds, steps, dtype=torch.float32):
    """The sampler's counter-based uniform in [0, 1): ``(splitmix64(seed, step) >> 40) *
    2**-24`` with ``z = seed + (step + 1) * 0x9E3779B97F4A7C15`` mixed by the splitmix64
    finaliser, all mod 2**64 (int64 tensors wrap the same way). ``seeds`` int64 [B],
    ``steps`` integer [B]."""
    z = seeds.to(torch.int64) + (steps.to(torch.int64) + 1) * _i64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    z = z ^ _lsr(z, 31)
    return _lsr(z, 40).to(dtype) * 2.0 ** -24


def _sample_logits_u(logits, temperature, top_k, top_p, u, vocab_size=None,
                     dtype=torch.float32):
    """``sample_logits`` with the uniforms ``u`` [B] given; the math runs in ``dtype``."""
    V = vocab_size or logits.shape[-1]
    x = logits[:, :V].to(dtype)  # the stored values, exactly
    dev = x.device
    idx = torch.arange(V, device=dev).expand_as(x)
    T = temperature.to(dtype)
    greedy = T == 0
    top = x.max(-1, keepdim=True).values
    greedy_tok = torch.where(x == top, idx, V).min(-1).values
    # top-k on the stored values: ties at the k-th value are all kept
    xs, order = x.sort(-1, descending=True)
    k = top_k.to(torch.int64)
    k_on = (k > 0) & (k < V)
    kth = xs.gather(1, (k.clamp(1, V) - 1).unsqueeze(1))
    keep = (x >= kth) | ~k_on.unsqueeze(1)
    xt = x / torch.where(greedy, torch.ones_like(T), T).unsqueeze(1)
    w = torch.where(keep, torch.exp(xt - xt.max(-1, keepdim=True).values), torch.zeros_like(x))
    # top-p: a token stays iff the normalised mass of the kept tokens with a strictly
    # larger logit is < p, so a class of equal logits stands or falls together
    ws = w.gather(1, order)
    before = ws.cumsum(-1) - ws  # mass in front of each sorted position
    pos = torch.arange(V, device=dev).expand_as(x)
    new_class = torch.ones_like(x, dtype=torch.bool)
    new_class[:, 1:] = xs[:, 1:] != xs[:, :-1]
    start = torch.where(new_class, pos, 0).cummax(-1).values  # first position of the class
    above = before.gather(1, start)
    keep_p = torch.zeros_like(keep).scatter(1, order, above / ws.sum(-1, keepdim=True)
                                            < top_p.to(dtype).unsqueeze(1))
    keep = keep & (keep_p | (x == top) | (top_p >= 1).unsqueeze(1))
    w = torch.where(keep, w, torch.zeros_like(w))
    # draw: the lowest kept index whose running sum, in index order, exceeds u * sum(w)
    c = w.cumsum(-1)
    hit = (c > u.to(dtype).unsqueeze(1) * w.sum(-1, keepdim=True)) & keep
    first = torch.where(hit, idx, V).min(-1).values
    last = torch.where(keep, idx, -1).max(-1).values
    tok = torch.where(first < V, first, last)
    return torch.where(greedy, greedy_tok, tok)


def sample_logits(logits, temperature, top_k, top_p, seeds, steps, vocab_size=None):
    """Per-row token sampling (ops/csrc/sample.hip semantics): the single definition.

    ``logits`` [B, Vs], of which the first ``V = vocab_size or Vs`` columns count; per row
    ``temperature`` fp32, ``top_k`` int32, ``top_p`` fp32, ``seeds`` int64, ``steps`` int32,
    all [B]. Returns int64 [B]. Per row, with x the stored logits:

    1. u = ``sample_uniform(seed, step)``.
    2. temperature 0: the lowest index holding the row maximum.
    3. top-k (off for k <= 0 or k >= V): keep {i : x_i >= k-th largest x}.
    4. w_i = exp(x_i / T - max) over the kept set.
    5. top-p (off for p >= 1): keep i iff the normalised mass of the kept tokens with
       x_j > x_i is < p; the top value class always survives.
    6. the token is the lowest kept index whose running sum of w in index order exceeds
       u * sum(w), else the last kept index.

    -inf logits are never chosen; NaN is out of contract."""
    u = sample_uniform(seeds, steps)
    return _sample_logits_u(logits, temperature, top_k, top_p, u, vocab_size)


def _place_rows(dst, at, ok, val):
    """``dst[at[b]] = val[b]`` along dim 0 for the rows with ``ok[b]``, IN PLACE; the other
    rows land in a spare entry, so ``dst`` keeps their bytes. No host sync."""
    n = dst.shape[0]
    ext = torch.cat([dst, dst.new_zeros((1,) + tuple(dst.shape[1:]))])
    ext.index_copy_(0, torch.where(ok, at, n), val.to(dst.dtype))
    dst.copy_(ext[:n])


def token_logprobs(logits, tok, top_n=0, vocab_size=None, out=None, rows=None, cols=None,
                   active=None):
    """Per-token log-probabilities (ops/csrc/logprobs.hip semantics): the single definition.

    ``logits`` [B, Vs], of which the first ``V = vocab_size or Vs`` columns count; ``tok``
    int64 [B]; ``top_n`` >= 0. Per row, with x the stored logits (the math runs in fp32, in
    fp64 for fp64 logits):

    * ``lse = max(x) + log(sum(exp(x - max(x))))`` and ``lp = x[tok] - lse``; a ``tok``
      outside ``[0, V)`` gives NaN, a ``-inf`` logit ``-inf``.
    * ``top_ids[j]``, ``top_lp[j]``, j < top_n: the ``top_n`` largest entries of x ordered by
      value descending, then index ascending (a stable order, exact on the stored values,
      -0 equal to +0), ``top_lp[j] = x[top_ids[j]] - lse``; ``(-1, -inf)`` for j >= V.

    The distribution is the model's own: temperature, top-k and top-p play no part. NaN
    logits and a row of all ``-inf`` are out of contract.

    Without ``out``: returns dense ``(lp [B], top_ids int32 [B, top_n], top_lp [B, top_n])``.
    With ``out = (lp_hist fp32 [R, cap], ids_hist int32 [R, cap, top_n], tlp_hist fp32
    [R, cap, top_n])``, ``rows`` int32 [B], ``cols`` int32 [B] and optionally ``active``
    uint8 [B]: row b's results go to ``[rows[b], cols[b]]`` IN PLACE; a row with
    ``active[b] == 0``, ``rows[b]`` outside ``[0, R)`` or ``cols[b]`` outside ``[0, cap)``
    writes nothing. Returns ``out``. No host sync."""
    B, Vs = logits.shape
    V = Vs if vocab_size is None else int(vocab_size)
    ct = torch.float64 if logits.dtype == torch.float64 else torch.float32
    x = logits[:, :V].to(ct)  # the stored values, exactly
    m = x.max(-1, keepdim=True).values
    lse = m + torch.log(torch.exp(x - m).sum(-1, keepdim=True))
    t = tok.long()
    ok = (t >= 0) & (t < V)
    xt = x.gather(1, t.clamp(0, V - 1).unsqueeze(1))
    lp = torch.where(ok, (xt - lse).squeeze(1), torch.full_like(lse.squeeze(1), float("nan")))
    n, k = int(top_n), min(int(top_n), V)
    ids = torch.full((B, n), -1, dtype=torch.int32, device=x.device)
    tlp = torch.full((B, n), float("-inf"), dtype=ct, device=x.device)
    if k:
        xs, order = torch.sort(x, dim=-1, descending=True, stable=True)
        ids[:, :k] = order[:, :k].to(torch.int32)
        tlp[:, :k] = xs[:, :k] - lse
    if out is None:
        return lp, ids, tlp
    lp_h, ids_h, tlp_h = out
    R, cap = lp_h.shape
    r, c = rows.long(), cols.long()
    ok = (r >= 0) & (r < R) & (c >= 0) & (c < cap)
    if active is not None:
        ok = ok & active.bool()
    at = r * cap + c
    _place_rows(lp_h.view(R * cap), at, ok, lp)
    if n:
        _place_rows(ids_h.view(R * cap, n), at, ok, ids)
        _place_rows(tlp_h.view(R * cap, n), at, ok, tlp)
    return out


_BITS = {torch.bfloat16: (torch.int16, 0x7FC0), torch.float16: (torch.int16, 0x7E00),
         torch.float32: (torch.int32, 0x7FC00000), torch.float64: (torch.int64, 0x7FF8 << 48)}


def logit_process(logits, prompt, prompt_len, out, n_out, repetition, presence, frequency,
                  min_new, bias_ids, bias_vals, n_bias, rows=None, extra=None, n_extra=None,
                  active=None, eos_token_id=None, vocab_size=None):
    """Logit processors (ops/csrc/logit_proc.hip semantics): the single definition. Edits
    ``logits`` IN PLACE and returns it. No host sync.

    ``logits`` [B, Vs], of which the first ``V = vocab_size or Vs`` columns count. The context
    of logits row b is row ``r = rows[b]`` (int32 [B], default b) of ``prompt`` int32 [R, P]
    with ``prompt_len`` int32 [R], ``out`` int64 [R, cap] with ``n_out`` int32 [R], and the
    parameters ``repetition``, ``presence``, ``frequency`` fp32 [R], ``min_new`` int32 [R],
    ``bias_ids`` int32 [R, NB], ``bias_vals`` fp32 [R, NB], ``n_bias`` int32 [R]; plus, per
    logits row, ``extra`` int64 [B, W] with ``n_extra`` int32 [B], the tokens that follow
    ``out[r, :n_out[r]]`` for this row (a speculative window up to the row's position).

    A row is skipped, its bytes kept, when ``active[b] == 0``, ``rows[b]`` is outside
    ``[0, R)``, a length is negative or exceeds its table, or its parameters are all neutral
    (``repetition == 1``, ``presence == frequency == 0``, ``n_bias == 0``, ``min_new == 0``).
    Otherwise *generated* is ``out[r, :n_out[r]]`` then ``extra[b, :n_extra[b]]``, *seen* is
    ``prompt[r, :prompt_len[r]]`` with *generated*, and c(v) counts v in *generated*; ids
    outside ``[0, V)`` in any table are ignored. Every token v that is in *seen*, is a bias
    id, or is ``eos_token_id`` while ``len(generated) < min_new[r]`` is edited exactly once,
    from ``x = float32(logits[b, v])``, every step rounded to fp32 on its own:

    1. v in *seen*: ``x = x / repetition`` if ``x > 0`` else ``x * repetition``.
    2. c(v) > 0: ``x = x - frequency * float32(c(v))``, then ``x = x - presence``.
    3. v a bias id: ``x = x + bias_vals[r, i]``, i the lowest index holding v.
    4. v is the banned EOS: ``x = -inf``.
    5. x is stored rounded once to the logits' dtype (nearest even); a NaN result is stored
       as the dtype's canonical quiet NaN (0x7FC0 for bf16).

    Every other element keeps its exact bytes, the columns at and beyond V included."""
    B, Vs = logits.shape
    V = Vs if vocab_size is None else int(vocab_size)
    dev = logits.device
    R, P = prompt.shape
    cap, NB = out.shape[1], bias_ids.shape[1]
    r = torch.arange(B, device=dev) if rows is None else rows.long()
    ok = (r >= 0) & (r < R)
    if active is not None:
        ok = ok & active.bool()
    rc = r.clamp(0, R - 1)
    pl, no, nb = prompt_len[rc].long(), n_out[rc].long(), n_bias[rc].long()
    ok = ok & (pl >= 0) & (pl <= P) & (no >= 0) & (no <= cap) & (nb >= 0) & (nb <= NB)
    gen = [(out[rc], no, cap)]
    n_gen = no
    if extra is not None:
        W = extra.shape[1]
        ne = n_extra.long()
        ok = ok & (ne >= 0) & (ne <= W)
        gen.append((extra.long(), ne, W))
        n_gen = no + ne
    rp, pp, fp = (t[rc].float().unsqueeze(1) for t in (repetition, presence, frequency))
    mn = min_new[rc].long()
    neutral = (rp == 1).squeeze(1) & (pp == 0).squeeze(1) & (fp == 0).squeeze(1) & (nb == 0) & \
        (mn == 0)
    ok = ok & ~neutral

    def cols(ids, n, width):
        # the ids that count as column indices, the others in the spare column V
        ids = ids.long()
        live = (torch.arange(width, device=dev).unsqueeze(0) < n.unsqueeze(1)) & (ids >= 0) & \
            (ids < V)
        return torch.where(live, ids, V)

    one = torch.ones(1, dtype=torch.int32, device=dev)
    in_prompt = torch.zeros(B, V + 1, dtype=torch.int32, device=dev)
    in_prompt.scatter_(1, cols(prompt[rc], pl, P), one.expand(B, P))
    cnt = torch.zeros(B, V + 1, dtype=torch.int32, device=dev)
    for ids, n, width in gen:
        cnt.scatter_add_(1, cols(ids, n, width), one.expand(B, width))
    in_prompt, cnt = in_prompt[:, :V].bool(), cnt[:, :V]
    gen_seen = cnt > 0
    seen = in_prompt | gen_seen
    named = seen
    view = logits[:, :V]
    x = view.float()
    x = torch.where(seen, torch.where(x > 0, x / rp, x * rp), x)
    x = torch.where(gen_seen, (x - fp * cnt.float()) - pp, x)
    if NB:
        first = torch.full((B, V + 1), NB, dtype=torch.int64, device=dev)
        first.scatter_reduce_(1, cols(bias_ids[rc], nb, NB),
                              torch.arange(NB, device=dev).expand(B, NB), "amin")
        first = first[:, :V]
        biased = first < NB
        x = torch.where(biased, x + bias_vals[rc].float().gather(1, first.clamp(max=NB - 1)), x)
        named = named | biased
    if eos_token_id is not None and 0 <= int(eos_token_id) < V:
        ban = torch.zeros(B, V, dtype=torch.bool, device=dev)
        ban[:, int(eos_token_id)] = n_gen < mn
        x = torch.where(ban, torch.full_like(x, float("-inf")), x)
        named = named | ban
    idt, nan = _BITS[logits.dtype]
    bits = torch.where(x.isnan(), torch.full((), nan, dtype=idt, device=dev),
                       x.to(logits.dtype).view(idt))
    raw = view.view(idt)
    raw.copy_(torch.where(named & ok.unsqueeze(1), bits, raw))
    return logits


from ray_amd.models.grammar import GRAMMAR_DEAD, GRAMMAR_NONE  # noqa: E402  (a row's state)


def grammar_advance(state, pos, out, n_out, table, max_steps):
    """Follows the emitted tokens through a token DFA (ops/csrc/grammar.hip semantics): the
    single definition. Edits ``state`` and ``pos`` (int32 [R]) IN PLACE. No host sync.

    ``table`` int16 [N, Vt]: ``table[q, t]`` is the state after token t in state q, negative
    when t is not allowed there. ``out`` int64 [R, cap] with ``n_out`` int32 [R] holds each
    row's tokens; ``pos[r]`` counts those ``state[r]`` has consumed. Per row, at most
    ``max_steps`` times while ``pos[r] < n_out[r]``: ``state[r] = table[state[r],
    out[r, pos[r]]]`` and ``pos[r] += 1``; a result outside ``[0, N)`` makes the state
    ``GRAMMAR_DEAD``. A row whose state is outside ``[0, N)`` (``GRAMMAR_NONE`` and
    ``GRAMMAR_DEAD`` included), whose ``pos`` is negative, whose ``n_out`` exceeds cap or
    whose next token is outside ``[0, Vt)`` is left alone from there on."""
    N, Vt = table.shape
    cap = out.shape[1]
    n = n_out.long()
    for _ in range(int(max_steps)):
        s, p = state.long(), pos.long()
        live = (s >= 0) & (s < N) & (p >= 0) & (p < n) & (n <= cap)
        tok = out.gather(1, p.clamp(0, cap - 1).unsqueeze(1)).squeeze(1)
        live = live & (tok >= 0) & (tok < Vt)
        nx = table[s.clamp(0, N - 1), tok.clamp(0, Vt - 1)].to(torch.int32)
        nx = torch.where((nx < 0) | (nx >= N), torch.full_like(nx, GRAMMAR_DEAD), nx)
        state.copy_(torch.where(live, nx, state))
        pos.copy_(torch.where(live, pos + 1, pos))
    return state, pos


def grammar_mask(logits, table, state, rows=None, extra=None, n_extra=None, active=None,
                 vocab_size=None):
    """Bans the tokens a row's grammar state does not allow (ops/csrc/grammar.hip semantics):
    the single definition. Edits ``logits`` IN PLACE and returns it. No host sync.

    ``logits`` [B, Vs], of which the first ``V = vocab_size or Vs`` columns count; ``table``
    int16 [N, Vt >= V] as in ``grammar_advance``; ``state`` int32 [R]. The state q of logits
    row b is ``state[rows[b]]`` (``rows`` int32 [B], default b) walked over ``extra[b,
    :n_extra[b]]`` (int64 [B, W], int32 [B]; a speculative window up to the row's position).
    Every element ``i < V`` with ``table[q, i] < 0`` becomes ``-inf`` (0xFF80 for bf16); every
    other byte of the buffer keeps its bits. A row keeps all its bytes when ``active[b] ==
    0``, ``rows[b]`` is outside ``[0, R)``, ``state`` is outside ``[0, N)`` (``GRAMMAR_NONE``
    and ``GRAMMAR_DEAD`` included), ``n_extra[b]`` is outside ``[0, W]``, or the walk meets a
    token outside ``[0, Vt)`` or a result outside ``[0, N)`` (a forbidden draft)."""
    B, Vs = logits.shape
    V = Vs if vocab_size is None else int(vocab_size)
    dev = logits.device
    N, Vt = table.shape
    R = state.shape[0]
    r = torch.arange(B, device=dev) if rows is None else rows.long()
    ok = (r >= 0) & (r < R)
    if active is not None:
        ok = ok & active.bool()
    q = state[r.clamp(0, R - 1)].long()
    ok = ok & (q >= 0) & (q < N)
    q = q.clamp(0, N - 1)
    if extra is not None:
        W = extra.shape[1]
        ne = n_extra.long()
        ok = ok & (ne >= 0) & (ne <= W)
        for j in range(W):
            step = ok & (j < ne)
            tok = extra[:, j].long()
            nx = table[q, tok.clamp(0, Vt - 1)].long()
            fine = (tok >= 0) & (tok < Vt) & (nx >= 0) & (nx < N)
            ok = ok & (fine | ~step)
            q = torch.where(step & fine, nx, q)
    banned = (table[q][:, :V] < 0) & ok.unsqueeze(1)
    idt = _BITS[logits.dtype][0]
    ninf = torch.full((), float("-inf"), dtype=logits.dtype, device=dev).view(idt)
    raw = logits[:, :V].view(idt)
    raw.copy_(torch.where(banned, ninf, raw))
    return logits


SEQ_MAX = 8      # ops/csrc/seq_rules.hip kSeqMax: sequences per row and kind
SEQ_MAX_LEN = 8  # kSeqMaxLen there: tokens per sequence, and the longest no-repeat n-gram


def seq_ban(logits, prompt, prompt_len, out, n_out, bad, bad_len, ngram, rows=None, extra=None,
            n_extra=None, active=None, vocab_size=None):
    """Banned token sequences and no-repeat n-grams (ops/csrc/seq_rules.hip semantics): the
    single definition. Edits ``logits`` IN PLACE and returns it. No host sync.

    ``logits`` [B, Vs], of which the first ``V = vocab_size or Vs`` columns count. ``rows``,
    ``extra``, ``n_extra`` and ``active`` as in ``logit_process``: the context of logits row b,
    with ``r = rows[b]``, is ``c = prompt[r, :prompt_len[r]] ++ out[r, :n_out[r]] ++ extra[b,
    :n_extra[b]]``, of length C. ``bad`` int32 [R, SEQ_MAX, SEQ_MAX_LEN] with ``bad_len`` int32
    [R, SEQ_MAX] (0, or anything outside ``1..SEQ_MAX_LEN``: unused), ``ngram`` int32 [R].

    * banned sequence q of length L: if ``L - 1 <= C`` and the last ``L - 1`` context tokens
      equal ``bad[r, q, :L-1]``, token ``bad[r, q, L-1]`` is banned (L = 1: always).
    * no-repeat with ``n = ngram[r]`` in ``1..SEQ_MAX_LEN``: for every i in ``[0, C - n]`` with
      ``c[i : i+n-1] == c[C-n+1 : C]``, token ``c[i+n-1]`` is banned (the Hugging Face rule,
      over prompt and output; n = 1 bans every context token, C < n nothing).

    A banned id inside ``[0, V)`` gets the dtype's ``-inf``; one outside is ignored, and every
    other byte of the buffer keeps its bits. A row keeps all its bytes when ``active[b] ==
    0``, ``rows[b]`` is outside ``[0, R)``, ``prompt_len`` / ``n_out`` / ``n_extra`` is
    negative or exceeds its table, or ``ngram[r]`` is outside ``0..SEQ_MAX_LEN``."""
    B, Vs = logits.shape
    V = Vs if vocab_size is None else int(vocab_size)
    dev = logits.device
    R, P = prompt.shape
    cap = out.shape[1]
    Q, ML = bad.shape[1], bad.shape[2]
    r = torch.arange(B, device=dev) if rows is None else rows.long()
    ok = (r >= 0) & (r < R)
    if active is not None:
        ok = ok & active.bool()
    rc = r.clamp(0, R - 1)
    pl, no, n = prompt_len[rc].long(), n_out[rc].long(), ngram[rc].long()
    ok = ok & (pl >= 0) & (pl <= P) & (no >= 0) & (no <= cap) & (n >= 0) & (n <= ML)
    parts = [prompt[rc].long(), out[rc].long()]
    W, ne = 0, torch.zeros_like(no)
    if extra is not None:
        W = extra.shape[1]
        ne = n_extra.long()
        ok = ok & (ne >= 0) & (ne <= W)
        parts.append(extra.long())
    T = P + cap + W
    # the context, left-aligned: ctx[b, i] = c[i] for i < C; column T is spare
    pl, no, ne = (torch.where(ok, t, torch.zeros_like(t)).unsqueeze(1) for t in (pl, no, ne))
    C = pl + no + ne
    i = torch.arange(T + 1, device=dev).unsqueeze(0)
    src = torch.where(i < pl, i, torch.where(i < pl + no, P + i - pl, P + cap + i - pl - no))
    full = torch.cat(parts + [torch.zeros(B, 1, dtype=torch.int64, device=dev)], 1)
    ctx = full.gather(1, src.clamp(0, T))

    def at(j):
        return ctx.gather(1, j.clamp(0, T))

    banned = torch.zeros(B, V + 1, dtype=torch.bool, device=dev)
    yes = torch.ones(1, dtype=torch.bool, device=dev)

    def ban(tok, when):
        tok = torch.where(when & (tok >= 0) & (tok < V), tok, V)
        banned.scatter_(1, tok, yes.expand_as(tok))

    n = n.unsqueeze(1)
    match = ok.unsqueeze(1) & (n >= 1) & (i <= C - n)
    for k in range(ML - 1):
        match = match & ((k >= n - 1) | (at(i + n - 2 - k) == at(C - 1 - k)))
    ban(at(i + n - 1), match)
    for q in range(Q):
        L = bad_len[rc, q].long().unsqueeze(1)
        use = ok.unsqueeze(1) & (L >= 1) & (L <= ML) & (L - 1 <= C)
        seq = bad[rc, q].long()
        for k in range(ML - 1):
            use = use & ((k >= L - 1) | (at(C - L + 1 + k) == seq[:, k: k + 1]))
        ban(seq.gather(1, (L - 1).clamp(0, ML - 1)), use)
    idt = _BITS[logits.dtype][0]
    ninf = torch.full((), float("-inf"), dtype=logits.dtype, device=dev).view(idt)
    raw = logits[:, :V].view(idt)
    raw.copy_(torch.where(banned[:, :V], ninf, raw))
    return logits


def stop_check(out, n_out, pos, stops, stop_len, hit, active=None, lens=None, done=None,
               max_span=None):
    """Stop sequences (ops/csrc/seq_rules.hip semantics): the single definition. Cuts each
    row's output after the first completed stop sequence, IN PLACE. No host sync.

    ``out`` int64 [R, cap]; ``n_out``, ``pos``, ``hit`` int32 [R]; ``stops`` int32 [R, SEQ_MAX,
    SEQ_MAX_LEN] with ``stop_len`` int32 [R, SEQ_MAX] (anything outside ``1..SEQ_MAX_LEN``:
    unused). Per row the output ends e in ``(pos, n_out]`` are looked at in ascending order
    (at most ``max_span`` of them; None: all): e matches when some sequence q with ``1 <= L_q
    <= e`` has ``out[e-L_q : e] == stops[q, :L_q]`` (a match may begin before ``pos``; only
    its end is new). The smallest matching e wins, and there the lowest q: ``n_out = e``,
    ``hit = q`` and, where given, ``active = 0`` (uint8), ``lens = SLOT_INACTIVE`` (int32),
    ``done = 1`` (uint8). ``pos`` becomes the new ``n_out``, or the last end that was checked
    when ``max_span`` cut the look short. ``active`` and ``done`` are never read: a row that
    was retired at a later EOS is still cut at its stop. A row with ``n_out`` outside ``[0,
    cap]`` or ``pos`` outside ``[0, n_out]`` has nothing written."""
    R, cap = out.shape
    Q, ML = stops.shape[1], stops.shape[2]
    dev = out.device
    n, p = n_out.long(), pos.long()
    ok = (n >= 0) & (n <= cap) & (p >= 0) & (p <= n)
    last = n if max_span is None else torch.minimum(n, p + int(max_span))
    e = torch.arange(1, cap + 1, device=dev).view(1, cap, 1)  # the ends
    L = stop_len.long().view(R, 1, Q)
    m = ok.view(R, 1, 1) & (e > p.view(R, 1, 1)) & (e <= last.view(R, 1, 1)) & (L >= 1) & \
        (L <= ML) & (L <= e)
    ext = torch.cat([out, out.new_zeros(R, 1)], 1)
    for k in range(ML):  # newest token first: out[e-1-k] against stops[q, L-1-k]
        a = ext.gather(1, (e - 1 - k).clamp(0, cap).expand(R, cap, Q).reshape(R, -1))
        s = stops.long().gather(2, (L - 1 - k).clamp(0, ML - 1).view(R, Q, 1)).view(R, 1, Q)
        m = m & ((k >= L) | (a.view(R, cap, Q) == s))
    none = (cap + 1) * Q
    key = torch.where(m, e * Q + torch.arange(Q, device=dev).view(1, 1, Q), none)
    key = key.view(R, -1).min(1).values
    found = key < none
    ee, qq = key // Q, key % Q
    new_n = torch.where(found, ee, n)
    new_p = torch.where(found, ee, last)
    n_out.copy_(torch.where(found, new_n, n).to(torch.int32))
    pos.copy_(torch.where(ok, new_p, p).to(torch.int32))
    hit.copy_(torch.where(found, qq.to(torch.int32), hit))
    if active is not None:
        active.masked_fill_(found, 0)
    if lens is not None:
        lens.masked_fill_(found, SLOT_INACTIVE)
    if done is not None:
        done.masked_fill_(found, 1)
    return n_out, pos, hit


def _f(x):
    return x.to(torch.promote_types(x.dtype, torch.float32))


def gae(rewards, values, dones, bootstrap, gamma, lam):
    """[T,B] time-major GAE. Returns (advantages, value_targets)."""
    rewards, values, dones, bootstrap = map(_f, (rewards, values, dones, bootstrap))
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last = torch.zeros_like(bootstrap)
    vnext = bootstrap
    for t in range(T - 1, -1, -1):
        nt = 1.0 - dones[t]
        delta = rewards[t] + gamma * vnext * nt - values[t]
        last = delta + gamma * lam * nt * last
        adv[t] = last
        vnext = values[t]
    return adv, adv + values


def vtrace(log_rhos, discounts, rewards, values, bootstrap, clip_rho=1.0, clip_c=1.0,
           clip_pg_rho=1.0, lam=1.0):
    """Time-major V-trace (Espeholt et al. 2018). Returns (vs, pg_advantages)."""
    log_rhos, discounts, rewards, values, bootstrap = map(
        _f, (log_rhos, discounts, rewards, values, bootstrap))
    rhos = torch.exp(log_rhos)
    crho = torch.clamp(rhos, max=clip_rho)
    cs = lam * torch.clamp(rhos, max=clip_c)
    vtp1 = torch.cat([values[1:], bootstrap[None]], 0)
    deltas = crho * (rewards + discounts * vtp1 - values)
    acc = torch.zeros_like(bootstrap)
    out = []
    for t in range(values.shape[0] - 1, -1, -1):
        acc = deltas[t] + discounts[t] * cs[t] * acc
        out.append(acc)
    vs_minus_v = torch.stack(out[::-1], 0)
    vs = values + vs_minus_v
    vs_tp1 = torch.cat([vs[1:], bootstrap[None]], 0)
    pg = torch.clamp(rhos, max=clip_pg_rho) * (rewards + discounts * vs_tp1 - values)
    return vs, pg


def ppo_loss(logits, old_logits, actions, old_logp, adv, vpred, vtarg, clip=0.2, vf_clip=10.0,
             vf_coeff=1.0, ent_coeff=0.0, kl_coeff=0.0):
    """RLlib PPO loss (ppo_torch_learner.compute_loss_for_module). Returns (total, stats)."""
    lp = torch.log_softmax(logits.float(), -1)
    logp = lp.gather(-1, actions.long()[:, None])[:, 0]
    ratio = torch.exp(logp - old_logp.float())
    surr = torch.minimum(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip))
    ent = -(lp.exp() * lp).sum(-1)
    if old_logits is not None:
        olp = torch.log_softmax(old_logits.float(), -1)
        kl = (olp.exp() * (olp - lp)).sum(-1)
    else:
        kl = torch.zeros_like(ent)
    if vpred is not None:
        vf = torch.clamp((vpred.float() - vtarg.float()) ** 2, 0, vf_clip)
    else:
        vf = torch.zeros_like(ent)
    total = (-surr + vf_coeff * vf - ent_coeff * ent + kl_coeff * kl).mean()
    clipfrac = ((ratio < 1 - clip) | (ratio > 1 + clip)).float().mean()
    stats = torch.stack([total.detach(), (-surr).mean().detach(), vf.mean().detach(),
                         ent.mean().detach(), kl.mean().detach(), clipfrac])
    return total, stats


def _c51_support(K, v_min, v_max, like):
    dz = (v_max - v_min) / (K - 1)
    return v_min + dz * torch.arange(K, device=like.device, dtype=like.dtype), dz


def c51_project(p, rewards, discounts, terminateds, v_min, v_max):
    """Categorical projection of the Bellman-shifted distribution onto the fixed support
    (Bellemare et al. 2017, Algorithm 1; reference: dqn_torch_learner.py): atom j of
    ``p`` [B, K] moves to clamp(r + disc (1 - term) z_j) and its mass is split between
    the two neighbouring atoms (floor / ceil + scatter_add). A target landing exactly on
    an atom (l == u) keeps its whole mass there. Computes in p's dtype."""
    K = p.shape[-1]
    z, dz = _c51_support(K, v_min, v_max, p)
    r, d, t = (torch.as_tensor(x, device=p.device).to(p.dtype).expand(p.shape[0])[:, None]
               for x in (rewards, discounts, terminateds))
    tz = (r + d * (1.0 - t) * z[None]).clamp(v_min, v_max)
    b = ((tz - v_min) / dz).clamp(0, K - 1)
    lo, up = b.floor(), b.ceil()
    m = torch.zeros_like(p)
    m.scatter_add_(1, lo.long(), p * (up - b + (lo == up).to(p.dtype)))
    m.scatter_add_(1, up.long(), p * (b - lo))
    return m


def c51_loss(logits, actions, next_online, next_target, rewards, discounts, terminateds,
             weights=None, v_min=-10.0, v_max=10.0):
    """Distributional (C51) DQN loss on [B, A, K] atom logits: the greedy next action is
    taken under ``next_online`` (double-Q; None: under ``next_target``), the target
    net's distribution of that action is projected (``c51_project``) and the loss is the
    importance-weighted mean cross-entropy against the taken action's distribution.
    Returns (loss, per-row ce, next_action, projected target [B, K])."""
    B, _, K = logits.shape
    rows = torch.arange(B, device=logits.device)
    with torch.no_grad():
        sel = next_target if next_online is None else next_online
        z, _ = _c51_support(K, v_min, v_max, sel)
        na = (torch.softmax(sel, -1) * z).sum(-1).argmax(-1)
        m = c51_project(torch.softmax(next_target, -1)[rows, na], rewards, discounts,
                        terminateds, v_min, v_max).to(logits.dtype)
    lp = torch.log_softmax(logits, -1)[rows, actions.long()]
    ce = -(m * lp).sum(-1)
    loss = ce.mean() if weights is None else (ce * weights.to(ce.dtype)).mean()
    return loss, ce.detach(), na, m


def image_normalize(x_u8_nhwc, mean, std, out_dtype=torch.float32):
    x = x_u8_nhwc.float().div(255.0).permute(0, 3, 1, 2)
    m = torch.as_tensor(mean, dtype=torch.float32, device=x.device).view(1, -1, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32, device=x.device).view(1, -1, 1, 1)
    return ((x - m) / s).to(out_dtype).contiguous()
