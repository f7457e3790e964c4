"""``ref.grammar_mask`` and ``ref.grammar_advance`` (the single definitions of the grammar ops)
against scalar Python loops, bit for bit, and the argument checks of ``rf.grammar_mask`` /
``rf.grammar_advance``. ``make_case`` / ``make_advance_case`` are shared with the GPU file,
which compares the kernels with the reference from the same bytes."""

import numpy as np
import pytest
import torch

from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

N_STATES = 37
W = 5
NINF = -128  # 0xFF80 as int16: bf16 -inf


def _raw(t):
    return t.view(torch.int16)


def _table(V, g):
    """int16 [37, Vt]: state 0 allows every token, state 1 exactly one, the others a sparse, a
    half or a nearly full set; the padding columns hold anything."""
    Vt = (V + 7) // 8 * 8
    nxt = torch.randint(0, N_STATES, (N_STATES, Vt), generator=g)
    p = torch.tensor([0.03, 0.5, 0.97])[torch.arange(N_STATES) % 3].unsqueeze(1)
    allowed = torch.rand(N_STATES, Vt, generator=g) < p
    allowed[0] = True
    allowed[1] = False
    allowed[1, (V * 2) // 3] = True
    # whole 16-byte slots banned and whole slots allowed, whatever the density
    if Vt >= 32:
        allowed[2:, 8:16] = False
        allowed[2:, 16:24] = True
    table = torch.where(allowed, nxt, torch.full_like(nxt, -1)).to(torch.int16)
    table[:, V:] = torch.randint(-1, N_STATES, (N_STATES, Vt - V), generator=g).to(torch.int16)
    return table


def _allowed_token(table, q, V, g, want=True):
    """A token < V that state q allows (``want``) or forbids, None if there is none."""
    ids = np.flatnonzero((table[q, :V].numpy() >= 0) == want)
    if len(ids) == 0:
        return None
    return int(ids[int(torch.randint(0, len(ids), (1,), generator=g))])


def make_case(V, B, seed=0):
    """The arguments of ``grammar_mask`` for B logits rows over V columns, CPU tensors, bf16
    logits. Logits row b uses context row ``R - 1 - b``. The rows 1..8 (those below B), and
    again 21..28, are in turn: ``GRAMMAR_NONE``, ``GRAMMAR_DEAD``, a state out of range,
    inactive, a bad ``rows`` entry, a window whose walk dies, the state that allows
    everything, the state that allows one token. Every other row walks 0..W allowed tokens."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + B)
    table = _table(V, g)
    R = B + 3
    rows = (R - 1 - torch.arange(B)).to(torch.int32)
    state = torch.randint(2, N_STATES, (R,), generator=g).to(torch.int32)
    active = torch.ones(B, dtype=torch.uint8)
    extra = torch.randint(0, V, (B, W), generator=g)
    n_extra = torch.randint(0, W + 1, (B,), generator=g).to(torch.int32)
    for b in range(B):
        kind = b % 20 if b < 40 else 0
        r = int(rows[b])
        if kind == 1:
            state[r] = ref.GRAMMAR_NONE
        elif kind == 2:
            state[r] = ref.GRAMMAR_DEAD
        elif kind == 3:
            state[r] = N_STATES + 3
        elif kind == 4:
            active[b] = 0
        elif kind == 5:
            rows[b] = -1 if b < 20 else R
        elif kind == 7:
            state[r], n_extra[b] = 0, 0
        elif kind == 8:
            state[r], n_extra[b] = 1, 0
        if kind in (1, 2, 3, 5):
            continue
        q = int(state[r])
        if kind == 6:
            n_extra[b] = max(int(n_extra[b]), 2)
        for j in range(int(n_extra[b])):
            t = _allowed_token(table, q, V, g, want=not (kind == 6 and j == 1))
            for _ in range(20):  # the dying walk first reaches a state that forbids something
                if kind != 6 or j != 0 or t is None or int(table[q, t]) >= 2:
                    break
                t = _allowed_token(table, q, V, g)
            if t is None:  # nothing to pick: the walk ends here
                n_extra[b] = j
                break
            extra[b, j] = t
            q = int(table[q, t])
            if q < 0:
                break
    x = (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16)
    flat = x.view(-1)
    specials = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0])
    flat[torch.randint(0, flat.numel(), (max(1, flat.numel() // 50),), generator=g)] = \
        specials[torch.randint(0, 4, (max(1, flat.numel() // 50),), generator=g)].to(x.dtype)
    return dict(logits=x, table=table, state=state, rows=rows, extra=extra, n_extra=n_extra,
                active=active, vocab_size=V)


def call(fn, c, logits=None):
    """``fn`` (``ref.grammar_mask`` or ``rf.grammar_mask``) on the case, on a copy of its
    logits unless ``logits`` is given."""
    x = c["logits"].clone() if logits is None else logits
    return fn(x, c["table"], c["state"], rows=c["rows"], extra=c["extra"], n_extra=c["n_extra"],
              active=c["active"], vocab_size=c["vocab_size"])


def row_state(c, b):
    """Scalar: the effective state of logits row b, or None when the row is skipped."""
    table, state = c["table"], c["state"]
    N, Vt = table.shape
    if not int(c["active"][b]):
        return None
    r = int(c["rows"][b])
    if not 0 <= r < state.shape[0]:
        return None
    q = int(state[r])
    if not 0 <= q < N:
        return None
    ne = int(c["n_extra"][b])
    if not 0 <= ne <= c["extra"].shape[1]:
        return None
    for j in range(ne):
        t = int(c["extra"][b, j])
        if not 0 <= t < Vt:
            return None
        q = int(table[q, t])
        if not 0 <= q < N:
            return None
    return q


def skipped_rows(c):
    return [b for b in range(c["logits"].shape[0]) if row_state(c, b) is None]


def scalar_mask(c):
    """The definition as loops over int16 bit patterns."""
    x = _raw(c["logits"]).clone()
    V = c["vocab_size"]
    for b in range(x.shape[0]):
        q = row_state(c, b)
        if q is None:
            continue
        trow = c["table"][q].tolist()
        for i in range(V):
            if trow[i] < 0:
                x[b, i] = NINF
    return x


@pytest.mark.parametrize("B", (1, 5, 67))
@pytest.mark.parametrize("V", (1, 7, 9, 509))
def test_mask_reference_equals_scalar_loops(V, B):
    c = make_case(V, B)
    got = call(ref.grammar_mask, c)
    assert torch.equal(_raw(got), scalar_mask(c))


def test_the_case_exercises_skips_and_bans():
    c = make_case(50257, 67)
    want = call(ref.grammar_mask, c)
    skipped = skipped_rows(c)
    changed = (_raw(want) != _raw(c["logits"])).any(1)
    assert len(skipped) >= 5 and not changed[skipped].any()
    assert changed.sum() > (67 - len(skipped)) // 2
    # per-row numpy check of the wide case (the scalar loops cover the small ones)
    for b in range(67):
        q = row_state(c, b)
        exp = _raw(c["logits"][b]).clone()
        if q is not None:
            exp[c["table"][q, :50257] < 0] = NINF
        assert torch.equal(_raw(want[b]), exp), b
    kinds = {b: row_state(c, b) for b in (6, 7, 8)}
    assert kinds[6] is None and kinds[7] == 0 and kinds[8] == 1
    assert not changed[7]  # everything allowed
    finite7 = ~(_raw(c["logits"][8]) == NINF)
    assert int(((_raw(want[8]) != NINF) & finite7).sum()) <= 1  # one token allowed


def test_mask_on_a_padded_view_and_other_dtypes():
    c = make_case(509, 5)
    want = call(ref.grammar_mask, c)
    wide = torch.full((5, 640), 0x7FA5, dtype=torch.int16).view(torch.bfloat16)
    wide[:, 3: 3 + 509] = c["logits"]
    out = call(rf.grammar_mask, c, wide[:, 3: 3 + 509])
    assert out.data_ptr() == wide[:, 3:].data_ptr()
    assert torch.equal(_raw(wide[:, 3: 3 + 509]), _raw(want))
    assert (_raw(wide[:, :3]) == 0x7FA5).all() and (_raw(wide[:, 512:]) == 0x7FA5).all()
    f32 = call(ref.grammar_mask, c, c["logits"].float())
    assert torch.equal(f32.view(torch.int32), want.float().view(torch.int32))
    # no rows / extra / active: row b uses state[b], no walk
    plain = ref.grammar_mask(c["logits"].clone(), c["table"], c["state"][:5].contiguous())
    for b in range(5):
        q = int(c["state"][b])
        exp = _raw(c["logits"][b]).clone()
        if 0 <= q < N_STATES:
            exp[c["table"][q, :509] < 0] = NINF
        assert torch.equal(_raw(plain[b]), exp)


# ------------------------------------------------------------------------------ advance
CAP = 12


def make_advance_case(V, R, seed=0):
    """The arguments of ``grammar_advance``: rows 1..8 (and 21..28) are ``GRAMMAR_NONE``,
    ``GRAMMAR_DEAD``, a state out of range, a negative ``pos``, ``n_out`` beyond cap, a token
    out of range in the way, a forbidden token in the way, nothing left to consume."""
    g = torch.Generator().manual_seed(77 * seed + V + R)
    table = _table(V, g)
    Vt = table.shape[1]
    state = torch.randint(0, N_STATES, (R,), generator=g).to(torch.int32)
    n_out = torch.randint(0, CAP + 1, (R,), generator=g).to(torch.int32)
    pos = (torch.rand(R, generator=g) * (n_out + 1)).to(torch.int32).clamp(max=n_out)
    out = torch.randint(0, V, (R, CAP), generator=g)
    for r in range(R):
        kind = r % 20 if r < 40 else 0
        if kind in (6, 7):
            n_out[r], pos[r] = CAP, 2
        q = int(state[r])
        for p in range(int(pos[r]), int(n_out[r])):
            t = _allowed_token(table, q, V, g)
            if t is None:
                break
            out[r, p] = t
            q = int(table[q, t])
        if kind == 1:
            state[r] = ref.GRAMMAR_NONE
        elif kind == 2:
            state[r] = ref.GRAMMAR_DEAD
        elif kind == 3:
            state[r] = N_STATES
        elif kind == 4:
            pos[r] = -1
        elif kind == 5:
            n_out[r] = CAP + 1
        elif kind == 6:
            out[r, 4] = Vt if r < 20 else -1
        elif kind == 7:
            q = int(state[r])
            for p in range(2, 4):
                q = int(table[q, int(out[r, p])])
            bad = _allowed_token(table, q, V, g, want=False) if q >= 0 else None
            if bad is not None:
                out[r, 4] = bad
        elif kind == 8:
            pos[r] = n_out[r]
    return dict(state=state, pos=pos, out=out, n_out=n_out, table=table)


def call_advance(fn, c, max_steps):
    s, p = c["state"].clone(), c["pos"].clone()
    got = fn(s, p, c["out"], c["n_out"], c["table"], max_steps)
    assert got[0] is s and got[1] is p
    return s, p


def scalar_advance(c, max_steps):
    state, pos = c["state"].tolist(), c["pos"].tolist()
    table, out = c["table"], c["out"]
    N, Vt = table.shape
    for r in range(len(state)):
        n = int(c["n_out"][r])
        for _ in range(max_steps):
            q, p = state[r], pos[r]
            if not (0 <= q < N and 0 <= p < n and n <= out.shape[1]):
                break
            t = int(out[r, p])
            if not 0 <= t < Vt:
                break
            nx = int(table[q, t])
            state[r] = nx if 0 <= nx < N else ref.GRAMMAR_DEAD
            pos[r] = p + 1
    return state, pos


@pytest.mark.parametrize("max_steps", (0, 1, 3, CAP + 2))
@pytest.mark.parametrize("V", (1, 9, 509))
def test_advance_reference_equals_scalar_loops(V, max_steps):
    c = make_advance_case(V, 67)
    s, p = call_advance(ref.grammar_advance, c, max_steps)
    ws, wp = scalar_advance(c, max_steps)
    assert s.tolist() == ws and p.tolist() == wp
    if max_steps == CAP + 2 and V == 509:
        assert ref.GRAMMAR_DEAD in [a for a, b in zip(ws, c["state"].tolist()) if a != b]
        assert ws[6] != c["state"].tolist()[6] and wp[6] == 4  # stopped at the bad token
        cut = call_advance(ref.grammar_advance, c, 1)[1]
        assert (cut - c["pos"]).max() == 1 and (p - c["pos"]).max() > 1


def test_argument_checks():
    c = make_case(9, 5)
    bad = dict(c, table=c["table"].int())
    with pytest.raises(ValueError, match="table"):
        call(rf.grammar_mask, bad)
    with pytest.raises(ValueError, match="table"):
        call(rf.grammar_mask, dict(c, table=c["table"][:, :9]))
    with pytest.raises(ValueError, match="state"):
        call(rf.grammar_mask, dict(c, state=c["state"].long()))
    with pytest.raises(ValueError, match="go together"):
        rf.grammar_mask(c["logits"].clone(), c["table"], c["state"], extra=c["extra"])
    with pytest.raises(ValueError, match="rows="):
        rf.grammar_mask(c["logits"].clone(), c["table"], c["state"][:2].contiguous())
    with pytest.raises(ValueError, match="vocab_size"):
        call(rf.grammar_mask, dict(c, vocab_size=10))
    a = make_advance_case(9, 5)
    with pytest.raises(ValueError, match="max_steps"):
        call_advance(rf.grammar_advance, a, -1)
    with pytest.raises(ValueError, match="pos"):
        call_advance(rf.grammar_advance, dict(a, pos=a["pos"].long()), 1)
