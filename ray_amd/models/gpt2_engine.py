"""Continuous batching for GPT-2 generation: a persistent KV cache of S slots that requests
enter and leave independently, between replays of ONE captured decode step.

    eng = GPT2Engine(model, slots=8)
    rid = eng.submit([464, 3290], 32, temperature=0.8, seed=7)
    while eng.has_work():
        for rid, new_tokens, finished in eng.step():
            ...

The device step is the one of ``generate(seeds=...)`` (``rf.sample_logits`` with the per-slot
parameters and ``cache.lens`` as the hash step, then ``decode_step`` back into the fixed
logits buffer) with the engine's bookkeeping, ``rf.slot_advance``, between the two: it
stores the token, counts it, retires the slot at ``max_new_tokens`` or EOS, and pins the
``cache.lens`` of every idle slot to ``SLOT_INACTIVE``, which the decode-attention kernel
treats as an inactive row (no cache write, zero output). The step has a fixed width S and
touches nothing on the host, so it is captured once and every later step is one replay.

Admission runs between replays: one ragged ``GPT2.prefill_into`` for all the prompts that
found a free slot (``rf.kv_insert`` moves their K/V into the slots' rows), then the
per-slot parameters and the prefill's logits rows go into the fixed buffers. A request's
tokens are those of ``model.generate(prompt, max_new_tokens, ..., seeds=[seed])`` on that
request alone, cut after the first EOS: whenever it was admitted, in whichever slot, and
whoever shared the step.

``poll_every``: device steps per ``step()`` call, between two polls. A poll is one download
and a host synchronisation, during which the GPU idles; at 8 (the default) the engine beat
static batching at both measured widths, at 1 only at S = 8 (profiles/r10/engine.md). The
price: tokens arrive in groups of up to ``poll_every``, and a slot that finishes inside a
group stays idle until the group ends.

Shared prompt prefixes (``prefix_slots=P``): ``add_prefix(tokens)`` prefills a prefix once
into a row of a second KV cache, and ``submit(tokens, ..., prefix=pid)`` takes ``tokens`` as
the continuation of it. At admission the slot gets the prefix's positions by one
``rf.kv_copy`` per round (all layers, K and V) and only the continuation runs through the
model, ``GPT2.extend_into`` (``rf.attn_extend``: new queries over cached keys).

Chunked prefill (``prefill_chunk=C``): no more than C prompt tokens per request are processed
per ``step()``, so a long prompt stalls the running requests for one chunk and not for its
whole prefill. A slot whose prompt is not finished is FILLING: occupied, cancellable, but
inactive on the device (``slot_advance`` keeps its ``cache.lens`` pinned, ``decode_step``
leaves its cache row alone) and it produces no event; the host keeps its ``base``, the
positions cached so far. Each ``step()`` admits, runs one chunk round for all filling slots
together (rows at ``base == 0`` through ``prefill_into``, the others through ONE ragged
``extend_into``), installs the rows whose prompt just completed and runs the device steps.
The captured step is untouched. With both options at their defaults the engine does what it
did without them. The guarantee above holds with ``prefix + tokens`` as the prompt, for every
``prefill_chunk``.

Adapters (``lora=LoRAStack``): ``submit(..., adapter=i)`` names one of the stack's adapters
for the request. The id goes into ``self.adapter`` (int32 [S], -1: the base model), one more
fixed-address buffer of the captured step, whose ``decode_step`` applies every slot's own
adapter (``rf.lora_add``); the prompt passes get the round's ids. ``load_adapter`` /
``unload_adapter`` rewrite the stack in place between steps, with no re-capture. A prefix
records the adapter it was prefilled with, since its K/V depend on it. The guarantee above
holds with ``generate(..., adapters=[adapter])``; without ``lora``, or with no request naming
an adapter, the engine produces the tokens it produced before.

Speculative decoding (``speculate=k``, 1..8; 0, the default, is the engine without it):
a device step then emits between 1 and k + 1 tokens per slot. After the sampler has drawn
``tok0`` for position ``lens[s]``, a drafter proposes up to k tokens to follow it, ONE
``GPT2.verify_step`` runs the whole window through the model (``rf.attn_extend`` over the
slot's cache, the logits after every window token), the sampler draws a token from each
of them with the hash step of ITS position, and ``rf.spec_accept`` keeps the drafts up to
the first one the sampler disagrees with. The sampler's randomness is a hash of (seed,
position), so the token at a position is a function of the logits there and the request's
parameters: an accepted draft IS the token the plain step would have drawn. There is no
rejection sampling and the output distribution does not change, for greedy and sampled
requests alike; the guarantee above holds for every k and every drafter that keeps its
contract. The default drafter is prompt lookup, ``rf.spec_draft``: the tokens that followed
the most recent earlier occurrence of the request's last ``ngram[1]`` .. ``ngram[0]``
tokens, looked up on the device in ``hist``, the request's tokens by position. Drafting
and accepting are two small integer kernels (ops/csrc/spec.hip), so the speculative step
touches nothing on the host either and is one graph replay. ``drafter``: any capturable
device function ``(tok0, hist, lens, n_out, max_new, active) -> (win int64 [S, k + 1],
n_win int32 [S])`` with ``win[:, 0] == tok0`` and ``0 <= n_win - 1 <= min(k, room - 1)``,
``room = min(max_new - n_out, max_len - lens)``, for the active slots and ``n_win = 0``
for the others: the hook for a draft model. Memory safety does not depend on that
contract (every kernel checks its bounds), the tokens do. ``spec_stats()`` reports how
many drafts were proposed and how many accepted.

Log-probabilities (``logprobs=N``, 0..8; None, the default, is the engine without them: no
buffer, no extra op, 3-tuple events): three more fixed-address tables, ``lp_hist``
[S, max_len] and the top-N ids and values beside it, and ONE more call in the captured
step, ``rf.token_logprobs`` between the sampler and ``rf.slot_advance`` with ``rows =
cache.rows``, ``cols = n_out``, ``active = active``: the entry lands at the output index of
the token ``slot_advance`` is about to store. The speculative step makes two calls before
``rf.spec_accept``: ``tok0`` at ``n_out``, and the window's ``cand`` at ``n_out + 1 + j``
for ``j < n_win``. ``submit(..., logprobs=m)``, m <= N, makes the request's events carry
them; a poll is still one download. A request's entries are those of ``generate(...,
seeds=[seed], logprobs=m)`` on it alone, cut after the first EOS, with prefixes, chunked
prefill, adapters, ``cancel`` and every ``speculate``.

Logit processors (``logit_processors=True``; False, the default, is the engine without them:
no buffer, no extra op, and ``submit`` rejects the fields): ``submit(..., repetition_penalty=,
presence_penalty=, frequency_penalty=, logit_bias=, min_new_tokens=)`` as in ``generate``. The
per-slot parameters, the bias lists and the prompts (``LogitControls``: int32 [S, max_len]
with their lengths, the prefix's tokens included) sit at fixed addresses and are written
when a slot's prompt is complete; ``rf.logit_process`` then edits that round's prefill logits
rows, ``rows`` naming their slots, before they go into ``self.buf``. The invariant: ``self.buf``
holds PROCESSED rows. The plain step keeps it with one more call at its end, after
``decode_step``, on ``self.logits`` with ``out``, ``n_out`` and ``active`` as ``slot_advance``
left them. The speculative step makes one call on the window's logits between
``verify_step`` and the window's sampler, with ``rows = slot``, ``extra = win[slot]`` and
``n_extra = j + 1`` for window row j (active iff ``j < n_win`` and the slot is): row j sees
exactly the tokens that precede its position, so the row ``rf.spec_accept`` copies into
``self.buf`` is already processed with every kept token and is not processed again. A
request's tokens and logprobs (those of the processed logits, the distribution the token
was drawn from) are those of ``generate(..., seeds=[seed], <same controls>)`` on it alone,
cut after the first EOS, with prefixes, chunked prefill, adapters, ``cancel``, every
``speculate`` and ``logprobs``; a request that names no control is untouched.

Grammar-constrained decoding (``grammar_states=N``; 0, the default, is the engine without it:
no buffer, no extra op, and ``submit`` rejects ``grammar=``): a pool ``gtable`` int16 [N, Vt]
of automaton states (``TokenDFA`` rows, models/grammar.py; Vt is the vocabulary rounded up to
8, so the pool costs about 100 KB per state at GPT-2's vocabulary) and per slot ``gstate``
(the automaton state, ``rf.GRAMMAR_NONE`` for a request without a grammar) and ``gpos`` (the
output tokens that state has consumed), all at fixed addresses. ``add_grammar(dfa)`` writes
the automaton's states, shifted to pool-global ids, into the first free range of rows that
fits, in place between steps and with no re-capture; ``submit(..., grammar=gid)`` names it;
``drop_grammar(gid)`` frees the rows once no queued or running request names it. When a slot's
prompt is complete, after the logit processors, ``gstate`` becomes the grammar's start state
and ``rf.grammar_mask`` bans what it does not allow in that round's prefill rows before they
go into ``self.buf``. The invariant: ``self.buf`` holds processed AND MASKED rows. The plain
step keeps it at its end: ``rf.grammar_advance`` (one step: the token ``slot_advance`` just
stored), the logit processors, then ``rf.grammar_mask`` on ``self.logits`` with ``active``.
The speculative step masks the window's logits between the logit processors and the window's
sampler: window row j of a slot uses the slot's state walked over ``win[slot, :j + 1]``, and
is live iff ``j < n_win`` and the slot is active; ``rf.grammar_advance`` (up to k + 1 steps)
follows what ``rf.spec_accept`` kept. That is exact: a draft the grammar forbids leaves its
own row and all later rows of the window unmasked, but it can never equal ``cand`` of the
masked row before it, so it and everything after it is rejected; and the row ``spec_accept``
copies into ``self.buf`` was walked over accepted tokens only, so it is already masked. Every
constrained request's output is a word of its grammar (a prefix where ``max_new_tokens`` cuts
it), and its tokens and logprobs are those of ``generate(..., seeds=[seed], grammar=dfa, <same
controls>)`` on it alone, with prefixes, chunked prefill, adapters, ``cancel``, ``logprobs``,
logit processors and every ``speculate``; a request without a grammar gets the tokens it got
before, whoever shares the step.

Sequence rules (``sequence_rules=True``; False, the default, is the engine without them: no
buffer, no extra op, and ``submit`` rejects the fields): ``submit(..., stop=, bad_words=,
no_repeat_ngram_size=)`` as in ``generate``, one request's value each. The tables
(``SequenceRules``: the stop and banned sequences with their lengths, the n-gram size, ``pos``
and ``hit`` per slot, and the prompts, ONE copy shared with the logit processors' when both
exist) sit at fixed addresses and are written when a slot's prompt is complete, the prefix's
tokens included, with ``pos = 0`` and ``hit = -1``; ``rf.seq_ban`` then edits that round's
prefill rows, after the logit processors and before the grammar mask, before they go into
``self.buf``. The invariant: ``self.buf`` holds rows with the banned tokens at ``-inf``. The
plain step runs ``rf.stop_check`` right after ``rf.slot_advance`` with ``active`` and
``cache.lens``, so a slot whose output just completed a stop sequence is an inactive row for
``decode_step`` already, and ``rf.seq_ban`` at its end between the logit processors and
``rf.grammar_mask``. The speculative step bans on the window's logits with the ``rows`` /
``extra`` / ``n_extra`` / ``live`` construction of the logit processors (row j sees exactly
the tokens before its position) and runs ``rf.stop_check`` with ``max_span = k + 1`` right
after ``rf.spec_accept``: it cuts ``n_out`` back to the first completed stop inside the
accepted window, also when ``spec_accept`` has already retired the slot at a later EOS or at
``max_new_tokens`` (``stop_check`` never reads ``active``). What lies beyond the cut in ``out``,
``hist`` and the logprob tables is never read. ``hit`` names the stop sequence that ended a
slot's request (-1: none); events keep their shape. A request's tokens, and its logprobs,
are those of ``generate(..., seeds=[seed], <same rules>)`` on it alone, cut after the first
EOS or the first completed stop sequence, whichever ends earlier, with prefixes, chunked
prefill, adapters, ``cancel``, logit processors, grammars (``stop`` only: ``bad_words`` or
``no_repeat_ngram_size > 0`` with a grammar is a ``ValueError``), ``logprobs`` and every
``speculate``; a request that names no rule gets the tokens it got before, whoever shares
the step.

Single-threaded by contract: every call comes from one thread."""

from __future__ import annotations

import collections
import math

import numpy as np
import torch

from ray_amd.models.gpt2 import (GPT2, KVCache, LogitControls, SequenceRules, checked_controls,
                                 checked_grammar, checked_grammar_sequences,
                                 checked_sequences)
from ray_amd.models.grammar import MAX_STATES, padded_vocab
from ray_amd.ops import functional as rf
from ray_amd.ops.graph_lock import CapturedStep


class _Request:
    __slots__ = ("rid", "tokens", "max_new", "temperature", "top_k", "top_p", "seed", "pid",
                 "adapter", "logprobs", "controls", "grammar", "rules")

    def __init__(self, rid, tokens, max_new, temperature, top_k, top_p, seed, pid=None,
                 adapter=-1, logprobs=None, controls=None, grammar=None, rules=None):
        # tokens: the whole prompt (the prefix's tokens included); pid: the prefix it names
        self.rid, self.tokens, self.max_new = rid, tokens, max_new
        self.temperature, self.top_k, self.top_p, self.seed = temperature, top_k, top_p, seed
        self.pid = pid
        self.adapter = adapter  # -1: the base model
        self.logprobs = logprobs  # None: the request reports none; else its top-n width
        self.controls = controls  # a checked_controls result (None: neutral)
        self.grammar = grammar  # an add_grammar id (None: unconstrained)
        self.rules = rules  # a checked_sequences result (None: no rule)


class GPT2Engine:
    def __init__(self, model: GPT2, slots=8, max_len=None, eos_token_id=None, graph=None,
                 poll_every=8, prefix_slots=0, prefill_chunk=None, lora=None, speculate=0,
                 ngram=(2, 4), drafter=None, logprobs=None, logit_processors=False,
                 grammar_states=0, sequence_rules=False):
        cfg = model.cfg
        dev = model.wte.device
        S = int(slots)
        if S < 1:
            raise ValueError("slots must be >= 1")
        if int(poll_every) < 1:
            raise ValueError("poll_every must be >= 1")
        if int(prefix_slots) < 0:
            raise ValueError("prefix_slots must be >= 0")
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("prefill_chunk must be None or >= 1")
        if isinstance(speculate, bool) or not isinstance(speculate, int) or \
                not 0 <= speculate <= rf.SPEC_MAX_DRAFTS:
            raise ValueError(f"speculate must be an int in 0..{rf.SPEC_MAX_DRAFTS}, got "
                             f"{speculate!r}")
        try:
            lo, hi = (int(n) for n in ngram)
        except (TypeError, ValueError):
            raise ValueError(f"ngram must be a pair (min, max), got {ngram!r}") from None
        if not 1 <= lo <= hi <= rf.SPEC_MAX_NGRAM:
            raise ValueError(f"ngram needs 1 <= min <= max <= {rf.SPEC_MAX_NGRAM}, got {ngram!r}")
        if drafter is not None and not speculate:
            raise ValueError("a drafter needs speculate >= 1")
        if logprobs is not None and (isinstance(logprobs, bool) or not isinstance(logprobs, int)
                                     or not 0 <= logprobs <= rf.LOGPROB_MAX_TOP):
            raise ValueError(f"logprobs must be None or an int in 0..{rf.LOGPROB_MAX_TOP}, got "
                             f"{logprobs!r}")
        if isinstance(grammar_states, bool) or not isinstance(grammar_states, int) or \
                not 0 <= grammar_states <= MAX_STATES:
            raise ValueError(f"grammar_states must be an int in 0..{MAX_STATES}, got "
                             f"{grammar_states!r}")
        if grammar_states and eos_token_id is None:
            raise ValueError("grammar_states needs eos_token_id: a grammar ends with EOS")
        if graph is None:
            graph = dev.type == "cuda"
        if graph and dev.type != "cuda":
            raise ValueError("graph=True needs the model on the GPU")
        self.model, self.slots, self.device = model, S, dev
        self.max_len = cfg.n_positions if max_len is None else int(max_len)
        self.eos = None if eos_token_id is None else int(eos_token_id)
        self.poll_every = int(poll_every)
        self.steps = 0  # device steps so far

        # everything the captured step reads or writes: allocated once, fixed addresses
        self.cache = KVCache(cfg, S, self.max_len, dev, model.wte.dtype)
        self.cache.lens.fill_(rf.SLOT_INACTIVE)
        self.buf = torch.zeros(S, cfg.padded_vocab, device=dev, dtype=model.wte.dtype)
        self.logits = self.buf[:, : cfg.vocab_size]
        self.temperature = torch.zeros(S, dtype=torch.float32, device=dev)
        self.top_k = torch.zeros(S, dtype=torch.int32, device=dev)
        self.top_p = torch.ones(S, dtype=torch.float32, device=dev)
        self.seeds = torch.zeros(S, dtype=torch.int64, device=dev)
        self.n_out = torch.zeros(S, dtype=torch.int32, device=dev)
        self.max_new = torch.zeros(S, dtype=torch.int32, device=dev)
        self.active = torch.zeros(S, dtype=torch.uint8, device=dev)
        self.out = torch.zeros(S, self.max_len, dtype=torch.int64, device=dev)
        self._seen = torch.zeros(S, dtype=torch.int64, device=dev)  # n_out at the last poll
        self.lora = lora
        self.adapter = None
        if lora is not None:
            model.attach_lora(lora)
            self.adapter = torch.full((S,), -1, dtype=torch.int32, device=dev)
        self.speculate, self.ngram = speculate, (lo, hi)
        self._drafter = drafter
        if speculate:
            W = speculate + 1  # the window: the sampled token and the drafts
            self.hist = torch.zeros(S, self.max_len, dtype=torch.int32, device=dev)
            self.win = torch.zeros(S, W, dtype=torch.int64, device=dev)
            self.n_win = torch.zeros(S, dtype=torch.int32, device=dev)
            self.logits_win = torch.zeros(S, W, cfg.padded_vocab, device=dev,
                                          dtype=model.wte.dtype)
            self.n_drafted = torch.zeros(S, dtype=torch.int32, device=dev)
            self.n_accepted = torch.zeros(S, dtype=torch.int32, device=dev)
            # every slot's sampler parameters once per window row (written at admission),
            # and the window rows' distance from lens
            self._win_params = [torch.zeros(S, W, dtype=t.dtype, device=dev)
                                for t in (self.temperature, self.top_k, self.top_p, self.seeds)]
            self._win_offs = torch.arange(1, W + 1, dtype=torch.int32, device=dev).unsqueeze(0)
            if drafter is None:
                self._drafter = self._ngram_drafter
        # a poll carries what poll_every steps can emit per slot
        self._ar = torch.arange(self.poll_every * (speculate + 1), device=dev).unsqueeze(0)
        self.logprobs = logprobs
        if logprobs is not None:
            # entry [s, i] describes out[s, i]: written by rf.token_logprobs inside the step
            self.lp_hist = torch.zeros(S, self.max_len, dtype=torch.float32, device=dev)
            self.top_ids_hist = torch.full((S, self.max_len, logprobs), -1, dtype=torch.int32,
                                           device=dev)
            self.top_lp_hist = torch.zeros(S, self.max_len, logprobs, dtype=torch.float32,
                                           device=dev)
            self._lp_out = (self.lp_hist, self.top_ids_hist, self.top_lp_hist)
            if speculate:
                self._win_rows = self.cache.rows.repeat_interleave(speculate + 1)
                self._win_idx = torch.arange(speculate + 1, dtype=torch.int32,
                                             device=dev).unsqueeze(0)

        self.ctl = None
        if logit_processors:
            self.ctl = LogitControls(S, self.max_len, dev)
            if speculate:
                W = speculate + 1
                self._ctl_rows = self.cache.rows.repeat_interleave(W)
                self._ctl_idx = torch.arange(W, dtype=torch.int32, device=dev).unsqueeze(0)
                self._ctl_n_extra = torch.arange(1, W + 1, dtype=torch.int32,
                                                 device=dev).repeat(S)

        if grammar_states:
            # the pool of automaton states and every slot's state: fixed addresses, rewritten
            # in place (add_grammar, _fill_rows); the attributes exist only with the option
            self.gtable = torch.full((grammar_states, padded_vocab(cfg.vocab_size)), -1,
                                     dtype=torch.int16, device=dev)
            self.gstate = torch.full((S,), rf.GRAMMAR_NONE, dtype=torch.int32, device=dev)
            self.gpos = torch.zeros(S, dtype=torch.int32, device=dev)
            self._gfree = [(0, grammar_states)]  # free ranges (first row, rows), by first row
            self._grammars = {}  # gid -> (first row, rows, the start state's pool id, dfa)
            self._next_gid = 0
            if speculate:
                W = speculate + 1
                self._g_rows = self.cache.rows.repeat_interleave(W)
                self._g_idx = torch.arange(W, dtype=torch.int32, device=dev).unsqueeze(0)
                self._g_n_extra = torch.arange(1, W + 1, dtype=torch.int32, device=dev).repeat(S)
        self._has_grammar = bool(grammar_states)

        self._has_seq = bool(sequence_rules)
        if sequence_rules:
            # the slots' sequence tables: fixed addresses, rewritten in place (_fill_rows); the
            # prompts are the logit processors' copy where there is one
            self.seq = SequenceRules(S, self.max_len, dev, controls=self.ctl)
            if speculate:
                W = speculate + 1
                self._seq_rows = self.cache.rows.repeat_interleave(W)
                self._seq_idx = torch.arange(W, dtype=torch.int32, device=dev).unsqueeze(0)
                self._seq_n_extra = torch.arange(1, W + 1, dtype=torch.int32,
                                                 device=dev).repeat(S)

        self._queue = collections.deque()
        self._slot_req = [None] * S  # the request running in each slot
        self._seen_host = [0] * S
        self._next_rid = 0
        # a filling slot's base: prompt positions cached so far (None: not filling)
        self._fill = [None] * S
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)
        self.prefix_slots = int(prefix_slots)
        self.prefix_cache = None
        if self.prefix_slots:
            self.prefix_cache = KVCache(cfg, self.prefix_slots, self.max_len, dev,
                                        model.wte.dtype)
        self._prefixes = {}  # pid -> (row of prefix_cache, tokens, adapter)
        self._prefix_free = list(range(self.prefix_slots))
        self._next_pid = 0
        self._graph = None
        if graph:
            with torch.no_grad():
                self._device_step()  # every slot idle: warms up what the capture needs
            self._graph = CapturedStep(self._device_step, dev)

    # ------------------------------------------------------------------ the device step
    def _device_step(self):
        if self.speculate:
            return self._spec_step()
        tok = rf.sample_logits(self.logits, self.temperature, self.top_k, self.top_p, self.seeds,
                               self.cache.lens, validate=False)
        if self.logprobs is not None:
            # the entry lands at the output index slot_advance is about to store tok at
            rf.token_logprobs(self.logits, tok, self.logprobs, out=self._lp_out,
                              rows=self.cache.rows, cols=self.n_out, active=self.active)
        rf.slot_advance(tok, self.cache.lens, self.n_out, self.max_new, self.active, self.out,
                        self.eos)
        if self._has_seq:
            # the token just stored may complete a stop sequence: the slot is then inactive
            # for decode_step already
            self.seq.check(self.out, self.n_out, active=self.active, lens=self.cache.lens,
                           max_span=1)
        self.model.decode_step(tok, self.cache, out=self.buf, adapters=self.adapter)
        if self._has_grammar:
            # the state follows tok (a slot without a grammar, or one that is idle and has
            # nothing new in out, stays as it is)
            rf.grammar_advance(self.gstate, self.gpos, self.out, self.n_out, self.gtable, 1)
        if self.ctl is not None:
            # out / n_out hold tok, and a slot that just finished is inactive
            self.ctl.process(self.logits, self.out, self.n_out, self.eos, active=self.active)
        if self._has_seq:
            self.seq.ban(self.logits, self.out, self.n_out, active=self.active)
        if self._has_grammar:
            rf.grammar_mask(self.logits, self.gtable, self.gstate, active=self.active)

    def _ngram_drafter(self, tok0, hist, lens, n_out, max_new, active):
        return rf.spec_draft(tok0, hist, lens, n_out, max_new, active, self.speculate,
                             *self.ngram, win=self.win, n_win=self.n_win)

    def _spec_step(self):
        """The speculative step, five calls: sample, draft, verify, sample the window, accept."""
        S, W, V = self.slots, self.speculate + 1, self.model.cfg.vocab_size
        lens = self.cache.lens
        tok0 = rf.sample_logits(self.logits, self.temperature, self.top_k, self.top_p, self.seeds,
                                lens, validate=False)
        win, n_win = self._drafter(tok0, self.hist, lens, self.n_out, self.max_new, self.active)
        self.model.verify_step(win, n_win, self.cache, out=self.logits_win,
                               adapters=self.adapter)
        if self.ctl is not None:
            # window row j: the logits after win[s, :j + 1], which follow out[s, :n_out]
            live = (self._ctl_idx < n_win.unsqueeze(1)) & self.active.bool().unsqueeze(1)
            self.ctl.process(self.logits_win.view(S * W, -1)[:, :V], self.out, self.n_out,
                             self.eos, rows=self._ctl_rows,
                             extra=win.unsqueeze(1).expand(S, W, W).reshape(S * W, W),
                             n_extra=self._ctl_n_extra,
                             active=live.to(torch.uint8).view(S * W))
        if self._has_seq:
            # window row j, as for the logit processors: its context ends with win[s, :j + 1]
            live = (self._seq_idx < n_win.unsqueeze(1)) & self.active.bool().unsqueeze(1)
            self.seq.ban(self.logits_win.view(S * W, -1)[:, :V], self.out, self.n_out,
                         rows=self._seq_rows,
                         extra=win.unsqueeze(1).expand(S, W, W).reshape(S * W, W),
                         n_extra=self._seq_n_extra, active=live.to(torch.uint8).view(S * W))
        if self._has_grammar:
            # window row j: the slot's state walked over win[s, :j + 1]; a forbidden draft
            # leaves its row and the later ones unmasked, and is rejected by the row before
            live = (self._g_idx < n_win.unsqueeze(1)) & self.active.bool().unsqueeze(1)
            rf.grammar_mask(self.logits_win.view(S * W, -1)[:, :V], self.gtable, self.gstate,
                            rows=self._g_rows,
                            extra=win.unsqueeze(1).expand(S, W, W).reshape(S * W, W),
                            n_extra=self._g_n_extra, active=live.to(torch.uint8).view(S * W))
        temperature, top_k, top_p, seeds = (t.view(S * W) for t in self._win_params)
        # window row i holds the logits at position lens + 1 + i
        cand = rf.sample_logits(self.logits_win.view(S * W, -1)[:, :V], temperature, top_k, top_p,
                                seeds, (lens.unsqueeze(1) + self._win_offs).view(S * W),
                                validate=False)
        if self.logprobs is not None:
            # tok0 goes to output index n_out; window row j holds the logits that decide
            # output index n_out + 1 + j, and cand[s, j] is the token they give. What is
            # written for drafts that are then rejected lies at or beyond the new n_out: a
            # later step overwrites it, and a poll never reads it
            rf.token_logprobs(self.logits, tok0, self.logprobs, out=self._lp_out,
                              rows=self.cache.rows, cols=self.n_out, active=self.active)
            live = (self._win_idx < n_win.unsqueeze(1)) & self.active.bool().unsqueeze(1)
            rf.token_logprobs(self.logits_win.view(S * W, -1)[:, :V], cand, self.logprobs,
                              out=self._lp_out, rows=self._win_rows,
                              cols=(self.n_out.unsqueeze(1) + self._win_offs).view(S * W),
                              active=live.to(torch.uint8).view(S * W))
        rf.spec_accept(win, n_win, cand.view(S, W), self.logits_win, lens, self.n_out,
                       self.max_new, self.active, self.out, self.hist, self.buf, self.n_drafted,
                       self.n_accepted, self.eos)
        if self._has_seq:
            # the first stop sequence completed inside the kept tokens cuts n_out back to its
            # end, also in a slot that spec_accept just retired at a later EOS or at max_new
            self.seq.check(self.out, self.n_out, active=self.active, lens=lens, max_span=W)
        if self._has_grammar:
            rf.grammar_advance(self.gstate, self.gpos, self.out, self.n_out, self.gtable, W)

    def spec_stats(self):
        """``{"drafted": n, "accepted": m}``: the draft tokens the verify passes checked so
        far and the ones that became output, over all requests. One download. With
        ``sequence_rules=True`` these keep counting what the sampler accepted: a draft that was
        accepted and then cut off by a stop sequence still counts as accepted."""
        if not self.speculate:
            return {"drafted": 0, "accepted": 0}
        n, m = torch.stack([self.n_drafted.sum(), self.n_accepted.sum()]).tolist()
        return {"drafted": n, "accepted": m}

    def _run_step(self):
        if self._graph is None:
            with torch.no_grad():
                self._device_step()
        else:
            self._graph.replay()
        self.steps += 1

    # ------------------------------------------------------------------ requests
    def _checked_tokens(self, tokens, what):
        cfg = self.model.cfg
        if isinstance(tokens, torch.Tensor):
            tokens = tokens.tolist()
        tokens = list(tokens)
        if not tokens:
            raise ValueError(f"a {what} needs a non-empty prompt")
        if any(isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < cfg.vocab_size
               for t in tokens):
            raise ValueError(f"tokens must be ints in [0, {cfg.vocab_size})")
        return tokens

    def _checked_adapter(self, adapter):
        """None -> -1 (the base model); else an int in [0, n_adapters) of the engine's stack."""
        if adapter is None:
            return -1
        if self.lora is None:
            raise ValueError("adapter given, but the engine has no adapter stack: lora=")
        if isinstance(adapter, bool) or not isinstance(adapter, int) or \
                not 0 <= adapter < self.lora.n_adapters:
            raise ValueError(f"adapter must be an int in [0, {self.lora.n_adapters}), got "
                             f"{adapter!r}")
        return adapter

    def _ids(self, adapters):
        """The round's adapter ids for a prompt pass (None without a stack)."""
        return None if self.lora is None else adapters.to(torch.int32)

    def _adapter_in_use(self, i):
        return any(r.adapter == i for r in self._queue) or \
            any(r is not None and r.adapter == i for r in self._slot_req) or \
            any(p[2] == i for p in self._prefixes.values())

    def load_adapter(self, i, state, alpha=None):
        """``lora.load(i, state, alpha)`` between steps, IN PLACE: no re-capture. ``ValueError``
        while a queued request, a running request or a registered prefix names ``i``."""
        if self._checked_adapter(i) < 0:
            raise ValueError("load_adapter needs an adapter slot")
        if self._adapter_in_use(i):
            raise ValueError(f"adapter {i} is in use")
        self.lora.load(i, state, alpha)

    def unload_adapter(self, i):
        """``lora.clear(i)`` between steps, IN PLACE; ``ValueError`` while ``i`` is in use."""
        if self._checked_adapter(i) < 0:
            raise ValueError("unload_adapter needs an adapter slot")
        if self._adapter_in_use(i):
            raise ValueError(f"adapter {i} is in use")
        self.lora.clear(i)

    def _need_pool(self, what):
        if not self._has_grammar:
            raise ValueError(f"{what}, but the engine has no grammar pool: grammar_states=")

    @property
    def grammar_free(self):
        """Free rows (automaton states) of the grammar pool."""
        self._need_pool("grammar_free")
        return sum(n for _, n in self._gfree)

    def add_grammar(self, dfa):
        """Writes ``dfa`` (a ``TokenDFA`` over the model's vocabulary that ends with the
        engine's ``eos_token_id``) into the first free range of pool rows that holds its
        states, IN PLACE between steps: no re-capture. Returns the grammar's id for
        ``submit(..., grammar=gid)``. ``ValueError`` for a bad automaton or when no free range
        is long enough; the pool then holds what it held."""
        self._need_pool("add_grammar")
        checked_grammar(dfa, self.model.cfg.vocab_size, self.eos)
        n = dfa.n_states
        for i, (first, rows) in enumerate(self._gfree):
            if rows >= n:
                break
        else:
            raise ValueError(f"the grammar pool is full: no free range of {n} states "
                             f"({self.grammar_free} of {self.gtable.shape[0]} rows are free)")
        table = torch.from_numpy(dfa.table(first))
        self.gtable[first: first + n].copy_(table)
        self._gfree[i: i + 1] = [(first + n, rows - n)] if rows > n else []
        gid = self._next_gid
        self._next_gid += 1
        self._grammars[gid] = (first, n, first + dfa.start, dfa)
        return gid

    def drop_grammar(self, gid):
        """Frees the grammar's rows of the pool. ``ValueError`` for an unknown id, or while a
        queued or running request names it."""
        self._need_pool("drop_grammar")
        if isinstance(gid, bool) or not isinstance(gid, int) or gid not in self._grammars:
            raise ValueError(f"unknown grammar {gid!r}")
        if any(r.grammar == gid for r in self._queue) or \
                any(r is not None and r.grammar == gid for r in self._slot_req):
            raise ValueError(f"grammar {gid} is in use")
        first, n = self._grammars.pop(gid)[:2]
        free = sorted(self._gfree + [(first, n)])
        merged = [free[0]]
        for f, m in free[1:]:
            if merged[-1][0] + merged[-1][1] == f:
                merged[-1] = (merged[-1][0], merged[-1][1] + m)
            else:
                merged.append((f, m))
        self._gfree = merged

    def add_prefix(self, tokens, adapter=None):
        """Prefills ``tokens`` (1 <= len < max_len) once into a row of the prefix store and
        returns the prefix's id for ``submit(..., prefix=pid)``. ``ValueError`` for bad
        tokens or a full store (``prefix_slots`` rows), which then holds what it held.
        ``adapter``: the prefix's K/V are those of that adapter, and only requests with the
        same adapter may name the prefix."""
        tokens = self._checked_tokens(tokens, "prefix")
        adapter = self._checked_adapter(adapter)
        if len(tokens) >= self.max_len:
            raise ValueError(f"prefix ({len(tokens)}) leaves no room in max_len "
                             f"({self.max_len})")
        if not self._prefix_free:
            raise ValueError(f"the prefix store is full ({self.prefix_slots} rows)")
        row = self._prefix_free.pop(0)
        dev = self.device
        self.model.prefill_into(torch.tensor([tokens], dtype=torch.long).to(dev),
                                torch.tensor([len(tokens)], dtype=torch.int32).to(dev),
                                self.prefix_cache,
                                torch.tensor([row], dtype=torch.int32).to(dev),
                                adapters=self._ids(torch.tensor([adapter]).to(dev)))
        pid = self._next_pid
        self._next_pid += 1
        self._prefixes[pid] = (row, tokens, adapter)
        return pid

    def drop_prefix(self, pid):
        """Frees the prefix's row of the store. Requests already admitted keep their copy;
        a request still queued is prefilled whole when its turn comes."""
        if pid not in self._prefixes:
            raise ValueError(f"unknown prefix {pid!r}")
        self._prefix_free.append(self._prefixes.pop(pid)[0])

    def submit(self, tokens, max_new_tokens, temperature=0.0, top_k=None, top_p=None, seed=0,
               prefix=None, adapter=None, logprobs=None, repetition_penalty=None,
               presence_penalty=None, frequency_penalty=None, logit_bias=None,
               min_new_tokens=None, grammar=None, stop=None, bad_words=None,
               no_repeat_ngram_size=None):
        """Queues a request and returns its id; a bad request raises ``ValueError`` and
        queues nothing. ``prefix``: an ``add_prefix`` id; ``tokens`` is then the non-empty
        continuation and the request's prompt is the prefix's tokens followed by it.
        ``adapter``: an int in [0, n_adapters) of the engine's stack (None: the base model,
        or the prefix's adapter when ``prefix`` is given; another adapter than the prefix's
        is an error). ``logprobs``: an int in 0..N on an engine built with ``logprobs=N``:
        the request's events carry the log-probability of every token and the ``logprobs``
        most likely tokens at its position (None: they carry none). ``repetition_penalty``,
        ``presence_penalty``, ``frequency_penalty``, ``logit_bias`` and ``min_new_tokens``: as
        in ``generate``, on an engine built with ``logit_processors=True``. ``grammar``: an
        ``add_grammar`` id on an engine built with ``grammar_states=N``: the output is a word
        of that grammar; not together with ``min_new_tokens > 0`` or a ``-inf``
        ``logit_bias``. ``stop``, ``bad_words`` (lists of token sequences, a bare int counting
        as one token) and ``no_repeat_ngram_size``: as in ``generate``, on an engine built with
        ``sequence_rules=True``; ``stop`` needs the engine's ``eos_token_id``, and a grammar
        goes with ``stop`` only."""
        tokens = self._checked_tokens(tokens, "request")
        if grammar is not None:
            self._need_pool("grammar given")
            if isinstance(grammar, bool) or not isinstance(grammar, int) or \
                    grammar not in self._grammars:
                raise ValueError(f"unknown grammar {grammar!r}")
        controls = {"repetition_penalty": repetition_penalty,
                    "presence_penalty": presence_penalty,
                    "frequency_penalty": frequency_penalty, "logit_bias": logit_bias,
                    "min_new_tokens": min_new_tokens}
        for k, v in controls.items():
            if v is not None and self.ctl is None:
                raise ValueError(f"{k} given, but the engine has no logit processors: "
                                 "logit_processors=True")
        rules = {"stop": stop, "bad_words": bad_words,
                 "no_repeat_ngram_size": no_repeat_ngram_size}
        for k, v in rules.items():
            if v is not None and not self._has_seq:
                raise ValueError(f"{k} given, but the engine has no sequence rules: "
                                 "sequence_rules=True")
        if logprobs is not None:
            if self.logprobs is None:
                raise ValueError("logprobs given, but the engine keeps none: logprobs=")
            if isinstance(logprobs, bool) or not isinstance(logprobs, int) or \
                    not 0 <= logprobs <= self.logprobs:
                raise ValueError(f"logprobs must be an int in 0..{self.logprobs}, got "
                                 f"{logprobs!r}")
        named = adapter is not None
        adapter = self._checked_adapter(adapter)
        if prefix is not None:
            if not isinstance(prefix, int) or prefix not in self._prefixes:
                raise ValueError(f"unknown prefix {prefix!r}")
            if named and adapter != self._prefixes[prefix][2]:
                raise ValueError(f"prefix {prefix} was prefilled with adapter "
                                 f"{self._prefixes[prefix][2]}, the request names {adapter}")
            adapter = self._prefixes[prefix][2]
            tokens = self._prefixes[prefix][1] + tokens
        max_new = int(max_new_tokens)
        if max_new < 1:
            raise ValueError("max_new_tokens must be >= 1")
        if len(tokens) + max_new > self.max_len:
            raise ValueError(f"prompt ({len(tokens)}) + max_new_tokens ({max_new}) exceeds "
                             f"max_len ({self.max_len})")
        temperature = float(temperature)
        if not (math.isfinite(temperature) and temperature >= 0):
            raise ValueError("temperature must be finite and >= 0")
        top_k = 0 if top_k is None else int(top_k)
        top_p = 1.0 if top_p is None else float(top_p)
        if not 0 < top_p <= 1:
            raise ValueError("top_p must be in (0, 1]")
        seed = int(seed)
        if not -2 ** 63 <= seed < 2 ** 64:
            raise ValueError("seed must fit 64 bits")
        if seed >= 2 ** 63:
            seed -= 2 ** 64
        top_k = max(0, min(top_k, 2 ** 31 - 1))
        controls = checked_controls(self.model.cfg.vocab_size, max_new, self.eos, **controls)
        rules = checked_sequences(self.model.cfg.vocab_size, self.eos, **rules)
        if grammar is not None:  # the combinations that could leave a row no token
            checked_grammar(self._grammars[grammar][3], self.model.cfg.vocab_size, self.eos,
                            controls)
            checked_grammar_sequences(self._grammars[grammar][3], rules)
        rid = self._next_rid
        self._next_rid += 1
        self._queue.append(_Request(rid, tokens, max_new, temperature, top_k, top_p, seed,
                                    prefix, adapter, logprobs, controls, grammar, rules))
        return rid

    def cancel(self, rid):
        """Drops a queued or running request (its slot is free for the next admission); no
        event follows for it. Returns whether the request was found."""
        for r in self._queue:
            if r.rid == rid:
                self._queue.remove(r)
                return True
        for s, r in enumerate(self._slot_req):
            if r is not None and r.rid == rid:
                self.active[s] = 0
                self.cache.lens[s] = rf.SLOT_INACTIVE
                self._slot_req[s] = None
                self._fill[s] = None
                return True
        return False

    def has_work(self):
        return bool(self._queue) or self.num_active > 0

    @property
    def num_active(self):
        """Occupied slots: decoding or filling."""
        return sum(r is not None for r in self._slot_req)

    @property
    def num_filling(self):
        return sum(b is not None for b in self._fill)

    @property
    def num_queued(self):
        return len(self._queue)

    # ------------------------------------------------------------------ admission
    def _admit(self):
        free = [s for s, r in enumerate(self._slot_req) if r is None]
        reqs = []
        while self._queue and len(reqs) < len(free):
            reqs.append(self._queue.popleft())
        # an admitted request starts FILLING at base 0, or at its prefix's length with the
        # prefix's K/V copied into the slot: one kv_copy per round, all layers
        copies = []
        for s, r in zip(free, reqs):
            self._slot_req[s] = r
            self._fill[s] = 0
            if r.pid in self._prefixes:  # (dropped meanwhile: the whole prompt is prefilled)
                row, head, _ = self._prefixes[r.pid]
                copies.append([row, s, len(head)])
                self._fill[s] = len(head)
        if copies:
            c = torch.tensor(copies, dtype=torch.int32).to(self.device)
            rf.kv_copy(self.prefix_cache.k, self.prefix_cache.v, self.cache.k, self.cache.v,
                       c[:, 0].contiguous(), c[:, 1].contiguous(), c[:, 2].contiguous())

    def _fill_round(self):
        """One chunk of prompt for every filling slot: the rows at base 0 through one ragged
        ``prefill_into``, the others (prefix continuations, later chunks) through one ragged
        ``extend_into``; the rows whose prompt is complete become active."""
        groups = [[s for s, b in enumerate(self._fill) if b is not None and (b > 0) == ext]
                  for ext in (False, True)]
        for ext, rows in zip((False, True), groups):
            if rows:
                self._fill_rows(rows, ext)

    def _fill_rows(self, rows, ext):
        dev = self.device
        reqs = [self._slot_req[s] for s in rows]
        bases = [self._fill[s] for s in rows]
        lens = [len(r.tokens) - b for r, b in zip(reqs, bases)]
        if self.prefill_chunk is not None:
            lens = [min(n, self.prefill_chunk) for n in lens]
        idx = torch.zeros(len(reqs), max(lens), dtype=torch.long)
        for b, r in enumerate(reqs):
            idx[b, : lens[b]] = torch.tensor(r.tokens[bases[b]: bases[b] + lens[b]],
                                             dtype=torch.long)
        # three uploads per round and path, however many requests it feeds
        ints = torch.tensor([[s, n, r.top_k, r.max_new, r.seed, b, r.adapter,
                              rf.GRAMMAR_NONE if r.grammar is None
                              else self._grammars[r.grammar][2]]
                             for s, n, r, b in zip(rows, lens, reqs, bases)],
                            dtype=torch.int64).to(dev)
        flts = torch.tensor([[r.temperature, r.top_p] for r in reqs],
                            dtype=torch.float32).to(dev)
        sl = ints[:, 0]
        if ext:
            logits = self.model.extend_into(idx.to(dev), ints[:, 1].to(torch.int32), self.cache,
                                            sl.to(torch.int32), ints[:, 5].to(torch.int32),
                                            adapters=self._ids(ints[:, 6]))
        else:
            logits = self.model.prefill_into(idx.to(dev), ints[:, 1].to(torch.int32),
                                             self.cache, sl.to(torch.int32),
                                             adapters=self._ids(ints[:, 6]))
        done = [j for j, r in enumerate(reqs) if bases[j] + lens[j] == len(r.tokens)]
        for j, s in enumerate(rows):
            self._fill[s] = bases[j] + lens[j]
        if len(done) < len(rows):
            # the unfinished rows stay inactive on the device: the model wrote their lens
            pend = torch.tensor([rows[j] for j in range(len(rows)) if j not in done]).to(dev)
            self.cache.lens.index_fill_(0, pend, rf.SLOT_INACTIVE)
            if not done:
                return
            sel = torch.tensor(done).to(dev)
            ints, flts, logits = ints[sel], flts[sel], logits[sel]
            sl = ints[:, 0]
        self.n_out.index_fill_(0, sl, 0)
        if self.ctl is not None:
            # the slots' tables (the whole prompt, the prefix's tokens included), then this
            # round's rows: self.buf only ever holds processed logits
            self.ctl.put(sl, [reqs[j].controls for j in done], [reqs[j].tokens for j in done])
            self.ctl.process(logits, self.out, self.n_out, self.eos, rows=sl.to(torch.int32))
        if self._has_seq:
            # the slots' rules (pos = 0, hit = -1; the prompts too unless the logit processors'
            # copy is shared), then this round's rows: self.buf only ever holds banned logits
            self.seq.put(sl, [reqs[j].rules for j in done], [reqs[j].tokens for j in done])
            self.seq.ban(logits, self.out, self.n_out, rows=sl.to(torch.int32))
        if self._has_grammar:
            # the slots' start states (GRAMMAR_NONE without a grammar), then this round's
            # rows: self.buf only ever holds masked logits
            self.gstate.index_copy_(0, sl, ints[:, 7].to(torch.int32))
            self.gpos.index_fill_(0, sl, 0)
            rf.grammar_mask(logits, self.gtable, self.gstate, rows=sl.to(torch.int32))
        self.logits.index_copy_(0, sl, logits)
        self.top_k.index_copy_(0, sl, ints[:, 2].to(torch.int32))
        self.max_new.index_copy_(0, sl, ints[:, 3].to(torch.int32))
        self.seeds.index_copy_(0, sl, ints[:, 4])
        if self.adapter is not None:
            self.adapter.index_copy_(0, sl, ints[:, 6].to(torch.int32))
        self.temperature.index_copy_(0, sl, flts[:, 0])
        self.top_p.index_copy_(0, sl, flts[:, 1])
        self._seen.index_fill_(0, sl, 0)
        if self.speculate:
            # the whole prompt by position, for the drafter: one more upload per round
            rows_h = torch.zeros(len(done), self.max_len, dtype=torch.int32)
            for i, j in enumerate(done):
                rows_h[i, : len(reqs[j].tokens)] = torch.tensor(reqs[j].tokens,
                                                               dtype=torch.int32)
            self.hist.index_copy_(0, sl, rows_h.to(dev))
            for wide, one in zip(self._win_params,
                                 (self.temperature, self.top_k, self.top_p, self.seeds)):
                wide.copy_(one.unsqueeze(1).expand_as(wide))
        self.active.index_fill_(0, sl, 1)
        for j in done:
            self._fill[rows[j]] = None
            self._seen_host[rows[j]] = 0

    # ------------------------------------------------------------------ poll
    def _poll(self):
        """One download, whatever S: per slot n_out, active and the (at most poll_every, times
        speculate + 1) tokens it produced since the last poll."""
        col = (self._seen.unsqueeze(1) + self._ar).clamp_(max=self.max_len - 1)
        if self.logprobs is not None:
            return self._poll_logprobs(col)
        host = torch.cat([self.n_out.long().unsqueeze(1), self.active.long().unsqueeze(1),
                          self.out.gather(1, col)], 1).tolist()
        self._seen.copy_(self.n_out)
        events = []
        for s, r in enumerate(self._slot_req):
            if r is None or self._fill[s] is not None:  # filling: inactive, not finished
                continue
            n, act = host[s][0], host[s][1]
            new = host[s][2: 2 + n - self._seen_host[s]]
            self._seen_host[s] = n
            if not act:
                self._slot_req[s] = None
            if new or not act:
                events.append((r.rid, new, not act))
        return events

    def _poll_logprobs(self, col):
        """``_poll`` on an engine with logprobs: still one download, a float64 table (it holds
        the token ids and the fp32 values exactly) of n_out, active and K = ``col.shape[1]``
        columns each of tokens and logprobs and K * N each of top ids and top logprobs.
        Events are ``(rid, new_tokens, finished, info)``."""
        S, K, N = self.slots, col.shape[1], self.logprobs
        colN = col.unsqueeze(2).expand(S, K, N)
        f64 = torch.float64
        host = torch.cat([self.n_out.to(f64).unsqueeze(1), self.active.to(f64).unsqueeze(1),
                          self.out.gather(1, col).to(f64), self.lp_hist.gather(1, col).to(f64),
                          self.top_ids_hist.gather(1, colN).to(f64).view(S, K * N),
                          self.top_lp_hist.gather(1, colN).to(f64).view(S, K * N)], 1)
        host = host.cpu().numpy()
        self._seen.copy_(self.n_out)
        head = host[:, :2].astype(np.int64).tolist()
        ids0, lps0 = 2 + 2 * K, 2 + 2 * K + K * N
        events = []
        for s, r in enumerate(self._slot_req):
            if r is None or self._fill[s] is not None:  # filling: inactive, not finished
                continue
            n, act = head[s]
            k = n - self._seen_host[s]
            row = host[s]  # only the k new columns of each block become Python objects
            new = row[2: 2 + k].astype(np.int64).tolist()
            self._seen_host[s] = n
            if not act:
                self._slot_req[s] = None
            if not (new or not act):
                continue
            info = None
            if r.logprobs is not None:
                m = r.logprobs
                info = {"logprobs": row[2 + K: 2 + K + k].tolist(),
                        "top_ids": row[ids0: ids0 + k * N].reshape(k, N)[:, :m]
                        .astype(np.int64).tolist(),
                        "top_logprobs": row[lps0: lps0 + k * N].reshape(k, N)[:, :m].tolist()}
            events.append((r.rid, new, not act, info))
        return events

    def step(self):
        """Admits queued requests into free slots, feeds every filling slot one chunk of its
        prompt (the whole prompt without ``prefill_chunk``), runs ``poll_every`` device steps
        if any slot is decoding and polls: ``[(rid, new_tokens, finished), ...]`` for the
        slots that produced tokens. On an engine built with ``logprobs=N`` the events are
        ``(rid, new_tokens, finished, info)``: ``info`` is None for a request that asked for
        none, else ``{"logprobs": [...], "top_ids": [[...m]], "top_logprobs": [[...m]]}``,
        aligned with ``new_tokens``."""
        self._admit()
        self._fill_round()
        if self.num_active == self.num_filling:
            return []
        for _ in range(self.poll_every):
            self._run_step()
        return self._poll()

    def run(self, logprobs=False):
        """Drives the engine until it is idle: ``{rid: tokens}`` of the requests that
        produced tokens on the way. ``logprobs=True`` (an engine built with ``logprobs=N``):
        ``{rid: (tokens, info)}``, ``info`` as in ``step`` over all the request's tokens."""
        if logprobs and self.logprobs is None:
            raise ValueError("logprobs=True, but the engine keeps none: logprobs=")
        got, infos = {}, {}
        while self.has_work():
            for ev in self.step():
                got.setdefault(ev[0], []).extend(ev[1])
                if logprobs:
                    info = infos.setdefault(ev[0], None if ev[3] is None else
                                            {k: [] for k in ev[3]})
                    if info is not None:
                        for k, v in ev[3].items():
                            info[k].extend(v)
        return {rid: (toks, infos[rid]) for rid, toks in got.items()} if logprobs else got
