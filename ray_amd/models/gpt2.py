"""GPT-2 (small/medium/large/xl) for MI355X, random init.

The headline Ray Train workload (BASELINE.json config 2: TorchTrainer GPT-2-small
DDP bf16). Architecture per Radford et al. 2019 / HF GPT2LMHeadModel (pre-LN,
learned positions, tanh-GELU, tied input/output embedding).

MI355X-first choices:
* bf16 weights/activations end to end (fp32 master lives in the flat optimizer).
* Every GEMM is a plain hipBLASLt GEMM with NO bias; the bias, activation and
  residual are fused into a single HBM pass by our HIP epilogue kernels
  (``bias_gelu``, ``bias_residual``), LayerNorm and the vocab cross-entropy are
  hand-written kernels (ray_amd/ops/csrc).
* Vocab padded 50257 → 50304 (multiple of 64/128) so the LM-head GEMM tiles
  cleanly on MFMA; padded columns are masked inside the fused cross-entropy.
* LM head + cross-entropy fused and chunked over tokens (``lm_head_cross_entropy``):
  the 64x1024x50304 logits tensor (6.6 GB) never exists; each chunk's logits are
  turned into dlogits in place by one register-resident HIP pass.
* Attention: our HIP MFMA causal flash attention (ops/csrc/attn.hip) reading the
  packed QKV GEMM output directly.
* Backward: split-K fp32 weight-gradient GEMMs and every parameter gradient
  (weights, biases, LayerNorm) accumulated in place into the flat DDP gradient
  buffer (no AccumulateGrad adds); the residual stream's two gradients are summed
  inside the LayerNorm backward kernel (``LayerNorm.fork``).
* Generation: ``prefill`` (flash attention over the right-padded prompts, K/V copied into
  a ``KVCache``, LM head on each row's last position only) and ``decode_step`` (one token
  per row through the HIP decode-attention kernel, ops/csrc/attn_decode.hip, with the
  row lengths kept on the device: no host sync, one HIP-graph capture serves every
  position); ``generate`` drives them. With ``seeds=`` the next token comes from the HIP
  sampler (ops/csrc/sample.hip: temperature, top-k, top-p and seed per row, one launch, no
  host sync) and the whole step, sampler included, is one graph replay. ``prefill_into``
  writes a prefill's K/V into device-chosen rows of a wider cache (ops/csrc/kv_slots.hip):
  the admission path of the continuous-batching engine, models/gpt2_engine.py.
  ``extend_into`` continues rows of such a cache with several new tokens each
  (ops/csrc/attn_extend.hip): the engine's shared prompt prefixes and chunked prefill.
  ``verify_step`` runs the same layers over a window of drafted tokens per row and returns
  the logits after every one of them: the engine's speculative decoding.
  Repetition / presence / frequency penalties, logit bias and a minimum length before EOS
  (``generate(..., repetition_penalty=, ...)``) are edits of the logits buffer by
  ``rf.logit_process`` (ops/csrc/logit_proc.hip) before the sampler reads it, on the device
  and inside the captured step.
  Grammar-constrained decoding (``generate(..., grammar=TokenDFA)``, models/grammar.py): each
  row's automaton state lives on the device, ``rf.grammar_advance`` follows the token just
  emitted and ``rf.grammar_mask`` (ops/csrc/grammar.hip) bans what the state does not allow,
  after the logit processors and before the sampler, inside the captured step as well.
  Sequence rules (``generate(..., stop=, bad_words=, no_repeat_ngram_size=)``): ``rf.seq_ban``
  bans the tokens that would complete a banned sequence or repeat an n-gram, between the
  logit processors and the grammar mask, and ``rf.stop_check`` ends a row whose output just
  completed a stop sequence (ops/csrc/seq_rules.hip), inside the captured step too.
  The three inference passes (prompt, extend, decode) run ONE layer loop, ``_layers``, and
  hand it their attention step; the training ``forward`` keeps its own (autograd ops).
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from ray_amd.models.grammar import TokenDFA
from ray_amd.ops import functional as rf
from ray_amd.ops.graph_lock import CapturedStep


@dataclass
class GPT2Config:
    vocab_size: int = 50257
    padded_vocab: int = 50304
    n_positions: int = 1024
    n_embd: int = 768
    n_layer: int = 12
    n_head: int = 12
    layer_norm_eps: float = 1e-5
    init_std: float = 0.02

    @staticmethod
    def small():
        return GPT2Config()

    @staticmethod
    def medium():
        return GPT2Config(n_embd=1024, n_layer=24, n_head=16)

    @staticmethod
    def large():
        return GPT2Config(n_embd=1280, n_layer=36, n_head=20)

    @staticmethod
    def xl():
        return GPT2Config(n_embd=1600, n_layer=48, n_head=25)

    @staticmethod
    def tiny():
        return GPT2Config(vocab_size=512, padded_vocab=512, n_positions=128, n_embd=64,
                          n_layer=2, n_head=4)


class LayerNorm(nn.Module):
    def __init__(self, d, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.bias = nn.Parameter(torch.zeros(d))
        self.eps = eps

    def forward(self, x):
        return rf.layer_norm(x, self.weight, self.bias, self.eps)

    def fork(self, x):
        """(x for the residual add, LN(x)) — the residual grads are summed in the LN bwd."""
        return rf.layer_norm_fork(x, self.weight, self.bias, self.eps)


class Block(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        C = cfg.n_embd
        self.n_head = cfg.n_head
        self.ln_1 = LayerNorm(C, cfg.layer_norm_eps)
        self.c_attn_w = nn.Parameter(torch.empty(3 * C, C))
        self.c_attn_b = nn.Parameter(torch.zeros(3 * C))
        self.c_proj_w = nn.Parameter(torch.empty(C, C))
        self.c_proj_b = nn.Parameter(torch.zeros(C))
        self.ln_2 = LayerNorm(C, cfg.layer_norm_eps)
        self.c_fc_w = nn.Parameter(torch.empty(4 * C, C))
        self.c_fc_b = nn.Parameter(torch.zeros(4 * C))
        self.mlp_proj_w = nn.Parameter(torch.empty(C, 4 * C))
        self.mlp_proj_b = nn.Parameter(torch.zeros(C))

    def attn(self, h):
        """Attention sub-block on the normalised input; returns the projection output
        WITHOUT its bias (added by the fused residual+LayerNorm seam)."""
        B, T, C = h.shape
        qkv = rf.linear(h, self.c_attn_w, self.c_attn_b)  # + bias epilogue
        # HIP MFMA flash attention straight off the packed QKV layout (no permutes/copies)
        y = rf.causal_attention_qkv(qkv.view(B, T, 3, self.n_head, C // self.n_head))
        return rf.linear(y.reshape(B, T, C), self.c_proj_w)

    def mlp(self, h):
        a = rf.bias_gelu(rf.linear(h, self.c_fc_w), self.c_fc_b)
        return rf.linear(a, self.mlp_proj_w)

    def forward(self, x):
        x, h = self.ln_1.fork(x)
        x = rf.bias_residual(self.attn(h), self.c_proj_b, x)
        x, h = self.ln_2.fork(x)
        return rf.bias_residual(self.mlp(h), self.mlp_proj_b, x)


class KVCache:
    """Per-layer K/V of a batch of sequences for ``GPT2.prefill`` / ``decode_step``:
    ``k``, ``v`` [n_layer, B, H, max_len, head_dim] and ``lens`` int32 [B], the positions
    cached per row (kept on the device: the decode kernel reads it there)."""

    def __init__(self, cfg: GPT2Config, batch: int, max_len: int, device=None, dtype=None):
        if max_len < 1 or max_len > cfg.n_positions:
            raise ValueError(f"max_len must be in 1..{cfg.n_positions}, got {max_len}")
        shape = (cfg.n_layer, batch, cfg.n_head, max_len, cfg.n_embd // cfg.n_head)
        self.k = torch.zeros(shape, device=device, dtype=dtype)
        self.v = torch.zeros(shape, device=device, dtype=dtype)
        self.lens = torch.zeros(batch, device=device, dtype=torch.int32)
        self.rows = torch.arange(batch, device=device, dtype=torch.int32)  # verify_step's slots
        self.max_len = max_len


class _GraphedStep:
    """``decode_step`` captured once in a HIP graph (one stream, no parallel branches) with
    static token and logits buffers; ``cache.lens`` lives on the device and is advanced
    inside the graph, so every replay is the step for the next position."""

    def __init__(self, model, cache, tok, adapters=None):
        self.tok = tok.clone()
        self.graph = CapturedStep(
            lambda: model.decode_step(self.tok, cache, adapters=adapters), tok.device)

    def __call__(self, tok):
        self.tok.copy_(tok)
        self.graph.replay()
        return self.graph.result  # the captured call's logits: a static buffer


class _SeededSampler:
    """The device-sampler step of ``generate(seeds=...)``: draws a token per row from the
    static logits buffer with per-row parameters (``rf.sample_logits``: the hash step is
    ``cache.lens[b]``, the position of the token being drawn, EOS latching fused), writes
    it into column ``col`` of ``out`` (``col`` lives on the device) and runs
    ``decode_step`` back into the logits buffer. Nothing in it touches the host, so
    ``capture`` records the whole step in ONE HIP graph (one stream, no parallel branches)
    and a token then costs one replay."""

    def __init__(self, model, cache, logits, out, temperature, top_k, top_p, seeds, eos,
                 adapters=None, logprobs=None, controls=None, grammar=None, rules=None):
        cfg = model.cfg
        dev = out.device
        B = out.shape[0]
        self.model, self.cache, self.out, self.eos = model, cache, out, eos
        self.adapters = adapters
        self.buf = torch.empty(B, cfg.padded_vocab, device=dev, dtype=logits.dtype)
        self.logits = self.buf[:, : cfg.vocab_size]
        self.logits.copy_(logits)
        self.temperature = torch.tensor(temperature, dtype=torch.float32, device=dev)
        self.top_k = torch.tensor(top_k, dtype=torch.int32, device=dev)
        self.top_p = torch.tensor(top_p, dtype=torch.float32, device=dev)
        self.seeds = torch.tensor(seeds, dtype=torch.int64, device=dev)
        self.done = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.col = torch.zeros(1, 1, dtype=torch.long, device=dev)
        # logprobs=n: the tables rf.token_logprobs fills at column ``col`` (None: no such call)
        self.lp = None
        if logprobs is not None:
            self.top_n = logprobs
            self.lp = _logprob_tables(B, out.shape[1], logprobs, dev)
            self.cols = torch.zeros(B, dtype=torch.int32, device=dev)
        # controls=(LogitControls, ...): the logits buffer holds PROCESSED logits whenever the
        # sampler reads it (rf.logit_process on the prefill's here, on decode_step's in _step);
        # n_out counts the tokens in ``out``, advanced where ``col`` is (None: no such call)
        self.ctl = controls
        if controls is not None or grammar is not None or rules is not None:
            self.n_out = torch.zeros(B, dtype=torch.int32, device=dev)
        if controls is not None:
            self.ctl.process(self.logits, self.out, self.n_out, self.eos)
        # rules=SequenceRules: the buffer holds logits with the banned sequences' and repeated
        # n-grams' tokens at -inf whenever the sampler reads it (rf.seq_ban after the logit
        # processors, before the grammar mask), and rf.stop_check latches ``done`` for a row
        # whose output just completed a stop sequence (None: no such call)
        self.rules = rules
        if rules is not None:
            rules.ban(self.logits, self.out, self.n_out)
        # grammar=(table int16 [N, Vt], start states int32 [B]): each row's automaton state and
        # the number of tokens of ``out`` it has consumed; the buffer holds MASKED logits
        # whenever the sampler reads it (None: no such call)
        self.gtable = None
        if grammar is not None:
            self.gtable, start = grammar
            self.gstate = start.clone()
            self.gpos = torch.zeros(B, dtype=torch.int32, device=dev)
            rf.grammar_mask(self.logits, self.gtable, self.gstate)
        self.tok = None  # the sampler's output (inside a capture: the graph's static buffer)
        self.graph = None

    def _draw(self):
        """Samples a token per row and writes it into column ``col`` of ``out``."""
        tok = rf.sample_logits(self.logits, self.temperature, self.top_k, self.top_p,
                               self.seeds, self.cache.lens, done=self.done,
                               eos_token_id=self.eos, validate=False)
        self.out.scatter_(1, self.col.expand(self.out.shape[0], 1), tok.unsqueeze(1))
        if self.lp is not None:
            rf.token_logprobs(self.logits, tok, self.top_n, out=self.lp, rows=self.cache.rows,
                              cols=self.cols)
        return tok

    def _step(self):
        self.tok = self._draw()
        self.col += 1
        if self.lp is not None:
            self.cols += 1
        self.model.decode_step(self.tok, self.cache, out=self.buf, adapters=self.adapters)
        if self.ctl is not None or self.gtable is not None or self.rules is not None:
            self.n_out += 1  # ``out`` already holds the token just drawn
        if self.rules is not None:
            # a stopped row is padded with EOS from here on, as a row that drew EOS is
            self.rules.check(self.out, self.n_out, done=self.done, max_span=1)
        if self.gtable is not None:
            rf.grammar_advance(self.gstate, self.gpos, self.out, self.n_out, self.gtable, 1)
        if self.ctl is not None:
            self.ctl.process(self.logits, self.out, self.n_out, self.eos)
        if self.rules is not None:
            self.rules.ban(self.logits, self.out, self.n_out)
        if self.gtable is not None:
            rf.grammar_mask(self.logits, self.gtable, self.gstate)

    def draw_last(self):
        """The last token of a call needs no ``decode_step`` after it."""
        self._draw()

    def capture(self):
        self.graph = CapturedStep(self._step, self.out.device)

    def __call__(self):
        if self.graph is None:
            self._step()
        else:
            self.graph.replay()


def _logprob_tables(rows, cap, top_n, device):
    """The ``out=`` tables of ``rf.token_logprobs``: ``(lp fp32 [rows, cap], top_ids int32
    [rows, cap, top_n], top_lp fp32 [rows, cap, top_n])``, filled with (NaN, -1, NaN)."""
    return (torch.full((rows, cap), float("nan"), dtype=torch.float32, device=device),
            torch.full((rows, cap, top_n), -1, dtype=torch.int32, device=device),
            torch.full((rows, cap, top_n), float("nan"), dtype=torch.float32, device=device))


def _checked_top_n(name, n):
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= rf.LOGPROB_MAX_TOP:
        raise ValueError(f"{name} must be an int in 0..{rf.LOGPROB_MAX_TOP}, got {n!r}")
    return n


def checked_controls(vocab_size, max_new_tokens, eos_token_id, repetition_penalty=None,
                     presence_penalty=None, frequency_penalty=None, min_new_tokens=None,
                     logit_bias=None):
    """One request's logit-processor controls, checked: ``(repetition, presence, frequency,
    min_new, [(id, value), ...])``, or None when none of them is given. ``ValueError`` for
    a penalty that is not finite and > 0, a presence / frequency that is not finite, a bias
    value that is neither finite nor ``-inf``, more than ``rf.LOGIT_BIAS_MAX`` bias entries,
    an id outside ``[0, vocab_size)``, or ``min_new_tokens`` outside ``0..max_new_tokens``
    (non-zero needs ``eos_token_id``)."""
    if repetition_penalty is None and presence_penalty is None and frequency_penalty is None \
            and min_new_tokens is None and logit_bias is None:
        return None

    def number(name, v, default):
        if v is None:
            return default
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{name} must be a number, got {v!r}")
        return float(v)

    rp = number("repetition_penalty", repetition_penalty, 1.0)
    if not (math.isfinite(rp) and rp > 0):
        raise ValueError("repetition_penalty must be finite and > 0")
    pp = number("presence_penalty", presence_penalty, 0.0)
    fp = number("frequency_penalty", frequency_penalty, 0.0)
    if not (math.isfinite(pp) and math.isfinite(fp)):
        raise ValueError("presence_penalty and frequency_penalty must be finite")
    mn = 0 if min_new_tokens is None else min_new_tokens
    if isinstance(mn, bool) or not isinstance(mn, int) or not 0 <= mn <= max_new_tokens:
        raise ValueError(f"min_new_tokens must be an int in 0..max_new_tokens "
                         f"({max_new_tokens}), got {min_new_tokens!r}")
    if mn and eos_token_id is None:
        raise ValueError("min_new_tokens needs eos_token_id")
    bias = []
    if logit_bias is not None:
        if not isinstance(logit_bias, dict):
            raise ValueError("logit_bias must be a dict {token: value}")
        if len(logit_bias) > rf.LOGIT_BIAS_MAX:
            raise ValueError(f"logit_bias has {len(logit_bias)} entries, at most "
                             f"{rf.LOGIT_BIAS_MAX} fit")
        for t, v in logit_bias.items():
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < vocab_size:
                raise ValueError(f"logit_bias ids must be ints in [0, {vocab_size}), got {t!r}")
            v = number("a logit_bias value", v, float("nan"))
            if not (math.isfinite(v) or v == float("-inf")):
                raise ValueError("logit_bias values must be finite or -inf")
            bias.append((t, v))
    return rp, pp, fp, mn, bias


class LogitControls:
    """The per-row tables of ``rf.logit_process`` for R rows, at fixed addresses: the
    parameters (neutral until ``put``), the bias lists and the prompts int32 [R, width]."""

    def __init__(self, R, width, device):
        i32, f32 = torch.int32, torch.float32
        self.repetition = torch.ones(R, dtype=f32, device=device)
        self.presence = torch.zeros(R, dtype=f32, device=device)
        self.frequency = torch.zeros(R, dtype=f32, device=device)
        self.min_new = torch.zeros(R, dtype=i32, device=device)
        self.bias_ids = torch.zeros(R, rf.LOGIT_BIAS_MAX, dtype=i32, device=device)
        self.bias_vals = torch.zeros(R, rf.LOGIT_BIAS_MAX, dtype=f32, device=device)
        self.n_bias = torch.zeros(R, dtype=i32, device=device)
        self.prompt = torch.zeros(R, width, dtype=i32, device=device)
        self.prompt_len = torch.zeros(R, dtype=i32, device=device)

    def put(self, rows, controls, prompts):
        """Writes rows ``rows`` (int64 [n] on the device): ``controls[i]`` a
        ``checked_controls`` result (None: neutral), ``prompts[i]`` the row's prompt tokens.
        Two uploads, however many rows."""
        n, NB = len(controls), rf.LOGIT_BIAS_MAX
        flt = torch.zeros(n, 3 + NB, dtype=torch.float32)
        ints = torch.zeros(n, 3 + NB + self.prompt.shape[1], dtype=torch.int32)
        for i, (c, p) in enumerate(zip(controls, prompts)):
            rp, pp, fp, mn, bias = c if c is not None else (1.0, 0.0, 0.0, 0, [])
            flt[i, :3] = torch.tensor([rp, pp, fp])
            ints[i, 0], ints[i, 1], ints[i, 2] = mn, len(bias), len(p)
            if bias:
                ints[i, 3: 3 + len(bias)] = torch.tensor([t for t, _ in bias], dtype=torch.int32)
                flt[i, 3: 3 + len(bias)] = torch.tensor([v for _, v in bias])
            ints[i, 3 + NB: 3 + NB + len(p)] = torch.as_tensor(p, dtype=torch.int32)
        flt, ints = flt.to(rows.device), ints.to(rows.device)
        for dst, src in ((self.repetition, flt[:, 0]), (self.presence, flt[:, 1]),
                         (self.frequency, flt[:, 2]), (self.bias_vals, flt[:, 3:]),
                         (self.min_new, ints[:, 0]), (self.n_bias, ints[:, 1]),
                         (self.prompt_len, ints[:, 2]), (self.bias_ids, ints[:, 3: 3 + NB]),
                         (self.prompt, ints[:, 3 + NB:])):
            dst.index_copy_(0, rows, src)

    def process(self, logits, out, n_out, eos, **kw):
        """``rf.logit_process`` on ``logits`` with these tables."""
        return rf.logit_process(logits, self.prompt, self.prompt_len, out, n_out,
                                self.repetition, self.presence, self.frequency, self.min_new,
                                self.bias_ids, self.bias_vals, self.n_bias, eos_token_id=eos,
                                **kw)


def checked_grammar(dfa, vocab_size, eos_token_id, controls=None):
    """One request's grammar, checked against the model and the request's ``checked_controls``
    result: ``ValueError`` for anything but a ``TokenDFA`` over this vocabulary that ends
    with this EOS, and for the two controls that can leave a row with no allowed token
    (``min_new_tokens > 0`` bans EOS, a ``-inf`` ``logit_bias`` bans a token), which the
    sampler declares out of contract."""
    if not isinstance(dfa, TokenDFA):
        raise ValueError(f"grammar must be a TokenDFA, got {type(dfa).__name__}")
    if eos_token_id is None:
        raise ValueError("grammar needs eos_token_id")
    if dfa.vocab_size != vocab_size or dfa.eos_token_id != int(eos_token_id):
        raise ValueError(f"grammar is over {dfa.vocab_size} tokens with EOS "
                         f"{dfa.eos_token_id}, the request over {vocab_size} with EOS "
                         f"{eos_token_id}")
    if controls is not None:
        if controls[3] > 0:
            raise ValueError("grammar and min_new_tokens > 0 cannot go together: the grammar "
                             "decides where EOS is allowed")
        if any(v == float("-inf") for _, v in controls[4]):
            raise ValueError("grammar and a -inf logit_bias cannot go together: no allowed "
                             "token might be left")
    return dfa


def checked_sequences(vocab_size, eos_token_id, stop=None, bad_words=None,
                      no_repeat_ngram_size=None):
    """One request's sequence rules, checked: ``(stops, bads, n)``, two lists of token lists
    and the no-repeat n-gram size (0: off), or None when none of the three is given. A bare
    int in ``stop`` or ``bad_words`` counts as a one-token sequence. ``ValueError`` for more
    than ``rf.SEQ_MAX`` sequences of one kind, an empty sequence or one longer than
    ``rf.SEQ_MAX_LEN``, an id outside ``[0, vocab_size)``, ``no_repeat_ngram_size`` outside
    ``0..rf.SEQ_MAX_LEN``, a bool or a non-int where an int belongs, and ``stop`` without
    ``eos_token_id`` (a stopped row of ``generate`` is padded with it)."""
    if stop is None and bad_words is None and no_repeat_ngram_size is None:
        return None

    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)

    def sequences(name, value):
        if value is None:
            return []
        if not isinstance(value, (list, tuple)):
            raise ValueError(f"{name} must be a list of token sequences, got {value!r}")
        if len(value) > rf.SEQ_MAX:
            raise ValueError(f"{name} has {len(value)} sequences, at most {rf.SEQ_MAX} fit")
        res = []
        for seq in value:
            seq = [seq] if is_int(seq) else seq
            if not isinstance(seq, (list, tuple)) or not 1 <= len(seq) <= rf.SEQ_MAX_LEN:
                raise ValueError(f"a {name} sequence must hold 1..{rf.SEQ_MAX_LEN} tokens, got "
                                 f"{seq!r}")
            if any(not is_int(t) or not 0 <= t < vocab_size for t in seq):
                raise ValueError(f"{name} ids must be ints in [0, {vocab_size}), got {seq!r}")
            res.append(list(seq))
        return res

    stops, bads = sequences("stop", stop), sequences("bad_words", bad_words)
    if stops and eos_token_id is None:
        raise ValueError("stop needs eos_token_id")
    n = 0 if no_repeat_ngram_size is None else no_repeat_ngram_size
    if not is_int(n) or not 0 <= n <= rf.SEQ_MAX_LEN:
        raise ValueError(f"no_repeat_ngram_size must be an int in 0..{rf.SEQ_MAX_LEN}, got "
                         f"{no_repeat_ngram_size!r}")
    return stops, bads, n


def checked_grammar_sequences(dfa, rules):
    """The check beside ``checked_grammar`` for a request with a grammar and a
    ``checked_sequences`` result: ``ValueError`` for ``bad_words`` or ``no_repeat_ngram_size >
    0``, either of which could leave a row with no allowed token. ``stop`` goes with a grammar:
    the output is then a prefix of a word, as at ``max_new_tokens``."""
    if dfa is None or rules is None:
        return
    if rules[1]:
        raise ValueError("grammar and bad_words cannot go together: no allowed token might be "
                         "left")
    if rules[2] > 0:
        raise ValueError("grammar and no_repeat_ngram_size > 0 cannot go together: no allowed "
                         "token might be left")


class SequenceRules:
    """The per-row tables of ``rf.seq_ban`` and ``rf.stop_check`` for R rows, at fixed
    addresses: ``stops`` / ``bad`` int32 [R, SEQ_MAX, SEQ_MAX_LEN] with ``stop_len`` /
    ``bad_len`` int32 [R, SEQ_MAX], ``ngram`` int32 [R] (all unused until ``put``), ``pos``
    int32 [R] (the output tokens ``check`` has looked at) and ``hit`` int32 [R] (the stop
    sequence that ended the row, -1: none), and the prompts int32 [R, width]. ``controls``: a
    ``LogitControls`` of the same R and width whose prompt table is then shared, one copy:
    its ``put`` writes the prompts, this one's does not."""

    def __init__(self, R, width, device, controls=None):
        i32, Q, ML = torch.int32, rf.SEQ_MAX, rf.SEQ_MAX_LEN
        self.stops = torch.zeros(R, Q, ML, dtype=i32, device=device)
        self.stop_len = torch.zeros(R, Q, dtype=i32, device=device)
        self.bad = torch.zeros(R, Q, ML, dtype=i32, device=device)
        self.bad_len = torch.zeros(R, Q, dtype=i32, device=device)
        self.ngram = torch.zeros(R, dtype=i32, device=device)
        self.pos = torch.zeros(R, dtype=i32, device=device)
        self.hit = torch.full((R,), -1, dtype=i32, device=device)
        self.shared = controls is not None
        if self.shared:
            if controls.prompt.shape != (R, width):
                raise ValueError("the shared prompt table has another shape")
            self.prompt, self.prompt_len = controls.prompt, controls.prompt_len
        else:
            self.prompt = torch.zeros(R, width, dtype=i32, device=device)
            self.prompt_len = torch.zeros(R, dtype=i32, device=device)

    def put(self, rows, rules, prompts):
        """Writes rows ``rows`` (int64 [n] on the device): ``rules[i]`` a ``checked_sequences``
        result (None: no rule), ``prompts[i]`` the row's prompt tokens; ``pos`` becomes 0 and
        ``hit`` -1. One upload, however many rows."""
        n, Q, ML = len(rules), rf.SEQ_MAX, rf.SEQ_MAX_LEN
        width = 0 if self.shared else self.prompt.shape[1]
        o_len, o_seq, o_p = 2, 2 + 2 * Q, 2 + 2 * Q + 2 * Q * ML
        ints = torch.zeros(n, o_p + width, dtype=torch.int32)
        for i, (r, p) in enumerate(zip(rules, prompts)):
            stops, bads, ng = r if r is not None else ([], [], 0)
            ints[i, 0], ints[i, 1] = ng, len(p)
            for k, seqs in enumerate((stops, bads)):
                for q, seq in enumerate(seqs):
                    ints[i, o_len + k * Q + q] = len(seq)
                    at = o_seq + (k * Q + q) * ML
                    ints[i, at: at + len(seq)] = torch.tensor(seq, dtype=torch.int32)
            if width:
                ints[i, o_p: o_p + len(p)] = torch.as_tensor(p, dtype=torch.int32)
        ints = ints.to(rows.device)
        seqs = ints[:, o_seq: o_p].view(n, 2, Q, ML)
        for dst, src in ((self.ngram, ints[:, 0]), (self.stop_len, ints[:, o_len: o_len + Q]),
                         (self.bad_len, ints[:, o_len + Q: o_seq]), (self.stops, seqs[:, 0]),
                         (self.bad, seqs[:, 1])):
            dst.index_copy_(0, rows, src)
        if width:
            self.prompt_len.index_copy_(0, rows, ints[:, 1])
            self.prompt.index_copy_(0, rows, ints[:, o_p:])
        self.pos.index_fill_(0, rows, 0)
        self.hit.index_fill_(0, rows, -1)

    def ban(self, logits, out, n_out, **kw):
        """``rf.seq_ban`` on ``logits`` with these tables."""
        return rf.seq_ban(logits, self.prompt, self.prompt_len, out, n_out, self.bad,
                          self.bad_len, self.ngram, **kw)

    def check(self, out, n_out, **kw):
        """``rf.stop_check`` on ``out`` / ``n_out`` with these tables."""
        return rf.stop_check(out, n_out, self.pos, self.stops, self.stop_len, self.hit, **kw)


def _per_row_sequences(name, value, B):
    """``generate``'s ``stop`` / ``bad_words`` as a list of B values. One value for all rows
    is a list of sequences (token lists or bare ints); the per-row form is a list of B entries,
    each None or such a list, recognised by an entry that is None or that holds a list."""
    if value is None:
        return [None] * B
    if isinstance(value, (list, tuple)) and any(
            v is None or (isinstance(v, (list, tuple)) and
                          any(isinstance(t, (list, tuple)) for t in v)) for v in value):
        if len(value) != B:
            raise ValueError(f"{name} has {len(value)} entries for {B} rows")
        return list(value)
    return [value] * B


def grammar_table(dfas):
    """One device table for several automata: ``(int16 numpy [N, Vt], [first row of each])``,
    every automaton's states shifted to its rows."""
    import numpy as np

    offs, n = [], 0
    for d in dfas:
        offs.append(n)
        n += d.n_states
    return np.concatenate([d.table(o) for d, o in zip(dfas, offs)]), offs


def _per_row(name, value, default, B, cast):
    """``value`` (None, a scalar or a per-row sequence) as a list of B ``cast`` values."""
    if value is None:
        value = default
    if isinstance(value, torch.Tensor):
        value = value.tolist()
    if isinstance(value, (list, tuple)):
        if len(value) != B:
            raise ValueError(f"{name} has {len(value)} entries for {B} rows")
        return [cast(default if v is None else v) for v in value]
    return [cast(value)] * B


class GPT2(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.cfg = cfg
        self.wte = nn.Parameter(torch.empty(cfg.padded_vocab, cfg.n_embd))
        self.wpe = nn.Parameter(torch.empty(cfg.n_positions, cfg.n_embd))
        self.h = nn.ModuleList([Block(cfg) for _ in range(cfg.n_layer)])
        self.ln_f = LayerNorm(cfg.n_embd, cfg.layer_norm_eps)
        self.lm_head_chunk = 8192  # tokens per fused LM-head/CE chunk
        self.lora = None  # a models.lora.LoRAStack: attach_lora
        self.reset_parameters()

    def reset_parameters(self):
        std = self.cfg.init_std
        proj_std = std / math.sqrt(2 * self.cfg.n_layer)
        with torch.no_grad():
            nn.init.normal_(self.wte, 0, std)
            self.wte[self.cfg.vocab_size:].zero_()
            nn.init.normal_(self.wpe, 0, 0.01)
            for b in self.h:
                nn.init.normal_(b.c_attn_w, 0, std)
                nn.init.normal_(b.c_fc_w, 0, std)
                nn.init.normal_(b.c_proj_w, 0, proj_std)
                nn.init.normal_(b.mlp_proj_w, 0, proj_std)

    def num_params(self, non_embedding=True):
        n = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n -= self.wpe.numel()
        return n

    def forward(self, idx, targets=None):
        B, T = idx.shape
        x = rf.embedding(idx, self.wte, self.wpe)
        # Pre-LN seams fused: every "x += sub_block(h) + bias; h = LN(x)" is ONE kernel
        # forward and ONE kernel backward (residual grads, LN grads and the projection-bias
        # grad together) — see ops.functional.residual_layer_norm.
        x, h = self.h[0].ln_1.fork(x)
        for i, blk in enumerate(self.h):
            x, h = rf.residual_layer_norm(blk.attn(h), blk.c_proj_b, x, blk.ln_2.weight,
                                          blk.ln_2.bias, blk.ln_2.eps)
            nxt = self.h[i + 1].ln_1 if i + 1 < len(self.h) else self.ln_f
            x, h = rf.residual_layer_norm(blk.mlp(h), blk.mlp_proj_b, x, nxt.weight, nxt.bias,
                                          nxt.eps)
        if targets is None:
            logits = F.linear(h, self.wte)  # tied LM head on ln_f(x), [B, T, padded_vocab]
            return logits[..., : self.cfg.vocab_size]
        # tied LM head + CE fused and chunked over tokens (never the full logits); the
        # embedding backward, which runs last, signals wte's DDP readiness
        return rf.lm_head_cross_entropy(h, self.wte, targets, self.cfg.vocab_size,
                                        chunk=self.lm_head_chunk, signal_w=False)

    # ------------------------------------------------------------------ generation
    def attach_lora(self, stack):
        """Attaches a ``models.lora.LoRAStack`` (``None`` detaches it): the inference passes
        then take ``adapters``, an int32 [B] tensor on the model's device with one adapter id
        per row, -1 for the base model, and add each row's adapter after the four linears
        of every layer (``rf.lora_add``). Without ``adapters`` they run as before. The
        training ``forward`` never sees the stack."""
        if stack is not None:
            cfg, sc = self.cfg, stack.cfg
            if (sc.n_layer, sc.n_embd) != (cfg.n_layer, cfg.n_embd):
                raise ValueError("the adapter stack was built for another model size")
            if stack.device != self.wte.device or stack.dtype != self.wte.dtype:
                raise ValueError(f"the adapter stack is {stack.dtype} on {stack.device}, the "
                                 f"model {self.wte.dtype} on {self.wte.device}")
        self.lora = stack

    def _adapter_ids(self, adapters, B):
        if adapters is None:
            return None
        if self.lora is None:
            raise ValueError("adapters given, but no adapter stack is attached: attach_lora")
        if not isinstance(adapters, torch.Tensor) or adapters.dtype != torch.int32 or \
                adapters.shape != (B,) or adapters.device != self.wte.device:
            raise ValueError(f"adapters must be an int32 tensor of shape [{B}] on "
                             f"{self.wte.device}")
        return adapters

    def _flash_ok(self, x) -> bool:
        return x.is_cuda and x.dtype == torch.bfloat16 and \
            self.cfg.n_embd // self.cfg.n_head == 64

    @torch.no_grad()
    def prefill(self, idx, lens, cache: KVCache, adapters=None):
        """Runs the right-padded prompts ``idx`` [B, T] (true lengths ``lens`` [B], >= 1)
        through the model, stores every layer's K/V in ``cache`` and returns the logits of
        each row's last real token, [B, vocab_size]. Causal attention keeps the padding
        out of the real positions; the padded positions' K/V are leftovers that the decode
        kernel masks out and overwrites."""
        B, T = idx.shape
        if B != cache.k.shape[1]:
            raise ValueError(f"cache holds {cache.k.shape[1]} rows, prompts have {B}")
        lens = torch.as_tensor(lens, device=idx.device).to(torch.int32)
        n = min(T, cache.max_len)

        def store(i, qkv):
            cache.k[i, :, :, :n].copy_(qkv[:, :n, 1].transpose(1, 2))
            cache.v[i, :, :, :n].copy_(qkv[:, :n, 2].transpose(1, 2))

        logits = self._prefill(idx, lens, store, adapters)
        cache.lens = lens.clone()
        return logits

    @torch.no_grad()
    def prefill_into(self, idx, lens, cache: KVCache, slots, adapters=None):
        """``prefill`` into rows of a cache that is wider than the prompts' batch: row b of
        ``idx`` [Bn, T] (true lengths ``lens`` [Bn], >= 1) goes to row ``slots[b]`` of
        ``cache`` (``slots`` int32 [Bn] on the device, distinct), through ``rf.kv_insert``:
        only positions below ``lens[b]`` of the named rows are written, the other rows and
        the padding keep their bytes. Writes ``cache.lens`` IN PLACE at ``slots`` (a
        captured step holds its address) and returns the logits of each row's last real
        token, [Bn, vocab_size]."""
        if not isinstance(slots, torch.Tensor) or slots.dtype != torch.int32 or \
                slots.shape != (idx.shape[0],) or slots.device != idx.device:
            raise ValueError(f"slots must be an int32 tensor of shape [{idx.shape[0]}] on "
                             f"{idx.device}")
        lens = torch.as_tensor(lens, device=idx.device).to(torch.int32)
        logits = self._prefill(
            idx, lens, lambda i, qkv: rf.kv_insert(qkv, cache.k[i], cache.v[i], slots, lens),
            adapters)
        # kv_insert skips a slot id outside the cache
        self._scatter_lens(cache, slots, (slots >= 0) & (slots < cache.lens.shape[0]), lens)
        return logits

    @torch.no_grad()
    def extend_into(self, idx, n_new, cache: KVCache, slots, base, adapters=None):
        """Continues sequences that already sit in ``cache``: row b of ``idx`` [Bn, Tn]
        (right-padded, true counts ``n_new`` [Bn], >= 1) holds the tokens at positions
        ``base[b] .. base[b] + n_new[b] - 1`` of the sequence in row ``slots[b]``, whose first
        ``base[b]`` positions are cached (``slots`` and ``base`` int32 [Bn] on the device,
        ``slots`` distinct). Every layer goes through ``rf.attn_extend`` (the new K/V are
        appended to the row, the new queries attend over the cached positions and, causally,
        over each other), any Tn, no padding to a multiple of 128. ``base`` is the caller's
        to keep: it is NOT read from ``cache.lens`` (the engine's device step pins the
        ``lens`` of every slot that is not decoding). Writes ``cache.lens[slots] = base +
        n_new`` IN PLACE for the rows ``rf.attn_extend`` treats as active and returns the
        logits of each row's last real token, [Bn, vocab_size]. No host synchronisation."""
        Bn, Tn = idx.shape
        for name, t in (("slots", slots), ("base", base)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or \
                    t.shape != (Bn,) or t.device != idx.device:
                raise ValueError(f"{name} must be an int32 tensor of shape [{Bn}] on "
                                 f"{idx.device}")
        if Bn < 1 or Tn < 1:
            raise ValueError("extend_into needs at least one token in every row")
        n_new = torch.as_tensor(n_new, device=idx.device).to(torch.int32)
        logits = self._last_logits(self._extend(idx, n_new, cache, slots, base, adapters),
                                   n_new)
        # the rows that attn_extend skips
        sl, bl, nl = slots.long(), base.long(), n_new.long()
        ok = (sl >= 0) & (sl < cache.lens.shape[0]) & (bl >= 0) & (nl >= 1) & (nl <= Tn) & \
            (bl + nl <= cache.k.shape[3])
        self._scatter_lens(cache, sl, ok, (bl + nl).to(torch.int32))
        return logits

    def _extend(self, idx, n_new, cache, slots, base, adapters=None):
        """The layers of ``extend_into`` / ``verify_step``: the tokens ``idx`` [Bn, Tn] at
        positions ``base[b] + i`` through ``rf.attn_extend`` over rows ``slots`` of ``cache``;
        returns ``ln_f`` of the result, [Bn, Tn, C]. Leaves ``cache.lens`` alone."""
        cfg = self.cfg
        Bn, Tn = idx.shape
        H, hd = cfg.n_head, cfg.n_embd // cfg.n_head
        # the padding's positions are clamped into the table; its outputs are dropped
        pos = (base.long().view(Bn, 1) + torch.arange(Tn, device=idx.device)).clamp(
            0, cfg.n_positions - 1)

        def attend(i, qkv):
            y = rf.attn_extend(qkv.view(Bn, Tn, 3, H, hd), cache.k[i], cache.v[i], slots, base,
                               n_new)
            return y.reshape(Bn, Tn, cfg.n_embd)

        return self._layers(self.wte[idx] + self.wpe[pos], attend, adapters)

    @torch.no_grad()
    def verify_step(self, win, n_win, cache: KVCache, out=None, adapters=None):
        """The verify pass of a speculative decode step: row s of ``win`` [S, W] (int64) holds
        ``n_win[s]`` tokens (int32 [S] on the device; the rest is padding) at positions
        ``cache.lens[s] + i`` of the sequence in row s of ``cache`` (S rows). Every layer
        goes through ``rf.attn_extend`` with ``slots = arange(S)``, ``base = cache.lens`` and
        ``n_new = n_win``: the window's K/V are appended to the row and token i attends over
        the cached positions and the window up to itself. ALL W positions meet the tied LM
        head: returns [S, W, vocab_size], where ``[s, i]`` are the logits after ``win[s, i]``
        (a view of ``out`` [S, W, padded_vocab] when given). ``cache.lens`` is NOT written:
        whoever decides how much of the window stands advances it (``rf.spec_accept``). A row
        with ``n_win[s] = 0`` or an inactive ``cache.lens[s]`` writes nothing to the cache,
        and its logits mean nothing. No host read: capturable."""
        cfg = self.cfg
        S = cache.lens.shape[0]
        if win.dim() != 2 or win.shape[0] != S or win.shape[1] < 1 or win.dtype != torch.int64:
            raise ValueError(f"win must be an int64 tensor [{S}, W], the cache's rows")
        W = win.shape[1]
        if not isinstance(n_win, torch.Tensor) or n_win.dtype != torch.int32 or \
                n_win.shape != (S,) or n_win.device != win.device:
            raise ValueError(f"n_win must be an int32 tensor of shape [{S}] on {win.device}")
        # (a drafter's token is clamped into the table: memory safety is not its contract)
        h = self._extend(win.clamp(0, cfg.vocab_size - 1), n_win, cache, cache.rows, cache.lens,
                         adapters)
        if out is None:
            return F.linear(h, self.wte)[..., : cfg.vocab_size]
        if out.shape != (S, W, cfg.padded_vocab) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous [{S}, {W}, {cfg.padded_vocab}] tensor")
        torch.mm(h.reshape(S * W, cfg.n_embd), self.wte.t(), out=out.view(S * W, -1))
        return out[..., : cfg.vocab_size]

    @staticmethod
    def _scatter_lens(cache, slots, ok, new_lens):
        """``cache.lens[slots[b]] = new_lens[b]`` for the rows with ``ok[b]``, IN PLACE (a
        captured step holds that address); the other rows land in a spare entry."""
        S = cache.lens.shape[0]
        sl = torch.where(ok, slots.long(), S)
        cache.lens.copy_(torch.cat([cache.lens, cache.lens.new_zeros(1)])
                         .scatter_(0, sl, new_lens)[:S])

    def _layers(self, x, attend, adapters=None):
        """The transformer layers of the inference paths on the embedded input ``x``
        [B, ..., C]; returns ``ln_f`` of the result. ``attend(i, qkv)`` takes layer i's c_attn
        output [..., 3C] and returns the attention output [..., C], the input of c_proj.
        ``adapters`` (int32 [B], -1: none): each row's adapter of the attached stack is added
        to the output of the four linears, before the bias where a later kernel adds it."""
        adapters = self._adapter_ids(adapters, x.shape[0])
        if adapters is None:
            def linear(i, target, inp, w, b=None):
                return F.linear(inp, w, b)
        else:
            st = self.lora

            def linear(i, target, inp, w, b=None):
                y = F.linear(inp, w, b)
                rf.lora_add(y, inp, st.a[target][i], st.b[target][i], st.scale, adapters)
                return y

        x, h = self.h[0].ln_1.fork(x)
        for i, blk in enumerate(self.h):
            qkv = linear(i, "c_attn", h, blk.c_attn_w, blk.c_attn_b)
            a = linear(i, "c_proj", attend(i, qkv), blk.c_proj_w)
            x, h = rf.residual_layer_norm(a, blk.c_proj_b, x, blk.ln_2.weight, blk.ln_2.bias,
                                          blk.ln_2.eps)
            nxt = self.h[i + 1].ln_1 if i + 1 < len(self.h) else self.ln_f
            u = rf.bias_gelu(linear(i, "c_fc", h, blk.c_fc_w), blk.c_fc_b)
            m = linear(i, "mlp_proj", u, blk.mlp_proj_w)
            x, h = rf.residual_layer_norm(m, blk.mlp_proj_b, x, nxt.weight, nxt.bias, nxt.eps)
        return h

    def _last_logits(self, h, n):
        """Only the last real position ``n[b] - 1`` of each row of ``h`` [B, T, C] meets the
        tied LM head, [B, C] x [C, V]: returns [B, vocab_size]."""
        B, T = h.shape[:2]
        last = (n.long() - 1).clamp(0, T - 1)
        hl = h[torch.arange(B, device=h.device), last]
        return F.linear(hl, self.wte)[:, : self.cfg.vocab_size]

    def _prefill(self, idx, lens, store, adapters=None):
        """The prompt pass of ``prefill`` / ``prefill_into``: ``store(i, qkv)`` takes layer
        i's packed c_attn output [B, Tp, 3, H, hd] (Tp >= T: the padded width)."""
        return self._last_logits(self._prompt_pass(idx, store, adapters), lens)

    def _prompt_pass(self, idx, store, adapters=None):
        """``idx`` [B, T] through the layers with causal (flash) attention: ``ln_f`` of the
        result, [B, Tp, C]. ``store`` as in ``_prefill`` (None: nothing is kept)."""
        cfg = self.cfg
        B, T = idx.shape
        H, hd = cfg.n_head, cfg.n_embd // cfg.n_head
        Tp = T
        if self._flash_ok(self.wte) and T % 128 and -(-T // 128) * 128 <= cfg.n_positions:
            # the MFMA flash kernel wants T % 128 == 0; more right padding is as harmless
            Tp = -(-T // 128) * 128
            idx = F.pad(idx, (0, Tp - T))

        def attend(i, qkv):
            qkv = qkv.view(B, Tp, 3, H, hd)
            if store is not None:
                store(i, qkv)
            return rf.causal_attention_qkv(qkv).reshape(B, Tp, cfg.n_embd)

        return self._layers(rf.embedding(idx, self.wte, self.wpe), attend, adapters)

    @torch.no_grad()
    def decode_step(self, tok, cache: KVCache, out=None, adapters=None):
        """One token per row: ``tok`` [B] is the token at position ``cache.lens[b]``;
        appends its K/V to the cache, returns the next-token logits [B, vocab_size] and
        advances ``cache.lens``. No host synchronisation: capturable in a HIP graph, and
        one capture serves every position. ``out`` [B, padded_vocab]: the LM head writes
        there and the result is a view of it (a graph whose next replay reads the logits
        needs them at a fixed address)."""
        cfg = self.cfg
        B = tok.shape[0]
        H, hd = cfg.n_head, cfg.n_embd // cfg.n_head
        pos = cache.lens.long().clamp(0, cfg.n_positions - 1)

        def attend(i, qkv):
            y = rf.attn_decode(qkv.view(B, 3, H, hd), cache.k[i], cache.v[i], cache.lens)
            return y.view(B, cfg.n_embd)

        h = self._layers(self.wte[tok] + self.wpe[pos], attend, adapters)
        if out is None:
            logits = F.linear(h, self.wte)[:, : cfg.vocab_size]
        else:
            logits = torch.mm(h, self.wte.t(), out=out)[:, : cfg.vocab_size]
        cache.lens += 1
        return logits

    @staticmethod
    def _pick(logits, temperature, top_k, generator):
        if temperature == 0.0:
            return logits.argmax(-1)
        lg = logits.float() / temperature
        if top_k is not None:
            kth = lg.topk(min(int(top_k), lg.shape[-1]), -1).values[:, -1:]
            lg = lg.masked_fill(lg < kth, float("-inf"))
        return torch.multinomial(torch.softmax(lg, -1), 1, generator=generator).squeeze(1)

    @torch.no_grad()
    def generate(self, idx, max_new_tokens, *, lens=None, temperature=0.0, top_k=None,
                 top_p=None, seeds=None, eos_token_id=None, generator=None, graph=False,
                 adapters=None, logprobs=None, repetition_penalty=None, presence_penalty=None,
                 frequency_penalty=None, min_new_tokens=None, logit_bias=None, grammar=None,
                 stop=None, bad_words=None, no_repeat_ngram_size=None):
        """Autoregressive generation with a KV cache: ``idx`` [B, T] prompts, right-padded
        to a common length with true lengths ``lens`` (default: all T). Returns the new
        tokens [B, max_new_tokens] (int64). ``temperature`` 0 is greedy, otherwise samples
        softmax(logits / temperature) over the ``top_k`` largest with ``generator``. A row
        that emits ``eos_token_id`` keeps emitting it. ``graph=True`` (GPU) captures one
        ``decode_step`` in a HIP graph and replays it per token; sampling stays outside,
        so the tokens are those of the eager loop.

        ``seeds`` (an int, or one per row) selects the device sampler
        (``rf.sample_logits``): ``temperature``, ``top_k`` and ``top_p`` may then be scalars
        or per-row sequences (0 / None / None switch a rule off), and the randomness of a
        token is a hash of the row's seed and the token's position, so a row's tokens
        depend on its prompt, its parameters and its seed only, never on its batch-mates.
        With ``graph=True`` the sampler, the EOS latch and the write into the result are
        captured with ``decode_step``: a token costs one graph replay and nothing else.

        ``adapters`` (an int, or one per row; -1 or None: the base model) names each row's
        adapter of the attached ``LoRAStack`` (``attach_lora``); the prompt pass and every
        step apply it, inside the captured graph too.

        ``logprobs=n`` (0..``rf.LOGPROB_MAX_TOP``; None, the default: the call as above):
        returns ``(tokens, lp fp32 [B, max_new_tokens], top_ids int32 [B, max_new_tokens, n],
        top_lp fp32 [B, max_new_tokens, n])``: the log-probability of every emitted token
        under the logits it was drawn from and the n most likely tokens there with theirs
        (``rf.token_logprobs``; the model's own distribution, whatever the sampling
        parameters). On every path; with ``seeds=`` and ``graph=True`` the call is captured
        with the step and a token still costs one replay.

        Logit processors (each a scalar or a per-row sequence, ``logit_bias`` a dict
        ``{token: value}`` or one per row; they need ``seeds=``): ``repetition_penalty`` (> 0;
        a token of the prompt or the output so far has its logit divided by it when
        positive, multiplied otherwise), ``presence_penalty`` and ``frequency_penalty``
        (subtracted once, and once per occurrence, for a token of the output so far),
        ``logit_bias`` (added; ``-inf`` bans a token; at most ``rf.LOGIT_BIAS_MAX`` entries)
        and ``min_new_tokens`` (``eos_token_id`` cannot be drawn before that many tokens).
        ``rf.logit_process`` edits the logits buffer in place before the sampler reads it,
        on the device and inside the captured step: a row's tokens still depend on that row
        alone and a token still costs one replay. ``logprobs=`` then reports the
        distribution the token was drawn from, the processed logits. With none of them
        given not one extra op runs and the results are what they were.

        ``grammar`` (a ``TokenDFA`` of models/grammar.py, or one per row with None for an
        unconstrained row; needs ``seeds=`` and ``eos_token_id``): the row's output is a word
        of the grammar followed by EOS, or a prefix of one where ``max_new_tokens`` cuts it,
        for every sampling setting. The distinct automata share one int16 table on the device
        (about 100 KB per state at GPT-2's vocabulary); ``rf.grammar_advance`` follows each
        emitted token and ``rf.grammar_mask`` sets the logits of the tokens the state does not
        allow to ``-inf``, after the logit processors and before the sampler, inside the
        captured step: a token still costs one replay, and ``logprobs=`` reports the masked
        distribution. ``min_new_tokens > 0`` or a ``-inf`` ``logit_bias`` on a row with a
        grammar is a ``ValueError`` (either could leave no token). Without ``grammar`` not
        one extra op runs.

        Sequence rules (they need ``seeds=``; ``stop`` and ``bad_words`` are one list of token
        sequences for all rows, a bare int counting as a one-token sequence, or a list with
        one entry per row, each None or such a list, recognised by an entry that is None or
        holds a list; ``no_repeat_ngram_size`` is an int or one per row): ``stop`` (needs
        ``eos_token_id``) ends a row right after the first of its sequences that the output
        completes, and the row is padded with EOS from there as after EOS itself;
        ``bad_words`` never lets the output, or the prompt followed by the output, complete one
        of its sequences; ``no_repeat_ngram_size=n`` (1..``rf.SEQ_MAX_LEN``; 0: off) never lets
        an n-gram occur twice in prompt plus output (the Hugging Face rule). At most
        ``rf.SEQ_MAX`` sequences of a kind with at most ``rf.SEQ_MAX_LEN`` tokens each.
        ``rf.seq_ban`` sets the banned tokens' logits to ``-inf`` after the logit processors
        and before the grammar mask, ``rf.stop_check`` follows the token just written
        (ops/csrc/seq_rules.hip), both on the device and inside the captured step: a row's
        tokens depend on that row alone and a token still costs one replay. ``logprobs=``
        reports the banned distribution. A grammar goes with ``stop`` only. With none of
        the three given not one extra op runs."""
        cfg = self.cfg
        B, T = idx.shape
        if logprobs is not None:
            _checked_top_n("logprobs", logprobs)
        ad = self._adapter_tensor(adapters, B, idx.device)
        named = {k: v for k, v in (("repetition_penalty", repetition_penalty),
                                   ("presence_penalty", presence_penalty),
                                   ("frequency_penalty", frequency_penalty),
                                   ("min_new_tokens", min_new_tokens),
                                   ("logit_bias", logit_bias)) if v is not None}
        seq_named = {k: v for k, v in (("stop", stop), ("bad_words", bad_words),
                                       ("no_repeat_ngram_size", no_repeat_ngram_size))
                     if v is not None}
        if seeds is None:
            if top_p is not None:
                raise ValueError("top_p needs the device sampler: pass seeds=")
            for k in list(named) + list(seq_named):
                raise ValueError(f"{k} needs the device sampler: pass seeds=")
            if grammar is not None:
                raise ValueError("grammar needs the device sampler: pass seeds=")
            if any(isinstance(v, (list, tuple, torch.Tensor)) for v in (temperature, top_k)):
                raise ValueError("per-row temperature / top_k need the device sampler: pass "
                                 "seeds=")
        elif generator is not None:
            raise ValueError("seeds and generator are two sources of randomness: pass one")
        lens_l = [T] * B if lens is None else [int(v) for v in torch.as_tensor(lens).tolist()]
        if B == 0 or T == 0 or len(lens_l) != B or min(lens_l) < 1:
            raise ValueError("generate needs a non-empty prompt in every row")
        if max(lens_l) > T:
            raise ValueError(f"lens {max(lens_l)} exceeds the prompt width {T}")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        if max(lens_l) + max_new_tokens > cfg.n_positions:
            raise ValueError(f"prompt ({max(lens_l)}) + max_new_tokens ({max_new_tokens}) "
                             f"exceeds n_positions ({cfg.n_positions})")
        if seeds is not None:
            temps = _per_row("temperature", temperature, 0.0, B, float)
            ks = _per_row("top_k", top_k, 0, B, int)
            ps = _per_row("top_p", top_p, 1.0, B, float)
            seeds_l = _per_row("seeds", seeds, 0, B, int)
            if min(temps) < 0 or any(t != t for t in temps):
                raise ValueError("temperature must be >= 0")
            if any(not p > 0 for p in ps):
                raise ValueError("top_p must be > 0")
            if any(not -2 ** 63 <= v < 2 ** 64 for v in seeds_l):
                raise ValueError("seeds must fit 64 bits")
            seeds_l = [v - 2 ** 64 if v >= 2 ** 63 else v for v in seeds_l]
        elif temperature < 0:
            raise ValueError("temperature must be >= 0")
        if graph and not idx.is_cuda:
            raise ValueError("graph=True needs the model and prompts on the GPU")
        dev = idx.device
        ctl = rows_c = None
        if named:
            cols = {k: _per_row(k, v, None, B, lambda x: x) if k != "logit_bias" or
                    not isinstance(v, dict) else [v] * B for k, v in named.items()}
            rows_c = [checked_controls(cfg.vocab_size, max_new_tokens, eos_token_id,
                                       **{k: col[b] for k, col in cols.items()})
                      for b in range(B)]
            ctl = LogitControls(B, T, dev)
            idx_l = idx.tolist()
            ctl.put(torch.arange(B, device=dev), rows_c,
                    [idx_l[b][: lens_l[b]] for b in range(B)])
        rows_s = None
        if seq_named:
            stops = _per_row_sequences("stop", stop, B)
            bads = _per_row_sequences("bad_words", bad_words, B)
            ngs = _per_row("no_repeat_ngram_size", no_repeat_ngram_size, None, B, lambda x: x)
            rows_s = [checked_sequences(cfg.vocab_size, eos_token_id, stops[b], bads[b], ngs[b])
                      for b in range(B)]
        gram = None
        if grammar is not None:
            per_row = _per_row("grammar", grammar, None, B, lambda x: x)
            dfas = []
            for b, d in enumerate(per_row):
                if d is not None and not any(d is e for e in dfas):
                    dfas.append(checked_grammar(d, cfg.vocab_size, eos_token_id))
                if d is not None and rows_c is not None:
                    checked_grammar(d, cfg.vocab_size, eos_token_id, rows_c[b])
                if rows_s is not None:
                    checked_grammar_sequences(d, rows_s[b])
            if dfas:
                table, offs = grammar_table(dfas)
                first = {id(d): o + d.start for d, o in zip(dfas, offs)}
                start = [rf.GRAMMAR_NONE if d is None else first[id(d)] for d in per_row]
                gram = (torch.from_numpy(table).to(dev),
                        torch.tensor(start, dtype=torch.int32, device=dev))
        rules = None
        if rows_s is not None and any(r is not None for r in rows_s):
            rules = SequenceRules(B, T, dev, controls=ctl)
            idx_l = idx.tolist()
            rules.put(torch.arange(B, device=dev), rows_s,
                      [idx_l[b][: lens_l[b]] for b in range(B)])
        cache = KVCache(cfg, B, max(lens_l) + max_new_tokens, dev, self.wte.dtype)
        logits = self.prefill(idx, torch.tensor(lens_l, dtype=torch.int32, device=dev), cache,
                              adapters=ad)
        out = torch.empty(B, max_new_tokens, dtype=torch.long, device=dev)
        if seeds is not None:
            eos = None if eos_token_id is None else int(eos_token_id)
            step = _SeededSampler(self, cache, logits, out, temps, ks, ps, seeds_l, eos, ad,
                                  logprobs, ctl, gram, rules)
            res = out if logprobs is None else (out,) + step.lp
            if max_new_tokens > 1:
                step()
                if graph:
                    # (the first step ran eagerly and warmed up what the capture needs.) The
                    # last replay's decode_step is spare: its position is still inside the
                    # cache, and the loop stays free of any launch but the replay
                    step.capture()
                    for _ in range(max_new_tokens - 1):
                        step()
                    return res
                for _ in range(max_new_tokens - 2):
                    step()
            step.draw_last()
            return res
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        step = None
        lp = None if logprobs is None else _logprob_tables(B, max_new_tokens, logprobs, dev)
        for t in range(max_new_tokens):
            tok = self._pick(logits, float(temperature), top_k, generator)
            if eos_token_id is not None:
                tok = torch.where(done, torch.full_like(tok, eos_token_id), tok)
                done |= tok == eos_token_id
            out[:, t] = tok
            if lp is not None:
                for table, got in zip(lp, rf.token_logprobs(logits, tok, logprobs)):
                    table[:, t] = got
            if t + 1 == max_new_tokens:
                break
            if not graph or t == 0:
                # (graph: the first step runs eagerly and warms up what the capture needs)
                logits = self.decode_step(tok, cache, adapters=ad)
            else:
                if step is None:
                    step = _GraphedStep(self, cache, tok, ad)
                logits = step(tok)
        return out if lp is None else (out,) + lp

    score_chunk = 1024  # rows of logits per LM-head chunk of ``score``

    @torch.no_grad()
    def score(self, idx, lens=None, top_n=0, adapters=None):
        """Teacher-forced scoring: ``lp`` fp32 [B, T] with ``lp[b, t]`` the log-probability of
        ``idx[b, t]`` given ``idx[b, :t]`` under the model's own distribution; position 0 and
        the positions ``>= lens[b]`` (``idx`` is right-padded, default: all T) are NaN. With
        ``top_n`` in 1..``rf.LOGPROB_MAX_TOP`` returns ``(lp, top_ids int32 [B, T, top_n],
        top_lp fp32 [B, T, top_n])``, the most likely tokens at every position with theirs
        (ids -1 and NaN where ``lp`` is NaN). ``adapters`` as in ``generate``.

        One pass through the layers with causal (flash) attention, no cache, no host sync.
        The LM head runs over ``score_chunk`` = 1024 of the B * (T - 1) rows at a time and
        ``rf.token_logprobs`` puts each chunk's results in place, so the logits buffer is
        bounded by 1024 x padded_vocab elements (103 MB of bf16 for GPT-2's 50304) whatever
        B and T."""
        cfg = self.cfg
        if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
            raise ValueError("score needs idx [B, T] with B, T >= 1")
        B, T = idx.shape
        if T > cfg.n_positions:
            raise ValueError(f"T ({T}) exceeds n_positions ({cfg.n_positions})")
        _checked_top_n("top_n", top_n)
        dev = idx.device
        if lens is None:
            lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        else:
            lens = torch.as_tensor(lens, device=dev).to(torch.int32)
            if lens.shape != (B,):
                raise ValueError(f"lens must have shape [{B}]")
        ad = self._adapter_tensor(adapters, B, dev)
        out = _logprob_tables(B, T, top_n, dev)
        N = B * (T - 1)
        if N:
            h = self._prompt_pass(idx, None, ad)[:, : T - 1].reshape(N, cfg.n_embd)
            tok = idx[:, 1:].reshape(N)
            rows = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(T - 1)
            cols = torch.arange(1, T, dtype=torch.int32, device=dev).repeat(B)
            active = (cols < lens[rows.long()]).to(torch.uint8)
            chunk = min(N, self.score_chunk)
            buf = torch.empty(chunk, cfg.padded_vocab, device=dev, dtype=h.dtype)
            for s in range(0, N, chunk):
                e = min(N, s + chunk)
                logits = torch.mm(h[s:e], self.wte.t(), out=buf[: e - s])[:, : cfg.vocab_size]
                rf.token_logprobs(logits, tok[s:e], top_n, out=out, rows=rows[s:e],
                                  cols=cols[s:e], active=active[s:e])
        return out if top_n else out[0]

    def _adapter_tensor(self, adapters, B, device):
        """``generate``'s ``adapters`` (None, an int or one per row) as int32 [B] on
        ``device``, or None."""
        if adapters is None:
            return None
        if self.lora is None:
            raise ValueError("adapters given, but no adapter stack is attached: "
                             "attach_lora")
        ad_l = _per_row("adapters", adapters, -1, B, int)
        if any(not -1 <= v < self.lora.n_adapters for v in ad_l):
            raise ValueError(f"adapters must be -1 or in [0, {self.lora.n_adapters})")
        return torch.tensor(ad_l, dtype=torch.int32).to(device)

    def flops_per_token(self, T: int) -> float:
        """6N + 12·L·H·hd·T (PaLM appendix B convention), training FLOPs per token."""
        cfg = self.cfg
        N = self.num_params()
        return 6 * N + 12 * cfg.n_layer * cfg.n_embd * T
