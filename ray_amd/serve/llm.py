"""Serving the GPT-2 that Train produced: a deployment that batches generation requests.

    app = build_gpt2_app("small", state_dict_path="ckpt.pt")
    handle = serve.run(app, name="gpt2")
    handle.remote({"tokens": [464, 3290], "max_new_tokens": 32}).result()["tokens"]

Concurrent requests are collected by ``@serve.batch``, right-padded into ONE ragged
``GPT2.generate`` call (KV cache, HIP decode attention on the GPU) that runs for the
longest ``max_new_tokens`` of the batch, and every request gets its own tokens back, cut
at its own ``max_new_tokens``. Greedy requests (temperature 0, the default) return what
an un-batched ``generate`` returns.

A request may carry its own ``temperature``, ``top_k``, ``top_p`` and ``seed``. A batch in
which any request samples, or names ``top_p`` or ``seed``, is still ONE ``generate`` call:
the device sampler (``rf.sample_logits``) takes every parameter per row, greedy requests
ride along at temperature 0, and a request without ``seed`` gets the server's. The
randomness of a token is a hash of the request's seed and the token's position, so a
request's tokens are those of ``generate(..., seeds=[seed])`` on that request alone,
whoever shared its batch. Every request is checked on its own before the call (empty
prompt, a bad value, prompt + ``max_new_tokens`` past ``n_positions``), so a bad request
is answered with an error and never fails its batch; a valid batch whose longest prompt
plus longest ``max_new_tokens`` would not fit ``n_positions`` is split.

``build_gpt2_app(..., continuous=True, slots=S)`` binds ``GPT2EngineServer`` instead:
continuous batching over S KV-cache slots (``models/gpt2_engine.py``). Requests enter and
leave between replays of one captured decode step, so a 5-token request does not wait for
a 900-token one, and ``handle.options(method_name="stream", stream=True)`` streams the
tokens as they are produced. The same request fields and the same per-request guarantee.
``prefixes={"name": [tokens], ...}`` registers shared prompt prefixes with the engine at
start-up (each is prefilled once); a request may then carry ``"prefix": "name"`` and its
``tokens`` are the continuation: it answers what the request with the whole prompt answers.
``prefill_chunk=C`` bounds the prompt tokens a request is fed per engine step.
``adapters={"name": path_or_state_dict, ...}`` loads low-rank adapters (``models/lora.py``,
up to ``lora_rank``) into the engine at start-up; a request may then carry ``"adapter":
"name"`` and shares its decode steps with requests of other adapters and of the base model.
A prefix may be bound to an adapter: ``prefixes={"name": {"tokens": [...], "adapter":
"name"}}``.

Log-probabilities: a request may carry ``"logprobs": m`` (0..8). Its response gains
``"logprobs": [...]``, the log-probability of every returned token under the model's own
distribution (whatever the sampling parameters), and ``"top_logprobs": [[[id, lp], ... m],
...]``, the m most likely tokens at every position with theirs; a streamed chunk carries the
slice for its tokens, and a non-finite value is ``None`` (JSON has no ``-inf``). The static
server routes such a batch through the device sampler, one ``generate(..., logprobs=max m)``
call, each result cut to its own m. The continuous server needs ``build_gpt2_app(...,
logprobs=N)``, which passes N to the engine; m above N, or m on an app built without it, is
that request's error. A request without the field gets the response it always got.

Logit processors: a request may carry ``"repetition_penalty"``, ``"presence_penalty"``,
``"frequency_penalty"``, ``"min_new_tokens"`` and ``"logit_bias"`` (a JSON object whose keys
are token ids, as strings or ints; ``-inf`` values arrive as the float), with the meaning
they have in ``GPT2.generate``. Each request is checked on its own and an error is that
request's. The static server routes a batch that contains any of them through the device
sampler, one ``generate`` call with every control per row (it has no ``eos_token_id``, so a
non-zero ``min_new_tokens`` is an error there). The continuous server needs
``build_gpt2_app(..., continuous=True, logit_processors=True)``, which passes the flag to the
engine; without it a request that names one of the fields gets an error. With
``"logprobs"`` the values describe the processed logits, the distribution the token was
drawn from.

Structured output: ``build_gpt2_app(..., grammars={"name": TokenDFA, ...}, eos_token_id=E)``
(``models/grammar.py``: ``from_choices``, ``from_regex``, ``from_byte_dfa``). A request may
carry ``"grammar": "name"``, or an inline ``"choices": [[token, ...], ...]`` ("answer with one
of these"), and its tokens are then a word of that grammar followed by E (a prefix of one where
``max_new_tokens`` cuts it), whatever its sampling parameters. The static server runs the
requests of a batch that name a grammar as one ``generate(..., grammar=[...])`` call through
the device sampler, apart from their batch-mates (which do not end at E), and cuts each result
after its E. The continuous server also takes ``grammar_states=N``, the rows of the engine's
pool: the named grammars are registered at start-up, an inline one when its request is
submitted, and it is dropped when the request ends, is cancelled or fails; a pool without
room is that request's error. An unknown name, both fields at once, a field the app was not
built for, and a grammar together with ``min_new_tokens > 0`` or a ``-inf`` ``logit_bias`` are
each that request's error.

Sequence rules: a request may carry ``"stop": [[token, ...] | token, ...]`` (the answer ends
right after the first of these sequences it completes, the sequence included),
``"bad_words": [...]`` (the answer, or the prompt followed by the answer, never completes one)
and ``"no_repeat_ngram_size": n`` (no n-gram occurs twice in prompt plus answer), with the
limits of ``GPT2.generate``. The static server routes such a batch through the device sampler;
``"stop"`` needs ``build_gpt2_app(..., eos_token_id=E)`` and its requests run with the grammar
requests, apart from their batch-mates (their call ends rows at E), each row cut after its
stop or its E. The continuous server needs ``build_gpt2_app(..., continuous=True,
sequence_rules=True)``. A bad value, a field the app was not built for, and a grammar together
with ``"bad_words"`` or ``"no_repeat_ngram_size" > 0`` are each that request's error."""

from __future__ import annotations

import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.serve.api import deployment
from ray_amd.serve.batching import batch


def _pick_device(device):
    if device is not None:
        return torch.device(device)
    try:
        import ray_amd

        gpus = ray_amd.get_gpu_ids()
    except Exception:  # noqa: BLE001  (not inside a worker: unit use)
        gpus = []
    # the raylet narrows the replica's visible devices to the ones it was assigned
    return torch.device("cuda", 0) if gpus and torch.cuda.is_available() else torch.device("cpu")


def _request_logprobs(r, limit, hint=""):
    """The request's checked ``"logprobs"`` (None: the field is absent) against ``limit``
    (None: the server keeps none)."""
    m = r.get("logprobs")
    if m is None:
        return None
    if isinstance(m, bool) or not isinstance(m, int) or m < 0:
        raise ValueError("logprobs must be an int >= 0")
    if limit is None:
        raise ValueError("'logprobs' needs build_gpt2_app(continuous=True, logprobs=N)")
    if m > limit:
        raise ValueError(f"logprobs ({m}) exceeds the server's {limit}{hint}")
    return m


CONTROL_FIELDS = ("repetition_penalty", "presence_penalty", "frequency_penalty",
                  "min_new_tokens", "logit_bias")


def _request_controls(cfg, r, new, eos, enabled=True):
    """The request's logit-processor fields as ``generate`` / ``submit`` keyword arguments,
    checked (``{}``: it names none). ``logit_bias`` keys may be strings."""
    from ray_amd.models.gpt2 import checked_controls

    kw = {k: r[k] for k in CONTROL_FIELDS if r.get(k) is not None}
    if not kw:
        return {}
    if not enabled:
        raise ValueError(f"{sorted(kw)[0]!r} needs build_gpt2_app(continuous=True, "
                         "logit_processors=True)")
    bias = kw.get("logit_bias")
    if bias is not None:
        if not isinstance(bias, dict):
            raise ValueError("logit_bias must be an object {token id: value}")
        try:
            kw["logit_bias"] = {t if isinstance(t, int) else int(str(t), 10): v
                                for t, v in bias.items()}
        except ValueError:
            raise ValueError("logit_bias keys must be token ids") from None
        if len(kw["logit_bias"]) != len(bias):
            raise ValueError("logit_bias names a token id twice")
    checked_controls(cfg.vocab_size, new, eos, **kw)
    return kw


def _request_grammar(cfg, r, grammars, eos, ctl, new, hint):
    """The request's grammar as a ``TokenDFA`` (None: it names none): ``"grammar"``, a name of
    ``grammars``, or inline ``"choices"``; checked against the request's controls ``ctl``.
    ``grammars`` None: the app was not built for grammars (``hint`` says how)."""
    from ray_amd.models.gpt2 import checked_controls, checked_grammar
    from ray_amd.models.grammar import TokenDFA

    name, choices = r.get("grammar"), r.get("choices")
    if name is None and choices is None:
        return None
    if name is not None and choices is not None:
        raise ValueError("'grammar' and 'choices' are two grammars: pass one")
    if grammars is None or eos is None:
        raise ValueError(f"{'grammar' if choices is None else 'choices'!r} needs {hint}")
    if name is not None:
        if not isinstance(name, str) or name not in grammars:
            raise ValueError(f"unknown grammar {name!r}")
        dfa = grammars[name]
    else:
        if not isinstance(choices, list) or \
                any(not isinstance(c, list) or
                    any(isinstance(t, bool) or not isinstance(t, int) for t in c)
                    for c in choices):
            raise ValueError("choices must be a list of lists of token ids")
        dfa = TokenDFA.from_choices(choices, cfg.vocab_size, eos)
    return checked_grammar(dfa, cfg.vocab_size, eos,
                           checked_controls(cfg.vocab_size, new, eos, **ctl) if ctl else None)


SEQUENCE_FIELDS = ("stop", "bad_words", "no_repeat_ngram_size")


def _request_sequences(cfg, r, eos, dfa=None, enabled=True):
    """The request's sequence-rule fields as ``generate`` / ``submit`` keyword arguments,
    checked, sequences as lists of lists (``{}``: it names none); ``dfa``: the request's
    grammar, which goes with ``"stop"`` only."""
    from ray_amd.models.gpt2 import checked_grammar_sequences, checked_sequences

    kw = {k: r[k] for k in SEQUENCE_FIELDS if r.get(k) is not None}
    if not kw:
        return {}
    if not enabled:
        raise ValueError(f"{sorted(kw)[0]!r} needs build_gpt2_app(continuous=True, "
                         "sequence_rules=True)")
    if "stop" in kw and eos is None:
        raise ValueError("'stop' needs build_gpt2_app(eos_token_id=...)")
    rules = checked_sequences(cfg.vocab_size, eos, **kw)
    checked_grammar_sequences(dfa, rules)
    for k, v in zip(SEQUENCE_FIELDS, rules):
        if k in kw:
            kw[k] = v
    return kw


def _finite(v):
    return v if v == v and abs(v) != float("inf") else None


def _logprob_fields(lp, ids, tlp, m):
    """The response fields for one request's tokens: ``lp`` [n], ``ids`` / ``tlp`` [n][>= m]
    as lists."""
    return {"logprobs": [_finite(v) for v in lp],
            "top_logprobs": [[[int(i), _finite(v)] for i, v in zip(ri[:m], rv[:m])]
                             for ri, rv in zip(ids, tlp)]}


class GPT2Server:
    def __init__(self, config="small", state_dict_path=None, seed=0, max_batch_size=8,
                 batch_wait_timeout_s=0.01, device=None, grammars=None, eos_token_id=None):
        cfg = getattr(GPT2Config, config)() if isinstance(config, str) else config
        # grammars: name -> TokenDFA (None: the server answers no grammar request); they,
        # and inline choices, end with eos_token_id (default: the first grammar's)
        self.grammars = None if grammars is None and eos_token_id is None else dict(grammars
                                                                                    or {})
        if eos_token_id is None and self.grammars:
            eos_token_id = next(iter(self.grammars.values())).eos_token_id
        self.eos = eos_token_id
        for name, dfa in (self.grammars or {}).items():
            from ray_amd.models.gpt2 import checked_grammar

            try:
                checked_grammar(dfa, cfg.vocab_size, self.eos)
            except ValueError as e:
                raise ValueError(f"grammar {name!r}: {e}") from None
        self.device = _pick_device(device)
        torch.manual_seed(seed)
        model = GPT2(cfg)
        if state_dict_path is not None:
            model.load_state_dict(torch.load(state_dict_path, map_location="cpu"))
        if self.device.type == "cuda":
            model = model.to(self.device, torch.bfloat16)
        self.model = model.eval()
        self.seed = seed
        self._generate_batch.set_max_batch_size(int(max_batch_size))
        self._generate_batch.set_batch_wait_timeout_s(float(batch_wait_timeout_s))

    def _run(self, reqs):
        """One ragged generate call for requests that share a temperature."""
        lens = [len(r["tokens"]) for r in reqs]
        new = [int(r.get("max_new_tokens", 16)) for r in reqs]
        idx = torch.zeros(len(reqs), max(lens), dtype=torch.long)
        for b, r in enumerate(reqs):
            idx[b, : lens[b]] = torch.tensor(r["tokens"], dtype=torch.long)
        temp = float(reqs[0].get("temperature", 0.0) or 0.0)
        gen = None
        if temp > 0:
            gen = torch.Generator(device=self.device).manual_seed(self.seed)
        out = self.model.generate(idx.to(self.device), max(new), lens=lens, temperature=temp,
                                  top_k=reqs[0].get("top_k"), generator=gen).cpu()
        return [out[b, : new[b]].tolist() for b in range(len(reqs))]

    def _params(self, r):
        """The request's checked (len, new, temperature, top_k, top_p, seed)."""
        if r.get("prefix") is not None:
            raise ValueError("'prefix' needs the continuous engine: build_gpt2_app("
                             "continuous=True, prefixes=...)")
        if r.get("adapter") is not None:
            raise ValueError("'adapter' needs the continuous engine: build_gpt2_app("
                             "continuous=True, adapters=...)")
        return _request_params(self.model.cfg, self.seed, r)

    def _run_sampled(self, reqs, params, lps=None, ctls=None, grs=None, seqs=None):
        """One ragged generate call through the device sampler, every parameter per row.
        ``lps`` (each request's ``logprobs`` or None; not all None): the call reports the
        batch's widest and every result is a dict cut to its own. ``ctls``: each request's
        ``_request_controls``. ``grs``: each request's ``TokenDFA`` or None (a request with
        ``"stop"`` only): the call ends rows at the server's EOS and every result is cut after
        its EOS or its first completed stop sequence. ``seqs``: each request's
        ``_request_sequences``."""
        lens = [p[0] for p in params]
        new = [p[1] for p in params]
        idx = torch.zeros(len(reqs), max(lens), dtype=torch.long)
        for b, r in enumerate(reqs):
            idx[b, : lens[b]] = torch.tensor(r["tokens"], dtype=torch.long)
        kw = dict(lens=lens, temperature=[p[2] for p in params], top_k=[p[3] for p in params],
                  top_p=[p[4] for p in params], seeds=[p[5] for p in params])
        if ctls is not None and any(ctls):
            # min_new_tokens is checked against the request's own max_new_tokens, above
            for k in CONTROL_FIELDS:
                if any(k in c for c in ctls):
                    kw[k] = [c.get(k) for c in ctls]
        if grs:
            kw.update(eos_token_id=self.eos)
            if any(g is not None for g in grs):
                kw.update(grammar=grs)
        if seqs is not None and any(seqs):
            for k in SEQUENCE_FIELDS:  # per row: an entry is None or a list of lists
                if any(s.get(k) for s in seqs):
                    kw[k] = [s.get(k) or None for s in seqs]

        def cut(out):
            """``new`` with every row ending after its first EOS or completed stop."""
            if not grs:
                return new
            res = []
            for b in range(len(reqs)):
                t = out[b, : new[b]].tolist()
                stops = (seqs[b].get("stop") or []) if seqs else []
                res.append(next((e for e in range(1, len(t) + 1) if t[e - 1] == self.eos or any(
                    len(s) <= e and t[e - len(s): e] == s for s in stops)), len(t)))
            return res

        if lps is None or all(m is None for m in lps):
            out = self.model.generate(idx.to(self.device), max(new), **kw).cpu()
            new = cut(out)
            toks = [out[b, : new[b]].tolist() for b in range(len(reqs))]
            return toks if lps is None else [{"tokens": t} for t in toks]
        out, lp, ids, tlp = (t.cpu() for t in self.model.generate(
            idx.to(self.device), max(new), logprobs=max(m for m in lps if m is not None), **kw))
        new = cut(out)
        res = []
        for b, m in enumerate(lps):
            res.append({"tokens": out[b, : new[b]].tolist()})
            if m is not None:
                res[-1].update(_logprob_fields(lp[b, : new[b]].tolist(), ids[b, : new[b]].tolist(),
                                               tlp[b, : new[b]].tolist(), m))
        return res

    @batch(max_batch_size=8, batch_wait_timeout_s=0.01)
    async def _generate_batch(self, reqs):
        from ray_amd.ops.functional import LOGPROB_MAX_TOP

        results = [None] * len(reqs)
        params, lps, ctls, grs, seqs = {}, {}, {}, {}, {}
        for i, r in enumerate(reqs):
            try:
                lps[i] = _request_logprobs(r, LOGPROB_MAX_TOP)
                p = self._params(r)
                ctls[i] = _request_controls(self.model.cfg, r, p[1], None)
                grs[i] = _request_grammar(self.model.cfg, r, self.grammars, self.eos, ctls[i],
                                          p[1], "build_gpt2_app(grammars=..., eos_token_id=...)")
                seqs[i] = _request_sequences(self.model.cfg, r, self.eos, grs[i])
                params[i] = p
            except Exception as e:  # noqa: BLE001  (one bad request must not fail its batch)
                results[i] = {"error": f"{type(e).__name__}: {e}"}
        if any(p[2] > 0 or reqs[i].get("top_p") is not None or reqs[i].get("seed") is not None
               or lps[i] is not None or ctls[i] or grs[i] is not None or seqs[i]
               for i, p in params.items()):
            # one call, split only where the longest prompt and the longest continuation
            # of the batch together would not fit the model's positions; the requests with a
            # grammar or a stop run apart (their call ends rows at EOS, their batch-mates'
            # does not)
            ends = {i: grs[i] is not None or "stop" in seqs[i] for i in params}
            chunks = []
            for constrained in (False, True):
                cur = []
                for i in params:
                    if ends[i] != constrained:
                        continue
                    trial = cur + [i]
                    if cur and max(params[j][0] for j in trial) + \
                            max(params[j][1] for j in trial) > self.model.cfg.n_positions:
                        chunks.append(cur)
                        trial = [i]
                    cur = trial
                if cur:
                    chunks.append(cur)
            for members in chunks:
                try:
                    got = self._run_sampled([reqs[i] for i in members],
                                            [params[i] for i in members],
                                            [lps[i] for i in members],
                                            [ctls[i] for i in members],
                                            [grs[i] for i in members]
                                            if ends[members[0]] else None,
                                            [seqs[i] for i in members])
                    for i, res in zip(members, got):
                        results[i] = res
                except ValueError as e:
                    for i in members:
                        results[i] = {"error": f"ValueError: {e}"}
            return results
        # all greedy, none of the sampler's fields: the scalar path
        groups = {}
        for i in params:
            groups.setdefault((0.0, reqs[i].get("top_k")), []).append(i)
        for members in groups.values():
            try:
                for i, toks in zip(members, self._run([reqs[i] for i in members])):
                    results[i] = {"tokens": toks}
            except ValueError as e:
                for i in members:
                    results[i] = {"error": f"ValueError: {e}"}
        return results

    async def __call__(self, request):
        if not isinstance(request, dict):  # HTTP: a JSON body
            request = await request.json()
        return await self._generate_batch(request)


def _request_params(cfg, default_seed, r):
    """A request's checked (len, new, temperature, top_k, top_p, seed)."""
    toks = r.get("tokens")
    if not toks:
        raise ValueError("request needs a non-empty 'tokens' list")
    if any(not isinstance(t, int) or not 0 <= t < cfg.vocab_size for t in toks):
        raise ValueError(f"tokens must be ints in [0, {cfg.vocab_size})")
    new = int(r.get("max_new_tokens", 16))
    if new < 1:
        raise ValueError("max_new_tokens must be >= 1")
    if len(toks) + new > cfg.n_positions:
        raise ValueError(f"prompt ({len(toks)}) + max_new_tokens ({new}) exceeds "
                         f"n_positions ({cfg.n_positions})")
    temp = float(r.get("temperature", 0.0) or 0.0)
    if not 0 <= temp < float("inf"):
        raise ValueError("temperature must be >= 0")
    top_k = r.get("top_k")
    top_k = 0 if top_k is None else int(top_k)
    top_p = r.get("top_p")
    top_p = 1.0 if top_p is None else float(top_p)
    if not 0 < top_p <= 1:
        raise ValueError("top_p must be in (0, 1]")
    seed = r.get("seed")
    seed = default_seed if seed is None else int(seed)
    if not -2 ** 63 <= seed < 2 ** 64:
        raise ValueError("seed must fit 64 bits")
    return len(toks), new, temp, top_k, top_p, seed


class GPT2EngineServer:
    """Continuous batching: requests enter and leave a ``GPT2Engine`` of ``slots`` KV-cache
    slots independently, so a short request never waits for a long one and tokens can be
    streamed as they are produced. ``__call__`` awaits the whole result,
    ``{"tokens": [...]}``; ``stream`` (``handle.options(method_name="stream", stream=True)``)
    yields ``{"tokens": [...new...]}`` chunks, the last one with ``"finished": True``. A
    request's tokens are those of ``generate(..., seeds=[seed])`` on that request alone,
    cut after the first ``eos_token_id``.

    One engine thread owns the model and every GPU call (construction, graph capture,
    replays). Requests reach it through a thread-safe queue, on which it blocks when idle;
    results go back to the caller's event loop with ``call_soon_threadsafe``."""

    def __init__(self, config="small", state_dict_path=None, seed=0, slots=None,
                 eos_token_id=None, device=None, poll_every=None, prefixes=None,
                 prefill_chunk=None, adapters=None, lora_rank=16, speculate=0, ngram=(2, 4),
                 logprobs=None, logit_processors=False, grammars=None, grammar_states=0,
                 sequence_rules=False):
        import queue
        import threading

        self.cfg = getattr(GPT2Config, config)() if isinstance(config, str) else config
        self.device = _pick_device(device)
        self.seed = seed
        self.engine = None
        self._inbox = queue.Queue()
        self._next_key = 0
        self._failure = None
        # prefix name -> (tokens, adapter name or None)
        self._prefixes = {k: (list(v["tokens"]), v.get("adapter")) if isinstance(v, dict)
                          else (list(v), None) for k, v in (prefixes or {}).items()}
        self._adapters = dict(adapters or {})  # adapter name -> path or state dict
        self._lora_rank = int(lora_rank)
        self._aids = {}  # adapter name -> the engine's adapter slot
        self._prefill_chunk = prefill_chunk
        self._speculate, self._ngram = speculate, ngram
        self._logprobs = logprobs  # the engine's N (None: it keeps none)
        self._logit_processors = bool(logit_processors)
        self._grammar_states = int(grammar_states)
        self._sequence_rules = bool(sequence_rules)
        # grammar name -> TokenDFA (None: the server answers no grammar request)
        self._grammars = dict(grammars or {}) if self._grammar_states else None
        if grammars and not self._grammar_states:
            raise ValueError("grammars need grammar_states=N, the rows of the engine's pool")
        self._gids = {}  # grammar name -> the engine's grammar id
        self._eos = eos_token_id
        self._pids = {}  # prefix name -> the engine's prefix id
        ready = threading.Event()
        self._thread = threading.Thread(
            target=self._engine_loop, name="gpt2-engine", daemon=True,
            args=(state_dict_path, 8 if slots is None else int(slots), eos_token_id,
                  poll_every, ready))
        self._thread.start()
        ready.wait()
        if self._failure is not None:
            raise self._failure

    # ------------------------------------------------------------------ the engine thread
    def _engine_loop(self, state_dict_path, slots, eos_token_id, poll_every, ready):
        import queue

        from ray_amd.models.gpt2_engine import GPT2Engine

        try:
            torch.manual_seed(self.seed)
            model = GPT2(self.cfg)
            if state_dict_path is not None:
                model.load_state_dict(torch.load(state_dict_path, map_location="cpu"))
            if self.device.type == "cuda":
                torch.cuda.set_device(self.device)
                model = model.to(self.device, torch.bfloat16)
            kw = {} if poll_every is None else {"poll_every": int(poll_every)}
            if self._adapters:
                from ray_amd.models.lora import LoRAStack

                kw["lora"] = LoRAStack(self.cfg, len(self._adapters), self._lora_rank,
                                       model.wte.device, model.wte.dtype)
            eng = GPT2Engine(model.eval(), slots=slots, eos_token_id=eos_token_id,
                             prefix_slots=len(self._prefixes),
                             prefill_chunk=self._prefill_chunk, speculate=self._speculate,
                             ngram=self._ngram, logprobs=self._logprobs,
                             logit_processors=self._logit_processors,
                             grammar_states=self._grammar_states,
                             sequence_rules=self._sequence_rules, **kw)
            for name, dfa in (self._grammars or {}).items():
                try:
                    self._gids[name] = eng.add_grammar(dfa)
                except ValueError as e:
                    raise ValueError(f"grammar {name!r}: {e}") from None
            for i, (name, state) in enumerate(self._adapters.items()):
                if not isinstance(state, dict):
                    state = torch.load(state, map_location="cpu")
                eng.load_adapter(i, state)
                self._aids[name] = i
            for name, (toks, adapter) in self._prefixes.items():
                if adapter is not None and adapter not in self._aids:
                    raise ValueError(f"prefix {name!r} names the unknown adapter {adapter!r}")
                self._pids[name] = eng.add_prefix(toks, adapter=self._aids.get(adapter))
            self.engine = eng
        except BaseException as e:  # noqa: BLE001  (reported to the constructor's caller)
            self._failure = e
            return
        finally:
            ready.set()
        sinks = {}  # engine request id -> (key, loop, asyncio queue)
        rids = {}   # key -> engine request id
        inline = {}  # engine request id -> the grammar registered for that request alone

        def retire(rid):
            gid = inline.pop(rid, None)
            if gid is not None:
                eng.drop_grammar(gid)

        while True:
            msgs = []
            if not eng.has_work():
                msgs.append(self._inbox.get())  # idle: block, no spinning
            try:
                while True:
                    msgs.append(self._inbox.get_nowait())
            except queue.Empty:
                pass
            for msg in msgs:
                if msg[0] == "stop":
                    return
                if msg[0] == "cancel":
                    rid = rids.pop(msg[1], None)
                    if rid is not None:
                        eng.cancel(rid)
                        sinks.pop(rid, None)
                        retire(rid)
                    continue
                _, key, req, p, ctl, dfa, loop, sink = msg
                gid = None
                try:
                    if dfa is not None:
                        # a named grammar is in the pool; an inline one enters it for the
                        # time of this request (no room: this request's error)
                        gid = self._gids.get(req.get("grammar"))
                        if gid is None:
                            gid = eng.add_grammar(dfa)
                    rid = eng.submit(req["tokens"], p[1], temperature=p[2], top_k=p[3],
                                     top_p=p[4], seed=p[5],
                                     prefix=self._pids.get(req.get("prefix")),
                                     adapter=self._aids.get(req.get("adapter")),
                                     logprobs=req.get("logprobs"),
                                     **({} if gid is None else {"grammar": gid}), **ctl)
                except ValueError as e:
                    if gid is not None and req.get("grammar") is None:
                        eng.drop_grammar(gid)
                    loop.call_soon_threadsafe(sink.put_nowait, ("error", f"ValueError: {e}"))
                    continue
                if gid is not None and req.get("grammar") is None:
                    inline[rid] = gid
                sinks[rid] = (key, loop, sink)
                rids[key] = rid
            if not eng.has_work():
                continue
            try:
                events = eng.step()
            except BaseException as e:  # noqa: BLE001  (every waiting caller learns of it)
                for key, loop, sink in sinks.values():
                    loop.call_soon_threadsafe(sink.put_nowait,
                                              ("error", f"{type(e).__name__}: {e}"))
                self._failure = e
                return
            for rid, new, finished, *info in events:
                key, loop, sink = sinks[rid]
                if finished:
                    del sinks[rid]
                    rids.pop(key, None)
                    retire(rid)
                # (an engine with logprobs: the event's fourth field, None for a request
                # that asked for none)
                loop.call_soon_threadsafe(sink.put_nowait,
                                          ("tokens", new, finished, info[0] if info else None))

    def close(self):
        self._inbox.put(("stop",))
        self._thread.join()

    # ------------------------------------------------------------------ the callers' side
    async def _chunks(self, request):
        """The request's ("tokens", new, finished, info) items as the engine's polls produce
        them, or one ("error", message); cancels the request when the consumer leaves."""
        import asyncio

        if not isinstance(request, dict):  # HTTP: a JSON body
            request = await request.json()
        try:
            p = _request_params(self.cfg, self.seed, request)
            _request_logprobs(request, self._logprobs)
            ctl = _request_controls(self.cfg, request, p[1], self._eos, self._logit_processors)
            dfa = _request_grammar(self.cfg, request, self._grammars, self._eos, ctl, p[1],
                                   "build_gpt2_app(continuous=True, grammar_states=N, "
                                   "eos_token_id=...)")
            ctl = {**ctl, **_request_sequences(self.cfg, request, self._eos, dfa,
                                               self._sequence_rules)}
            name = request.get("prefix")
            if name is not None and (not isinstance(name, str) or name not in self._pids):
                raise ValueError(f"unknown prefix {name!r}")
            name = request.get("adapter")
            if name is not None and (not isinstance(name, str) or name not in self._aids):
                raise ValueError(f"unknown adapter {name!r}")
        except Exception as e:  # noqa: BLE001  (a bad request touches nothing else)
            yield ("error", f"{type(e).__name__}: {e}")
            return
        if self._failure is not None:
            yield ("error", f"engine stopped: {self._failure}")
            return
        key = self._next_key
        self._next_key += 1
        sink = asyncio.Queue()
        self._inbox.put(("submit", key, request, p, ctl, dfa, asyncio.get_running_loop(), sink))
        finished = False
        try:
            while not finished:
                item = await sink.get()
                finished = item[0] == "error" or item[2]
                yield item
        finally:
            if not finished:  # the generator was closed or the task cancelled
                self._inbox.put(("cancel", key))

    @staticmethod
    def _fields(request, info):
        """A chunk's logprob fields ({} for a request that asked for none)."""
        if info is None:
            return {}
        return _logprob_fields(info["logprobs"], info["top_ids"], info["top_logprobs"],
                               request["logprobs"])

    async def __call__(self, request):
        if not isinstance(request, dict):  # HTTP: a JSON body
            request = await request.json()
        res = {"tokens": []}
        async for item in self._chunks(request):
            if item[0] == "error":
                return {"error": item[1]}
            res["tokens"].extend(item[1])
            for k, v in self._fields(request, item[3]).items():
                res.setdefault(k, []).extend(v)
        return res

    async def stream(self, request):
        if not isinstance(request, dict):  # HTTP: a JSON body
            request = await request.json()
        chunks = self._chunks(request)
        try:
            async for item in chunks:
                if item[0] == "error":
                    yield {"error": item[1], "finished": True}
                elif item[2]:
                    yield {"tokens": item[1], **self._fields(request, item[3]),
                           "finished": True}
                else:
                    yield {"tokens": item[1], **self._fields(request, item[3])}
        finally:
            await chunks.aclose()


def build_gpt2_app(config="small", state_dict_path=None, seed=0, max_batch_size=8,
                   batch_wait_timeout_s=0.01, device=None, continuous=False, slots=None,
                   eos_token_id=None, prefixes=None, prefill_chunk=None, adapters=None,
                   lora_rank=16, speculate=0, ngram=(2, 4), logprobs=None,
                   logit_processors=False, grammars=None, grammar_states=0,
                   sequence_rules=False):
    """A Serve application around one ``GPT2Server`` replica (``serve.run`` it). ``config``
    names a ``GPT2Config`` preset; without ``state_dict_path`` the weights are the seeded
    random init. ``device`` None: the GPU assigned to the replica, else the CPU.

    ``continuous=True`` binds a ``GPT2EngineServer`` instead: continuous batching over
    ``slots`` (default 8) KV-cache slots with streaming, requests ending at
    ``eos_token_id``; ``max_batch_size`` and ``batch_wait_timeout_s`` do not apply.
    ``prefixes`` (``{"name": [tokens], ...}``: shared prompt prefixes a request names with
    ``"prefix": "name"``) and ``prefill_chunk`` need ``continuous=True``. So does ``adapters``
    (``{"name": path_or_state_dict, ...}``: low-rank adapters of rank up to ``lora_rank`` in
    the ``LoRAStack.load`` format, paths read with ``torch.load``), which a request names
    with ``"adapter": "name"``; a ``prefixes`` value may be ``{"tokens": [...], "adapter":
    "name"}``. ``speculate=k`` (1..8; needs ``continuous=True`` too) turns on the engine's
    speculative decoding with prompt-lookup drafts of the n-gram lengths ``ngram=(lo, hi)``:
    the same tokens, up to k + 1 of them per device step. ``logprobs=N`` (0..8, with
    ``continuous=True``): the engine keeps per-token log-probabilities and the top N
    alternatives, and a request may ask for ``"logprobs": m`` <= N. The static server
    needs no option and ignores this one: it answers ``"logprobs": m`` up to 8.
    ``logit_processors=True`` (with ``continuous=True``): the engine keeps the per-slot tables
    of the repetition / presence / frequency penalties, ``logit_bias`` and
    ``min_new_tokens``, and a request may name them; the static server needs no option.
    ``grammars={"name": TokenDFA, ...}`` (both servers; they end with ``eos_token_id``, by
    default the first grammar's on the static server): a request may name one with
    ``"grammar": "name"`` or carry inline ``"choices"``, and answers with a word of it. The
    continuous server also needs ``grammar_states=N``, the rows of the engine's pool (about
    100 KB each at GPT-2's vocabulary): the named grammars' states plus room for the inline
    grammars of the requests in flight. ``sequence_rules=True`` (with ``continuous=True``): the
    engine keeps the per-slot tables of ``"stop"``, ``"bad_words"`` and
    ``"no_repeat_ngram_size"``, and a request may name them; the static server needs no option
    (``"stop"`` needs ``eos_token_id`` on both)."""
    if continuous:
        dep = deployment(GPT2EngineServer, name="GPT2EngineServer")
        return dep.bind(config, state_dict_path, seed, slots, eos_token_id, device, None,
                        prefixes, prefill_chunk, adapters, lora_rank, speculate, ngram, logprobs,
                        logit_processors, grammars, grammar_states, sequence_rules)
    if sequence_rules:
        raise ValueError("sequence_rules needs continuous=True (the static server needs no "
                         "option)")
    if prefixes or prefill_chunk is not None or adapters or speculate or grammar_states:
        raise ValueError("prefixes, prefill_chunk, adapters, speculate and grammar_states need "
                         "continuous=True")
    dep = deployment(GPT2Server, name="GPT2Server")
    return dep.bind(config, state_dict_path, seed, max_batch_size, batch_wait_timeout_s, device,
                    grammars, eos_token_id)
