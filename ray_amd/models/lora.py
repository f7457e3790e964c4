"""Low-rank adapters (LoRA) for GPT-2 inference: a fixed number of adapter slots that requests
of one batch choose between per row (``GPT2.attach_lora``, ``rf.lora_add``).

    stack = LoRAStack(cfg, n_adapters=4, rank=16, device=dev, dtype=torch.bfloat16)
    stack.load(0, {"h.0.c_attn.lora_A": A, "h.0.c_attn.lora_B": B, ...}, alpha=32)
    model.attach_lora(stack)
    model.generate(idx, 32, adapters=[0, -1])        # row 1: the base model

Every buffer is allocated once and written IN PLACE by ``load`` / ``clear``: a captured step
holds the addresses, so adapters come and go without a re-capture. A zero adapter (a fresh or
cleared slot) changes nothing."""

from __future__ import annotations

import re

import torch

TARGETS = ("c_attn", "c_proj", "c_fc", "mlp_proj")
MAX_RANK = 64
_KEY = re.compile(r"^h\.(\d+)\.(\w+)\.lora_([AB])$")


def target_dims(cfg):
    """``{target: (Din, Dout)}`` of the four adapted linears."""
    C = cfg.n_embd
    return {"c_attn": (C, 3 * C), "c_proj": (C, C), "c_fc": (C, 4 * C), "mlp_proj": (4 * C, C)}


class LoRAStack:
    """``a[target]`` [n_layer, n_adapters, R, Din], ``b[target]`` [n_layer, n_adapters, Dout,
    R] for the targets ``c_attn``, ``c_proj``, ``c_fc`` and ``mlp_proj``, and ``scale`` fp32
    [n_adapters]; R is ``rank`` rounded up to a multiple of 16 (<= 64). All zero at first."""

    def __init__(self, cfg, n_adapters, rank, device=None, dtype=None):
        n_adapters, rank = int(n_adapters), int(rank)
        if n_adapters < 1:
            raise ValueError("n_adapters must be >= 1")
        if not 1 <= rank <= MAX_RANK:
            raise ValueError(f"rank must be in 1..{MAX_RANK}, got {rank}")
        self.cfg, self.n_adapters, self.max_rank = cfg, n_adapters, rank
        self.rank = R = -(-rank // 16) * 16
        self.dims = target_dims(cfg)
        L = cfg.n_layer
        self.a = {t: torch.zeros(L, n_adapters, R, din, device=device, dtype=dtype)
                  for t, (din, _) in self.dims.items()}
        self.b = {t: torch.zeros(L, n_adapters, dout, R, device=device, dtype=dtype)
                  for t, (_, dout) in self.dims.items()}
        self.scale = torch.zeros(n_adapters, device=device, dtype=torch.float32)

    @property
    def device(self):
        return self.scale.device

    @property
    def dtype(self):
        return self.a["c_attn"].dtype

    def buffers(self):
        """Every tensor the kernels read: their addresses never change."""
        return [self.a[t] for t in TARGETS] + [self.b[t] for t in TARGETS] + [self.scale]

    def _slot(self, i):
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < self.n_adapters:
            raise ValueError(f"adapter slot must be an int in [0, {self.n_adapters}), got {i!r}")
        return i

    def load(self, i, state, alpha=None):
        """Writes an adapter into slot ``i`` IN PLACE. ``state`` maps ``h.{l}.{target}.lora_A``
        ([r, Din]) and ``h.{l}.{target}.lora_B`` ([Dout, r]) to tensors, one ``r <= rank`` for
        the whole adapter; targets or layers it does not name stay zero. ``scale[i]`` becomes
        ``alpha / r``, with ``alpha`` the argument, else ``state["alpha"]``, else ``r``. Bad
        keys, shapes or ranks raise ``ValueError`` and leave the slot as it was."""
        i = self._slot(i)
        if not isinstance(state, dict):
            raise ValueError("an adapter's state must be a dict")
        if alpha is None:
            alpha = state.get("alpha")
        pairs, r = {}, None
        for key, w in state.items():
            if key == "alpha":
                continue
            m = _KEY.match(key) if isinstance(key, str) else None
            if m is None or m.group(2) not in self.dims or \
                    int(m.group(1)) >= self.cfg.n_layer:
                raise ValueError(f"unknown adapter key {key!r}")
            if not isinstance(w, torch.Tensor) or w.dim() != 2:
                raise ValueError(f"{key} must be a 2-D tensor")
            layer, target, which = int(m.group(1)), m.group(2), m.group(3)
            din, dout = self.dims[target]
            kr = w.shape[0] if which == "A" else w.shape[1]
            if tuple(w.shape) != ((kr, din) if which == "A" else (dout, kr)):
                raise ValueError(f"{key} has shape {tuple(w.shape)}, expected "
                                 f"{'[r, %d]' % din if which == 'A' else '[%d, r]' % dout}")
            if not 1 <= kr <= self.max_rank:
                raise ValueError(f"{key} has rank {kr}, this stack takes 1..{self.max_rank}")
            if r is not None and kr != r:
                raise ValueError(f"{key} has rank {kr}, the adapter's other tensors {r}")
            r = kr
            pairs.setdefault((layer, target), {})[which] = w
        for (layer, target), p in pairs.items():
            if len(p) != 2:
                raise ValueError(f"h.{layer}.{target} needs both lora_A and lora_B")
        if alpha is not None:
            alpha = float(alpha)
            if not alpha == alpha or alpha in (float("inf"), float("-inf")):
                raise ValueError("alpha must be finite")
        # everything checked: from here on nothing raises
        self.clear(i)
        for (layer, target), p in pairs.items():
            self.a[target][layer, i, :r].copy_(p["A"])
            self.b[target][layer, i, :, :r].copy_(p["B"])
        if r is not None:
            self.scale[i] = (r if alpha is None else alpha) / r

    def clear(self, i):
        """Zeroes slot ``i`` IN PLACE: the adapter then changes nothing."""
        i = self._slot(i)
        for t in TARGETS:
            self.a[t][:, i].zero_()
            self.b[t][:, i].zero_()
        self.scale[i] = 0.0
