"""Serving the GPT-2 that Train produced: a deployment that batches generation requests.

    app = build_gpt2_app("small", state_dict_path="ckpt.pt")
    handle = serve.run(app, name="gpt2")
    handle.remote({"tokens": [464, 3290], "max_new_tokens": 32}).result()["tokens"]

Concurrent requests are collected by ``@serve.batch``, right-padded into ONE ragged
``GPT2.generate`` call (KV cache, HIP decode attention on the GPU) that runs for the
longest ``max_new_tokens`` of the batch, and every request gets its own tokens back, cut
at its own ``max_new_tokens``. Greedy requests (temperature 0, the default) return what
an un-batched ``generate`` returns; requests are grouped by temperature, because one
``generate`` call samples at one temperature."""

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


class GPT2Server:
    def __init__(self, config="small", state_dict_path=None, seed=0, max_batch_size=8,
                 batch_wait_timeout_s=0.01, device=None):
        cfg = getattr(GPT2Config, config)() if isinstance(config, str) else config
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

    @batch(max_batch_size=8, batch_wait_timeout_s=0.01)
    async def _generate_batch(self, reqs):
        results = [None] * len(reqs)
        groups = {}
        for i, r in enumerate(reqs):
            try:
                if not r.get("tokens"):
                    raise ValueError("request needs a non-empty 'tokens' list")
                key = (float(r.get("temperature", 0.0) or 0.0), r.get("top_k"))
                groups.setdefault(key, []).append(i)
            except Exception as e:  # noqa: BLE001  (one bad request must not fail its batch)
                results[i] = {"error": f"{type(e).__name__}: {e}"}
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


def build_gpt2_app(config="small", state_dict_path=None, seed=0, max_batch_size=8,
                   batch_wait_timeout_s=0.01, device=None):
    """A Serve application around one ``GPT2Server`` replica (``serve.run`` it). ``config``
    names a ``GPT2Config`` preset; without ``state_dict_path`` the weights are the seeded
    random init. ``device`` None: the GPU assigned to the replica, else the CPU."""
    dep = deployment(GPT2Server, name="GPT2Server")
    return dep.bind(config, state_dict_path, seed, max_batch_size, batch_wait_timeout_s, device)
