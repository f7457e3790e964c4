"""One process-wide lock around HIP-graph capture. A capture in ``global`` mode makes any
other thread's synchronizing call in the same process fail, so the threads that share a
GPU context — the learner capturing its update graph and an in-process policy server
replaying its inference graph (rllib/env/policy_server.py) — take turns through it."""

import threading

import torch

CAPTURE_LOCK = threading.RLock()


class CapturedStep:
    """``fn()`` recorded once in a HIP graph (one stream, no parallel branches) after a
    device synchronisation, under ``CAPTURE_LOCK`` and ``torch.no_grad()``; ``result`` is
    what the recorded call returned (static buffers), ``replay`` runs the graph under the
    lock. Whatever the capture needs warmed up, the caller has run eagerly before."""

    def __init__(self, fn, device):
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with CAPTURE_LOCK, torch.no_grad(), torch.cuda.graph(self.graph):
            self.result = fn()

    def replay(self):
        with CAPTURE_LOCK:
            self.graph.replay()
