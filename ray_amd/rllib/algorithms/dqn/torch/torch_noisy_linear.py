"""``NoisyLinear`` (reference: python/ray/rllib/algorithms/dqn/torch/torch_noisy_linear.py):
the factorised-Gaussian noisy layer lives next to ``QModule``."""

from ray_amd.rllib.core.rl_module.default import NoisyLinear  # noqa: F401
