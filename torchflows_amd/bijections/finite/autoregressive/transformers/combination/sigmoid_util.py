"""Log-space helpers of the sigmoidal transformers (reference ``transformers/combination/sigmoid_util.py``)."""
import torch
import torch.nn.functional as F


def log_softmax(x: torch.Tensor, dim: int) -> torch.Tensor:
    """Through the log-sum-exp, not ``F.log_softmax``: the fixtures pin this rounding."""
    return x - torch.logsumexp(x, dim=dim, keepdim=True)


def log_sigmoid(x: torch.Tensor) -> torch.Tensor:
    return -F.softplus(-x)


def log_dot(m1: torch.Tensor, m2: torch.Tensor) -> torch.Tensor:
    """``log(A @ B)`` from ``m1 = log A (..., d0, d1)`` and ``m2 = log B (..., d1, d2)``."""
    return torch.logsumexp(m1[..., :, :, None] + m2[..., None, :, :], dim=-2)
