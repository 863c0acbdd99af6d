"""numpy f64 restatement of ops.spectral_norm_weight (csrc/mappo_ops.hip k_sn_power): the pre-forward hook of
torch.nn.utils.spectral_norm (torch/nn/utils/spectral_norm.py SpectralNorm.compute_weight) for a 2-D weight W (A, H) with the stored
vectors u (A,), v (H,)."""
import numpy as np


def normalize(x, eps):
    """F.normalize(x, dim=0, eps=eps): x / max(||x||_2, eps)"""
    return x / max(float(np.sqrt((x * x).sum())), eps)


def power_iteration(W, u, v, eps=1e-12, n_power_iterations=1):
    """-> (W / sigma, u, v), f64; with n_power_iterations = 0 (the eval-mode hook) u and v come back as they went in"""
    W, u, v = (np.array(x, np.float64) for x in (W, u, v))
    for _ in range(n_power_iterations):
        v = normalize(W.T @ u, eps)                                 # v = normalize(torch.mv(weight_mat.t(), u), dim=0, eps=self.eps, out=v)
        u = normalize(W @ v, eps)                                   # u = normalize(torch.mv(weight_mat, v), dim=0, eps=self.eps, out=u)
    sigma = u @ (W @ v)                                             # sigma = torch.dot(u, torch.mv(weight_mat, v))
    return W / sigma, u, v                                          # weight = weight / sigma
