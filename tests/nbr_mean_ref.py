"""numpy f64 restatement of ops.fcra_mean / ops.fcra_mean_pair_multi (csrc/mappo_ops.hip k_nbr_mean, k_nbr_mean4): DHGN.fcra's
neighbour mean `torch.matmul(F.normalize(adj, p=1, dim=-1), z)` (reference DHGN/mappo_parallel.py:204-233), plus an optional bias
and ReLU.  z (R, P, E), adj (R, P, P), bias (E,)."""
import numpy as np


def normalize_l1(adj):
    """F.normalize(adj, p=1, dim=-1): adj / max(sum_j |adj_ij|, 1e-12)"""
    adj = np.asarray(adj, np.float64)
    return adj / np.maximum(np.abs(adj).sum(-1, keepdims=True), 1e-12)


def nbr_mean(z, adj, bias=None, relu=False):
    """the actor's aggregate, f64; the critic's is nbr_mean(z, np.ones_like(adj), ...) (normalize(ones_like(adj)): 1 / P everywhere)"""
    y = np.matmul(normalize_l1(adj), np.asarray(z, np.float64))     # torch.matmul(F.normalize(adj, p=1, dim=-1), hist)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    return np.maximum(y, 0.0) if relu else y


def scale(z, adj, bias=None):
    """sum_j |abar_ij| |z_j| + |bias|: the magnitude each output's rounding errors are relative to"""
    s = np.matmul(np.abs(normalize_l1(adj)), np.abs(np.asarray(z, np.float64)))
    return s + np.abs(np.asarray(bias, np.float64)) if bias is not None else s
