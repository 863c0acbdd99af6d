"""The specification of the env_3d actor's team attention (algo.e3d_comm: attention; include/mappo_ops.h team_*)
in torch, written as the formulas read: callable in float64 or float32, on the CPU or the GPU, differentiable by autograd; and the
mask rule in numpy.  No kernel of the package is called here."""
import numpy as np
import torch

E = 128
HEADS = (1, 2, 4, 8)


def comm_words(pp_adj, live):
    """pp_adj (G, P, P), live (G, P), anything non-zero is true -> (G, P) int64: bit j of word [g, i] iff j == i, or i and j are both
    live and pp_adj[g, i, j] and pp_adj[g, j, i] are both set"""
    pp_adj, live = np.asarray(pp_adj) != 0, np.asarray(live) != 0
    G, P = live.shape
    words = np.zeros((G, P), dtype=np.uint64)
    for g in range(G):
        for i in range(P):
            w = 1 << i
            for j in range(P):
                if live[g, i] and live[g, j] and pp_adj[g, i, j] and pp_adj[g, j, i]:
                    w |= 1 << j
            words[g, i] = w
    return words.view(np.int64)


def hand_made_masks():
    """(pp_adj, live, expected bit lists): an asymmetric adjacency, a dead pursuer in the middle, an all-dead group"""
    full = np.ones((3, 3), np.float32)
    asym = np.array([[1, 1, 0], [0, 1, 1], [0, 1, 1]], np.float32)         # 0 -> 1 without 1 -> 0: no link; 1 <-> 2 is one
    adj = np.stack([asym, full, full])
    live = np.array([[1, 1, 1], [1, 0, 1], [0, 0, 0]], np.float32)
    want = [[[0], [1, 2], [1, 2]], [[0, 2], [1], [0, 2]], [[0], [1], [2]]]
    return adj, live, want


def hears(words, P):
    """(G, P) int64 words -> (G, P, P) bool: [g, i, j] iff j is in M_i; bits at or above P are dropped and bit i is taken as set"""
    w = np.asarray(words).view(np.uint64)
    m = ((w[:, :, None] >> np.arange(P, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    return m | np.eye(P, dtype=bool)[None]


def attention(qkv, words, heads):
    """qkv (G P, 384) = q | k | v, words (G, P) int64 (numpy or torch) -> out (G P, 128), lse (G, H, P); head h is columns [h D, (h + 1) D)"""
    words = words.cpu().numpy() if torch.is_tensor(words) else np.asarray(words)
    G, P = words.shape
    D = E // heads
    M = torch.from_numpy(hears(words, P)).to(qkv.device)                    # (G, P, P)
    q, k, v = (qkv[:, n * E:(n + 1) * E].reshape(G, P, E) for n in range(3))
    out, lse = [], []
    for h in range(heads):
        qh, kh, vh = (t[:, :, h * D:(h + 1) * D] for t in (q, k, v))        # (G, P, D)
        s = (qh[:, :, None, :] * kh[:, None, :, :]).sum(-1) / D ** 0.5       # s[g, i, j] = q_i . k_j / sqrt(D)
        s = torch.where(M, s, torch.full_like(s, -float("inf")))
        smax = s.max(dim=2, keepdim=True).values
        p = torch.exp(s - smax)                                              # exactly 0 outside M_i
        l = p.sum(dim=2, keepdim=True)
        a = p / l
        out.append((a[:, :, :, None] * vh[:, None, :, :]).sum(2))            # o_i = sum_j a_ij v_j
        lse.append((smax + torch.log(l))[:, :, 0])
    return torch.cat(out, dim=2).reshape(G * P, E), torch.stack(lse, dim=1)


def attention_grads(qkv, words, heads, d_out):
    """-> (out, lse, d_qkv) of attention() under the upstream gradient d_out, in qkv's dtype on qkv's device"""
    x = qkv.detach().clone().requires_grad_(True)
    out, lse = attention(x, words, heads)
    out.backward(d_out)
    return out.detach(), lse.detach(), x.grad


def layer(emb, words, heads, w_qkv, b_qkv, w_out, b_out):
    """the whole layer on (G P, 128) embeddings: emb + out(attention(qkv(emb)))"""
    o, _ = attention(torch.nn.functional.linear(emb, w_qkv, b_qkv), words, heads)
    return emb + torch.nn.functional.linear(o, w_out, b_out)
