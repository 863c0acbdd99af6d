"""float64 reference of one DHGN relation message + mean (include/mappo_ops.h, dhgn_msg_agg_*), plain numpy.

    z_ij  = W[:, :4] (p_i - q_j) (+ W[:, 4:8] (p_i - e)) + b
    out_i = sum_j abar_ij relu(z_ij),    abar = adj / max(sum_j |adj|, 1e-12)

The (R, P, K, E) pre-activation is materialised in row chunks, so memory stays bounded whatever R is.

The weight gradient of a ReLU message is discontinuous at z = 0: an fp32 kernel and this reference may legitimately disagree on
[z > 0] where |z| is below the fp32 evaluation error of z.  The reference therefore also returns an AMBIGUITY BUDGET per gradient
element.  An entry is ambiguous when |z_ij| < guard_ij,

    guard_ij = 2^-19 (|b| + sum_k |W_k| (|p_k| + |q_k|) [+ sum_k |W_4+k| (|p_k| + |e_k|)])

-- sixteen fp32 ulps (2^-23) of the magnitudes that enter z, i.e. a few roundings of each of the up to nine terms; derived from the
arithmetic, not tuned -- and the budget of a gradient element is  amb = sum over ambiguous entries of |g_ij| |x|  with g_ij the
entry's upstream weight (abar_ij gout_i, plus gout_critic_i / K in the pair form) and x its input coordinate (1 for db): what the
element moves by if every ambiguous entry is decided the other way.
"""
import numpy as np

GUARD = 2.0 ** -19
CHUNK_ENTRIES = 1 << 21       # (rows, P, K, E) entries materialised at once


def f64(t):
    """torch tensor / array -> float64 numpy array (exact for fp32 inputs)"""
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def abar(source, R, P, K, adj=None, kvalid=None, q_div=1):
    """the normalised weights (R, P, K) of an adjacency source: 'tensor' (adj: any float adjacency), 'ones' (all K neighbours),
    'valid' (ones over the first kvalid[r // q_div] neighbours)"""
    if source == "tensor":
        a = f64(adj).reshape(R, P, K)
        return a / np.maximum(np.abs(a).sum(-1, keepdims=True), 1e-12)
    if source == "ones":
        return np.full((R, P, K), 1.0 / max(K, 1e-12)) if K else np.zeros((R, P, 0))
    if source == "valid":
        kv = np.repeat(np.asarray(kvalid, dtype=np.int64).reshape(-1), q_div)[:R]
        a = (np.arange(K)[None, :] < kv[:, None]).astype(np.float64)
        a = a / np.maximum(a.sum(-1, keepdims=True), 1e-12)
        return np.broadcast_to(a[:, None, :], (R, P, K)).copy()
    raise ValueError(source)


def relation(p, q, e, W, b, abars, jobs=(), q_div=1, chunk_entries=CHUNK_ENTRIES):
    """One relation for several weightings of the same messages.
    p (R, P, 4); q (R / q_div, K, 4); e (R, 4) or None (din = 4); W (E, din); b (E,);
    abars: list of (R, P, K) normalised weights (see abar());
    jobs: gradient jobs, each a list of (index into abars, gout (R, P, E)) terms whose upstream weights add up -- one term: a single
          network; the pair form: [(actor's abar, gout_actor), (ones, gout_critic)].
    -> dict(out=[(R, P, E) per abar], fwd_amb=[(R, P, E) per abar], grads=[dict(dW, db, amb_W, amb_b) per job]);
       fwd_amb: sum over ambiguous entries of |abar_ij| |z_ij| -- what an output moves by if they are decided the other way."""
    p, q, e, W, b = f64(p), f64(q), f64(e), f64(W), f64(b)
    R, P = p.shape[:2]
    K = q.shape[1]
    E, din = W.shape
    assert din == (8 if e is not None else 4) and q.shape[0] * q_div == R
    outs = [np.zeros((R, P, E)) for _ in abars]
    fambs = [np.zeros((R, P, E)) for _ in abars]
    grads = [dict(dW=np.zeros((E, din)), db=np.zeros(E), amb_W=np.zeros((E, din)), amb_b=np.zeros(E)) for _ in jobs]
    if K == 0 or R == 0:
        return dict(out=outs, fwd_amb=fambs, grads=grads)
    aW, ab = np.abs(W), np.abs(b)
    step = max(1, chunk_entries // (P * K * E))
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        n = r1 - r0
        pc = p[r0:r1]
        qc = q[np.arange(r0, r1) // q_div]
        x = pc[:, :, None, :] - qc[:, None, :, :]                           # (n, P, K, 4)
        mag = np.abs(pc)[:, :, None, :] + np.abs(qc)[:, None, :, :]
        if din == 8:
            ec = e[r0:r1]
            x = np.concatenate((x, np.broadcast_to((pc - ec[:, None, :])[:, :, None, :], (n, P, K, 4))), -1)
            mag = np.concatenate((mag, np.broadcast_to((np.abs(pc) + np.abs(ec)[:, None, :])[:, :, None, :], (n, P, K, 4))), -1)
        z = x @ W.T + b                                                     # (n, P, K, E)
        ambiguous = np.abs(z) < GUARD * (mag @ aW.T + ab)
        act = np.maximum(z, 0.0)
        pos = z > 0
        zamb = np.where(ambiguous, np.abs(z), 0.0)
        for k, a in enumerate(abars):
            ac = a[r0:r1]
            outs[k][r0:r1] = np.einsum("npk,npke->npe", ac, act)
            fambs[k][r0:r1] = np.einsum("npk,npke->npe", np.abs(ac), zamb)
        ax = np.abs(x)
        for job, g in zip(jobs, grads):
            up = np.zeros((n, P, K, E))
            for k, gout in job:
                up += abars[k][r0:r1][..., None] * f64(gout)[r0:r1][:, :, None, :]
            gm = np.where(pos, up, 0.0)
            g["dW"] += np.einsum("npke,npkd->ed", gm, x)
            g["db"] += gm.sum((0, 1, 2))
            ga = np.where(ambiguous, np.abs(up), 0.0)
            g["amb_W"] += np.einsum("npke,npkd->ed", ga, ax)
            g["amb_b"] += ga.sum((0, 1, 2))
    return dict(out=outs, fwd_amb=fambs, grads=grads)


def msg_agg(p, q, e, W, b, source, adj=None, kvalid=None, q_div=1, gout=None, gout_ones=None):
    """one relation under one adjacency source; gout: its gradient job; gout_ones: the pair form (the critic's gout under ones over
    all K on top of the actor's under `source`).  -> dict(out, fwd_amb[, dW, db, amb_W, amb_b])"""
    R, P = p.shape[:2]
    K = q.shape[1]
    abars = [abar(source, R, P, K, adj, kvalid, q_div)]
    jobs = []
    if gout is not None:
        job = [(0, gout)]
        if gout_ones is not None:
            abars.append(abar("ones", R, P, K))
            job.append((1, gout_ones))
        jobs.append(job)
    res = relation(p, q, e, W, b, abars, jobs, q_div)
    out = dict(out=res["out"][0], fwd_amb=res["fwd_amb"][0])
    if jobs:
        out.update(res["grads"][0])
    return out


def pos_part(p, Wp, bp):
    """the position part of DHGN's semantic layer: bp + Wp p, (R, P, E)"""
    return f64(p) @ f64(Wp).T + f64(bp)


FWD_ATOL = FWD_RTOL = 2e-5
GRAD_RTOL = 2e-4


def fwd_err(dev, ref):
    """max of |dev - ref| in units of the forward bound 2e-5 + 2e-5 |ref|"""
    dev = f64(dev)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    assert np.isfinite(dev).all()
    return float((np.abs(dev - ref) / (FWD_ATOL + FWD_RTOL * np.abs(ref))).max())


def grad_err(dev, ref, amb):
    """max of |dev - ref| in units of the gradient bound 2e-4 max|ref| + amb (element-wise).  An exactly zero reference (an empty
    relation) leaves a zero bound: the device gradient must then be exactly zero."""
    dev = f64(dev)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    assert np.isfinite(dev).all()
    bound = GRAD_RTOL * np.abs(ref).max() + amb
    d = np.abs(dev - ref)
    zero = bound == 0
    if d[zero].any():
        return float("inf")
    return float((d[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
