"""numpy restatement -- and the specification -- of the direction-vector action head of the env_3d policy (algo.gauss_squash: direction;
csrc/direction_action.hpp), in f64.

The policy is a diagonal Gaussian over u = (u_x, u_y, u_z, s), u = mu + exp(ls) z with the noise of gauss_ref.normals(..., A=4).  The
environment receives, in f64 from the fp32 u,
    a0 = atan2(u_y, u_x) / pi,   a1 = atan2(u_z, hypot(u_x, u_y)) / (pi / 2),   a2 = s,   each clamped to [-1, 1]
(divisions by the f64 constants: atan2(+0, -1) / pi is exactly 1).  The log-probability is the plain Normal log-density of u over its
four dimensions -- the action of the MDP is u and the map is part of the environment, so there is no Jacobian term -- and the entropy
is the latent Gaussian's.  The teacher's label of a guidance action g = (heading / pi, pitch / (pi / 2), speed) is
    (cos gam cos phi, cos gam sin phi, sin gam, g2),   phi = g0 pi, gam = g1 pi / 2,   in f64, rounded to fp32.
"""
import numpy as np

from tests import gauss_sd_ref

LATENT, ENV_A = 4, 3

# u -> the exact environment action (IEEE conventions of atan2 at the edges)
EDGES = [((-1.0, +0.0, 0.0, 0.25), (1.0, 0.0, 0.25)),
         ((-1.0, -0.0, 0.0, 0.25), (-1.0, 0.0, 0.25)),
         ((0.0, 0.0, 0.0, 2.0), (0.0, 0.0, 1.0)),
         ((0.0, 0.0, 1.0, -3.0), (0.0, 1.0, -1.0)),
         ((0.0, 1.0, 0.0, 0.25), (0.5, 0.0, 0.25))]


def to_env(u):
    """u (..., 4) as fp32 values -> (..., 3) f64"""
    u = np.asarray(u, np.float32).astype(np.float64)
    a0 = np.arctan2(u[..., 1], u[..., 0]) / np.pi
    a1 = np.arctan2(u[..., 2], np.hypot(u[..., 0], u[..., 1])) / (np.pi / 2)
    return np.clip(np.stack([a0, a1, u[..., 3]], -1), -1.0, 1.0)


def label(g):
    """guidance actions g (..., 3) f64 -> labels (..., 4) fp32"""
    g = np.asarray(g, np.float64)
    phi, gam = g[..., 0] * np.pi, g[..., 1] * np.pi / 2
    cg = np.cos(gam)
    return np.stack([cg * np.cos(phi), cg * np.sin(phi), np.sin(gam), g[..., 2]], -1).astype(np.float32)


def angle(mu, d):
    """the angle in radians between mu[..., :3] and d[..., :3], f64: atan2(|mu x d|, mu . d); pi / 2 where |mu[:3]|^2 is 0"""
    m, d = np.asarray(mu, np.float64)[..., :3], np.asarray(d, np.float64)[..., :3]
    ang = np.arctan2(np.linalg.norm(np.cross(m, d), axis=-1), (m * d).sum(-1))
    return np.where((m * m).sum(-1) == 0.0, np.pi / 2, ang)


def head_sample(feat, W, b, log_std, seed, counter, greedy=False, lo=-np.inf, hi=np.inf):
    """-> (mu, ls_raw, z, u, logp) in f64 with A = 4: gauss_sd_ref.head_sample's clip mode without its environment action (the
    environment's is to_env of the fp32 u the kernel stores)"""
    assert np.asarray(W).shape[0] == LATENT
    mu, ls_raw, z, u, _, logp = gauss_sd_ref.head_sample(feat, W, b, log_std, seed, counter, greedy, lo, hi, "clip")
    return mu, ls_raw, z, u, logp


def ppo_loss(*args, squash="direction", **kw):
    """the PPO loss of the mode: gauss_sd_ref.ppo_loss on the latent u, no Jacobian term (squash "clip") -- one definition, so that the
    equality with clip at A = 4 is by construction and a test of it guards the construction"""
    assert squash == "direction"
    return gauss_sd_ref.ppo_loss(*args, squash="clip", **kw)


def e3d_select(guide, follow, env_action):
    """guide, env_action (N, P, 3) f64, follow (N,) -> (labels (N, P, 4) fp32, the executed actions (N, P, 3) f64)"""
    guide = np.asarray(guide, np.float64)
    return label(guide), np.where(np.asarray(follow).astype(bool)[:, None, None], guide, np.asarray(env_action, np.float64))
