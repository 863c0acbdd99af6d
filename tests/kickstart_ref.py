"""numpy restatement -- and the specification -- of the fused loss launches of teacher-regularised PPO (csrc/kickstart.hpp:
ppo_bc_loss_gauss_fwd_bwd, ppo_bc_loss_cat_fwd_bwd; algo.bc_coef), in f64.

A launch is the PPO launch of its policy plus coef times the imitation launch, on the same mu / ls_raw / prob and values:
    actor_loss = ppo.actor_loss + coef bc.actor_loss,   g_x = ppo.g_x + coef bc.g_x   for x in (mu, ls_raw) or prob,
the critic loss and g_v are the PPO launch's (the imitation launch has the same), and the three sums are the imitation launch's metric
sum (sum d^2, the angles, or the label hits), its live-row count, and sum_i active_i la_bc_i -- the unweighted imitation loss times the
count.  The eight update diagnostics are those of the PPO row (tests/ppo_diag_ref.py).  The parts are the existing specifications:
tests/gauss_sd_ref.ppo_loss, tests/imitation_ref.bc_loss_gauss / bc_loss_cat, and a categorical PPO row on gauss_sd_ref._ppo."""
import numpy as np

from tests import gauss_sd_ref as gs
from tests import imitation_ref as im
from tests import ppo_diag_ref as pd

P_EPS = im.P_EPS


def coef_at(coef, decay, iterations, j):
    """lambda_j of PPO iteration j (0-based): coef decay^j in Python floats, 0 once iterations > 0 and j >= iterations"""
    if coef <= 0.0 or j < 0 or (iterations > 0 and j >= iterations):
        return 0.0
    return coef * decay ** j


def angle_sum(mu, target, active):
    """sum_i active_i angle(mu_i[:3], target_i[:3]) in radians: atan2(|m x t|, m . t), pi / 2 where |m|^2 is 0"""
    m, t = np.asarray(mu, np.float64)[..., :3], np.asarray(target, np.float64)[..., :3]
    ang = np.arctan2(np.linalg.norm(np.cross(m, t), axis=-1), (m * t).sum(-1))
    ang = np.where((m * m).sum(-1) == 0.0, np.pi / 2, ang)
    return float((ang * np.asarray(active, np.float64)).sum())


def ppo_loss_cat(prob, action, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef, use_value_clip=True):
    """torch.distributions.Categorical(prob) -- renormalisation, probs_to_logits' clamp to [eps32, 1 - eps32], gather, entropy -- into
    the PPO row; -> (actor_loss, critic_loss, g_prob, g_v).  The clamp passes the gradient on its closed range."""
    prob = np.asarray(prob, np.float64)
    a = np.asarray(action).astype(np.int64)
    vn, lo_old, ad, act, vt = (np.asarray(x, np.float64) for x in (values_now, logp_old, adv, active, v_target))
    vo = None if values_old is None else np.asarray(values_old, np.float64)
    s = prob.sum(-1, keepdims=True)
    p = prob / s
    c = np.clip(p, P_EPS, 1.0 - P_EPS)
    l = np.log(c)
    onehot = np.arange(prob.shape[-1]) == a[..., None]
    lp, ent = (l * onehot).sum(-1), -(l * p).sum(-1)
    la, lc, g_lp, g_ent, g_v = gs._ppo(lp, ent, vn, lo_old, ad, act, vo, vt, eps, ent_coef, use_value_clip)
    passes = (p >= P_EPS) & (p <= 1.0 - P_EPS)
    gl = onehot * g_lp[..., None] - g_ent[..., None] * p                 # d / d logits: the gather, the entropy's logits * probs
    gp = np.where(passes, gl / c, 0.0) - g_ent[..., None] * l            # d / d probs
    return la, lc, (gp - (gp * p).sum(-1, keepdims=True)) / s, g_v       # through probs = prob / prob.sum(-1)


def _diag(lp, ent, logp_old, values_now, v_target, active, eps):
    lr = np.asarray(lp, np.float64) - np.asarray(logp_old, np.float64)
    return pd.sums(pd.row_terms(lr, np.exp(lr), ent, np.asarray(values_now, np.float64), np.asarray(v_target, np.float64), active, eps))


def ppo_bc_loss_gauss(mu, ls_raw, action, target, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef, coef,
                      use_value_clip=True, lo=-np.inf, hi=np.inf, squash="clip", fit_std=False, wrap0=False, metric="mse"):
    """shapes as gauss_sd_ref.ppo_loss / imitation_ref.bc_loss_gauss.  -> dict: actor_loss, critic_loss, g_mu, g_ls, g_v, sums (3,):
    the metric's sum (metric "angle": of angles, and wrap0 is ignored), the live rows, sum active la_bc; diag (8,)"""
    squash = "clip" if squash == "direction" else squash     # the map to the angles is the environment's: no Jacobian term
    wrap0 = wrap0 and metric != "angle"
    la, lc, g_mu, g_ls, g_v = gs.ppo_loss(mu, ls_raw, action, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef,
                                          use_value_clip, lo, hi, squash)
    bc = im.bc_loss_gauss(mu, ls_raw, target, values_now, active, values_old, v_target, eps, use_value_clip, lo, hi, fit_std, wrap0)
    msum = angle_sum(mu, target, active) if metric == "angle" else bc["sq_sum"]
    lp, ent = pd.gaussian(np.asarray(mu), np.asarray(ls_raw), np.asarray(action), lo, hi, squash == "tanh")
    return dict(actor_loss=la + coef * bc["actor_loss"], critic_loss=lc, g_mu=g_mu + coef * bc["g_mu"], g_ls=g_ls + coef * bc["g_ls"], g_v=g_v,
                sums=np.array([msum, bc["rows"], bc["actor_loss"] * bc["rows"]]),
                diag=_diag(lp, ent, logp_old, values_now, v_target, active, eps))


def ppo_bc_loss_cat(prob, action, label, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef, coef, use_value_clip=True):
    """-> dict: actor_loss, critic_loss, g_prob, g_v, sums (3,): the label hits, the live rows, sum active (-log p[label]); diag (8,)"""
    la, lc, g_prob, g_v = ppo_loss_cat(prob, action, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef, use_value_clip)
    bc = im.bc_loss_cat(prob, label, values_now, active, values_old, v_target, eps, use_value_clip)
    lp, ent = pd.categorical(np.asarray(prob), np.asarray(action))
    return dict(actor_loss=la + coef * bc["actor_loss"], critic_loss=lc, g_prob=g_prob + coef * bc["g_prob"], g_v=g_v,
                sums=np.array([bc["hits"], bc["rows"], bc["actor_loss"] * bc["rows"]]),
                diag=_diag(lp, ent, logp_old, values_now, v_target, active, eps))
