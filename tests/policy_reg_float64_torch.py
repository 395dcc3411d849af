"""Test helper (no test in here): the two regularisers of the policy phase as plain torch ops in any float dtype, float64
by default, with the closed forms of their gradients beside the autograd ones.

  policy_kl_ref     the global KL row (include/ppo_amd.h, ppo_policy_kl_loss_f32; rl/rollout.py:1723-1738)
  ppo_side_ref      the discrete PPO loss with SIDE (ppo_ppo_loss_side_f32; rl/rollout.py:1640-1682, 1744-1753)
  policy_loss_ref   Runner.train_policy_minibatch's loss of one minibatch with either or both: mean_b(-gain_b) x loss_scale,
                    where gkl_loss = penalty x global_kl comes off every sample's gain
  global_kl_ref     F.kl_div(merge_down(old), merge_down(new), reduction="batchmean", log_target=True): the arrays are
                    flattened to [S * nA] first, so "batchmean" divides by S * nA
"""
import torch
import torch.nn.functional as F


def tilted_log_policy(logits, g):
    """An old policy that is not the new one, as make_inputs of tests/test_distil_modes_gpu.py builds it: the new logits
    tilted by -2 .. 2 over the actions plus N(0, 0.3^2), never a policy that happens to lie next to the new one.  With old
    = new the KL and its gradient are zero and a comparison shows nothing; and the KL is a sum of terms of both signs that
    float32 carries to ~1e-7 of its largest TERM, so two nearly equal policies would ask the statistic - for B = 1 the
    bar is relative to the one sample's own KL - for digits no float32 sum of those terms has."""
    B, nA = logits.shape
    tilt = torch.linspace(-2.0, 2.0, nA) + 0.3 * torch.randn(B, nA, generator=g)
    return F.log_softmax(logits.float() + tilt, dim=1)


def global_kl_ref(new_lp, old_lp):
    """The reference's global_kl of new / old log-policies [S, nA] (rl/rollout.py:1728-1731)."""
    return F.kl_div(old_lp.reshape(-1), new_lp.reshape(-1), reduction="batchmean", log_target=True)


def policy_kl_ref(z, old, nA, grad_scale, dt=torch.float64):
    """-> (d sum_b grad_scale kl_b / d heads [B, ldo], kl_b [B]) by autograd on heads z [B, ldo]."""
    z = z.to(dt).requires_grad_(True)
    lp = F.log_softmax(z[:, :nA], dim=1)
    kl = (lp.exp() * (lp - old.to(dt))).sum(1)
    (grad_scale * kl.sum()).backward()
    return z.grad, kl.detach()


def policy_kl_closed_form(z, old, nA, grad_scale, dt=torch.float64):
    """dheads[b, a] = grad_scale p_a ((lp_a - old_a) - kl_b), zeros in the columns past nA."""
    z = z.to(dt)
    lp = F.log_softmax(z[:, :nA], dim=1)
    p, d = lp.exp(), lp - old.to(dt)
    kl = (p * d).sum(1, keepdim=True)
    g = torch.zeros_like(z)
    g[:, :nA] = grad_scale * p * (d - kl)
    return g, kl[:, 0]


def _ppo_terms(z, actions, old_log_pac, adv, ret, c, dt):
    nA, vh, eps, B = c["nA"], c["vh"], c["eps"], z.shape[0]
    lp = F.log_softmax(z[:, :nA], dim=1)
    logpac = lp[torch.arange(B), actions.long()]
    rho = torch.exp(logpac - old_log_pac.to(dt))
    A = adv.to(dt)
    loss_clip = torch.min(rho * A, torch.clamp(rho, 1 - eps, 1 + eps) * A)
    entropy = -(lp.exp() * lp).sum(1)
    vloss = (c["vf_coef"] * (z[:, nA:nA + vh] - ret.to(dt).reshape(B, vh)) ** 2).sum(1) if vh else torch.zeros(B, dtype=dt)
    return lp, logpac, rho, loss_clip, entropy, vloss


def ppo_side_ref(z, actions, old_log_pac, old_log_policy, adv, ret, target, c, dt=torch.float64):
    """-> (d sum_b grad_scale (-gain_b) / d heads, statistics [B, 8] in the order of ST_* in csrc/loss_rows.h with the SIDE
    gain in the gain column, kl_penalty [B]); gain_b = loss_clip - ent_coef (KL(new || target) - H) - value loss."""
    z = z.to(dt).requires_grad_(True)
    lp, logpac, rho, loss_clip, entropy, vloss = _ppo_terms(z, actions, old_log_pac, adv, ret, c, dt)
    kl_penalty = (lp.exp() * (lp - target.to(dt)[None, :])).sum(1) - entropy
    gain = loss_clip - c["ent_coef"] * kl_penalty - vloss
    (c["grad_scale"] * (-gain).sum()).backward()
    with torch.no_grad():
        kl_true = (lp.exp() * (lp - old_log_policy.to(dt))).sum(1)
        stats = torch.stack([loss_clip, entropy, vloss, (torch.abs(rho - 1.0) > c["eps"]).to(dt), old_log_pac.to(dt) - logpac,
                             kl_true, gain, rho], 1)
    return z.grad, stats.detach(), kl_penalty.detach()


def ppo_side_closed_form(z, actions, old_log_pac, adv, ret, target, c, dt=torch.float64):
    """d(-gain)/dz_j = -[ w (1{j=act} - p_j) + c ( -2 p_j (lp_j + H) + p_j (t_j - sum p t) ) ] on the policy columns, w =
    d loss_clip / d rho x rho as in ppo_loss_row_z; 2 vf_coef (V - R) on the value columns; times grad_scale."""
    z = z.to(dt)
    nA, vh, eps, B = c["nA"], c["vh"], c["eps"], z.shape[0]
    with torch.no_grad():
        lp, logpac, rho, loss_clip, entropy, vloss = _ppo_terms(z, actions, old_log_pac, adv, ret, c, dt)
        A, t = adv.to(dt), target.to(dt)
        s1, s2 = rho * A, torch.clamp(rho, 1 - eps, 1 + eps) * A
        inside = (rho >= 1 - eps) & (rho <= 1 + eps)
        dclip = torch.where(inside, A, torch.where(s1 < s2, A, torch.where(s1 == s2, 0.5 * A, torch.zeros_like(A))))
        w = (dclip * rho)[:, None]
        p = lp.exp()
        onehot = F.one_hot(actions.long(), nA).to(dt)
        pt = (p * t).sum(1, keepdim=True)
        H = entropy[:, None]
        g = torch.zeros_like(z)
        g[:, :nA] = -(w * (onehot - p) + c["ent_coef"] * (-2 * p * (lp + H) + p * (t[None, :] - pt)))
        if vh:
            g[:, nA:nA + vh] = 2 * c["vf_coef"] * (z[:, nA:nA + vh] - ret.to(dt).reshape(B, vh))
    return c["grad_scale"] * g


def policy_loss_ref(z, gz, data, c, dt=torch.float64):
    """Runner.train_policy_minibatch (rl/rollout.py:1610-1771) on the minibatch's heads z [B, ldo] and the global states'
    heads gz [S, ldo] (None without the global KL).  data: actions, log_pac, advantages, returns, and - as the
    configuration c asks - global_log_policy, side_target_logp.  c: nA, vh, eps, ent_coef, vf_coef, loss_scale, side (bool),
    gkl_penalty (None = no global KL).  -> (loss, global_kl or None, d loss / d z, d loss / d gz or None)."""
    z = z.to(dt).requires_grad_(True)
    lp, _logpac, _rho, loss_clip, entropy, vloss = _ppo_terms(z, data["actions"], data["log_pac"], data["advantages"],
                                                              data["returns"], c, dt)
    gain = loss_clip
    if c["side"]:
        gain = gain - c["ent_coef"] * ((lp.exp() * (lp - data["side_target_logp"].to(dt)[None, :])).sum(1) - entropy)
    else:
        gain = gain + c["ent_coef"] * entropy
    global_kl = None
    if c["gkl_penalty"] is not None:
        gz = gz.to(dt).requires_grad_(True)
        global_kl = global_kl_ref(F.log_softmax(gz[:, :c["nA"]], dim=1), data["global_log_policy"].to(dt))
        if c["gkl_penalty"] != 0:
            gain = gain - c["gkl_penalty"] * global_kl
    gain = gain - vloss
    loss = ((-gain) * c["loss_scale"]).mean()
    loss.backward()
    ggz = None if global_kl is None else (gz.grad if gz.grad is not None else torch.zeros_like(gz))
    return float(loss.detach()), None if global_kl is None else float(global_kl.detach()), z.grad, ggz
