"""Test helper (no test in here): the fused MLP step of csrc/mlp_fused.hip - fc1 -> tanh -> fc2 -> tanh | relu -> heads,
one of the four minibatch losses, backward - as plain torch ops in any float dtype, float64 by default, on plain
`w1, b1, w2, b2, wh, bh` tensors.  The forward is the arithmetic of oracle/model_torch.mlp_forward, the losses are the
references the direct loss-kernel tests use (tests/test_minibatch_rows_gpu.py imports them from here) and, for the
discrete kind, oracle.model_torch.ppo_loss.

Also the shapes at which tests/test_mlp_fused_gpu.py calls the kernels and tests/test_mlp_float64_cpu.py checks the
input conditions (`CASES`, `make_case`), and the kernel's LDS rule restated (`lds_stride`, `mlp_lds_bytes`,
`mlp_supported`)."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import model_torch as R

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
VALUE, DISTIL, GAUSSIAN, PPO = 1, 2, 3, 4  # PPO_MLP_LOSS_* (include/ppo_amd.h)
N_STATS = {VALUE: 4, DISTIL: 4, GAUSSIAN: 8, PPO: 8}
# the statistics columns a loss kind fills with something else than zeros (the others are spare columns, written as 0)
LIVE_STATS = {VALUE: (0, 1, 2), DISTIL: (0, 1, 2, 3), GAUSSIAN: (0, 2, 3, 4, 6, 7), PPO: (0, 1, 2, 3, 4, 5, 6, 7)}


def value_loss_ref(z, ret, tvf_ret, w, c, dt):
    """include/ppo_amd.h, ppo_value_loss_f32: sum_i vf_coef (V_i - R_i)^2 + tvf_coef 0.5 sqrt(K) mean_k w_k (T_k - P_k)^2
    per sample -> (d sum_b grad_scale loss_b / d heads, statistics [B, 4])."""
    z = z.to(dt).requires_grad_(True)
    V = z[:, c["value_col"]:c["value_col"] + c["vh"]]
    P = z[:, c["tvf_col"]:c["tvf_col"] + c["K"] * c["stride"]:c["stride"]]
    vloss = (c["vf_coef"] * (V - ret.to(dt)) ** 2).sum(1)
    tloss = c["tvf_coef"] * 0.5 * math.sqrt(c["K"]) * (w.to(dt) * (tvf_ret.to(dt) - P) ** 2).mean(1)
    (c["grad_scale"] * (vloss + tloss).sum()).backward()
    stats = torch.stack([vloss, tloss, vloss + tloss, torch.zeros_like(vloss)], 1).detach()
    return z.grad, stats


def distil_loss_ref(z, targets, old, w, log_std, c, dt):
    """include/ppo_amd.h, ppo_distil_loss_f32: 0.5 w_k (T_k - P_k)^2 [sqrt(n_pred) mean_k] + beta x policy term, the
    policy term KL(new || old) on log-probabilities, or (log_std given) 2 x 0.5 mean_a (mu_old - mu)^2 / (1e-5 + 2
    sigma_a^2) -> (d sum_b grad_scale loss_b / d heads, statistics [B, 4])."""
    z = z.to(dt).requires_grad_(True)
    nA, n = c["nA"], c["n_pred"]
    P = z[:, c["pred_col"]:c["pred_col"] + n * c["stride"]:c["stride"]]
    w = torch.ones(n, dtype=dt) if w is None else w.to(dt)
    diff = P - targets.to(dt).reshape(-1, n)
    vscale = math.sqrt(n) / n if c["vector"] else 1.0
    vloss = (0.5 * vscale * w * diff ** 2).sum(1)
    if log_std is None:
        lp = F.log_softmax(z[:, :nA], dim=1)
        pol = (lp.exp() * (lp - old.to(dt))).sum(1)
    else:
        den = 1e-5 + 2.0 * torch.exp(log_std.to(dt)) ** 2
        pol = 2.0 * (0.5 * (old.to(dt) - z[:, :nA]) ** 2 / den).mean(1)
    total = vloss + c["beta"] * pol
    (c["grad_scale"] * total.sum()).backward()
    stats = torch.stack([vloss, c["beta"] * pol, total, ((w * diff) ** 2).mean(1)], 1).detach()
    return z.grad, stats


def gaussian_loss_ref(z, act, old, adv, ret, log_std, c, dt):
    """include/ppo_amd.h, ppo_gaussian_loss_f32: gain_b = mean_a min(rho_a A, clip(rho_a) A) - sum_heads vf_coef (V - R)^2,
    rho_a = exp(log N(a_a; mu_a, sigma_a) - old_log_pac_a); loss = -gain -> (d sum_b grad_scale loss_b / d heads,
    the same per sample / d log_std [B, nA], statistics [B, 8], rho [B, nA])."""
    z = z.to(dt).requires_grad_(True)
    nA, vh, eps = c["nA"], c["vh"], c["eps"]
    ls = log_std.to(dt).expand(z.shape[0], nA).clone().requires_grad_(True)  # one copy per sample: per-sample gradients
    mu = z[:, :nA]
    logpac = -((act.to(dt) - mu) ** 2) / (2.0 * torch.exp(ls) ** 2) - ls - LOG_SQRT_2PI
    rho = torch.exp(logpac - old.to(dt))
    A = adv.to(dt)[:, None]
    loss_clip = torch.min(rho * A, torch.clamp(rho, 1 - eps, 1 + eps) * A).mean(1)
    vloss = (c["vf_coef"] * (z[:, nA:nA + vh] - ret.to(dt)) ** 2).sum(1)
    gain = loss_clip - vloss
    (c["grad_scale"] * (-gain).sum()).backward()
    zero = torch.zeros_like(gain)
    stats = torch.stack([loss_clip, zero, vloss, (torch.abs(rho - 1.0) > eps).to(dt).mean(1),
                         (old.to(dt) - logpac).mean(1), zero, gain, rho.mean(1)], 1).detach()
    return z.grad, ls.grad, stats, rho.detach()


def ppo_loss_ref(z, actions, old_log_pac, old_log_policy, adv, ret, c, dt):
    """include/ppo_amd.h, ppo_ppo_loss_f32 with one value head: oracle.model_torch.ppo_loss (the mean over the minibatch
    of -gain x loss_scale, so loss_scale = grad_scale x B makes it sum_b grad_scale loss_b) -> (d / d heads, statistics
    [B, 8] in the order of ST_* in csrc/loss_rows.h, rho [B])."""
    z = z.to(dt).requires_grad_(True)
    nA, eps, B = c["nA"], c["eps"], z.shape[0]
    assert c["vh"] == 1
    lp = F.log_softmax(z[:, :nA], dim=1)
    out = {"log_policy": lp, "value": z[:, nA:nA + 1]}
    old, A = old_log_pac.to(dt), adv.to(dt)
    R.ppo_loss(out, actions.long(), old, A, ret.to(dt), eps=eps, ent_coef=c["ent_coef"], vf_coef=c["vf_coef"],
               loss_scale=c["grad_scale"] * B).backward()
    with torch.no_grad():
        logpac = lp[torch.arange(B), actions.long()]
        rho = torch.exp(logpac - old)
        loss_clip = torch.min(rho * A, torch.clamp(rho, 1 - eps, 1 + eps) * A)
        entropy = -(lp.exp() * lp).sum(1)
        vloss = c["vf_coef"] * (z[:, nA] - ret.to(dt)[:, 0]) ** 2
        kl_true = (lp.exp() * (lp - old_log_policy.to(dt))).sum(1)
        stats = torch.stack([loss_clip, entropy, vloss, (torch.abs(rho - 1.0) > eps).to(dt), old - logpac, kl_true,
                             loss_clip + c["ent_coef"] * entropy - vloss, rho], 1)
    return z.grad, stats, rho


def mlp_reference(params, x, act, relu_gate=None):
    """params: (w1 [H, F], b1 [H], w2 [H, H], b2 [H], wh [NH, H], bh [NH] or None), x [B, F], one dtype throughout; act:
    "tanh" | "relu", the encoder activation behind fc2.  relu_gate (bool [B, H], relu only): the ReLU mask is taken from
    it and not re-decided (the shared kinks of oracle.model_torch.forward_shared_kinks).  Autograd runs through to
    whichever of `params` require gradients.  -> dict(a1, h_pre, hact, heads)."""
    w1, b1, w2, b2, wh, bh = params
    a1 = torch.tanh(F.linear(x, w1, b1))
    h_pre = F.linear(a1, w2, b2)
    if act == "tanh":
        hact = torch.tanh(h_pre)
    elif relu_gate is None:
        hact = F.relu(h_pre)
    else:
        hact = h_pre * relu_gate.to(h_pre.dtype)
    return {"a1": a1, "h_pre": h_pre, "hact": hact, "heads": F.linear(hact, wh, bh)}


def mlp_step_reference(params, x, act, kind, c, rows, log_std=None, dt=torch.float64, relu_gate=None):
    """One training minibatch: forward, the loss `kind` with configuration `c` on the per-sample arrays `rows` (the B
    gathered rows, in the argument order of the loss reference), backward through heads.backward(dL / d heads).
    -> dict(a1, h_pre, hact, heads, dheads, stats [B, n], stat_sums [n], dlog_std_rows [B, nA] | None, dlog_std [nA] |
    None, rho | None, grads: [dw1, db1, dw2, db2, dwh, dbh | None]), everything in `dt`."""
    leaves = [None if p is None else p.detach().to(dt).clone().requires_grad_(True) for p in params]
    fwd = mlp_reference(leaves, x.to(dt), act, relu_gate)
    z = fwd["heads"].detach()
    rows_ls, rho = None, None
    if kind == VALUE:
        if c["K"] > 0:
            dheads, stats = value_loss_ref(z, rows[0], rows[1], c["w"], c, dt)
        else:  # no TVF heads (the mean over none of them is undefined): one stand-in head at coefficient 0
            cc = dict(c, K=1, stride=1, tvf_col=0, tvf_coef=0.0)
            dheads, stats = value_loss_ref(z, rows[0], torch.zeros(z.shape[0], 1), torch.ones(1), cc, dt)
    elif kind == DISTIL:
        dheads, stats = distil_loss_ref(z, rows[0], rows[1], c["w"], log_std, c, dt)
    elif kind == GAUSSIAN:
        dheads, rows_ls, stats, rho = gaussian_loss_ref(z, rows[0], rows[1], rows[2], rows[3], log_std, c, dt)
    else:
        dheads, stats, rho = ppo_loss_ref(z, rows[0], rows[1], rows[2], rows[3], rows[4], c, dt)
    fwd["heads"].backward(dheads)
    out = {k: v.detach() for k, v in fwd.items()}
    out.update(dheads=dheads, stats=stats, stat_sums=stats.sum(0), dlog_std_rows=rows_ls,
               dlog_std=None if rows_ls is None else rows_ls.sum(0), rho=rho,
               grads=[None if p is None else p.grad for p in leaves])
    return out


# ---------------------------------------------------------------------------------------------- the kernel's LDS rule
def lds_stride(n):
    """csrc/mlp_fused.hip: a row of n floats, padded to 16 and then to a stride of 4 (mod 32) floats."""
    v = (n + 15) // 16 * 16
    return v + ((4 - v % 32) + 32) % 32


def mlp_lds_bytes(F_, H, NH, train=True):
    ldx, ldh, ldo = lds_stride(F_), lds_stride(H), lds_stride(NH)
    fl = 16 * (ldx + 2 * ldh + ldo) + (16 * (ldo + 2 * ldh) if train else 16 * ldh)
    return (fl + 16 * 64) * 4


def mlp_supported(F_, H, NH):
    return F_ > 0 and H > 0 and NH > 0 and H % 16 == 0 and mlp_lds_bytes(F_, H, NH) <= 160 * 1024


# ---------------------------------------------------------------------------------------------- the cases
# name -> shape, minibatch rows, loss kind and its configuration (the keys the loss references read), generator seed.
# The smallest shapes that reach each tiling path of the kernels (tests/test_mlp_fused_gpu.py says which); every loss
# kind occurs with more than 128 rows and with a ragged last tile of rows.
CASES = {
    "tiny-1": dict(F=1, H=16, NH=1, act="tanh", B=1, kind=VALUE, head_bias=False, seed=1,
                   c=dict(value_col=0, vh=1, tvf_col=0, K=0, stride=1, vf_coef=0.5, tvf_coef=0.0, grad_scale=0.37)),
    "tiny-17": dict(F=1, H=16, NH=1, act="tanh", B=17, kind=VALUE, head_bias=False, seed=2,
                    c=dict(value_col=0, vh=1, tvf_col=0, K=0, stride=1, vf_coef=0.5, tvf_coef=0.0, grad_scale=0.37)),
    "ragged-F-33": dict(F=13, H=64, NH=7, act="relu", B=33, kind=DISTIL, head_bias=True, seed=3,
                        c=dict(nA=3, pred_col=5, n_pred=1, stride=1, vector=0, beta=0.8, grad_scale=0.37)),
    "ragged-F-145": dict(F=13, H=64, NH=7, act="relu", B=145, kind=DISTIL, head_bias=True, seed=4,
                         c=dict(nA=3, pred_col=5, n_pred=1, stride=1, vector=0, beta=0.8, grad_scale=0.37)),
    "ragged-F-gauss": dict(F=13, H=64, NH=7, act="relu", B=37, kind=GAUSSIAN, head_bias=True, seed=5,
                           c=dict(nA=3, vh=2, eps=0.2, vf_coef=0.5, grad_scale=0.37)),
    "wide-hidden": dict(F=24, H=512, NH=20, act="tanh", B=130, kind=VALUE, head_bias=True, seed=6,
                        c=dict(value_col=2, vh=2, tvf_col=6, K=6, stride=2, vf_coef=0.5, tvf_coef=0.7, grad_scale=0.37)),
    "wide-heads": dict(F=530, H=272, NH=260, act="relu", B=300, kind=PPO, head_bias=True, seed=7,
                       c=dict(nA=15, vh=1, eps=0.2, ent_coef=0.01, vf_coef=0.5, grad_scale=0.37)),
    "humanoid": dict(F=377, H=256, NH=163, act="tanh", B=256, kind=GAUSSIAN, head_bias=True, seed=15,
                     c=dict(nA=17, vh=1, eps=0.2, vf_coef=0.5, grad_scale=0.37)),
}
REFUSED_SHAPE = (530, 512, 260)  # every field valid, 208640 bytes of LDS
SOURCE_FACTOR = 3                # the indexed calls read their rows out of a source of 3 B rows


def used_columns(case):
    """bool [NH]: the head columns the case's loss reads."""
    c, kind = case["c"], case["kind"]
    used = torch.zeros(case["NH"], dtype=torch.bool)
    if kind == VALUE:
        used[c["value_col"]:c["value_col"] + c["vh"]] = True
        used[c["tvf_col"]:c["tvf_col"] + c["K"] * c["stride"]:c["stride"]] = True
    elif kind == DISTIL:
        used[:c["nA"]] = True
        used[c["pred_col"]:c["pred_col"] + c["n_pred"] * c["stride"]:c["stride"]] = True
    else:
        used[:c["nA"] + c["vh"]] = True
    return used


def _moving_selection(B, g):
    """[B] rows of a source of SOURCE_FACTOR * B rows, all different, none at its own position."""
    n = B * SOURCE_FACTOR
    order = torch.randperm(n, generator=g)
    perm = torch.empty(n, dtype=torch.int64)
    perm[order] = order.roll(-1)  # one cycle: every row moves
    return perm[:B].contiguous()


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The seeded float32 tensors of CASES[name] (never modified by a test): params, log_std, the source `x_big`
    [3 B, F] and per-sample arrays `big` (each [3 B, ...]), `idx` [B] into them, the gathered `x` and `rows`, and the
    float64 step `ref` of the gathered minibatch.  Weights are N(0, 1 / fan_in) x 1.3, biases N(0, 0.1): activations of
    order one, tanh away from saturation.  Actions and old log-probabilities of the two policy kinds are built as in
    test_gaussian_loss_index_against_float64: around the new policy, so that the ratios straddle the clip range."""
    case = dict(CASES[name])
    F_, H, NH, B, kind, c = case["F"], case["H"], case["NH"], case["B"], case["kind"], dict(case["c"])
    g = torch.Generator().manual_seed(1000 + case["seed"])

    def rn(*shape, s=1.0):
        return torch.randn(*shape, generator=g) * s

    params = [rn(H, F_, s=1.3 / math.sqrt(F_)), rn(H, s=0.1), rn(H, H, s=1.3 / math.sqrt(H)), rn(H, s=0.1),
              rn(NH, H, s=1.3 / math.sqrt(H)), rn(NH, s=0.1) if case["head_bias"] else None]
    Bt = B * SOURCE_FACTOR
    x_big = rn(Bt, F_)
    idx = _moving_selection(B, g)
    x = x_big[idx].contiguous()
    with torch.no_grad():
        z = mlp_reference([None if p is None else p.double() for p in params], x.double(), case["act"])["heads"].float()
    log_std = None
    if kind == VALUE:
        c["w"] = torch.rand(c["K"], generator=g) + 0.25 if c["K"] else None
        big = [rn(Bt, c["vh"])] + ([rn(Bt, c["K"], s=2.0)] if c["K"] else [])
    elif kind == DISTIL:
        c["w"] = None
        big = [rn(Bt, c["n_pred"], s=2.0), F.log_softmax(rn(Bt, c["nA"], s=1.5), dim=1)]
    elif kind == GAUSSIAN:
        nA = c["nA"]
        log_std = rn(nA, s=0.5)
        act_big, adv_big, ret_big, old_big = rn(Bt, nA, s=1.5), rn(Bt), rn(Bt, c["vh"]), rn(Bt, nA)
        act_big[idx] = z[:, :nA] + torch.exp(log_std) * 1.5 * rn(B, nA)
        new_lp = -((act_big[idx] - z[:, :nA]) ** 2) / (2.0 * torch.exp(log_std) ** 2) - log_std - LOG_SQRT_2PI
        old_big[idx] = new_lp + 0.3 * rn(B, nA)
        big = [act_big, old_big, adv_big, ret_big]
    else:
        nA = c["nA"]
        act_big = torch.randint(0, nA, (Bt,), generator=g).int()
        adv_big, ret_big, old_big = rn(Bt), rn(Bt, 1), rn(Bt)
        oldpol_big = F.log_softmax(rn(Bt, nA, s=1.5), dim=1)
        new_lp = F.log_softmax(z[:, :nA], dim=1)
        old_big[idx] = new_lp[torch.arange(B), act_big[idx].long()] + 0.3 * rn(B)
        oldpol_big[idx] = F.log_softmax(z[:, :nA] + 0.5 * rn(B, nA), dim=1)
        big = [act_big, old_big, oldpol_big, adv_big, ret_big]
    rows = [t[idx].contiguous() for t in big]
    case.update(name=name, c=c, params=params, log_std=log_std, x_big=x_big, big=big, idx=idx, x=x, rows=rows,
                n_stats=N_STATS[kind], used=used_columns(case))
    case["ref"] = mlp_step_reference(params, x, case["act"], kind, c, rows, log_std)
    return case
