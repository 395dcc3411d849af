"""float64 references (numpy / torch on the CPU), data sets, float32 comparison evaluations and bars for the direct
tests of the discrete-policy kernels (csrc/policy.hip, policy_act.h, loss_rows.h), ppo_gaussian_act_f32
(csrc/heads_loss.hip), the optimiser (csrc/optim.hip) and the small batch operations (csrc/batch_ops.hip, ppo_colsum_f32
of csrc/gemm.hip).  tests/test_policy_float64_gpu.py, test_optim_float64_gpu.py and test_batch_ops_float64_gpu.py compare
the kernels with these; tests/test_policy_optim_float64_cpu.py checks, without a GPU, that the bars mean something.

Bars that follow from the arithmetic
  * ppo_moments_f64: a sum of n doubles (the float32 inputs and their squares are exact doubles) in any order is within
    (n - 1) u S (1 + O(n u)) of the exact sum, u = 2^-53, S = sum |x| (Higham, Accuracy and Stability, 4.2): the bar
    n 2^-52 S has a factor 2 to spare and no measured term.  The reference is math.fsum, exact.  The count is an integer.
  * ppo_accumulate_f32, ppo_mask_mul_f32: one float32 operation per element, correctly rounded: bit-equal to numpy.
  * ppo_axpy_f32: two correctly rounded operations, product then sum, not fused: bit-equal to numpy's float32
    dst + alpha * src.  axpy_data() plants elements where a fused multiply-add rounds differently.
  * actions, the greedy argmax, the 0 / 1 clipped column: integers, equal or not.  raw_policy / values: copies, bit-equal.

Bars that do not: everything with an expf / logf / sqrtf / division chain or a float32 summation tree of its own.  There
the bar is measured, not chosen: the same operation in plain float32 torch on the CPU on the same tensors against the
float64 reference, per element and relative to a local scale (below), its maximum times MULTIPLE = 4 (the margin the
convolution tests give a different summation tree and different expf / logf implementations).  A result cannot be
asked to be closer than its own rounding, so a bar is never below FLOOR = 2^-23 of the local scale (two roundings to
nearest of a value as large as the scale).  Local scales, so that a wrong small value cannot hide behind a large one:
  * log-probabilities: the row's 1 + max |z / T|;
  * loss gradient: the row's grad_scale (|adv| ratio + ent_coef + 2 vf_coef max |V - R|);
  * statistics: a column formed from the row's log-probabilities (entropy, kl_approx, kl_true, ratio, loss_clip, gain)
    takes their scale, 1 + max |z| (+ |old_log_pac|, max |old_log_policy| where they enter; times ratio, |adv| where the
    column is multiplied by them), value_loss 1 + itself (_loss_eval's stat_scales).  The kernels form lse = max + log(sum)
    before subtracting it, so a log-probability carries ulp(max |z|) where torch's (z - max) - log(sum) carries ulp(lp):
    on the +-60 rows that is 30 x float32 torch's error against 1 + |lp|, and inside the bar against 1 + max |z|;
  * Adam: ulp(w) + |dw| per element, dw the reference's update of that step; m: |m| + |g'|; v: v + g'^2 (g' the
    clipped gradient); the norm: itself;
  * normalise: (|x| + |mean|) / (std + eps); column sums: sum |x| (+ |out| when accumulating);
  * gaussian action: |mu| + sigma (1 + |n|); its log-probability: 1 + n^2 + |log_std|.

Actions are compared where the float64 decision is clear: a row counts when its top-two float64 score gap exceeds
2 (bar_lp scale_row + GUMBEL_ERR (1 + max |g|)), g = -log(-log u): twice what the log-probability bar and a float32
logf(-logf(u)) (a few ulp of g, and of 1 where -log u is near 1) can move one score.  At most EXCLUDED_CAP = 2 % of the
rows may fail that; the CPU test checks the cap on the float32 evaluation for the seeds used here."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MULTIPLE = 4.0
FLOOR = 2.0 ** -23
GUMBEL_ERR = 8.0 * 2.0 ** -24
EXCLUDED_CAP = 0.02
U_MAX = np.float32(1.0 - 2.0 ** -24)  # the largest float32 below 1
LOG_SQRT_2PI = 0.91893853320467274178


def bar_from(f32_max):
    return max(MULTIPLE * f32_max, FLOOR)


def report(tag, got_max, f32_max):
    """One POLOPT64_ERR line: tag, kernel max, float32 max, ratio; -> the bar."""
    ratio = got_max / f32_max if f32_max > 0 else (0.0 if got_max == 0 else float("inf"))
    print(f"POLOPT64_ERR {tag} kernel_max={got_max:.3e} f32_max={f32_max:.3e} ratio={ratio:.2f} bar={bar_from(f32_max):.3e}")
    return bar_from(f32_max)


def rel_err(got, ref, scale):
    """max |got - ref| / scale over all elements (float64 numpy); NaN or inf anywhere -> inf."""
    got, ref, scale = (np.asarray(a, dtype=np.float64) for a in (got, ref, scale))
    if got.size == 0:
        return 0.0
    e = np.abs(got - ref) / scale
    return float("inf") if not np.isfinite(e).all() else float(e.max())


# --------------------------------------------------------------------------------------------- the counter-based uniform
def _mix(seed, counter):
    c = np.atleast_1d(np.asarray(counter, dtype=np.uint64))
    s = np.full(1, seed, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = s + np.uint64(0x9E3779B97F4A7C15) * (c + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def u_unclamped(k):
    """((float)k + 0.5f) * 2^-24 in float32: the formula before the clamp (1.0 at k = 2^24 - 1)."""
    return (np.asarray(k).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def u_from_k(k):
    """The float32 u the kernel must produce from the 24-bit integer k."""
    return np.minimum(u_unclamped(k), U_MAX)


def uniform01_ref(seed, counter):
    """uniform01 of csrc/policy_act.h on uint64 numpy with wraparound: (k, u), k = the top 24 bits of the mixed word."""
    k = (_mix(seed, counter) >> np.uint64(40)).astype(np.uint32)
    return k, u_from_k(k)


BAD_SEED = 123
BAD_COUNTERS = (6731227, 27322404, 29048622)  # k = 2^24 - 1 under BAD_SEED


# --------------------------------------------------------------------------------------------- discrete action step
ACT_NA = (1, 2, 3, 7, 32, 4, 6, 15, 18)
ACT_B = (1, 63, 64, 65, 130)
ACT_T = (0.5, 1.0, 3.0)
ACT_DATA = ("plain", "pm80", "shift1e4", "equal_row")
ACT_VH = (0, 2)
ACT_SENTINEL = 3.0e38  # in the head columns past the logits and values: must not influence anything


def act_seed(nA, data):
    return 1000 * ACT_DATA.index(data) + nA


def act_logits(nA, data, B=max(ACT_B)):
    """[B, nA] float32 logits; the smaller batches are its leading rows."""
    g = torch.Generator().manual_seed(act_seed(nA, data))
    z = torch.randn(B, nA, generator=g) * 1.5
    if data == "pm80":
        z = torch.where(torch.rand(B, nA, generator=g) < 0.5, torch.full_like(z, -80.0), torch.full_like(z, 80.0))
    elif data == "shift1e4":
        z = z + 1.0e4
    elif data == "equal_row":
        z[0] = z[0, 0]
    return z.contiguous()


def act_uniforms(nA, data, B=max(ACT_B)):
    g = torch.Generator().manual_seed(act_seed(nA, data) + 500000)
    return torch.rand(B, nA, generator=g).clamp_(1e-6, 1 - 1e-6).contiguous()


def act_heads(z, vh, spare=3):
    """[B, nA + vh + spare] head rows: the logits, value columns, then the sentinel."""
    B, nA = z.shape
    g = torch.Generator().manual_seed(7 * nA + vh)
    h = torch.full((B, nA + vh + spare), ACT_SENTINEL)
    h[:, :nA] = z
    h[:, nA:nA + vh] = torch.randn(B, vh, generator=g)
    return h.contiguous()


def policy_act_ref(z, T, u=None):
    """float64 of the float32 logits z [B, nA]: log_softmax(z / T), the row scale 1 + max |z / T|, the greedy argmax of the
    raw logits (first index on ties) and, with the float32 uniforms u, the Gumbel scores lp - log(-log u), their argmax,
    the top-two gap and max |g| per row."""
    zt = z.double() / float(np.float32(T))
    lp = F.log_softmax(zt, dim=1)
    out = {"lp": lp, "scale": 1.0 + zt.abs().max(dim=1).values, "greedy": torch.from_numpy(np.argmax(z.numpy(), axis=1))}
    if u is not None:
        g = -torch.log(-torch.log(torch.as_tensor(u).double()))
        s = lp + g
        out["scores"], out["action"] = s, torch.from_numpy(np.argmax(s.numpy(), axis=1))
        top = s.topk(min(2, s.shape[1]), dim=1).values
        out["gap"] = (top[:, 0] - top[:, 1]) if s.shape[1] > 1 else torch.full((s.shape[0],), float("inf"), dtype=torch.float64)
        out["gmax"] = g.abs().max(dim=1).values
    return out


def policy_act_f32(z, T, u=None, variant=None):
    """Plain float32 torch on the CPU; variant: 'temp_multiplied' (z * T where z / T is meant), 'no_max' (log-softmax
    without the max subtraction)."""
    T32 = torch.tensor(T, dtype=torch.float32)
    zt = z * T32 if variant == "temp_multiplied" else z / T32
    lp = zt - torch.log(torch.exp(zt).sum(dim=1, keepdim=True)) if variant == "no_max" else F.log_softmax(zt, dim=1)
    out = {"lp": lp}
    if u is not None:
        s = lp - torch.log(-torch.log(torch.as_tensor(u)))
        out["scores"], out["action"] = s, torch.from_numpy(np.argmax(s.numpy(), axis=1))
    return out


def lp_err(lp, ref):
    """max over elements of |lp - ref| / the row's scale."""
    return rel_err(lp.double().numpy(), ref["lp"].numpy(), ref["scale"].numpy()[:, None])


def clear_rows(ref, bar_lp):
    """Rows whose float64 top-two gap exceeds the margin derived from the log-probability bar."""
    margin = 2.0 * (bar_lp * ref["scale"] + GUMBEL_ERR * (1.0 + ref["gmax"]))
    return ref["gap"] > margin


# internal-generator cases (nA, seed, offset): one templated and one run-time action count, seeds above 2^32
GEN_CASES = ((6, 0x1234567890ABCDEF, 987654321), (7, 0xFEDCBA9876543211, 5000000011))


def gen_uniforms(seed, offset, B, nA):
    """The float32 u of (row b, action a): counter offset + b nA + a."""
    return uniform01_ref(seed, np.uint64(offset) + np.arange(B * nA, dtype=np.uint64))[1].reshape(B, nA)


def bad_draw_case(counter, a_star, nA=6):
    """One row whose action a_star draws `counter`: logit -40 there against zeros -> (z [1, nA], u [1, nA], offset)."""
    offset = counter - a_star
    z = torch.zeros(1, nA)
    z[0, a_star] = -40.0
    return z, gen_uniforms(BAD_SEED, offset, 1, nA), offset


# --------------------------------------------------------------------------------------------- gaussian action step
def gaussian_normals_ref(seed, offset, n):
    """Box-Muller on counters 2 (offset + i) and 2 (offset + i) + 1, float64 of the float32 uniforms: (normal, u1, u2)."""
    i = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        u1 = uniform01_ref(seed, np.uint64(2) * i)[1]
        u2 = uniform01_ref(seed, np.uint64(2) * i + np.uint64(1))[1]
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * math.pi * u2.astype(np.float64)), u1, u2


def gaussian_act_ref(mu, log_std, normal):
    """mu [B, nA] float32, log_std [nA] float32, normal [B, nA] float64 -> float64 action, log-probability and their local
    scales."""
    mu, ls, n = np.asarray(mu, np.float64), np.asarray(log_std, np.float64)[None, :], np.asarray(normal, np.float64)
    sigma = np.exp(ls)
    act = n * sigma + mu
    lpa = -((act - mu) ** 2) / (2.0 * sigma * sigma) - ls - LOG_SQRT_2PI
    return {"action": act, "log_pac": lpa, "action_scale": np.abs(mu) + sigma * (1.0 + np.abs(n)),
            "log_pac_scale": 1.0 + n * n + np.abs(ls)}


def gaussian_act_f32(mu, log_std, normal=None, u1=None, u2=None):
    """Plain float32 torch on the CPU (Box-Muller from the float32 uniforms when no normals are given)."""
    mu, ls = torch.as_tensor(mu), torch.as_tensor(log_std)[None, :]
    if normal is None:
        u1, u2 = torch.as_tensor(u1).view(mu.shape), torch.as_tensor(u2).view(mu.shape)
        normal = torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(np.float32(2.0 * math.pi) * u2)
    else:
        normal = torch.as_tensor(normal, dtype=torch.float32).view(mu.shape)
    sigma = torch.exp(ls)
    act = normal * sigma + mu
    lpa = -((act - mu) ** 2) / (2.0 * sigma * sigma) - ls - np.float32(LOG_SQRT_2PI)
    return {"action": act.numpy(), "log_pac": lpa.numpy()}


# --------------------------------------------------------------------------------------------- discrete PPO loss
LOSS_NA = (2, 3, 7, 32, 4, 6, 15, 18)
LOSS_VH = (0, 1, 2)
LOSS_B = (1, 63, 65, 200)
LOSS_COEF = dict(eps_clip=0.2, ent_coef=0.01, vf_coef=0.5, grad_scale=0.5 / 200)
N_PLANTED = 10
ST_NAMES = ("loss_clip", "entropy", "value_loss", "clipped", "kl_approx", "kl_true", "gain", "ratio")


def loss_inputs(nA, vh, B=max(LOSS_B), spare=3):
    """Head rows [B, nA + vh + spare] (the spare columns hold a sentinel), actions, old log-probabilities, advantages and
    returns.  Rows 0 .. N_PLANTED - 1 are planted (the smaller batches keep the leading ones):
      0 ratio e (> 1 + eps), adv +1     1 ratio e, adv -1      2 ratio 1 / e (< 1 - eps), adv +1     3 ratio 1 / e, adv -1
      4 old_log_pac = the new logpac (ratio 1)     5 advantage 0     6 logits +-60, the action on a +60
      7 logits +-60, the action on a -60 with old_log_pac next to its logpac     8 ratio 1, adv 0     9 ratio e^3, adv -2"""
    g = torch.Generator().manual_seed(97 * nA + vh)
    ldo = nA + vh + spare
    heads = torch.full((B, ldo), ACT_SENTINEL)
    z = torch.randn(B, nA, generator=g) * 1.5
    actions = torch.randint(0, nA, (B,), generator=g)
    pm = torch.where(torch.arange(nA) % 2 == 0, torch.tensor(60.0), torch.tensor(-60.0))
    if B > 6:
        z[6], actions[6] = pm, 0
    if B > 7:
        z[7], actions[7] = pm, 1
    heads[:, :nA] = z
    heads[:, nA:nA + vh] = torch.randn(B, vh, generator=g)
    old_lp = F.log_softmax(torch.randn(B, nA, generator=g) * 1.5, dim=1)
    logpac = F.log_softmax(z.double(), dim=1).gather(1, actions[:, None])[:, 0]
    old_pac = (logpac + torch.randn(B, generator=g).double() * 0.3).float()
    adv = torch.randn(B, generator=g)
    ret = torch.randn(B, vh, generator=g)
    shift = {0: -1.0, 1: -1.0, 2: 1.0, 3: 1.0, 4: 0.0, 6: 0.05, 7: 0.05, 8: 0.0, 9: -3.0}
    advs = {0: 1.0, 1: -1.0, 2: 1.0, 3: -1.0, 5: 0.0, 8: 0.0, 9: -2.0}
    for r, s in shift.items():
        if r < B:
            old_pac[r] = (logpac[r] + s).float()
    for r, a in advs.items():
        if r < B:
            adv[r] = a
    return {"heads": heads.contiguous(), "actions": actions.int().contiguous(), "old_log_pac": old_pac.contiguous(),
            "old_log_policy": old_lp.contiguous(), "adv": adv.contiguous(), "ret": ret.contiguous(), "nA": nA, "vh": vh}


def _loss_eval(inp, B, with_old, dtype, variant=None, eps_clip=0.2, ent_coef=0.01, vf_coef=0.5, grad_scale=0.5 / 200):
    """The loss of test_ppo_loss_matches_reference_formula_autograd (tests/test_nn_ops_gpu.py) in `dtype`, by autograd.
    The float32 coefficients the kernel receives are used at their float32 values.  variant 'clamp_grad': d loss_clip /
    d ratio taken as clamp's gradient on the clipped branch (adv inside the interval, 0 outside) where torch.min's
    selects the smaller surrogate."""
    nA, vh = inp["nA"], inp["vh"]
    eps, ent, vfc, gs = (float(np.float32(c)) for c in (eps_clip, ent_coef, vf_coef, grad_scale))
    heads = inp["heads"][:B].to(dtype).clone().requires_grad_(True)
    act = inp["actions"][:B].long()
    old_pac, adv, ret = inp["old_log_pac"][:B].to(dtype), inp["adv"][:B].to(dtype), inp["ret"][:B].to(dtype)
    logps = F.log_softmax(heads[:, :nA], dim=1)
    logpac = logps.gather(1, act[:, None])[:, 0]
    ratio = torch.exp(logpac - old_pac)
    clipped = torch.clamp(ratio, 1 - eps, 1 + eps)
    if variant == "clamp_grad":
        loss_clip = torch.min(ratio * adv, clipped * adv).detach() + (clipped * adv - (clipped * adv).detach())
    else:
        loss_clip = torch.min(ratio * adv, clipped * adv)
    entropy = -(logps.exp() * logps).sum(-1)
    diff = heads[:, nA:nA + vh] - ret
    vloss = (vfc * diff * diff).sum(-1)
    gain = loss_clip + ent * entropy - vloss
    (gs * (-gain)).sum().backward()
    dh = heads.grad.clone()
    dh[:, nA + vh:] = 0.0  # the spare columns take no part
    with torch.no_grad():
        kl_true = (logps.exp() * (logps - inp["old_log_policy"][:B].to(dtype))).sum(-1) if with_old else torch.zeros_like(gain)
        stats = torch.stack([loss_clip, entropy, vloss, (torch.abs(ratio - 1.0) > eps).to(dtype), old_pac - logpac, kl_true,
                             gain, ratio], dim=1).detach()
        maxdiff = diff.abs().max(dim=1).values if vh else torch.zeros_like(gain)
        out = {"dheads": dh, "stats": stats, "ratio": ratio.detach(), "eps": eps,
               "row_scale": gs * (adv.abs() * ratio + ent + 2.0 * vfc * maxdiff).detach()}
        # L: the scale of the row's log-probabilities, 1 + max |z| as in the action step, + |old_log_pac| where it enters
        one = torch.ones_like(gain)
        zmax = 1.0 + heads[:, :nA].detach().abs().max(dim=1).values
        L = zmax + old_pac.abs()
        olpmax = inp["old_log_policy"][:B].to(dtype).abs().max(dim=1).values if with_old else 0.0 * one
        s_clip, s_v = one + adv.abs() * torch.clamp(ratio, min=1.0) * L, one + vloss
        out["stat_scales"] = torch.stack([s_clip, zmax, s_v, one, L, zmax + olpmax, s_clip + zmax + s_v, ratio * L + 1e-300],
                                         dim=1).detach()
    return out


def ppo_loss_ref(inp, B, with_old, **coef):
    return _loss_eval(inp, B, with_old, torch.float64, **coef)


def ppo_loss_f32(inp, B, with_old, variant=None, **coef):
    return _loss_eval(inp, B, with_old, torch.float32, variant, **coef)


def loss_errs(dheads, stats, ref):
    """-> (max over rows of |dheads - ref| / the row's scale, {statistic: max |e| / scale} without the clipped column)."""
    d = rel_err(dheads.double().numpy(), ref["dheads"].double().numpy(), ref["row_scale"].double().numpy()[:, None])
    s = {}
    for c, name in enumerate(ST_NAMES):
        if name != "clipped":
            s[name] = rel_err(stats[:, c].double().numpy(), ref["stats"][:, c].double().numpy(), ref["stat_scales"][:, c].double().numpy())
    return d, s


def clip_decided(ref, bar_ratio):
    """Rows whose float64 | |ratio - 1| - eps | exceeds twice what the ratio's bar can move it."""
    r = ref["ratio"].double()
    margin = 2.0 * bar_ratio * ref["stat_scales"][:, 7].double() + 2.0 ** -23
    return (torch.abs(torch.abs(r - 1.0) - ref["eps"]) > margin)


# --------------------------------------------------------------------------------------------- Adam + global-norm clip
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_REGIMES = ("1e-8", "1e-3", "1", "1e4", "mix", "zero")
ADAM_MAX_NORM = ("off", "above", "below")
ADAM_GRAD_DIV = (1.0, 8.0)
ADAM_SIZES = (1, 3, 4, 5, 255, 256, 257, 4096, 4097, 262147, 1048580)
ADAM_HP = dict(lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-5)
ADAM_N_SMALL = 260  # a multiple of 4: the 16-byte path when aligned, the scalar path one float further


def adam_inputs(n, regime, w_zero, seed=0, n_steps=3):
    """float32 numpy: w, the given m and v (of the gradients' magnitude, v >= 0) and n_steps gradients."""
    rng = np.random.default_rng(seed * 1000003 + n * 7 + ADAM_REGIMES.index(regime))
    if regime == "mix":
        mag = np.array([1e-8, 1e-3, 1.0, 1e4])[rng.integers(0, 4, n)]
    elif regime == "zero":
        mag = np.zeros(n)
    else:
        mag = np.full(n, float(regime))
    gs = [(rng.standard_normal(n) * mag).astype(np.float32) for _ in range(n_steps)]
    mmag = np.where(mag == 0, 1e-3, mag)
    m = (rng.standard_normal(n) * mmag * 0.5).astype(np.float32)
    v = ((rng.standard_normal(n) * mmag) ** 2).astype(np.float32)
    w = np.zeros(n, np.float32) if w_zero else rng.standard_normal(n).astype(np.float32)
    return w, m, v, gs


def adam_max_norm(kind, g, grad_div):
    """The float32 max_grad_norm of a case: 0 (off), or the first gradient's norm times 1 +- 2^-10."""
    if kind == "off":
        return np.float32(0.0)
    norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2))) / grad_div
    return np.float32(norm * (1.0 + 2.0 ** -10 if kind == "above" else 1.0 - 2.0 ** -10))


def adam_ref(w, m, v, gs, step0, max_norm, grad_div, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-5, sumsq=None):
    """float64, free-running over len(gs) steps from the float32 w, m, v: global-norm clip min(1, max_norm / (norm +
    1e-6)) with norm = sqrt(sum g^2) / grad_div, gradient g / grad_div, Adam with eps outside the root and the bias
    corrections as double 1 - beta^step.  lr, betas and eps enter at the float32 values the kernel receives
    ((float)lr, (float)(1 - beta1), (float)beta2, (float)(1 - beta2), (float)eps); max_norm and grad_div are float32
    already.  sumsq: the sum of squares to take for the norm (the presummed entry point).  -> one dict per step."""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    lr_, omb1, b2, omb2, eps_ = f32(lr), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps)
    w, m, v = (np.asarray(a, np.float64).copy() for a in (w, m, v))
    max_norm, grad_div = float(max_norm), float(grad_div)
    out = []
    for t, g in enumerate(gs):
        step = step0 + t
        g = np.asarray(g, np.float64)
        tot = float(sumsq) if sumsq is not None else math.fsum((g * g).tolist())
        norm = math.sqrt(tot) / grad_div
        clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
        gc = g * (clip / grad_div)
        bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
        m_old, v_old = m, v
        m = m + (gc - m) * omb1
        v = v * b2 + omb2 * gc * gc
        dw = -(lr_ / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps_))
        w = w + dw
        out.append({"w": w.copy(), "m": m.copy(), "v": v.copy(), "norm": norm, "dw": dw,
                    "w_scale": np.spacing(np.abs(w).astype(np.float32)).astype(np.float64) + np.abs(dw),
                    "m_scale": np.abs(m_old) + np.abs(gc) + 1e-300, "v_scale": v_old + gc * gc + 1e-300})
    return out


def adam_f32(w, m, v, gs, step0, max_norm, grad_div, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-5, variant=None):
    """Plain float32 torch on the CPU, the operations of torch.optim.Adam and clip_grad_norm_.  Variants:
    'eps_in_root' sqrt(v / bc2 + eps); 'eps_before_bc' (sqrt(v) + eps) / sqrt(bc2); 'bc_float' the betas rounded to float32
    before pow; 'clip_no_1e-6' max_norm / norm."""
    w, m, v = (torch.from_numpy(np.array(a, np.float32)) for a in (w, m, v))
    out = []
    for t, g in enumerate(gs):
        step = step0 + t
        g = torch.from_numpy(np.asarray(g, np.float32)) / np.float32(grad_div)
        norm = torch.linalg.vector_norm(g)
        if max_norm > 0:
            coef = np.float32(max_norm) / (norm + (0.0 if variant == "clip_no_1e-6" else np.float32(1e-6)))
            g = g * torch.clamp(coef, max=1.0)
        b1p, b2p = (float(np.float32(beta1)), float(np.float32(beta2))) if variant == "bc_float" else (beta1, beta2)
        bc1, bc2 = 1.0 - b1p ** step, 1.0 - b2p ** step
        m = torch.lerp(m, g, 1.0 - beta1)
        v = v * beta2 + (1.0 - beta2) * g * g
        if variant == "eps_in_root":
            denom = torch.sqrt(v / bc2 + eps)
        elif variant == "eps_before_bc":
            denom = (torch.sqrt(v) + eps) / math.sqrt(bc2)
        else:
            denom = torch.sqrt(v) / math.sqrt(bc2) + eps
        w = w - (lr / bc1) * (m / denom)
        out.append({"w": w.numpy().copy(), "m": m.numpy().copy(), "v": v.numpy().copy(), "norm": float(norm)})
    return out


def adam_errs(got, ref):
    """got / ref: per-step dicts -> max over the steps of the relative errors of w, m, v and the norm."""
    e = {"w": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0}
    for a, r in zip(got, ref):
        for k in ("w", "m", "v"):
            e[k] = max(e[k], rel_err(a[k], r[k], r[k + "_scale"]))
        if a.get("norm") is not None:
            e["norm"] = max(e["norm"], rel_err(a["norm"], r["norm"], r["norm"] if r["norm"] > 0 else 1.0))
    return e


# --------------------------------------------------------------------------------------------- batch operations
def moments_ref(x):
    """(sum, sum of squares, count, sum |x|) of the float32 array, exact (math.fsum of the exact doubles)."""
    xs = np.asarray(x, np.float64)
    return math.fsum(xs.tolist()), math.fsum((xs * xs).tolist()), float(xs.size), math.fsum(np.abs(xs).tolist())


def normalize_ref(x, moments, eps):
    """float64 (x - mean) / (sqrt(max(var, 0)) + eps), population variance from [sum, sumsq, count]; -> out, mean, std and
    the local scale (|x| + |mean|) / (std + eps)."""
    x = np.asarray(x, np.float64)
    mean = moments[0] / moments[2]
    var = max(moments[1] / moments[2] - mean * mean, 0.0)
    std, eps = math.sqrt(var), float(np.float32(eps))
    return (x - mean) / (std + eps), mean, std, (np.abs(x) + abs(mean)) / (std + eps)


def normalize_f32(x, pool, eps, variant=None):
    """Plain float32 torch: (x - pool.mean()) / (pool.std() + eps), population std ('sample_var': the unbiased one)."""
    x, pool = torch.as_tensor(x), torch.as_tensor(pool)
    return ((x - pool.mean()) / (pool.std(unbiased=variant == "sample_var") + np.float32(eps))).numpy()


def colsum_ref(X, prev=None):
    """float64 column sums of the float32 [rows, cols] (+ prev when accumulating) and the scale sum |x| (+ |prev|)."""
    X = np.asarray(X, np.float64)
    s, a = X.sum(0), np.abs(X).sum(0)
    if prev is not None:
        s, a = s + np.asarray(prev, np.float64), a + np.abs(np.asarray(prev, np.float64))
    return s, a + 1e-300


def colsum_f32(X, prev=None):
    s = torch.as_tensor(X).sum(0)
    return (s + torch.as_tensor(prev) if prev is not None else s).numpy()


def axpy_two_roundings(dst, src, alpha):
    """numpy float32: the product rounded, then the sum rounded."""
    prod = np.float32(alpha) * np.asarray(src, np.float32)
    return np.asarray(dst, np.float32) + prod


def axpy_fused(dst, src, alpha):
    """What one fused multiply-add gives: the exact product (a double holds it) added and rounded.  (The double sum rounds
    once more on the way; that can only matter within 2^-29 of a float32 tie.)"""
    return (np.asarray(dst, np.float64) + float(np.float32(alpha)) * np.asarray(src, np.float64)).astype(np.float32)


def axpy_data(n, seed=5):
    """dst, src, alpha with full-mantissa values: a fused multiply-add differs from two roundings on a good share."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32), np.float32(0.7310585975646973)


# --------------------------------------------------------------------------------------------- guarded device buffers
PAD = 1024           # sentinel elements on either side of an output
SENTINEL = -7.25e30  # float buffers; integer buffers take -7, byte buffers 255


def guarded(shape, dev, shift=0, dtype=torch.float32, sentinel=SENTINEL, init=None):
    """An output of `shape` inside a sentinel-filled buffer, `shift` elements past the buffer's (256-byte aligned) start
    + PAD (tests/test_conv_float64_gpu.py's guarded): (whole buffer, the output view), the view holding init if given."""
    numel = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((PAD + shift + numel + PAD,), sentinel, dtype=dtype, device=dev)
    view = buf[PAD + shift:PAD + shift + numel].view(shape)
    if init is not None:
        view.copy_(torch.as_tensor(init).view(shape))
    return buf, view


def guards_intact(buf, out, sentinel=SENTINEL):
    lo = (out.data_ptr() - buf.data_ptr()) // buf.element_size()
    hi = lo + out.numel()
    return bool((buf[:lo] == sentinel).all().item()) and bool((buf[hi:] == sentinel).all().item())


def same_bits(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {4: torch.int32, 8: torch.int64, 1: torch.uint8}[a.element_size()]
    return bool(torch.equal(a.view(it), b.view(it)))
