"""GPU: ppo_distil_loss_modes_f32, the distillation loss with every choice of the reference's --distil_loss,
--distil_value_loss, --distil_target and --distil_max_heads (rl/rollout.py:1331-1449), against a float64 autograd
restatement of the formulas in include/ppo_amd.h.

The bar is the one tests/test_minibatch_rows_gpu.py holds ppo_distil_loss_f32 to: |err| <= 1e-5 x the largest reference
entry, for dheads and for each statistics column.  The float32 kernel and the float64 restatement may take different
branches only at a kink of a loss (|d| = 0, delta, 1), so the targets are built as T = P - d with every |d| at least 1e-3
away from each kink, which is asserted on the float32 values that are uploaded; the kinks themselves are pinned by a
separate test on exactly representable values."""
import math

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from ppo_amd import _lib  # noqa: E402

DEV = "cuda"
MARGIN = 1e-3
POLICY = _lib.DISTIL_POLICY_LOSSES
VALUE = _lib.DISTIL_VALUE_LOSSES


def _p(t):
    return None if t is None else t.data_ptr()


def within(got, ref, what, tol=1e-5):
    """|got - ref| <= tol x the largest |ref|."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got - ref).abs().max())
    print(f"{what}: max err {err / scale:.3e} of the largest entry (bar {tol:.0e})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def value_term(d, c, dt):
    """The loss of one prediction, d = P - T (include/ppo_amd.h, ppo_distil_loss_modes_f32)."""
    vl = c["value_loss"]
    if vl == "mse":
        return 0.5 * d ** 2
    if vl == "l1":
        return c["l1_scale"] * d.abs()
    if vl == "clipped_mse":
        return torch.clip(d, -1, 1) ** 2
    assert vl == "huber"
    if c["delta"] == 0:
        return d.abs()
    return F.huber_loss(d, torch.zeros_like(d), reduction="none", delta=c["delta"])


def modes_ref(z, targets, old, w, log_std, actions, c, dt=torch.float64):
    """-> (d sum_b grad_scale loss_b / d heads, statistics [B, 4]) in float64.  targets / old / actions: the rows of the
    minibatch, already gathered."""
    z = z.to(dt).requires_grad_(True)
    nA, n, B = c["nA"], c["n_pred"], z.shape[0]
    if actions is None:
        P = z[:, c["pred_col"]:c["pred_col"] + n * c["stride"]:c["stride"]]
    else:
        P = z[torch.arange(B), c["pred_col"] + actions.long()][:, None]
    w = torch.ones(n, dtype=dt) if w is None else w.to(dt)
    n_active = c["n_active"] or n
    d = P - targets.to(dt).reshape(-1, n)
    vscale = 1.0 / math.sqrt(n_active) if c["vector"] else 1.0
    vloss = (vscale * w * value_term(d, c, dt)).sum(1)
    zp, o = z[:, :nA], old.to(dt)
    if log_std is not None:
        den = 1e-5 + 2.0 * torch.exp(log_std.to(dt)) ** 2
        pol = 2.0 * (0.5 * (o - zp) ** 2 / den).mean(1)
    elif c["policy_loss"] == "kl_policy":
        lp = F.log_softmax(zp, dim=1)
        pol = (lp.exp() * (lp - o)).sum(1)
    elif c["policy_loss"] == "mse_policy":
        pol = 0.5 * ((o - F.log_softmax(zp, dim=1)) ** 2).mean(1)
    else:
        assert c["policy_loss"] == "mse_logit"
        pol = 0.5 * ((o - zp) ** 2).mean(1)
    total = vloss + c["beta"] * pol
    (c["grad_scale"] * total.sum()).backward()
    stats = torch.stack([vloss, c["beta"] * pol, total, ((w * d) ** 2).sum(1) / n_active], 1).detach()
    return z.grad, stats


def run_modes(z, targets, old, w, log_std, idx, actions, c):
    B = z.shape[0]
    dh = torch.full((B, c["ldo"]), float("nan"), device=DEV)
    stats = torch.full((B, 4), float("nan"), device=DEV)
    rc = _lib.load().ppo_distil_loss_modes_f32(
        _p(z), B, c["ldo"], c["nA"], c["pred_col"], c["n_pred"], c["stride"], c["vector"], _p(targets), _p(w), _p(old),
        _p(log_std), c["beta"], c["grad_scale"], _p(dh), _p(stats), _p(idx), POLICY[c["policy_loss"]],
        VALUE[c["value_loss"]], c["delta"], c["l1_scale"], _p(actions), c["n_active"], _lib.current_stream())
    _lib.check(rc, "ppo_distil_loss_modes_f32")
    torch.cuda.synchronize()
    return dh, stats


def kinks(c):
    return (0.0, 1.0) + ((c["delta"],) if c["delta"] > 0 else ())


def off_the_kinks(d, c):
    """Move every d whose |d| lies within MARGIN of a kink to twice that margin beyond it (sign kept, 0 counts as +)."""
    sign = torch.where(d < 0, -1.0, 1.0).to(d.dtype)
    a = d.abs()
    for k in kinks(c):
        a = torch.where((a - k).abs() < MARGIN, torch.full_like(a, k + 2 * MARGIN), a)
    return sign * a


def case(nA, target, **kw):
    """scalar: one prediction right behind the policy columns' neighbour; vector: 40 heads at stride 2 far enough out
    that the row is longer than 128 columns (the kernel's 64-column loop runs three times); adv: the advantage block."""
    if target == "vector":
        c = dict(ldo=nA + 40 + 80 + 11, nA=nA, pred_col=nA + 40, n_pred=40, stride=2, vector=1)
    else:
        c = dict(ldo=2 * nA + 7, nA=nA, pred_col=nA + 2, n_pred=1, stride=1, vector=0)
    c.update(beta=0.8, grad_scale=0.37, policy_loss="kl_policy", value_loss="mse", delta=0.0, l1_scale=0.0, n_active=0,
             form="discrete", subset=None, actions=False)
    c.update(kw)
    return c


SUBSET = [3, 9, 15, 21, 27, 33, 39]
VALUE_CASES = [("mse", 0.0), ("l1", 0.0), ("clipped_mse", 0.0), ("huber", 0.0), ("huber", 0.1), ("huber", 1.5)]
CASES = {}
for _vl, _delta in VALUE_CASES:
    for _t, _nA in (("scalar", 2), ("vector", 15)):
        CASES[f"{_vl}-{_delta}-{_t}"] = case(_nA, _t, value_loss=_vl, delta=_delta, l1_scale=1 / 30)
for _pl in ("kl_policy", "mse_policy", "mse_logit"):
    for _nA in (2, 15):
        CASES[f"{_pl}-nA{_nA}"] = case(_nA, "scalar", policy_loss=_pl, value_loss="l1", l1_scale=0.3)
CASES["gaussian-huber"] = case(3, "vector", form="gaussian", value_loss="huber", delta=0.1, policy_loss="mse_policy")
CASES["subset-mse"] = case(2, "vector", subset=SUBSET, n_active=7)
CASES["subset-clipped"] = case(15, "vector", subset=SUBSET, n_active=7, value_loss="clipped_mse", policy_loss="mse_logit")
CASES["actions-mse"] = case(15, "scalar", actions=True)
CASES["actions-huber"] = case(15, "scalar", actions=True, value_loss="huber", delta=0.1, policy_loss="mse_policy")


def make_inputs(c, B, factor, seed):
    """z [B, ldo]; targets / old / actions over a source of B * factor rows, idx [B] into it (None: factor 1, in order).
    d = P - T is drawn over all three zones of every loss and kept MARGIN off the kinks."""
    g = torch.Generator().manual_seed(seed)
    nA, n, Bt = c["nA"], c["n_pred"], B * factor
    z = torch.randn(B, c["ldo"], generator=g) * 1.5
    idx = (torch.randperm(Bt, generator=g)[:B] if factor > 1 else torch.arange(B)).contiguous()
    actions_big = torch.randint(0, nA, (Bt,), generator=g).int() if c["actions"] else None
    if c["actions"]:
        P = z[torch.arange(B), c["pred_col"] + actions_big[idx].long()][:, None]
    else:
        P = z[:, c["pred_col"]:c["pred_col"] + n * c["stride"]:c["stride"]]
    # a third of the d small (inside huber's delta 0.1), the rest up to |d| ~ 3 (beyond clipped_mse's 1, huber's 1.5)
    d = torch.randn(B, n, generator=g).double() * torch.where(torch.rand(B, n, generator=g) < 1 / 3, 0.05, 1.2)
    d = off_the_kinks(d, c)
    t_big = torch.randn(Bt, n, generator=g) * 2.0
    t_big[idx] = (P.double() - d).float()
    d32 = (P.double() - t_big[idx].double()).abs()  # what the kernel sees
    for k in kinks(c):
        assert float((d32 - k).abs().min()) >= MARGIN, f"a d within {MARGIN} of the kink {k}"
    if c["form"] == "gaussian":
        old_big, log_std = torch.randn(Bt, nA, generator=g), torch.randn(nA, generator=g) * 0.5
    else:
        # The old policy of every minibatch row is the new one tilted by -2 .. 2 over the actions (plus noise), never a
        # policy that happens to lie next to it: the KL is a sum of terms of both signs, float32 carries it to ~1e-7 of
        # its largest TERM, and the bar is relative to the largest KL of the batch - which for B = 1 is the one sample's
        # own.  Two nearly equal policies would ask the statistic for digits no float32 sum of those terms has.
        old_logits = torch.randn(Bt, nA, generator=g) * 1.5
        tilt = torch.linspace(-2.0, 2.0, nA) + 0.3 * torch.randn(B, nA, generator=g)
        old_logits[idx] = z[:, :nA] + tilt
        old_big, log_std = (old_logits if c["policy_loss"] == "mse_logit" else F.log_softmax(old_logits, dim=1)), None
    w = None
    if c["vector"]:
        w = torch.rand(n, generator=g) + 0.25
        if c["subset"] is not None:
            mask = torch.zeros(n)
            mask[c["subset"]] = 1.0
            w = w * mask
    return z, t_big, old_big, log_std, w, actions_big, idx


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("name", list(CASES))
def test_modes_against_float64(name, B):
    c = CASES[name]
    nA, n = c["nA"], c["n_pred"]
    for factor in (1, 3):
        z, t_big, old_big, log_std, w, actions_big, idx = make_inputs(c, B, factor, 1000 + 13 * B + factor + len(name))
        acts = None if actions_big is None else actions_big[idx]
        want_dh, want_st = modes_ref(z, t_big[idx], old_big[idx], w, log_std, acts, c)
        dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
        idxd = idx.int().to(DEV) if factor > 1 else None
        dh, st = run_modes(dev(z), dev(t_big), dev(old_big), dev(w), dev(log_std), idxd, dev(actions_big), c)
        what = f"{name} B={B} x{factor}"
        within(dh, want_dh, f"{what} dheads")
        for col, stat in enumerate(("value loss", "policy loss", "total", "squared error")):
            within(st[:, col], want_st[:, col], f"{what} {stat}")
        # columns the loss does not use: exactly 0
        used = torch.zeros(B, c["ldo"], dtype=torch.bool)
        used[:, :nA] = True
        if acts is not None:
            used[torch.arange(B), c["pred_col"] + acts.long()] = True
            block = dh[:, c["pred_col"]:c["pred_col"] + nA].cpu()
            taken = F.one_hot(acts.long(), nA).bool()
            assert float(block[~taken].abs().max()) == 0.0, "a non-taken advantage column got gradient"
            assert bool((block[taken] != 0).all())
        else:
            heads = range(n) if c["subset"] is None else c["subset"]
            used[:, [c["pred_col"] + k * c["stride"] for k in heads]] = True
        assert float(dh.cpu()[~used].abs().max()) == 0.0
        assert bool(torch.isfinite(dh).all()) and bool(torch.isfinite(st).all())


@pytest.mark.parametrize("target", ["scalar", "vector"])
@pytest.mark.parametrize("form", ["discrete", "gaussian"])
def test_zero_modes_are_the_old_entry(form, target):
    """All-zero modes: torch.equal dheads and statistics to ppo_distil_loss_f32 on the same inputs."""
    c = case(15 if form == "discrete" else 3, target, form=form)
    B = 37
    z, t_big, old_big, log_std, w, _a, idx = make_inputs(c, B, 3, 77)
    zd, td, od, idxd = z.to(DEV), t_big.to(DEV), old_big.to(DEV), idx.int().to(DEV)
    wd = None if w is None else w.to(DEV)
    lsd = None if log_std is None else log_std.to(DEV)
    dh, st = run_modes(zd, td, od, wd, lsd, idxd, None, c)
    dh0 = torch.full((B, c["ldo"]), float("nan"), device=DEV)
    st0 = torch.full((B, 4), float("nan"), device=DEV)
    rc = _lib.load().ppo_distil_loss_f32(_p(zd), B, c["ldo"], c["nA"], c["pred_col"], c["n_pred"], c["stride"], c["vector"],
                                         _p(td), _p(wd), _p(od), _p(lsd), c["beta"], c["grad_scale"], _p(dh0), _p(st0),
                                         _p(idxd), _lib.current_stream())
    _lib.check(rc, "ppo_distil_loss_f32")
    torch.cuda.synchronize()
    assert torch.equal(dh, dh0) and torch.equal(st, st0)
    assert bool(torch.isfinite(dh0).all()) and bool(torch.isfinite(st0).all())


D_TIES = [0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5]
SIGN = [0.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0]
TIES = {
    # mode: (delta, l1_scale, d loss / d P, loss) at D_TIES; every value exact in float32
    "mse": (0.0, 0.0, D_TIES, [0.0, 0.5, 0.5, 0.125, 0.125, 1.125, 1.125]),
    "l1": (0.0, 0.25, [0.25 * s for s in SIGN], [0.25 * abs(d) for d in D_TIES]),
    "clipped_mse": (0.0, 0.0, [0.0, 2.0, -2.0, 1.0, -1.0, 0.0, 0.0], [0.0, 1.0, 1.0, 0.25, 0.25, 1.0, 1.0]),
    "huber": (0.5, 0.0, [0.0, 0.5, -0.5, 0.5, -0.5, 0.5, -0.5], [0.0, 0.375, 0.375, 0.125, 0.125, 0.625, 0.625]),
    "huber0": (0.0, 0.0, SIGN, [abs(d) for d in D_TIES]),
}


@pytest.mark.parametrize("mode", list(TIES))
def test_subgradients_at_the_kinks(mode):
    """d in {0, +-1, +-delta} (and +-1.5 beyond the clip), exactly representable: sign(0) = 0, clipped_mse passes the
    gradient AT +-1 (torch.clip), huber is quadratic strictly inside delta."""
    delta, l1_scale, want_g, want_l = TIES[mode]
    c = case(2, "scalar", value_loss=mode.rstrip("0"), delta=delta, l1_scale=l1_scale, beta=0.0, grad_scale=1.0)
    B = len(D_TIES)
    z = torch.zeros(B, c["ldo"])
    z[:, c["pred_col"]] = torch.tensor([0.25, 0.75, -1.25, 2.0, 0.5, -0.25, 1.0])
    targets = (z[:, c["pred_col"]] - torch.tensor(D_TIES))[:, None].contiguous()
    assert torch.equal(z[:, c["pred_col"]] - targets[:, 0], torch.tensor(D_TIES))
    old = F.log_softmax(torch.zeros(B, c["nA"]), dim=1)
    dh, st = run_modes(z.to(DEV), targets.to(DEV), old.to(DEV), None, None, None, None, c)
    assert torch.equal(dh[:, c["pred_col"]].cpu(), torch.tensor(want_g))
    assert torch.equal(st[:, 0].cpu(), torch.tensor(want_l))
    assert torch.equal(st[:, 3].cpu(), torch.tensor(D_TIES) ** 2)
