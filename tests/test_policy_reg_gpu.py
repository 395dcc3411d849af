"""GPU: the two regularisers of the policy phase - the global KL penalty (--gkl_*, rl/rollout.py:1723-1738, 1922-1934)
and SIDE, state-independent exploration (--side_*, rl/rollout.py:1662-1679, 1903-1918) - from the row kernels up to the
Runner.

  1. ppo_policy_kl_loss_f32 and ppo_ppo_loss_side_f32 against the float64 restatement (tests/policy_reg_float64_torch.py)
     at the project's bar for loss rows, |err| <= 1e-5 x the largest reference entry, at block edges (64 samples per
     workgroup) and templated / run-time / maximal action counts; the indexed form against the gathered one, bit for bit
  2. nothing that ran before changes: a null target is ppo_ppo_loss_f32's launch, zeroed new fields are the fused MLP
     kind's old result
  3. the fused MLP kinds against the op-by-op launches and float64, at a tiling-edge shape
  4. DualHeadNet.policy_kl_minibatch = training forward + KL row + backward, bit for bit; indexed = gathered; the value
     head gets exact zeros
  5. Runner.train_policy_minibatch against the reference's recorded minibatch (tests/golden/policy_reg_golden.npz)
  6. the Runner: where the global rows are drawn in the np.random stream, what reaches the optimiser, the statistics,
     --gkl_penalty=0, the SIDE redraw, the data-parallel refusal
"""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import mlp_float64_torch as M  # noqa: E402
import policy_reg_float64_torch as P  # noqa: E402
from oracle import trained_params as T  # noqa: E402
from ppo_amd import _lib, logger, models, rollout  # noqa: E402
from ppo_amd.config import args  # noqa: E402

DEV = "cuda"
NAN = float("nan")
HERE = os.path.dirname(__file__)


def _p(t):
    return None if t is None else t.data_ptr()


def within(got, ref, what, tol=1e-5):
    """|got - ref| <= tol x the largest |ref| (`within` of tests/test_distil_modes_gpu.py; no NaN passes)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got.reshape(ref.shape) - ref).abs().max())
    print(f"{what}: max err {err / scale:.3e} of the largest entry (bar {tol:.0e})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


TOP_LEVEL = ("max_micro_batch_size", "entropy_bonus", "disable_logging")


@pytest.fixture(autouse=True)
def restore_top_level_flags():
    """Top-level flags keep their value through a later args.setup() that does not name them: put back the ones the
    tests here set."""
    before = {k: getattr(args, k) for k in TOP_LEVEL}
    yield
    for k, v in before.items():
        setattr(args, k, v)


# ====================================================================== 1. the row kernels against float64
BATCHES = [1, 63, 64, 65, 130]       # block edges: 64 samples per workgroup
ACTIONS = [2, 4, 7, 18, 32]          # templated (4, 18), run-time (2, 7), kMaxActions (32)


def rows(B, nA, seed):
    """Head rows [B, 2 nA + 3] and the per-sample arrays of a discrete policy minibatch, old policies tilted away from
    the new one, ratios that straddle the clip range, a random SIDE target."""
    g = torch.Generator().manual_seed(1000 * B + nA + seed)
    ldo = 2 * nA + 3
    z = torch.randn(B, ldo, generator=g)
    new_lp = F.log_softmax(z[:, :nA], dim=1)
    actions = torch.randint(0, nA, (B,), generator=g).int()
    old_lp = P.tilted_log_policy(z[:, :nA], g)  # (as make_inputs of tests/test_distil_modes_gpu.py)
    old_log_pac = new_lp[torch.arange(B), actions.long()] + 0.3 * torch.randn(B, generator=g)
    adv, ret = torch.randn(B, generator=g), torch.randn(B, 2, generator=g)
    target = F.log_softmax(torch.randn(nA, generator=g), dim=0)
    return dict(z=z, actions=actions, old_log_pac=old_log_pac, old_lp=old_lp, adv=adv, ret=ret, target=target, ldo=ldo)


def run_kl(z, old, nA, grad_scale, with_rows=True):
    B, ldo = z.shape
    dh = torch.full((B, ldo), NAN, device=DEV)
    kl = torch.full((B,), NAN, device=DEV)
    rc = _lib.load().ppo_policy_kl_loss_f32(_p(z), B, ldo, nA, _p(old), grad_scale, _p(dh), _p(kl) if with_rows else None,
                                            _lib.current_stream())
    _lib.check(rc, "ppo_policy_kl_loss_f32")
    torch.cuda.synchronize()
    return dh, kl


def run_side(z, c, actions, old_log_pac, old_lp, adv, ret, target, idx=None, entry="ppo_ppo_loss_side_f32", penalty=True):
    B, ldo = z.shape
    dh = torch.full((B, ldo), NAN, device=DEV)
    stats = torch.full((B, 8), NAN, device=DEV)
    pen = torch.full((B,), NAN, device=DEV)
    a = (_p(z), B, ldo, c["nA"], c["vh"], _p(actions), _p(old_log_pac), _p(old_lp), _p(adv), _p(ret), c["eps"], c["ent_coef"],
         c["vf_coef"], c["grad_scale"], _p(dh), _p(stats), _p(idx))
    if entry == "ppo_ppo_loss_side_f32":
        a += (_p(target), _p(pen) if penalty else None)
    rc = getattr(_lib.load(), entry)(*a, _lib.current_stream())
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    return dh, stats, pen


@pytest.mark.parametrize("nA", ACTIONS)
@pytest.mark.parametrize("B", BATCHES)
def test_kl_row_against_float64(B, nA):
    r = rows(B, nA, 1)
    z, old = r["z"].to(DEV), r["old_lp"].to(DEV)
    dh, kl = run_kl(z, old, nA, 0.37)
    ref_dh, ref_kl = P.policy_kl_ref(r["z"], r["old_lp"], nA, 0.37)
    assert float(ref_kl.min()) > 0  # the old policies differ from the new ones
    within(dh[:, :nA], ref_dh[:, :nA], f"kl dheads B={B} nA={nA}")
    within(kl, ref_kl, f"kl rows B={B} nA={nA}")
    assert float(dh[:, nA:].abs().max()) == 0.0  # over the NaN it was filled with
    dh2, kl2 = run_kl(z, old, nA, 0.37, with_rows=False)  # kl_rows is nullable
    assert torch.equal(dh, dh2) and bool(torch.isnan(kl2).all())


@pytest.mark.parametrize("ent_coef", [0.01, 0.0])
@pytest.mark.parametrize("nA", ACTIONS)
@pytest.mark.parametrize("B", BATCHES)
def test_side_row_against_float64(B, nA, ent_coef):
    r = rows(B, nA, 2)
    c = dict(nA=nA, vh=2, eps=0.2, ent_coef=ent_coef, vf_coef=0.5, grad_scale=0.37)
    d = {k: v.to(DEV) for k, v in r.items() if torch.is_tensor(v)}
    dh, stats, pen = run_side(d["z"], c, d["actions"], d["old_log_pac"], d["old_lp"], d["adv"], d["ret"], d["target"])
    ref_dh, ref_stats, ref_pen = P.ppo_side_ref(r["z"], r["actions"], r["old_log_pac"], r["old_lp"], r["adv"], r["ret"],
                                                r["target"], c)
    within(dh[:, :nA + 2], ref_dh[:, :nA + 2], f"side dheads B={B} nA={nA} c={ent_coef}")
    assert float(dh[:, nA + 2:].abs().max()) == 0.0
    for col, name in enumerate(("loss_clip", "entropy", "value_loss", "clipped", "kl_approx", "kl_true", "gain", "ratio")):
        within(stats[:, col], ref_stats[:, col], f"side stats[{name}] B={B} nA={nA} c={ent_coef}")
    within(pen, ref_pen, f"side kl_penalty B={B} nA={nA} c={ent_coef}")
    dh2, stats2, pen2 = run_side(d["z"], c, d["actions"], d["old_log_pac"], d["old_lp"], d["adv"], d["ret"], d["target"],
                                 penalty=False)  # side_penalty is nullable
    assert torch.equal(dh, dh2) and torch.equal(stats, stats2) and bool(torch.isnan(pen2).all())


@pytest.mark.parametrize("B,nA", [(65, 4), (130, 7), (64, 32)])
def test_side_indexed_form_equals_the_gathered_form(B, nA):
    r = rows(3 * B, nA, 3)
    g = torch.Generator().manual_seed(B)
    idx = torch.randperm(3 * B, generator=g)[:B]
    c = dict(nA=nA, vh=2, eps=0.2, ent_coef=0.01, vf_coef=0.5, grad_scale=0.37)
    z = r["z"][:B].contiguous().to(DEV)  # the minibatch's head rows; the per-sample arrays are read through the index
    big = [r[k].to(DEV) for k in ("actions", "old_log_pac", "old_lp", "adv", "ret")]
    gathered = [r[k][idx].contiguous().to(DEV) for k in ("actions", "old_log_pac", "old_lp", "adv", "ret")]
    target = r["target"].to(DEV)
    a = run_side(z, c, *big, target, idx=idx.int().to(DEV))
    b = run_side(z, c, *gathered, target)
    for what, x, y in zip(("dheads", "stats", "kl_penalty"), a, b):
        assert torch.equal(x, y), what
    assert float(a[0][:, :nA].abs().max()) > 0


# ====================================================================== 2. unchanged behaviour
@pytest.mark.parametrize("B,nA", [(65, 6), (130, 7), (63, 18)])
def test_null_target_is_the_ppo_entry_bit_for_bit(B, nA):
    r = rows(B, nA, 4)
    c = dict(nA=nA, vh=2, eps=0.2, ent_coef=0.01, vf_coef=0.5, grad_scale=0.37)
    d = [r[k].to(DEV) for k in ("z", "actions", "old_log_pac", "old_lp", "adv", "ret")]
    dh_s, st_s, pen = run_side(d[0], c, *d[1:], None)
    dh_p, st_p, _ = run_side(d[0], c, *d[1:], None, entry="ppo_ppo_loss_f32")
    assert bool(torch.isfinite(dh_p).all()) and bool(torch.isfinite(st_p).all())
    assert torch.equal(dh_s, dh_p) and torch.equal(st_s, st_p)
    assert bool(torch.isnan(pen).all())  # no target: side_penalty stays untouched
    # ... and the target changes the result (the check above can fail)
    dh_t, st_t, _ = run_side(d[0], c, *d[1:], r["target"].to(DEV))
    assert not torch.equal(dh_t, dh_p) and not torch.equal(st_t[:, 6], st_p[:, 6])


# ---- the fused MLP launches at a tiling-edge shape of tests/mlp_float64_torch.py: F 13 (16-byte weight loads run past the
# rows' ends), NH 7 (scalar stores of heads and dheads), 33 rows (a ragged last tile of one row), relu
SHAPE = M.CASES["ragged-F-33"]
MLP_NA, MLP_VH = 3, 1


@pytest.fixture(scope="module")
def mlp_case():
    F_, H, NH, B = SHAPE["F"], SHAPE["H"], SHAPE["NH"], SHAPE["B"]
    g = torch.Generator().manual_seed(77)

    def rn(*shape, s=1.0):
        return torch.randn(*shape, generator=g) * s

    params = [rn(H, F_, s=1.3 / F_ ** 0.5), rn(H, s=0.1), rn(H, H, s=1.3 / H ** 0.5), rn(H, s=0.1),
              rn(NH, H, s=1.3 / H ** 0.5), rn(NH, s=0.1)]
    x = rn(B, F_)
    with torch.no_grad():
        z = M.mlp_reference([p.double() for p in params], x.double(), "relu")["heads"].float()
    new_lp = F.log_softmax(z[:, :MLP_NA], dim=1)
    actions = torch.randint(0, MLP_NA, (B,), generator=g).int()
    case = dict(params=params, x=x, actions=actions, old_lp=P.tilted_log_policy(z[:, :MLP_NA], g),
                old_log_pac=new_lp[torch.arange(B), actions.long()] + 0.3 * rn(B), adv=rn(B), ret=rn(B, 1),
                target=F.log_softmax(rn(MLP_NA), dim=0))
    case["dev"] = {k: (v.to(DEV) if torch.is_tensor(v) else [p.to(DEV) for p in v]) for k, v in case.items()}
    return case


def mlp_train(case, kind, n_stats, **fields):
    """ppo_mlp_train_f32 on the case's net and rows with the loss `kind` -> heads, dheads, stats rows, their column sums
    and the six gradients, on the device."""
    lib = _lib.load()
    F_, H, NH, B = SHAPE["F"], SHAPE["H"], SHAPE["NH"], SHAPE["B"]
    d = case["dev"]
    w1, b1, w2, b2, wh, bh = d["params"]
    net = _lib.MlpNet(w1=_p(w1), b1=_p(b1), w2=_p(w2), b2=_p(b2), wh=_p(wh), bh=_p(bh), F=F_, H=H, NH=NH, act=2)
    g = {n: torch.full(s, NAN, device=DEV) for n, s in (("dw1", (H, F_)), ("db1", (H,)), ("dw2", (H, H)), ("db2", (H,)),
                                                        ("dwh", (NH, H)), ("dbh", (NH,)))}
    G = _lib.MlpGrads(**{k: _p(v) for k, v in g.items()}, dlog_std=None, n_log_std=0)
    ws = torch.full((int(lib.ppo_mlp_train_workspace_floats(B, F_, H, NH)),), NAN, device=DEV)
    heads, stats = torch.full((B, NH), NAN, device=DEV), torch.full((B, n_stats), NAN, device=DEV)
    sums = torch.full((n_stats,), NAN, device=DEV)
    partials, n_part = torch.zeros(256, device=DEV), ctypes.c_int(-1)
    L = _lib.MlpLoss()
    L.kind, L.grad_scale, L.stats = kind, 0.37, _p(stats)
    for k, v in fields.items():
        setattr(L, k, v)
    rc = lib.ppo_mlp_train_f32(_p(d["x"]), ctypes.addressof(net), ctypes.addressof(G), None, 0, B, ctypes.addressof(L), _p(ws),
                               _p(heads), _p(sums), n_stats, 0, _p(partials), ctypes.byref(n_part), _lib.current_stream())
    _lib.check(rc, "ppo_mlp_train_f32")
    torch.cuda.synchronize()
    return dict(heads=heads, dheads=ws[4 * B * H:4 * B * H + B * NH].view(B, NH).clone(), stats=stats, sums=sums, grads=g)


def ppo_fields(d, **more):
    return dict(n_actions=MLP_NA, n_value_heads=MLP_VH, returns=_p(d["ret"]), vf_coef=0.5, actions_i=_p(d["actions"]),
                old_log_pac=_p(d["old_log_pac"]), old_log_policy=_p(d["old_lp"]), advantages=_p(d["adv"]), eps_clip=0.2,
                ent_coef=0.01, **more)


PPO_C = dict(nA=MLP_NA, vh=MLP_VH, eps=0.2, ent_coef=0.01, vf_coef=0.5, grad_scale=0.37)


def float64_backward(case, heads_dev, dheads64):
    """The six parameter gradients of heads.backward(dheads64) in float64, the ReLU gate taken from the kernel's own
    forward (float64_step of tests/test_mlp_fused_gpu.py)."""
    leaves = [p.double().clone().requires_grad_(True) for p in case["params"]]
    F_, H, NH, B = SHAPE["F"], SHAPE["H"], SHAPE["NH"], SHAPE["B"]
    d = case["dev"]
    w1, b1, w2, b2, wh, bh = d["params"]
    net = _lib.MlpNet(w1=_p(w1), b1=_p(b1), w2=_p(w2), b2=_p(b2), wh=_p(wh), bh=_p(bh), F=F_, H=H, NH=NH, act=2)
    heads, h_pre = torch.empty((B, NH), device=DEV), torch.empty((B, H), device=DEV)
    rc = _lib.load().ppo_mlp_forward_f32(_p(d["x"]), ctypes.addressof(net), None, B, _p(heads), _p(h_pre), None,
                                         _lib.current_stream())
    _lib.check(rc, "ppo_mlp_forward_f32")
    torch.cuda.synchronize()
    gate = (h_pre > 0).cpu()
    fwd = M.mlp_reference(leaves, case["x"].double(), "relu", relu_gate=gate)
    within(heads_dev, fwd["heads"], "fused heads", 1e-4)
    fwd["heads"].backward(dheads64)
    return dict(zip(("dw1", "db1", "dw2", "db2", "dwh", "dbh"), [p.grad for p in leaves]))


def test_fused_ppo_kind_with_zeroed_new_fields_is_unchanged(mlp_case):
    """side_target_logp = NULL: the kind's old code path - the bits of ppo_ppo_loss_f32 on the same head rows (one body,
    csrc/loss_rows.h) - whatever side_penalty holds, and side_penalty is not written."""
    d = mlp_case["dev"]
    B = SHAPE["B"]
    a = mlp_train(mlp_case, _lib.MLP_LOSS_PPO, 8, **ppo_fields(d))
    pen = torch.full((B,), NAN, device=DEV)
    b = mlp_train(mlp_case, _lib.MLP_LOSS_PPO, 8, **ppo_fields(d, side_target_logp=None, side_penalty=_p(pen)))
    assert bool(torch.isnan(pen).all())
    dh, stats, _ = run_side(a["heads"], PPO_C, d["actions"], d["old_log_pac"], d["old_lp"], d["adv"], d["ret"], None,
                            entry="ppo_ppo_loss_f32")
    for x in (a, b):
        assert torch.equal(x["dheads"], dh) and torch.equal(x["stats"], stats)
        assert all(torch.equal(x["grads"][k], a["grads"][k]) and bool(torch.isfinite(x["grads"][k]).all()) for k in a["grads"])


# ====================================================================== 3. fused MLP against the op-by-op launches
def test_fused_side_kind_against_the_loss_launch_and_float64(mlp_case):
    """Bars of tests/test_mlp_fused_gpu.py: dheads and statistics rows 1e-5, gradients 2e-5, statistics column sums 2e-5
    of B x the largest entry."""
    d = mlp_case["dev"]
    B = SHAPE["B"]
    pen = torch.full((B,), NAN, device=DEV)
    got = mlp_train(mlp_case, _lib.MLP_LOSS_PPO, 8, **ppo_fields(d, side_target_logp=_p(d["target"]), side_penalty=_p(pen)))
    dh, stats, pen2 = run_side(got["heads"], PPO_C, d["actions"], d["old_log_pac"], d["old_lp"], d["adv"], d["ret"], d["target"])
    within(got["dheads"], dh, "fused side dheads vs the loss launch")
    within(pen, pen2, "fused side kl_penalty vs the loss launch")
    for col in range(8):
        within(got["stats"][:, col], stats[:, col], f"fused side stats[{col}] vs the loss launch")
    ref_dh, ref_stats, ref_pen = P.ppo_side_ref(got["heads"].cpu(), mlp_case["actions"], mlp_case["old_log_pac"],
                                                mlp_case["old_lp"], mlp_case["adv"], mlp_case["ret"], mlp_case["target"], PPO_C)
    within(got["dheads"], ref_dh, "fused side dheads vs float64")
    within(pen, ref_pen, "fused side kl_penalty vs float64")
    for col in range(8):
        scale = B * max(float(ref_stats[:, col].abs().max()), 1e-30)
        assert abs(float(got["sums"][col]) - float(ref_stats[:, col].sum())) <= 2e-5 * scale, col
    for name, ref in float64_backward(mlp_case, got["heads"], ref_dh).items():
        within(got["grads"][name], ref, f"fused side {name}", 2e-5)


def test_fused_kl_kind_against_the_loss_launch_and_float64(mlp_case):
    d = mlp_case["dev"]
    B = SHAPE["B"]
    got = mlp_train(mlp_case, _lib.MLP_LOSS_POLICY_KL, 1, n_actions=MLP_NA, old_log_policy=_p(d["old_lp"]))
    dh, kl = run_kl(got["heads"], d["old_lp"], MLP_NA, 0.37)
    within(got["dheads"], dh, "fused kl dheads vs the loss launch")
    within(got["stats"][:, 0], kl, "fused kl rows vs the loss launch")
    ref_dh, ref_kl = P.policy_kl_ref(got["heads"].cpu(), mlp_case["old_lp"], MLP_NA, 0.37)
    within(got["dheads"][:, :MLP_NA], ref_dh[:, :MLP_NA], "fused kl dheads vs float64")
    within(got["stats"][:, 0], ref_kl, "fused kl rows vs float64")
    assert float(got["dheads"][:, MLP_NA:].abs().max()) == 0.0
    assert abs(float(got["sums"][0]) - float(ref_kl.sum())) <= 2e-5 * B * float(ref_kl.max())
    refs = float64_backward(mlp_case, got["heads"], ref_dh)
    for name in ("dw1", "db1", "dw2", "db2"):
        within(got["grads"][name], refs[name], f"fused kl {name}", 2e-5)
    within(got["grads"]["dwh"][:MLP_NA], refs["dwh"][:MLP_NA], "fused kl dwh (policy rows)", 2e-5)
    within(got["grads"]["dbh"][:MLP_NA], refs["dbh"][:MLP_NA], "fused kl dbh (policy rows)", 2e-5)
    # parameters the KL does not reach: exact zeros (the value head and every column behind it)
    assert float(got["grads"]["dwh"][MLP_NA:].abs().max()) == 0.0 and float(got["grads"]["dbh"][MLP_NA:].abs().max()) == 0.0


# ====================================================================== 4. the network layer
N_ACTIONS, NB = 6, 8


def make_net(kind):
    torch.manual_seed(11)
    if kind == "impala":  # the smallest geometry whose first convolution has its specialised kernels
        net = models.DualHeadNet("impala", (3, 64, 64), N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda")
        g = torch.Generator().manual_seed(5)
        big = torch.randint(0, 256, (3 * NB, 3, 64, 64), generator=g, dtype=torch.uint8).cuda()
    else:
        net = models.DualHeadNet("mlp", (11,), N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda",
                                 activation_fn="tanh")
        g = torch.Generator().manual_seed(5)
        big = torch.randn((3 * NB, 11), generator=g).cuda()
    net.load_state_dict(T.perturbed_state_dict(net.state_dict(), seed=21))
    idx = torch.randperm(3 * NB, generator=g)[:NB]
    x = big[idx.cuda()].contiguous()
    with torch.no_grad():
        lp = net.forward(x)["log_policy"].cpu()
    old = P.tilted_log_policy(lp, g).cuda()
    return net, big, idx.int().cuda(), x, old


def value_head_grads(net):
    nA = net.n_actions
    return [net.g_w_heads.view(net.nh, -1)[nA:], net.g_b_heads[nA:]]


@pytest.mark.parametrize("kind", ["impala", "mlp-op-by-op"])
def test_policy_kl_minibatch_is_forward_row_and_backward(kind, monkeypatch):
    if kind == "mlp-op-by-op":
        monkeypatch.setattr(models, "FUSE_MLP", 0)
    net, big, idx, x, old = make_net(kind.split("-")[0])
    assert not net.mlp_fused
    net.grad.fill_(NAN)
    kl_m = net.policy_kl_minibatch(x, old, 0.3 / (NB * N_ACTIONS), loss_scale=0.5).clone()
    grad_m = net.grad.clone()
    net.grad.fill_(NAN)
    acts, o, B_, dheads = net._train_forward(x)
    kl = torch.full((NB, 1), NAN, device=DEV)
    net._call("ppo_policy_kl_loss_f32", o.data_ptr(), NB, net.nh, N_ACTIONS, old.data_ptr(), 0.3 / (NB * N_ACTIONS) * 0.5,
              dheads.data_ptr(), kl.data_ptr())
    net.backward(acts, dheads)
    torch.cuda.synchronize()
    assert B_ == NB and float(kl.min()) > 0
    live = torch.isfinite(grad_m)
    assert bool(live.any()) and float(grad_m[live].abs().max()) > 0
    assert torch.equal(kl_m, kl) and torch.equal(torch.nan_to_num(grad_m, nan=-7.0), torch.nan_to_num(net.grad, nan=-7.0))
    for g in value_head_grads(net):
        assert float(g.abs().max()) == 0.0
    if net.takes_obs_index(big):
        net.grad.fill_(NAN)
        kl_i = net.policy_kl_minibatch(big, old, 0.3 / (NB * N_ACTIONS), loss_scale=0.5, index=idx, obs_indexed=True)
        torch.cuda.synchronize()
        assert torch.equal(kl_i, kl) and torch.equal(torch.nan_to_num(grad_m, nan=-7.0), torch.nan_to_num(net.grad, nan=-7.0))
    else:
        assert kind != "impala"
    # the statistic alone: the same rows, and the gradient stays as it is
    before = net.grad.clone()
    kl_r = net.policy_kl_rows(x, old)
    torch.cuda.synchronize()
    assert torch.equal(kl_r, kl) and torch.equal(torch.nan_to_num(before, nan=-7.0), torch.nan_to_num(net.grad, nan=-7.0))


def test_policy_kl_minibatch_on_the_fused_mlp_path():
    """The fused launches against the op-by-op ones of the same net (2e-5 of each gradient's largest entry, the bar of
    check_grads), indexed = gathered bit for bit, exact zeros on the value head."""
    net, big, idx, x, old = make_net("mlp")
    assert net.mlp_fused
    sums = torch.full((1,), NAN, device=DEV)

    def named():
        return {k: v.clone() for k, v in net.grads.items()}
    net.grad.fill_(NAN)
    kl_g = net.policy_kl_minibatch(x, old, 0.3 / (NB * N_ACTIONS), stat_sums=sums).clone()
    grads_g = named()
    net.grad.fill_(NAN)
    kl_i = net.policy_kl_minibatch(big, old, 0.3 / (NB * N_ACTIONS), index=idx, obs_indexed=True).clone()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in grads_g.values())  # every parameter's gradient is written
    assert torch.equal(kl_g, kl_i) and all(torch.equal(v, net.grads[k]) for k, v in grads_g.items())
    assert float(kl_g.min()) > 0 and float(grads_g["encoder.fc1.weight"].abs().max()) > 0
    assert abs(float(sums[0]) - float(kl_g.double().sum())) <= 1e-5 * float(kl_g.double().sum())
    for g in value_head_grads(net):
        assert float(g.abs().max()) == 0.0
    fused = {k: v.clone() for k, v in net.grads.items()}
    net.mlp_fused = False  # the same parameters through the op-by-op launches
    try:
        net.grad.zero_()
        kl_o = net.policy_kl_minibatch(x, old, 0.3 / (NB * N_ACTIONS))
        torch.cuda.synchronize()
        within(kl_g, kl_o, "fused kl rows vs op-by-op")
        for name, ref in net.grads.items():
            if float(ref.abs().max()) == 0.0:
                assert float(fused[name].abs().max()) == 0.0, name
            else:
                within(fused[name], ref, f"fused kl grad {name} vs op-by-op", 2e-5)
    finally:
        net.mlp_fused = True


def test_side_minibatch_is_forward_loss_launch_and_backward():
    """ppo_minibatch with a target: the loss runs as ppo_ppo_loss_side_f32 after the dense + heads launch; without one the
    fused tail is taken as before."""
    net, _big, _idx, x, old = make_net("impala")
    g = torch.Generator().manual_seed(17)
    actions = torch.randint(0, N_ACTIONS, (NB,), generator=g, dtype=torch.int32).cuda()
    old_log_pac = old.gather(1, actions.long()[:, None])[:, 0].contiguous()
    adv, ret = torch.randn(NB, generator=g).cuda(), torch.randn(NB, 1, generator=g).cuda()
    target = F.log_softmax(torch.randn(N_ACTIONS, generator=g), dim=0).cuda()
    pen_m = torch.full((NB,), NAN, device=DEV)
    calls, orig = [], net._call
    net._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
    stats_m = net.ppo_minibatch(x, actions, old_log_pac, old, adv, ret, side_target_logp=target, side_penalty=pen_m).clone()
    grad_m = net.grad.clone()
    assert "ppo_ppo_loss_side_f32" in calls and "ppo_dense_heads_loss_forward_f32" not in calls
    calls.clear()
    net.ppo_minibatch(x, actions, old_log_pac, old, adv, ret)
    net._call = orig
    assert "ppo_dense_heads_loss_forward_f32" in calls and "ppo_ppo_loss_side_f32" not in calls
    assert not torch.equal(net.grad, grad_m)
    acts, o, _B, dheads = net._train_forward(x)
    stats, pen = torch.full((NB, 8), NAN, device=DEV), torch.full((NB,), NAN, device=DEV)
    net._call("ppo_ppo_loss_side_f32", o.data_ptr(), NB, net.nh, N_ACTIONS, net.vh, actions.data_ptr(), old_log_pac.data_ptr(),
              old.data_ptr(), adv.data_ptr(), ret.data_ptr(), 0.2, 0.01, 0.5, 1.0 / NB, dheads.data_ptr(), stats.data_ptr(), None,
              target.data_ptr(), pen.data_ptr())
    net.backward(acts, dheads)
    torch.cuda.synchronize()
    assert torch.equal(stats_m, stats) and torch.equal(pen_m, pen) and torch.equal(grad_m, net.grad)
    with pytest.raises(ValueError):
        net.ppo_minibatch(x, actions, old_log_pac, old, adv, ret, side_target_logp=target[:3].contiguous())
    with pytest.raises(ValueError):
        net.policy_kl_minibatch(x, old[:, :3].contiguous(), 1.0)


# ====================================================================== 5. the reference's recorded minibatch
GOLD = np.load(os.path.join(HERE, "golden", "policy_reg_golden.npz"))
META = json.load(open(os.path.join(HERE, "golden", "policy_reg_golden.json")))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("tag", ["gkl", "side", "both"])
def test_minibatch_equals_the_reference_s(tag):
    """Bars of tests/test_distil_golden_gpu.py: the loss (and global_kl) to 2e-6 of max(1, |value|), gradients to 2e-5 of
    the tensor's largest entry, parameters the reference leaves without a gradient exact zeros."""
    m, MB = META[tag], META["minibatch"]
    args.setup(["--model_encoder=mlp", "--env_type=synthetic", "--seed=7", "--disable_logging=True", "--device=cuda",
                "--model_architecture=single", f"--agents={MB}", "--n_steps=4", f"--policy_opt_mini_batch_size={MB}", *m["flags"]])
    assert args._ignored == []
    assert (bool(args.gkl.enabled), bool(args.side.enabled), args.entropy_bonus) == (m["gkl_enabled"], m["side_enabled"],
                                                                                    m["entropy_bonus"])
    torch.manual_seed(7)
    model = models.TVFModel("mlp", input_dims=tuple(META["input_dims"]), actions=META["n_actions"], device="cuda",
                            architecture="single", hidden_units=META["hidden"], encoder_activation_fn="relu",
                            head_scale=m["head_scale"], head_bias=m["head_bias"], value_head_names=("ext",))
    pol = model.policy_net
    assert pol.mlp_fused
    pol.load_state_dict({name: torch.from_numpy(GOLD[f"init_{name}"]) for name in pol.state_dict()})
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.side_target_policy_logp = cuda(GOLD["side_target_logp"])
    data = {k: cuda(GOLD[k]) for k in ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns")}
    data["*global_states"], data["*global_log_policy"] = cuda(GOLD["global_states"]), cuda(GOLD["global_log_policy"])
    pol.grad.zero_()
    res = r.train_policy_minibatch(data, loss_scale=1.0)
    torch.cuda.synchronize()
    want_loss, want_gkl = GOLD[f"{tag}_result"]
    print(f"{tag}: loss {res['loss']:.9g} (reference {want_loss:.9g}), global_kl {res.get('global_kl')} ({want_gkl:.9g})")
    assert abs(res["loss"] - want_loss) < 2e-6 * max(1, abs(want_loss))
    if m["gkl_enabled"]:
        assert abs(float(res["global_kl"]) - want_gkl) < 2e-6 * max(1, abs(want_gkl))
    else:
        assert "global_kl" not in res
    seen = 0
    for name in pol.params:
        key = f"{tag}_grad_{name}"
        got = pol.grads[name].detach().cpu().numpy()
        if key in GOLD:
            ref = GOLD[key]
            scale = max(float(np.abs(ref).max()), 1e-6)
            err = float(np.abs(got.reshape(ref.shape) - ref).max())
            print(f"{tag} grad {name}: max err {err / scale:.3e} of the largest entry (bar 2e-05)")
            assert err <= 2e-5 * scale, f"grad {name}: max err {err:.3e} vs scale {scale:.3e}"
            seen += 1
        else:
            assert name in m["grad_none"], name
            assert float(np.abs(got).max()) == 0.0, f"{name} should get no gradient"
    assert seen == 8


# ====================================================================== 6. the Runner
class DiscreteFloatVecEnv:
    """Deterministic in-process vector env: flat float observations, discrete actions the reward depends on."""

    def __init__(self, A, dim, seed):
        self.num_envs, self.dim = A, dim
        self.rng = np.random.default_rng(seed)
        self.t = np.zeros(A, np.int64)

    def reset(self):
        self.t[:] = 0
        return self.rng.standard_normal((self.num_envs, self.dim)).astype(np.float32)

    def step(self, actions):
        actions = np.asarray(actions)
        self.t += 1
        rew = (0.5 * (actions % 3) - 0.3 + 0.1 * self.rng.standard_normal(self.num_envs)).astype(np.float32)
        done = self.rng.random(self.num_envs) < 0.1
        infos = [{"time": int(t), "ep_length": int(t), "ep_score": float(t)} for t in self.t]
        self.t[done] = 0
        return self.rng.standard_normal((self.num_envs, self.dim)).astype(np.float32), rew, done, infos


RUNNER_FLAGS = ["--seed=5", "--device=cuda", "--disable_logging=True", "--model_architecture=single", "--env_type=synthetic",
                "--env_embed_time=False", "--model_encoder=mlp", "--model_hidden_units=64", "--agents=8", "--n_steps=8",
                "--policy_opt_mini_batch_size=32", "--max_micro_batch_size=16", "--policy_opt_epochs=2",
                "--policy_opt_lr=0.01"]  # (a large step: the policy moves visibly between minibatches)
GKL_FLAGS = ["--gkl_enabled=True", "--gkl_samples=16", "--gkl_penalty=0.3"]
SHUFFLE_SEED = 31


def make_runner(extra=(), rollout_=True):
    args.setup([*RUNNER_FLAGS, *extra])
    assert args._ignored == []
    torch.manual_seed(5)
    np.random.seed(5)
    model = models.TVFModel("mlp", input_dims=(4,), actions=6, device="cuda", architecture="single", hidden_units=64,
                            encoder_activation_fn="tanh", head_scale=0.1, head_bias=True, value_head_names=("ext",))
    assert model.policy_net.mlp_fused
    r = rollout.Runner(model, logger.Logger(quiet=True))
    if rollout_:
        r.vec_env = DiscreteFloatVecEnv(8, 4, seed=4)
        r.reset()
        r.generate_rollout()
        r.calculate_returns()
        torch.cuda.synchronize()
    return r


def recorded_train(r):
    """r.train() from SHUFFLE_SEED; -> per optimiser step (parameters before it, the gradient handed to it)."""
    steps, orig = [], r.optimizer_step

    def spy(optimizer=None, label="policy", norm_out=None):
        steps.append((r.net.flat.clone(), r.net.grad.clone(), r.net._presummed))
        return orig(optimizer, label, norm_out=norm_out)
    r.optimizer_step = spy
    np.random.seed(SHUFFLE_SEED)
    r.train()
    r.optimizer_step = orig
    torch.cuda.synchronize()
    return steps


def host_replay():
    """The np.random stream of a policy phase with the global KL: the global rows, then one shuffle per epoch."""
    np.random.seed(SHUFFLE_SEED)
    rows_ = np.random.choice(64, 16, replace=False)
    orders = []
    for _ in range(2):
        o = np.arange(64, dtype=np.int32)
        np.random.shuffle(o)
        orders.append(o)
    return rows_, orders, np.random.get_state()


@pytest.fixture(scope="module")
def gkl_run():
    before = {k: getattr(args, k) for k in TOP_LEVEL}  # (a module fixture is set up before the function fixture above)
    r = make_runner(GKL_FLAGS)
    assert r.N * r.A == 64
    steps = recorded_train(r)
    state = np.random.get_state()
    old = r.net._buf("gkl_old_log_policy", (16, 6)).clone()
    stats = r.fetch_stats()
    yield r, steps, state, old, stats
    for k, v in before.items():
        setattr(args, k, v)


def test_global_rows_are_drawn_at_the_reference_s_place_in_the_stream(gkl_run):
    r, steps, state, _old, _stats = gkl_run
    rows_, _orders, want_state = host_replay()
    assert r._gkl_rows.dtype == torch.int32 and np.array_equal(r._gkl_rows.cpu().numpy(), rows_)
    assert len(set(rows_.tolist())) == 16
    assert state[0] == want_state[0] and np.array_equal(state[1], want_state[1]) and state[2:] == want_state[2:]
    assert len(steps) == 4


def test_optimiser_gets_the_sum_of_the_ppo_passes_and_the_kl_pass(gkl_run):
    r, steps, _state, old, _stats = gkl_run
    net = r.net
    rows_, orders, _ = host_replay()
    flat_before, grad_handed, presummed = steps[1]  # the second minibatch: the policy has moved, the KL is not zero
    assert presummed == 0  # three passes contributed: the last pass's sums of g^2 are not the sum's
    saved = net.flat.clone()
    try:
        net.flat.copy_(flat_before)
        net.mark_weights_changed()
        obs = r.all_obs[:r.N].view(64, -1)
        order = torch.from_numpy(orders[0]).cuda()
        passes = []
        for u in range(2):
            idx = order[32 + 16 * u:32 + 16 * (u + 1)].contiguous()
            net.ppo_minibatch(obs, r.actions, r.log_pac, r.log_policy, r.norm_advantage, r.returns, eps_clip=r.ppo_epsilon,
                              ent_coef=r.current_entropy_bonus, vf_coef=args.ppo_vf_coef, loss_scale=0.5, index=idx,
                              obs_indexed=True)
            passes.append(net.grad.clone())
        kl = net.policy_kl_minibatch(obs, old, 0.3 / (16 * 6), index=r._gkl_rows, obs_indexed=True).clone()
        passes.append(net.grad.clone())
        acc = passes[0].clone()
        for g in passes[1:]:
            r._call("ppo_accumulate_f32", _p(acc), _p(g), acc.numel())
        torch.cuda.synchronize()
        assert float(kl.min()) > 1e-7 and float(passes[2].abs().max()) > 0
        assert torch.equal(acc, grad_handed)
        # ... and the first minibatch after the rollout: the policy has not moved, the KL pass adds (next to) nothing
        net.flat.copy_(steps[0][0])
        net.mark_weights_changed()
        kl0 = net.policy_kl_minibatch(obs, old, 0.3 / (16 * 6), index=r._gkl_rows, obs_indexed=True)
        assert float(kl0.abs().max()) < 1e-6
    finally:
        net.flat.copy_(saved)
        net.mark_weights_changed()


def test_statistics_of_the_global_kl(gkl_run):
    r, steps, _state, old, stats = gkl_run
    net = r.net
    obs = r.all_obs[:r.N].view(64, -1)
    saved = net.flat.clone()
    sums = []
    try:
        for flat_before, _g, _ps in steps:
            net.flat.copy_(flat_before)
            net.mark_weights_changed()
            sums.append(float(net.policy_kl_rows(obs, old, index=r._gkl_rows, obs_indexed=True).double().sum()))
    finally:
        net.flat.copy_(saved)
        net.mark_weights_changed()
    want = np.mean([0.3 * s / (16 * 6) for s in sums])
    print(f"*loss_gkl {stats['*loss_gkl']:.9g}, by hand {want:.9g}; per minibatch sums of kl {sums}")
    # 16 float32 terms per sum, the sums then taken in float64: 1e-5 relative (the bar of a statistics column sum)
    assert want > 0 and abs(stats["*loss_gkl"] - want) <= 1e-5 * want
    assert abs(stats["global_kl"] - want / 0.3) <= 1e-5 * want / 0.3
    rows_, _norms, mb = r._phase_stats["policy"]
    gain = (rows_.cpu().numpy().astype(np.float64)[:, 6] / mb).mean()
    assert stats["loss_policy"] == pytest.approx(gain - stats["*loss_gkl"], abs=1e-12)
    assert stats["loss_policy"] < gain


def test_penalty_zero_trains_as_without_the_global_kl():
    r0 = make_runner(GKL_FLAGS[:2] + ["--gkl_penalty=0"])
    steps0 = recorded_train(r0)
    stats0 = r0.fetch_stats()
    r1 = make_runner()
    # without the global KL no rows are drawn: draw them by hand so that both runs shuffle alike
    steps1, orig = [], r1.optimizer_step

    def spy(optimizer=None, label="policy", norm_out=None):
        steps1.append(r1.net._presummed)
        return orig(optimizer, label, norm_out=norm_out)
    r1.optimizer_step = spy
    np.random.seed(SHUFFLE_SEED)
    np.random.choice(64, 16, replace=False)
    r1.train()
    torch.cuda.synchronize()
    stats1 = r1.fetch_stats()
    assert len(steps0) == 4 and len(steps1) == 4
    assert torch.equal(r0.net.flat, r1.net.flat) and torch.equal(r0.net.exp_avg, r1.net.exp_avg)
    assert "*loss_gkl" not in stats0 and "global_kl" in stats0 and "global_kl" not in stats1
    assert stats0["global_kl"] > 0  # the statistic is still produced (the policy moved after the first minibatch)
    assert stats0["loss_policy"] == stats1["loss_policy"]


def test_side_target_is_redrawn_every_period_rollouts():
    r = make_runner(["--side_enabled=True", "--side_period=2", "--side_noise_std=1.0", "--disable_logging=False"])
    assert r.side_target_policy_logp is None
    targets = []
    for counter in range(5):
        assert r.batch_counter == counter
        np.random.seed(SHUFFLE_SEED)
        r.train()
        t = r.side_target_policy_logp
        assert t.shape == (6,) and t.is_cuda and abs(float(t.exp().sum()) - 1.0) < 1e-5
        targets.append(t.clone())
    stats = r.fetch_stats()
    for counter in range(1, 5):
        assert torch.equal(targets[counter], targets[counter - 1]) == (counter % 2 != 0), counter
    # kl_penalty = KL(new || target) - H >= -H >= -log(6); its mean is logged through the statistics path, the target's
    # entropy at draw time
    assert np.isfinite(stats["side_kl_penalty"]) and stats["side_kl_penalty"] >= -np.log(6) - 1e-6
    drawn = [float(-(t.double().exp() * t.double()).sum()) for t in targets[::2]]  # one entry per draw
    assert r.log["side_target_entropy"] == pytest.approx(np.mean(drawn), rel=1e-6)
    assert r.log.vars["side_target_entropy"].display_name == "ste" and r.log.vars["side_kl_penalty"].display_name == "skl"
    assert "*loss_gkl" not in stats and "global_kl" not in stats


def test_refusals(monkeypatch):
    with pytest.raises(ValueError, match="exceeds the rollout"):
        make_runner(["--gkl_enabled=True", "--gkl_samples=65"], rollout_=False)
    with pytest.raises(ValueError, match="multiple"):
        make_runner(["--gkl_enabled=True", "--gkl_samples=24"], rollout_=False)
    monkeypatch.setattr(rollout.parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        make_runner(GKL_FLAGS, rollout_=False)
