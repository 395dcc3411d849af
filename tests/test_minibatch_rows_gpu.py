"""GPU: which rows a training minibatch reads.  A minibatch picks its rows in three ways - the gather launch
(ppo_gather_rows), the first convolution reading uint8 images through the permutation, the fused MLP reading float rows
through it - while every loss kernel reads its per-sample arrays through the same `index`.  If the observation side and
the loss side disagree, observation b is paired with another sample's action, advantage and return: nothing crashes, the
run learns from noise.  So every indexed read is tested here, and in particular the case the other files leave out: the
minibatch that IS the whole batch (a permutation of all its rows), which the host once told apart from a gathered
minibatch by comparing shapes.  `obs_indexed=True` now says that `prev_state` is the array `index` points into.

Rules of this file: seeded generators only; every permutation moves at least 90 % of its rows (asserted: a permutation
close to the identity would hide a wrong pairing); references are float64 torch on the CPU, or the reference's recorded
gradients in tests/golden/variants_golden.npz."""
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from ppo_amd import _lib, envs, logger, models, rollout  # noqa: E402
from ppo_amd.config import args  # noqa: E402
from mlp_float64_torch import LOG_SQRT_2PI, distil_loss_ref, gaussian_loss_ref, value_loss_ref  # noqa: E402

HERE = os.path.dirname(__file__)
GOLD = np.load(os.path.join(HERE, "golden", "variants_golden.npz"))
META = json.load(open(os.path.join(HERE, "golden", "variants_golden.json")))
DEV = "cuda"


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return _lib.current_stream()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def moving_perm(n, g):
    """A permutation of n rows that is ONE random cycle: for n > 1 every row moves."""
    order = torch.randperm(n, generator=g)
    perm = torch.empty(n, dtype=torch.int64)
    perm[order] = order.roll(-1)
    return perm


def assert_moves(idx):
    """At least 90 % of the minibatch rows b read another row than b."""
    idx = torch.as_tensor(idx).cpu().long()
    n = idx.numel()
    moved = int((idx != torch.arange(n)).sum())
    assert moved >= 0.9 * n, f"only {moved} of {n} rows move"


def scatter(t, perm):
    """Row perm[b] of the result holds row b of t (perm: a permutation of all rows)."""
    out = torch.empty_like(t)
    out[perm.to(t.device)] = t
    return out


# ====================================================================== a. fused MLP, minibatch equal to batch
def build(tag):
    """As tests/test_variants_gpu.py: the reference's seeded MLP variant `tag`."""
    m = META[tag]
    tvf = f"{tag}_tvf_horizons" in GOLD
    torch.manual_seed(7)
    model = models.TVFModel(
        "mlp", input_dims=tuple(m["input_dims"]), actions=m["n_actions"], device="cuda", architecture="dual",
        hidden_units=m["hidden"], encoder_activation_fn=m["activation"], head_scale=m["head_scale"],
        head_bias=m["head_bias"], tvf_fixed_head_horizons=list(GOLD[f"{tag}_tvf_horizons"]) if tvf else None,
        tvf_fixed_head_weights=list(GOLD[f"{tag}_tvf_weights"]) if tvf else None)
    assert model.policy_net.mlp_fused == bool(models.FUSE_MLP) and model.value_net.mlp_fused == bool(models.FUSE_MLP)
    if f"{tag}_log_std" in GOLD:
        model.policy_net.params["log_std"].copy_(cuda(GOLD[f"{tag}_log_std"]))
    return model, m


def close(a, want, tol, what):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(a.reshape(want.shape) - want).max())
    print(f"{what}: max err {err:.3e} = {err / scale:.3e} of the largest entry (bar {tol:.0e})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def check_grads(net, tag, phase, m, tol=2e-5):
    """As tests/test_variants_gpu.py: every parameter gradient against the reference's, 2e-5 of its largest entry."""
    none = set(m.get("grad_none", {}).get(f"{tag}_{phase}", []))
    seen = 0
    for name in net.params:
        key = f"{tag}_{phase}_grad_{name}"
        if key in GOLD:
            close(net.grads[name], GOLD[key], tol, f"{phase} grad {name}")
            seen += 1
        else:
            assert name in none, name
            assert float(net.grads[name].abs().max()) == 0.0, f"{phase}: {name} should get no gradient"
    assert seen >= 6


MLP_CASES = [("mlp_disc", "policy"), ("mlp_disc", "value"), ("mlp_disc", "distil"),
             ("mlp_gauss_tvf", "policy"), ("mlp_gauss_tvf", "value"), ("mlp_gauss_tvf", "distil")]


def mlp_phase(tag, phase, model, m):
    """(net, statistics columns, per-sample arrays, call(x, arrays, **kw) -> statistics rows) of one training phase of
    the fixture `tag`, with the arguments tests/test_variants_gpu.py passes."""
    def G(k):
        return cuda(GOLD[f"{tag}_{k}"])

    pol, val = model.policy_net, model.value_net
    if phase == "value":
        if tag == "mlp_disc":
            return val, 4, [G("value_returns")], lambda x, r, **kw: val.value_minibatch(
                x, returns=r[0], vf_coef=m["ppo_vf_coef"], **kw)
        w = G("tvf_weights")
        return val, 4, [G("value_returns"), G("value_tvf_returns")], lambda x, r, **kw: val.value_minibatch(
            x, returns=r[0], tvf_returns=r[1], tvf_weights=w, vf_coef=m["ppo_vf_coef"], tvf_coef=m["tvf_coef"], **kw)
    if tag == "mlp_disc":
        if phase == "policy":
            rows = [G("policy_actions").int(), G("policy_log_pac"), G("policy_log_policy"), G("policy_advantages")]
            return pol, 8, rows, lambda x, r, **kw: pol.ppo_minibatch(
                x, r[0], r[1], r[2], r[3], None, eps_clip=m["ppo_epsilon"], ent_coef=m["entropy_bonus"], vf_coef=0.0, **kw)
        rows = [G("distil_distil_targets"), G("distil_old_log_policy")]
        return pol, 4, rows, lambda x, r, **kw: pol.distil_minibatch(x, r[0], r[1], beta=m["distil_beta"], **kw)
    if phase == "policy":
        rows = [G("policy_actions"), G("policy_log_pac"), G("policy_advantages")]
        return pol, 8, rows, lambda x, r, **kw: pol.gaussian_minibatch(
            x, r[0], r[1], r[2], None, eps_clip=m["ppo_epsilon"], **kw)
    w = G("tvf_weights")
    rows = [G("distil_distil_targets"), G("distil_old_raw_policy")]
    return pol, 4, rows, lambda x, r, **kw: pol.distil_minibatch(
        x, r[0], r[1], beta=m["distil_beta"], use_tvf=True, weights=w, gaussian=True, **kw)


@pytest.mark.parametrize("tag,phase", MLP_CASES)
def test_fused_mlp_whole_batch_minibatch_reads_rows_through_the_permutation(monkeypatch, tag, phase):
    """Minibatch = batch on the fused MLP launches, every loss kind: observations and per-sample arrays scattered so
    that row perm[b] holds sample b, read back with index=perm, obs_indexed=True.  Gradient buffer and statistics rows
    are the bits of the plain call on the unscattered arrays (a net that took the scattered observations in order would
    pair observation perm^-1[b] with sample b's targets); the reference's gradients hold at check_grads' 2e-5."""
    monkeypatch.setattr(models, "FUSE_MLP", 1)
    model, m = build(tag)
    net, n_stats, rows, call = mlp_phase(tag, phase, model, m)
    x = cuda(GOLD[f"{tag}_x"])
    MB = x.shape[0]
    net.grad.zero_()
    s_plain = call(x, rows).clone()
    g_plain = net.grad.clone()
    check_grads(net, tag, phase, m)
    assert s_plain.shape == (MB, n_stats)

    perm = moving_perm(MB, torch.Generator().manual_seed(11))
    assert_moves(perm)
    assert torch.equal(perm.sort().values, torch.arange(MB))  # all MB rows: minibatch = batch
    xs, rs = scatter(x, perm), [scatter(r, perm) for r in rows]
    idx = perm.int().cuda()
    assert xs.shape[0] == idx.shape[0] == MB
    net.grad.zero_()
    sums = torch.full((n_stats,), 7.0, device="cuda")
    s_idx = call(xs, rs, index=idx, obs_indexed=True, stat_sums=sums).clone()
    torch.cuda.synchronize()
    gmax = float(g_plain.abs().max())
    print(f"{tag}/{phase}: indexed vs plain gradient max |diff| = {float((net.grad - g_plain).abs().max()) / gmax:.3e} of "
          f"the largest entry; statistics max |diff| = {float((s_idx - s_plain).abs().max()):.3e}")
    assert torch.equal(net.grad, g_plain), "the whole-batch minibatch did not read its observations through the index"
    assert torch.equal(s_idx, s_plain)
    check_grads(net, tag, phase, m)
    assert torch.allclose(sums, s_idx.sum(0), rtol=1e-5, atol=1e-6)  # overwritten, not added to

    # the gathered minibatch: the index applies to the per-sample arrays only
    net.grad.zero_()
    call(xs[idx.long()].contiguous(), rs, index=idx, obs_indexed=False)
    check_grads(net, tag, phase, m)
    # what prev_state holds is said, never inferred
    with pytest.raises(ValueError):
        call(xs, rs, obs_indexed=True)  # no index to read through
    with pytest.raises(ValueError):
        call(xs, rs, index=idx[:MB // 2].contiguous())  # 32 rows are not a gathered minibatch of 16


@pytest.mark.parametrize("tag,phase", MLP_CASES)
def test_op_by_op_mlp_refuses_indexed_observations_and_takes_the_gathered_minibatch(monkeypatch, tag, phase):
    """The op-by-op MLP path cannot read observations through an index: asked to (obs_indexed=True) it raises, also
    when the array has as many rows as the minibatch; given the gathered rows and the index for the per-sample arrays
    it meets the reference's gradients."""
    monkeypatch.setattr(models, "FUSE_MLP", 0)
    model, m = build(tag)
    net, _n_stats, rows, call = mlp_phase(tag, phase, model, m)
    x = cuda(GOLD[f"{tag}_x"])
    perm = moving_perm(x.shape[0], torch.Generator().manual_seed(11))
    assert_moves(perm)
    xs, rs = scatter(x, perm), [scatter(r, perm) for r in rows]
    idx = perm.int().cuda()
    with pytest.raises(ValueError):
        call(xs, rs, index=idx, obs_indexed=True)
    net.grad.zero_()
    call(xs[idx.long()].contiguous(), rs, index=idx, obs_indexed=False)
    check_grads(net, tag, phase, m)


# ====================================================================== b. IMPALA uint8, minibatch equal to batch
def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize("dims,nA,B", [((4, 84, 84), 6, 5), ((4, 84, 84), 6, 32), ((3, 64, 64), 15, 32)])
def test_impala_whole_batch_minibatch_reads_images_through_the_permutation(dims, nA, B):
    """uint8 images, idx a permutation of ALL B rows: the first convolution and its weight gradient read the batch
    through idx (both indexed entry points run) and give the bits of the gathered minibatch.  Then the gradient itself:
    float64 autograd on the CPU of the same function - obs[idx] / 255 paired with the arrays read through idx, ReLU masks
    and max-pool taps taken from the HIP forward's own saved maps (oracle/model_torch.forward_shared_kinks) - to 1e-5 of
    each gradient's largest entry, the bar of test_model_gpu.py::test_backward_is_exact_given_shared_kinks.  The float64
    gradient of the WRONG pairing (observations in order, arrays through idx) is more than 100 bars away on the dense
    layer: this test can fail."""
    from oracle import model_torch as R
    torch.manual_seed(5)
    net = models.DualHeadNet("impala", dims, nA, hidden_units=256, head_scale=0.1, head_bias=True, device="cuda")
    g = torch.Generator().manual_seed(B + nA)
    obs = torch.randint(0, 256, (B, *dims), dtype=torch.uint8, generator=g).cuda()
    perm = moving_perm(B, g)
    assert_moves(perm)
    idx = perm.int().cuda()
    actions = torch.randint(0, nA, (B,), generator=g).int().cuda()
    adv = torch.randn(B, generator=g).cuda()
    ret = torch.randn(B, 1, generator=g).cuda()
    lp = torch.log_softmax(torch.randn(B, nA, generator=g), dim=1).cuda()
    pac = lp.gather(1, actions.long()[:, None])[:, 0].contiguous()
    assert net.takes_obs_index(obs)
    gathered = obs[idx.long()].contiguous()
    net.grad.zero_()
    s_g = net.ppo_minibatch(gathered, actions, pac, lp, adv, ret, index=idx).clone()
    g_g = net.grad.clone()
    calls = []
    orig = net._call
    net._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
    net.grad.zero_()
    s_i = net.ppo_minibatch(obs, actions, pac, lp, adv, ret, index=idx, obs_indexed=True).clone()
    net._call = orig
    torch.cuda.synchronize()
    gmax = float(g_g.abs().max())
    print(f"indexed vs gathered: gradient max |diff| = {float((net.grad - g_g).abs().max()) / gmax:.3e} of the largest "
          f"entry, statistics max |diff| = {float((s_i - s_g).abs().max()):.3e}")
    assert "ppo_conv3x3_pool_forward_packed_indexed_f32" in calls
    assert "ppo_conv3x3_backward_weight_slabs_pooled_indexed_f32" in calls
    assert gmax > 0
    assert torch.equal(s_g, s_i) and torch.equal(g_g, net.grad)
    got = {k: v.detach().cpu().numpy().copy() for k, v in net.grads.items()}
    # the index was an argument of that call and nothing of it stays on the net: a plain gathered minibatch afterwards
    # gives the gathered bits again
    net.grad.zero_()
    s_n = net.ppo_minibatch(gathered, actions, pac, lp, adv, ret, index=idx).clone()
    assert torch.equal(s_g, s_n) and torch.equal(g_g, net.grad)
    assert not [a for a in ("obs_index", "loss_tail", "act_tail", "allow_chain_split") if hasattr(net, a)]

    def float64_grads(images, kinks):
        """d ppo_loss / d parameters in float64 on the CPU: row b = images[b] with the kinks of `kinks`, paired with the
        per-sample arrays read through idx."""
        sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in net.params.items()}
        kinks = {k: v.cpu() for k, v in kinks.items() if torch.is_tensor(v)}
        i = perm
        out = R.forward_shared_kinks(sd, images.cpu().double() / 255.0, kinks)
        R.ppo_loss(out, actions.cpu().long()[i], pac.cpu().double()[i], adv.cpu().double()[i],
                   ret.cpu().double()[i]).backward()
        return {k: (None if p.grad is None else p.grad.numpy()) for k, p in sd.items()}

    # the saved maps of the minibatch's forward (same buffers, same values: bit-identical to the indexed call's, above)
    right = float64_grads(gathered, net.encode(gathered, train=True))
    wrong = float64_grads(obs, net.encode(obs, train=True))
    worst = 0.0
    for name, ref in right.items():
        if ref is None:
            assert float(np.abs(got[name]).max()) == 0.0, name
            continue
        e = rel_err(got[name], ref)
        worst = max(worst, e)
        assert e < 1e-5, (name, e)
    apart = rel_err(wrong["encoder.dense.weight"], right["encoder.dense.weight"])
    print(f"worst gradient rel err vs float64: {worst:.3e}; the wrong pairing's dense gradient is {apart:.3e} away")
    assert apart > 100 * 1e-5


# ====================================================================== c. through the runner
IMPALA_FLAGS = ["--agents=16", "--n_steps=16", "--model_architecture=single", "--model_encoder=impala",
                "--env_type=synthetic", "--env_embed_time=False", "--seed=6", "--device=cuda",
                "--policy_opt_mini_batch_size=256", "--policy_opt_epochs=1", "--disable_logging=True"]


def make_impala_runner():
    """As make() of tests/test_train_batch_gpu.py, with one minibatch = the whole rollout of 16 x 16 samples."""
    args.setup(IMPALA_FLAGS)
    torch.manual_seed(6)
    shape, nA = envs.get_env_spec()
    model = models.TVFModel("impala", input_dims=shape, actions=nA, device="cuda", architecture="single",
                            hidden_units=256, head_scale=0.1, head_bias=True)
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = envs.create_envs_classic()
    r.reset()
    np.random.seed(6)
    r.generate_rollout()
    r.calculate_returns()
    return r


def epoch_shuffle(seed, n):
    """The epoch's permutation as Runner._run_epochs draws it (its first draw from np.random)."""
    np.random.seed(seed)
    order = np.arange(n, dtype=np.int32)
    np.random.shuffle(order)
    return order


def test_runner_impala_whole_batch_minibatch_equals_the_gather_launch_path(monkeypatch):
    """Runner.train with minibatch = batch: the default path (images read through the permutation inside the first
    convolution) against the gather launch (GATHER_IN_CONV = 0) - same seeds, same shuffle - bit for bit: parameters,
    first moments (the clipped gradient) and the policy statistics."""
    assert_moves(epoch_shuffle(77, 256))
    out = []
    for in_conv in (1, 0):
        monkeypatch.setattr(models, "GATHER_IN_CONV", in_conv)
        r = make_impala_runner()
        assert r.N * r.A == 256 and bool(r.net.takes_obs_index(r.all_obs)) == bool(in_conv)
        calls = []
        orig = r._call
        r._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
        np.random.seed(77)
        r.train()
        r._call = orig
        torch.cuda.synchronize()
        assert ("ppo_gather_rows" in calls) == (not in_conv)
        assert r.net._adam_step == 1
        rows, norms, mb = r._phase_stats["policy"]
        assert mb == 256 and rows.shape == (1, 8)
        out.append((r.net.flat.clone(), r.net.exp_avg.clone(), rows.clone(), norms.clone(), r.fetch_stats()))
    (flat_a, m_a, rows_a, norm_a, st_a), (flat_b, m_b, rows_b, norm_b, st_b) = out
    mmax = float(m_b.abs().max())
    print(f"in-conv vs gather: exp_avg max |diff| = {float((m_a - m_b).abs().max()) / mmax:.3e} of the largest entry, "
          f"statistics {rows_a.tolist()} vs {rows_b.tolist()}")
    assert mmax > 0
    assert torch.equal(flat_a, flat_b) and torch.equal(m_a, m_b)
    assert torch.equal(rows_a, rows_b) and torch.equal(norm_a, norm_b)
    assert st_a == st_b


class DiscreteFloatVecEnv:
    """Deterministic in-process vector env: flat float observations, two discrete actions (the float counterpart,
    FloatVecEnv of tests/test_runner_modes_gpu.py, takes continuous ones)."""

    def __init__(self, A, dim, seed):
        self.num_envs, self.dim = A, dim
        self.rng = np.random.default_rng(seed)
        self.t = np.zeros(A, np.int64)

    def reset(self):
        self.t[:] = 0
        return self.rng.standard_normal((self.num_envs, self.dim)).astype(np.float32)

    def step(self, actions):
        actions = np.asarray(actions).reshape(self.num_envs)
        assert set(np.unique(actions).tolist()) <= {0, 1}
        self.t += 1
        rew = (1.0 - 0.5 * actions).astype(np.float32)
        done = self.rng.random(self.num_envs) < 0.05
        infos = [{"time": int(t), "ep_length": int(t), "ep_score": float(t)} for t in self.t]
        self.t[done] = 0
        return self.rng.standard_normal((self.num_envs, self.dim)).astype(np.float32), rew, done, infos


def test_runner_mlp_whole_batch_minibatch_fused_path_equals_the_op_by_op_path(monkeypatch):
    """Float observations, single architecture, discrete actions, 8 x 32 = 256 samples in ONE minibatch: the fused MLP
    path (rows read through the permutation) against the op-by-op path (gather launch).  After the single optimiser
    step exp_avg = (1 - beta1) x the clipped gradient.  Each path is held to 2e-5 of the reference gradient's largest
    entry by check_grads, so two correct paths differ by at most 4e-5; a margin of 2.5 for the clip factor: 1e-4.
    Gradient norms: 2e-6 relative, the bar of test_variants_gpu.py for two reductions of one gradient."""
    assert_moves(epoch_shuffle(77, 256))
    out = []
    for fuse in (1, 0):
        monkeypatch.setattr(models, "FUSE_MLP", fuse)
        args.setup(["--agents=8", "--n_steps=32", "--model_architecture=single", "--model_encoder=mlp",
                    "--model_hidden_units=64", "--env_type=classic", "--env_name=CartPole", "--seed=9", "--device=cuda",
                    "--policy_opt_mini_batch_size=256", "--policy_opt_epochs=1", "--env_reward_normalization=off",
                    "--disable_logging=True"])
        torch.manual_seed(9)
        np.random.seed(9)
        model = models.TVFModel("mlp", input_dims=(4,), actions=2, device="cuda", architecture="single", hidden_units=64,
                                head_scale=0.1, head_bias=True)
        assert model.policy_net.mlp_fused == bool(fuse)
        r = rollout.Runner(model, logger.Logger(quiet=True))
        r.vec_env = DiscreteFloatVecEnv(8, 4, seed=4)
        r.reset()
        r.generate_rollout()
        r.calculate_returns()
        assert r.N * r.A == 256 and r.all_obs.dtype == torch.float32
        calls = []
        orig = r._call
        r._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
        np.random.seed(77)
        r.train()
        r._call = orig
        torch.cuda.synchronize()
        assert ("ppo_gather_rows" in calls) == (not fuse)
        assert r.net._adam_step == 1
        _rows, norms, mb = r._phase_stats["policy"]
        assert mb == 256 and norms.shape == (1,)
        out.append((r.actions.clone(), r.net.exp_avg.clone(), float(norms[0])))
    (act_a, m_a, norm_a), (act_b, m_b, norm_b) = out
    assert torch.equal(act_a, act_b), "the two rollouts drew different actions: nothing to compare"
    mmax = float(m_b.abs().max())
    print(f"fused vs op-by-op: exp_avg max |diff| = {float((m_a - m_b).abs().max()) / mmax:.3e} of the largest entry "
          f"(bar 1e-4), gradient norms {norm_a:.9g} vs {norm_b:.9g}: {abs(norm_a - norm_b) / norm_b:.3e} relative (bar 2e-6)")
    assert mmax > 0 and norm_b > 0
    assert float((m_a - m_b).abs().max()) <= 1e-4 * mmax
    assert abs(norm_a - norm_b) <= 2e-6 * norm_b


# ====================================================================== d. the loss kernels' index, against float64
SHAPES = [(B, f) for B in (1, 37, 256) for f in (1, 3)]  # (minibatch rows, source rows / minibatch rows)


def selection(B, factor, g):
    """[B] int32 rows of a source of factor * B rows: a permutation of all of them (factor 1) or a selection; every
    row moves (the one permutation of a single row cannot)."""
    idx = moving_perm(B * factor, g)[:B].contiguous()
    if B * factor > 1:
        assert_moves(idx)
    return idx


def within(got, ref, what, tol=1e-5):
    """|got - ref| <= tol x the largest |ref|."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got - ref).abs().max())
    print(f"{what}: max err {err / scale:.3e} of the largest entry (bar {tol:.0e})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


VAL = dict(ldo=20, value_col=3, vh=2, tvf_col=6, K=5, stride=2, vf_coef=0.5, tvf_coef=0.7, grad_scale=0.37)


def run_value_loss(z, ret, tvf_ret, w, idx, c, keep=1.0, seed=0, offset=0):
    B = z.shape[0]
    dh = torch.full((B, c["ldo"]), float("nan"), device=DEV)
    stats = torch.full((B, 4), float("nan"), device=DEV)
    rc = _lib.load().ppo_value_loss_f32(_p(z), B, c["ldo"], c["value_col"], c["vh"], _p(ret), c["vf_coef"], c["tvf_col"],
                                        c["K"], c["stride"], _p(tvf_ret), _p(w), c["tvf_coef"], c["grad_scale"], _p(dh),
                                        _p(stats), _p(idx), keep, seed, offset, _st())
    _lib.check(rc, "ppo_value_loss_f32")
    torch.cuda.synchronize()
    return dh, stats


@pytest.mark.parametrize("B,factor", SHAPES)
def test_value_loss_index_against_float64(B, factor):
    """ppo_value_loss_f32: 2 value heads, 5 TVF heads at stride 2 with their own weights, a row of 20 columns of which
    7 are used; per-sample arrays of factor * B rows read through the index."""
    c = VAL
    g = torch.Generator().manual_seed(100 + 7 * B + factor)
    Bt = B * factor
    z = torch.randn(B, c["ldo"], generator=g) * 1.5
    ret_big = torch.randn(Bt, c["vh"], generator=g)
    tvf_big = torch.randn(Bt, c["K"], generator=g) * 2.0
    w = torch.rand(c["K"], generator=g) + 0.25
    idx = selection(B, factor, g)
    want_dh, want_st = value_loss_ref(z, ret_big[idx], tvf_big[idx], w, c, torch.float64)
    zd, wd, idxd = z.cuda(), w.cuda(), idx.int().cuda()
    ret_d, tvf_d = ret_big.cuda(), tvf_big.cuda()
    dh, st = run_value_loss(zd, ret_d, tvf_d, wd, idxd, c)
    within(dh, want_dh, "dheads")
    used = torch.zeros(c["ldo"], dtype=torch.bool)
    used[c["value_col"]:c["value_col"] + c["vh"]] = True
    used[c["tvf_col"]:c["tvf_col"] + c["K"] * c["stride"]:c["stride"]] = True
    assert int(used.sum()) == 7 and not used[15:].any()
    assert float(dh[:, ~used.cuda()].abs().max()) == 0.0  # exact zeros (NaN before), the tail of the row included
    for col, name in enumerate(("value loss", "TVF loss", "total")):
        within(st[:, col], want_st[:, col], name)
    assert float(st[:, 3].abs().max()) == 0.0
    ret_g, tvf_g = ret_d[idxd.long()].contiguous(), tvf_d[idxd.long()].contiguous()
    dh2, st2 = run_value_loss(zd, ret_g, tvf_g, wd, None, c)
    assert torch.equal(dh, dh2) and torch.equal(st, st2)


def test_value_loss_horizon_dropout_by_property():
    """tvf_keep_prob = 0.5 over 256 x 64 (sample, head) terms.  The counter-based generator cannot be reproduced on the
    host, so: every TVF entry of dheads is an exact 0 or twice the undropped entry (1e-5), the kept share is within 4
    sigma of the binomial (0.5 +- 0.0157 for 16384 draws), the draw is keyed by (seed, offset) and the minibatch row -
    the same bits whether the targets are read through the index or gathered - and another offset draws another mask."""
    c = dict(ldo=68, value_col=0, vh=2, tvf_col=2, K=64, stride=1, vf_coef=0.5, tvf_coef=0.7, grad_scale=0.37)
    B, factor = 256, 3
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(B, c["ldo"], generator=g) * 1.5).cuda()
    ret_big = torch.randn(B * factor, c["vh"], generator=g).cuda()
    tvf_big = (torch.randn(B * factor, c["K"], generator=g) * 2.0).cuda()
    w = (torch.rand(c["K"], generator=g) + 0.25).cuda()
    idx = selection(B, factor, g).int().cuda()
    full, _ = run_value_loss(z, ret_big, tvf_big, w, idx, c)
    drop, st = run_value_loss(z, ret_big, tvf_big, w, idx, c, keep=0.5, seed=1234, offset=640)
    tv = slice(c["tvf_col"], c["tvf_col"] + c["K"])
    assert torch.equal(drop[:, :c["tvf_col"]], full[:, :c["tvf_col"]])  # the value heads are not dropped
    assert float(drop[:, c["tvf_col"] + c["K"]:].abs().max()) == 0.0
    f, d = full[:, tv].double(), drop[:, tv].double()
    assert bool((f != 0).all())
    kept = d != 0
    assert bool(((d - 2 * f).abs() <= 1e-5 * (2 * f).abs())[kept].all())
    share = float(kept.double().mean())
    print(f"kept share {share:.4f}")
    assert abs(share - 0.5) <= 4 * math.sqrt(0.25 / (B * c["K"]))
    assert torch.isfinite(st).all()
    ret_g, tvf_g = ret_big[idx.long()].contiguous(), tvf_big[idx.long()].contiguous()
    again, st2 = run_value_loss(z, ret_g, tvf_g, w, None, c, keep=0.5, seed=1234, offset=640)
    assert torch.equal(again, drop) and torch.equal(st2, st)
    other, _ = run_value_loss(z, ret_big, tvf_big, w, idx, c, keep=0.5, seed=1234, offset=640 + B * c["K"])
    other_kept = other[:, tv] != 0
    assert not torch.equal(other_kept, kept)
    assert bool(((other[:, tv].double() - 2 * f).abs() <= 1e-5 * (2 * f).abs())[other_kept].all())


def run_distil_loss(z, targets, old, w, log_std, idx, c):
    B = z.shape[0]
    dh = torch.full((B, c["ldo"]), float("nan"), device=DEV)
    stats = torch.full((B, 4), float("nan"), device=DEV)
    rc = _lib.load().ppo_distil_loss_f32(_p(z), B, c["ldo"], c["nA"], c["pred_col"], c["n_pred"], c["stride"], c["vector"],
                                         _p(targets), _p(w), _p(old), _p(log_std), c["beta"], c["grad_scale"], _p(dh),
                                         _p(stats), _p(idx), _st())
    _lib.check(rc, "ppo_distil_loss_f32")
    torch.cuda.synchronize()
    return dh, stats


@pytest.mark.parametrize("B,factor", SHAPES)
@pytest.mark.parametrize("targets", ["tvf", "ext"])
@pytest.mark.parametrize("form", ["kl_policy", "gaussian"])
def test_distil_loss_index_against_float64(form, targets, B, factor):
    """ppo_distil_loss_f32, both policy terms (KL on 6 discrete actions; gaussian means of 3 actions with log_std),
    vector targets on 5 TVF heads at stride 2 with weights, or one scalar target; row longer than the columns used."""
    nA = 6 if form == "kl_policy" else 3
    c = dict(ldo=nA + 16, nA=nA, pred_col=nA + 2, n_pred=5 if targets == "tvf" else 1, stride=2 if targets == "tvf" else 1,
             vector=1 if targets == "tvf" else 0, beta=0.8, grad_scale=0.37)
    g = torch.Generator().manual_seed(200 + 7 * B + factor + nA)
    Bt = B * factor
    z = torch.randn(B, c["ldo"], generator=g) * 1.5
    t_big = torch.randn(Bt, c["n_pred"], generator=g) * 2.0
    if form == "kl_policy":
        old_big, log_std = F.log_softmax(torch.randn(Bt, nA, generator=g) * 1.5, dim=1), None
    else:
        old_big, log_std = torch.randn(Bt, nA, generator=g), torch.randn(nA, generator=g) * 0.5
    w = torch.rand(c["n_pred"], generator=g) + 0.25 if targets == "tvf" else None
    idx = selection(B, factor, g)
    want_dh, want_st = distil_loss_ref(z, t_big[idx], old_big[idx], w, log_std, c, torch.float64)
    zd, idxd = z.cuda(), idx.int().cuda()
    t_d, old_d = t_big.cuda(), old_big.cuda()
    wd = None if w is None else w.cuda()
    lsd = None if log_std is None else log_std.cuda()
    dh, st = run_distil_loss(zd, t_d, old_d, wd, lsd, idxd, c)
    within(dh, want_dh, "dheads")
    used = torch.zeros(c["ldo"], dtype=torch.bool)
    used[:nA] = True
    used[c["pred_col"]:c["pred_col"] + c["n_pred"] * c["stride"]:c["stride"]] = True
    assert not used[c["pred_col"] + (c["n_pred"] - 1) * c["stride"] + 1:].any()
    assert float(dh[:, ~used.cuda()].abs().max()) == 0.0
    for col, name in enumerate(("value loss", "policy loss", "total", "squared error")):
        within(st[:, col], want_st[:, col], name)
    dh2, st2 = run_distil_loss(zd, t_d[idxd.long()].contiguous(), old_d[idxd.long()].contiguous(), wd, lsd, None, c)
    assert torch.equal(dh, dh2) and torch.equal(st, st2)


GAUSS = dict(ldo=9, nA=3, vh=2, eps=0.2, vf_coef=0.5, grad_scale=0.37)


def run_gaussian_loss(z, act, old, adv, ret, log_std, idx, c):
    B = z.shape[0]
    dh = torch.full((B, c["ldo"]), float("nan"), device=DEV)
    rows = torch.full((B, c["nA"]), float("nan"), device=DEV)
    stats = torch.full((B, 8), float("nan"), device=DEV)
    rc = _lib.load().ppo_gaussian_loss_f32(_p(z), B, c["ldo"], c["nA"], c["vh"], _p(act), _p(old), _p(adv), _p(ret),
                                           _p(log_std), c["eps"], c["vf_coef"], c["grad_scale"], _p(dh), _p(rows),
                                           _p(stats), _p(idx), _st())
    _lib.check(rc, "ppo_gaussian_loss_f32")
    torch.cuda.synchronize()
    return dh, rows, stats


@pytest.mark.parametrize("B,factor", SHAPES)
def test_gaussian_loss_index_against_float64(B, factor):
    """ppo_gaussian_loss_f32: 3 actions, 2 value heads, a row of 9 columns.  The 0 / 1 `clipped` decisions (their mean
    over the actions is the statistic) are compared on the rows where every | |rho - 1| - eps | > 1e-5; at most 1 % of
    the rows may be left out, and a float32 evaluation of the reference on the CPU decides those rows as float64 does."""
    c = GAUSS
    nA = c["nA"]
    g = torch.Generator().manual_seed(300 + 7 * B + factor)
    Bt = B * factor
    z = torch.randn(B, c["ldo"], generator=g) * 1.5
    log_std = torch.randn(nA, generator=g) * 0.5
    act_big = torch.randn(Bt, nA, generator=g) * 1.5
    adv_big = torch.randn(Bt, generator=g)
    adv_big[:3] = 0.0
    ret_big = torch.randn(Bt, c["vh"], generator=g)
    idx = selection(B, factor, g)
    # actions as a rollout leaves them: drawn around the means on the scale of sigma (a little wider, for a policy that
    # has moved since), so that the log-densities are O(1) and float32 resolves the ratio to ~1e-7, not to 1e-7 x 200
    act_big[idx] = z[:, :nA] + torch.exp(log_std) * 1.5 * torch.randn(B, nA, generator=g)
    # old log-probabilities near the new ones, so that the ratios spread around 1 on both sides of the clip range
    new_lp = -((act_big[idx] - z[:, :nA]) ** 2) / (2.0 * torch.exp(log_std) ** 2) - log_std - LOG_SQRT_2PI
    old_big = torch.randn(Bt, nA, generator=g)
    old_big[idx] = new_lp + 0.3 * torch.randn(B, nA, generator=g)
    want_dh, want_rows, want_st, rho = gaussian_loss_ref(z, act_big[idx], old_big[idx], adv_big[idx], ret_big[idx],
                                                        log_std, c, torch.float64)
    decided = ((torch.abs(rho - 1.0) - c["eps"]).abs() > 1e-5).all(1)
    left_out = int((~decided).sum())
    assert left_out <= 0.01 * B, f"{left_out} of {B} rows sit on the clip threshold"
    _, _, st32, _ = gaussian_loss_ref(z, act_big[idx], old_big[idx], adv_big[idx], ret_big[idx], log_std, c, torch.float32)
    n_clipped = torch.round(want_st[:, 3] * nA)  # the statistic is k / 3: compare k
    assert torch.equal(torch.round(st32[:, 3].double() * nA)[decided], n_clipped[decided])

    zd, lsd, idxd = z.cuda(), log_std.cuda(), idx.int().cuda()
    act_d, old_d, adv_d, ret_d = act_big.cuda(), old_big.cuda(), adv_big.cuda(), ret_big.cuda()
    dh, rows, st = run_gaussian_loss(zd, act_d, old_d, adv_d, ret_d, lsd, idxd, c)
    within(dh, want_dh, "dheads")
    assert float(dh[:, nA + c["vh"]:].abs().max()) == 0.0  # columns past the used ones: exact zeros (NaN before)
    within(rows, want_rows, "dlog_std_rows")
    for col, name in ((0, "loss_clip"), (2, "value loss"), (4, "old_log_pac - log_pac"), (6, "gain"), (7, "rho")):
        within(st[:, col], want_st[:, col], name)
    assert float(st[:, 1].abs().max()) == 0.0 and float(st[:, 5].abs().max()) == 0.0
    assert float((st[:, 3].double().cpu() * nA - torch.round(st[:, 3].double().cpu() * nA)).abs().max()) <= 1e-6
    assert torch.equal(torch.round(st[:, 3].double().cpu() * nA)[decided], n_clipped[decided])
    L = idxd.long()
    dh2, rows2, st2 = run_gaussian_loss(zd, act_d[L].contiguous(), old_d[L].contiguous(), adv_d[L].contiguous(),
                                        ret_d[L].contiguous(), lsd, None, c)
    assert torch.equal(dh, dh2) and torch.equal(rows, rows2) and torch.equal(st, st2)


# ====================================================================== e. ppo_gather_rows
CANARY = 0xA5


def gather(src, row_bytes, n_src, idx, n_rows, dst):
    rc = _lib.load().ppo_gather_rows(_p(src), row_bytes, n_src, _p(idx), n_rows, _p(dst), _st())
    torch.cuda.synchronize()
    return rc


def gather_case(row_bytes, n_rows, g, dst_offset=0):
    """(source, indices with a repeat, destination of n_rows rows + one canary row starting dst_offset bytes into an
    aligned allocation)."""
    n_src = n_rows + 7
    src = torch.randint(0, 256, (n_src, row_bytes), dtype=torch.uint8, generator=g)
    idx = torch.randint(0, n_src, (n_rows,), generator=g)
    idx = torch.where(idx == torch.arange(n_rows), idx + 1, idx)  # no row reads its own number
    if n_rows > 1:
        idx[-1] = idx[0]  # a repeated index
    assert_moves(idx)
    buf = torch.full((dst_offset + (n_rows + 1) * row_bytes,), CANARY, dtype=torch.uint8, device=DEV)
    dst = buf[dst_offset:].view(n_rows + 1, row_bytes)
    assert buf.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == dst_offset % 16
    return src, idx, dst


@pytest.mark.parametrize("n_rows", [1, 37, 256])
@pytest.mark.parametrize("row_bytes", [16, 1508, 12288, 28224])
def test_gather_rows_equals_cpu_fancy_indexing(row_bytes, n_rows):
    """Rows of 16 bytes (one 16-byte word), 1508 (377 floats: the byte path), 12288, and 28224 (1764 words: not a
    multiple of the 2048 words a workgroup takes per step, so the last step's loads are clamped)."""
    g = torch.Generator().manual_seed(row_bytes + n_rows)
    src, idx, dst = gather_case(row_bytes, n_rows, g)
    src_d, idx_d = src.cuda(), idx.int().cuda()
    assert src_d.data_ptr() % 16 == 0
    assert gather(src_d, row_bytes, src.shape[0], idx_d, n_rows, dst) == 0
    assert torch.equal(dst[:n_rows].cpu(), src[idx])
    assert bool((dst[n_rows] == CANARY).all())  # nothing written past the last row


def test_gather_rows_into_a_destination_off_the_16_byte_grid():
    """A 16-byte-multiple row into a destination that starts 4 bytes into an aligned allocation: the byte path."""
    row_bytes, n_rows = 12288, 37
    g = torch.Generator().manual_seed(4)
    src, idx, dst = gather_case(row_bytes, n_rows, g, dst_offset=4)
    src_d, idx_d = src.cuda(), idx.int().cuda()
    assert dst.data_ptr() % 16 == 4
    assert gather(src_d, row_bytes, src.shape[0], idx_d, n_rows, dst) == 0
    assert torch.equal(dst[:n_rows].cpu(), src[idx])
    assert bool((dst[n_rows] == CANARY).all())


def test_gather_rows_edges():
    """Indices outside [0, n_src_rows) read row 0 (include/ppo_amd.h); no rows: PPO_OK and nothing written; rows of no
    bytes: PPO_E_INVALID."""
    row_bytes, n_src = 1508, 9
    g = torch.Generator().manual_seed(9)
    src = torch.randint(0, 256, (n_src, row_bytes), dtype=torch.uint8, generator=g)
    src_d = src.cuda()
    idx = torch.tensor([-1, n_src, 5, 5, 8, -1, 1], dtype=torch.int32)
    n_rows = idx.numel()
    dst = torch.full((n_rows + 1, row_bytes), CANARY, dtype=torch.uint8, device=DEV)
    assert gather(src_d, row_bytes, n_src, idx.cuda(), n_rows, dst) == 0
    want = src[torch.tensor([0, 0, 5, 5, 8, 0, 1])]
    assert torch.equal(dst[:n_rows].cpu(), want)
    assert bool((dst[n_rows] == CANARY).all())
    dst.fill_(CANARY)
    assert gather(src_d, row_bytes, n_src, idx.cuda(), 0, dst) == 0  # PPO_OK
    assert bool((dst == CANARY).all())
    assert gather(src_d, 0, n_src, idx.cuda(), n_rows, dst) == -1  # PPO_E_INVALID
    assert bool((dst == CANARY).all())
