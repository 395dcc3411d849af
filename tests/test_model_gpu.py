"""GPU: the HIP IMPALA policy/value network and PPO update against the REFERENCE's own outputs
(tests/golden/model_golden.npz, produced by running the reference's TVFModel, Runner.train_policy_minibatch
and Runner.optimizer_step on CPU; see tests/golden/make_model_golden.py).

Tolerances: forward / loss / grads rel 1e-4 of the tensor's max (fp32 conv
reassociation); greedy actions: exact index equality.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import models  # noqa: E402


class _Prefixed:
    """View of an npz with a key prefix (shapes_golden.npz holds two fixtures: c3_*, c4_*)."""

    def __init__(self, z, prefix):
        self.z, self.prefix = z, prefix
        self.files = [k[len(prefix):] for k in z.files if k.startswith(prefix)]

    def __getitem__(self, k):
        return self.z[self.prefix + k]

    def __contains__(self, k):
        return self.prefix + k in self.z.files


def _load(golden_dir, tag):
    if tag == "c2":
        return (_Prefixed(np.load(os.path.join(golden_dir, "model_golden.npz")), ""),
                json.load(open(os.path.join(golden_dir, "model_golden.json"))))
    return (_Prefixed(np.load(os.path.join(golden_dir, "shapes_golden.npz")), tag + "_"),
            json.load(open(os.path.join(golden_dir, "shapes_golden.json")))[tag])


@pytest.fixture(scope="module")
def gold(golden_dir):
    return _load(golden_dir, "c2")


@pytest.fixture(scope="module", params=["c2", "c3", "c4"])
def gold_shapes(request, golden_dir):
    """c2: Pong 4x84x84 / 6 actions; c3: procgen 3x64x64 / 15 actions; c4: Breakout 4x84x84 / 4 actions — each a seeded
    reference TVFModel run on CPU (tests/golden/make_model_golden.py)."""
    return _load(golden_dir, request.param)


def make_net(meta):
    torch.manual_seed(meta["seed"])
    return models.DualHeadNet("impala", tuple(meta["input_dims"]), meta["n_actions"], hidden_units=meta["hidden_units"],
                              head_scale=meta["head_scale"], head_bias=meta["head_bias"], device="cuda")


def rel_err(a, ref):
    a = np.asarray(a, np.float64)
    ref = np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def test_forward_matches_reference(gold_shapes):
    g, meta = gold_shapes
    net = make_net(meta)
    assert net.n_parameters() == sum(int(np.prod(v["shape"])) for v in meta["params"].values())
    x = torch.from_numpy(g["fwd_x"]).cuda()
    out = net.forward(x, policy_temperature=1.0)
    torch.cuda.synchronize()
    for k in ("raw_policy", "log_policy", "value", "advantage"):
        assert rel_err(out[k].cpu().numpy(), g[f"fwd_{k}"]) < 1e-4, k
    # greedy: actions index-exact, blended log-policy close (rl/models.py:475-485)
    out0 = net.forward(x, policy_temperature=0.0)
    assert np.array_equal(out0["argmax_policy"].cpu().numpy(), g["fwd_greedy_argmax_policy"])
    assert np.array_equal(out0["argmax_policy"].argmax(1).cpu().numpy(), g["fwd_greedy_actions"])
    assert rel_err(out0["log_policy"].cpu().numpy(), g["fwd_greedy_log_policy"]) < 1e-4
    assert g["fwd_logit_margin"].min() > 1e-5  # fixture has no near-tie that reassociation could flip


@pytest.mark.parametrize("tag", ["c2", "c3", "c4"])
def test_greedy_actions_index_exact_on_256_observations(tag, golden_dir):
    """The north star's gate "greedy actions bit-exact on fixed seeds", on 256 observations per network shape and with
    two policy heads (tests/golden/make_greedy_golden.py): the freshly initialised one, and a stored wide head whose
    logits are centred over the batch so that every action is some observation's greedy choice.  Index-exact on every
    row whose reference top-1 / top-2 margin exceeds 1e-5; the rows at or below it are counted and must be few."""
    import hashlib
    z = np.load(os.path.join(golden_dir, "greedy_golden.npz"))
    jm = json.load(open(os.path.join(golden_dir, "greedy_golden.json")))
    _g, meta = _load(golden_dir, tag)
    dims = tuple(jm["shapes"][tag][0])
    x = np.random.default_rng(jm["obs_seed"][tag]).integers(0, 256, size=(jm["batch"], *dims), dtype=np.uint8)
    assert hashlib.sha256(x.tobytes()).hexdigest() == jm["obs_sha256"][tag], "this NumPy draws different observations"
    net = make_net(meta)
    xd = torch.from_numpy(x).cuda()
    checked = 0
    for prefix in ("", "wide_"):
        if prefix:
            net.params["policy_head.weight"].copy_(torch.from_numpy(z[f"{tag}_wide_head_weight"]).cuda())
            net.params["policy_head.bias"].copy_(torch.from_numpy(z[f"{tag}_wide_head_bias"]).cuda())
        out0 = net.forward(xd, policy_temperature=0.0)
        out1 = net.forward(xd, policy_temperature=1.0)
        torch.cuda.synchronize()
        want, margin = z[f"{tag}_{prefix}greedy_actions"], z[f"{tag}_{prefix}logit_margin"]
        assert rel_err(out1["raw_policy"].cpu().numpy(), z[f"{tag}_{prefix}raw_policy"]) < 1e-4
        got = out0["argmax_policy"].argmax(1).cpu().numpy()
        assert np.array_equal(got, out1["raw_policy"].argmax(1).cpu().numpy())
        decided = margin > 1e-5
        assert int((~decided).sum()) <= 2, f"{int((~decided).sum())} fixture rows are near-ties"
        bad = np.flatnonzero(decided & (got != want))
        assert bad.size == 0, (prefix, bad.tolist(), margin[bad].tolist())
        checked += int(decided.sum())
        if prefix:
            assert len(np.unique(want)) == meta["n_actions"], "the wide head must exercise every action"
    assert checked >= 2 * jm["batch"] - 4


def test_forward_is_batch_size_independent(gold):
    g, meta = gold
    net = make_net(meta)
    x = torch.from_numpy(g["fwd_x"]).cuda()
    full = net.forward(x)["raw_policy"].clone()
    for b in (1, 3):
        part = net.forward(x[:b].contiguous())["raw_policy"]
        assert torch.equal(part, full[:b])


def test_ppo_update_matches_reference_runner(gold):
    g, meta = gold
    net = make_net(meta)
    stride = meta["dense_row_stride"]

    def sub(name, t):
        a = t.detach().cpu().numpy()
        return a[::stride] if name == "encoder.dense.weight" else a

    norm = torch.zeros(1, device="cuda")
    for step in range(4):
        d = {k: g[f"mb{step}_{k}"] for k in ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns")}
        stats = net.ppo_minibatch(
            torch.from_numpy(d["prev_state"]).cuda(), torch.from_numpy(d["actions"].astype(np.int32)).cuda(),
            torch.from_numpy(d["log_pac"]).cuda(), torch.from_numpy(d["log_policy"]).cuda(),
            torch.from_numpy(d["advantages"]).cuda(), torch.from_numpy(d["returns"]).cuda(),
            eps_clip=meta["ppo_epsilon"], ent_coef=meta["entropy_bonus"], vf_coef=meta["ppo_vf_coef"], loss_scale=1.0)
        s = stats.cpu().numpy().astype(np.float64)
        loss, kl_approx, kl_true, clip_frac = g[f"mb{step}_result"]
        assert abs(-s[:, 6].mean() - loss) < 1e-4 * max(1.0, abs(loss)), step        # loss = mean(-gain)
        assert abs(s[:, 4].mean() - kl_approx) < 1e-5 + 1e-4 * abs(kl_approx), step
        assert abs(s[:, 5].mean() - kl_true) < 1e-5 + 1e-4 * abs(kl_true), step
        assert abs(s[:, 3].mean() - clip_frac) < 1e-9, step
        if step == 0:
            for name in meta["param_names"]:
                key = "grad0_" + name
                if meta["params"][name].get("grad_none"):
                    # advantage head / log_std never enter the loss: the reference leaves grad=None
                    assert float(net.grads[name].abs().max()) == 0.0, name
                    continue
                ref = g[key]
                got = sub(name, net.grads[name])
                assert got.shape == ref.shape, name
                # Unaligned, the bar is set by the network's kinks, not by arithmetic: a pre-activation within
                # ~1e-7 of zero gets the opposite ReLU mask in the two forward passes and moves every upstream
                # gradient by ~1e-3 of its max.  test_gradients_match_reference_with_kinks_aligned counts those
                # elements and holds the gradients to 1e-5 / 1e-4 once they are aligned; this line only guards
                # the un-patched path against gross errors.
                assert rel_err(got, ref) < 5e-3, (name, rel_err(got, ref))
        net.adam_step(lr=meta["lr"], beta1=meta["betas"][0], beta2=meta["betas"][1], eps=meta["adam_epsilon"],
                      max_grad_norm=meta["max_grad_norm"], grad_norm_out=norm)
        assert abs(norm.item() - float(g[f"mb{step}_grad_norm"])) < 2e-4 * float(g[f"mb{step}_grad_norm"]), step
        if step in (0, 3):
            for name in meta["param_names"]:
                ref = g[f"param_after{step + 1}_" + name]
                got = sub(name, net.params[name])
                # Adam's first steps move each weight by ~lr * g/(|g| + eps) regardless of gradient scale, so
                # compare the update, not the weight.  Where |g| ~ eps the kink noise above (dg ~ 1e-3 of
                # the tensor's max) is amplified to a fraction of lr; everywhere else the updates agree
                # to a few percent of lr.  (ppo_adam_step_f32 itself is held to 2e-6 against
                # torch.optim.Adam in test_nn_ops_gpu.py.)
                d = np.abs(got - ref)
                assert np.median(d) < 0.02 * meta["lr"] * (step + 1), (name, step, np.median(d))


def _kink_tensors(acts, n_stacks=3, n_block=2):
    """fixture key -> the HIP path's saved pre-activation whose sign decides that ReLU."""
    m = {"relu_encoder.dense": acts["flat"], "relu_heads": acts["h"]}
    for si in range(n_stacks):
        for bi in range(n_block):
            m[f"relu_encoder.stacks.{si}.blocks.{bi}.conv0"] = acts[f"q{si}_{bi}_in"]
            m[f"relu_encoder.stacks.{si}.blocks.{bi}.conv1"] = acts[f"a{si}_{bi}"]
    return m


def test_gradients_match_reference_with_kinks_aligned(gold_shapes):
    """The reference's fp32 gradients (Runner.train_policy_minibatch, rl/rollout.py:1610-1771) against the HIP
    backward.  ReLU / max-pool decisions are discontinuities: an element whose pre-activation is ~1e-7 from zero may
    fall on the other side in two fp32 implementations and then shifts every upstream gradient by ~1e-3.  The fixture
    holds the reference's own decision for every ReLU input and max-pool window (G5k), so this test
      1. COUNTS the elements on which the HIP forward decides differently and checks each is a genuine near-tie
         (|pre-activation| < 1e-5 of the tensor's max; pool: the two taps' values within 1e-5),
      2. writes the reference's decision into the saved activations at exactly those elements (sign-carrying 1e-30,
         the tap index) — the backward kernels read their gates from these tensors — and
      3. holds every gradient to the arithmetic bar: 1e-5 of the tensor's max for heads and dense layer, 1e-4 for
         the convolutions."""
    g, meta = gold_shapes
    net = make_net(meta)
    stride = meta["dense_row_stride"]
    x = torch.from_numpy(g["mb0_prev_state"]).cuda()
    acts, o, B, dheads = net._train_forward(x)
    stats = net._buf("loss_stats", (B, 8))
    t = {k: torch.from_numpy(g[f"mb0_{k}"]).cuda() for k in ("log_pac", "log_policy", "advantages", "returns")}
    actions = torch.from_numpy(g["mb0_actions"].astype(np.int32)).cuda()
    net._call("ppo_ppo_loss_f32", o.data_ptr(), B, net.nh, net.n_actions, net.vh, actions.data_ptr(),
              t["log_pac"].data_ptr(), t["log_policy"].data_ptr(), t["advantages"].data_ptr(), t["returns"].data_ptr(),
              float(meta["ppo_epsilon"]), float(meta["entropy_bonus"]), float(meta["ppo_vf_coef"]), 1.0 / B,
              dheads.data_ptr(), stats.data_ptr(), None)
    flips, total = {}, 0
    for key, pre in _kink_tensors(acts).items():
        ref = torch.from_numpy(np.unpackbits(g["kink0_" + key])[:pre.numel()].astype(bool)).cuda().view(pre.shape)
        diff = (pre > 0) != ref
        n = int(diff.sum())
        total += pre.numel()
        if n:
            flips[key] = n
            assert float(pre[diff].abs().max()) < 1e-5 * float(pre.abs().max()), key  # genuine near-ties only
            pre[diff] = torch.where(ref[diff], 1e-30, -1e-30).to(pre.dtype)
    for si in range(3):
        idx = acts[f"idx{si}"]
        ref = torch.from_numpy(g[f"kink0_pool_{si}"]).cuda()
        diff = idx != ref
        n = int(diff.sum())
        total += idx.numel()
        if n:
            flips[f"pool_{si}"] = n
            idx[diff] = ref[diff]
    n_flips = sum(flips.values())
    print(f"kink decisions differing from the reference: {n_flips} of {total}: {flips}")
    assert n_flips <= 16, flips
    net.backward(acts, dheads)
    torch.cuda.synchronize()
    worst = {}
    for name in meta["param_names"]:
        if meta["params"][name].get("grad_none"):
            assert float(net.grads[name].abs().max()) == 0.0, name
            continue
        got = net.grads[name].detach().cpu().numpy()
        got = got[::stride] if name == "encoder.dense.weight" else got
        e = rel_err(got, g["grad0_" + name])
        worst[name] = e
        bar = 1e-4 if name.startswith("encoder.stacks.") else 1e-5
        assert e < bar, (name, e, flips)
    print("worst gradient rel err vs the reference:", max(worst.values()), max(worst, key=worst.get))


def test_ppo_step_matches_reference_at_config_shapes(gold_shapes):
    """One Runner.train_policy_minibatch + optimizer_step of the reference at each config's network shape: loss
    statistics, gradient norm and the parameter update."""
    g, meta = gold_shapes
    net = make_net(meta)
    stride = meta["dense_row_stride"]
    d = {k: g[f"mb0_{k}"] for k in ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns")}
    stats = net.ppo_minibatch(
        torch.from_numpy(d["prev_state"]).cuda(), torch.from_numpy(d["actions"].astype(np.int32)).cuda(),
        torch.from_numpy(d["log_pac"]).cuda(), torch.from_numpy(d["log_policy"]).cuda(),
        torch.from_numpy(d["advantages"]).cuda(), torch.from_numpy(d["returns"]).cuda(),
        eps_clip=meta["ppo_epsilon"], ent_coef=meta["entropy_bonus"], vf_coef=meta["ppo_vf_coef"], loss_scale=1.0)
    s = stats.cpu().numpy().astype(np.float64)
    loss, kl_approx, kl_true, clip_frac = g["mb0_result"]
    assert abs(-s[:, 6].mean() - loss) < 1e-4 * max(1.0, abs(loss))
    assert abs(s[:, 4].mean() - kl_approx) < 1e-5 + 1e-4 * abs(kl_approx)
    assert abs(s[:, 5].mean() - kl_true) < 1e-5 + 1e-4 * abs(kl_true)
    assert abs(s[:, 3].mean() - clip_frac) < 1e-9
    norm = torch.zeros(1, device="cuda")
    net.adam_step(lr=meta["lr"], beta1=meta["betas"][0], beta2=meta["betas"][1], eps=meta["adam_epsilon"],
                  max_grad_norm=meta["max_grad_norm"], grad_norm_out=norm)
    assert abs(norm.item() - float(g["mb0_grad_norm"])) < 2e-4 * float(g["mb0_grad_norm"])
    for name in meta["param_names"]:
        got = net.params[name].detach().cpu().numpy()
        got = got[::stride] if name == "encoder.dense.weight" else got
        assert np.median(np.abs(got - g["param_after1_" + name])) < 0.02 * meta["lr"], name


def test_backward_is_exact_given_shared_kinks(gold):
    """Full backward vs float64 autograd of the same function with the ReLU masks and max-pool
    selections fixed to the HIP forward's own (oracle/model_torch.forward_shared_kinks): isolates
    kernel arithmetic from kink flips.  Bar: 1e-5 of each gradient's max."""
    from oracle import model_torch as R
    g, meta = gold
    net = make_net(meta)
    x = torch.from_numpy(g["mb1_prev_state"]).cuda()
    B = x.shape[0]
    actions = torch.from_numpy(g["mb1_actions"]).cuda()
    old_log_pac = torch.from_numpy(g["mb1_log_pac"]).cuda()
    adv = torch.from_numpy(g["mb1_advantages"]).cuda()
    ret = torch.from_numpy(g["mb1_returns"]).cuda()
    net.ppo_minibatch(x, actions.int(), old_log_pac, torch.from_numpy(g["mb1_log_policy"]).cuda(), adv, ret,
                      eps_clip=0.2, ent_coef=0.01, vf_coef=0.5, loss_scale=1.0)
    acts = net.encode(x, train=True)  # same buffers, same values: the saved kinks
    sd = {k: v.detach().double().requires_grad_(True) for k, v in net.params.items()}
    out = R.forward_shared_kinks(sd, x.double() / 255.0, acts)
    loss = R.ppo_loss(out, actions, old_log_pac.double(), adv.double(), ret.double())
    loss.backward()
    worst = 0.0
    for name, p in sd.items():
        if p.grad is None:
            assert float(net.grads[name].abs().max()) == 0.0
            continue
        e = rel_err(net.grads[name].cpu().numpy(), p.grad.cpu().numpy())
        worst = max(worst, e)
        assert e < 1e-5, (name, e)
    print("worst gradient rel err vs float64:", worst)


def test_state_dict_round_trip(gold):
    _, meta = gold
    a = make_net(meta)
    torch.manual_seed(123)
    b = models.DualHeadNet("impala", tuple(meta["input_dims"]), meta["n_actions"], hidden_units=meta["hidden_units"],
                           head_scale=meta["head_scale"], head_bias=meta["head_bias"], device="cuda")
    assert not torch.equal(a.flat, b.flat)
    b.load_state_dict({k: v.cpu() for k, v in a.state_dict().items()})
    assert torch.equal(a.flat, b.flat)
    assert list(a.state_dict())[0] == "log_std"
    with pytest.raises(KeyError):
        b.load_state_dict({"nope": torch.zeros(1)})


@pytest.mark.parametrize("dims,nA", [((4, 84, 84), 6), ((3, 64, 64), 15)])
def test_fused_stack_tail_is_bit_identical_to_four_convolutions(monkeypatch, dims, nA):
    """csrc/stack_fused.hip: the two residual blocks of the 11x11 stack in one launch (image resident in LDS) give
    the same bits as the four convolution launches — inference rows, the saved maps of a training forward, and every
    gradient of a PPO minibatch — at ragged batch sizes too."""
    from ppo_amd import models
    torch.manual_seed(3)
    monkeypatch.setattr(models, "FUSE_STACK_TAIL", 1)
    monkeypatch.setattr(models, "FUSE_STACK_FULL", 1)
    monkeypatch.setattr(models, "FUSE_STACK_FULL_BWD", 1)
    monkeypatch.setattr(models, "FUSE_STACK_CHAIN", 1)
    monkeypatch.setattr(models, "FUSE_STACK_TAIL_BWD", 7)  # every backward instance, whatever the default mask
    monkeypatch.setattr(models, "FUSE_STACK16_MIN_BATCH", 1)  # ... and the 16-channel form at every batch size
    a = models.DualHeadNet("impala", dims, nA, hidden_units=256, head_scale=0.1, head_bias=True, device="cuda")
    assert a.lib.ppo_impala_stack_tail_supported(32, 11, 11) == 1 and a.lib.ppo_impala_stack_tail_supported(32, 21, 21) == 1
    assert a.lib.ppo_impala_stack_tail_supported(16, 42, 42) == 1 and a.lib.ppo_impala_stack_tail_supported(32, 8, 8) == 1
    assert a.lib.ppo_impala_stack_tail_supported(16, 21, 21) == 0
    assert a.lib.ppo_impala_stack_full_supported(32, 16, 16) == 1 and a.lib.ppo_impala_stack_full_supported(32, 11, 11) == 0
    b = models.DualHeadNet("impala", dims, nA, hidden_units=256, head_scale=0.1, head_bias=True, device="cuda")
    b.load_state_dict(a.state_dict())
    g = torch.Generator(device="cuda").manual_seed(5)
    for B in ((1, 37, 256, 300) if dims[1] == 84 else (5, 256)):
        x = torch.randint(0, 256, (B, *dims), dtype=torch.uint8, device="cuda", generator=g)
        for _ in range(2):  # the second pass replays the recorded launch plan
            monkeypatch.setattr(models, "FUSE_STACK_TAIL", 1)
            ha = a.forward(x)["_heads"].clone()
            assert {0, 1, ("full", 2)} <= set(a._tail_ptrs), "the fused paths did not engage (blocks of stacks 0 and 1, whole stack 2)"
            monkeypatch.setattr(models, "FUSE_STACK_TAIL", 0)
            hb = b.forward(x)["_heads"].clone()
            assert not b._tail_ptrs
            assert torch.equal(ha, hb), B
        actions = torch.randint(0, nA, (B,), dtype=torch.int32, device="cuda", generator=g)
        logp = torch.log_softmax(torch.randn(B, nA, device="cuda", generator=g), dim=1)
        pac = logp.gather(1, actions.long()[:, None])[:, 0].contiguous()
        adv, ret = torch.randn(B, device="cuda", generator=g), torch.randn(B, 1, device="cuda", generator=g)
        monkeypatch.setattr(models, "FUSE_STACK_TAIL", 1)
        monkeypatch.setattr(models, "WGRAD_POOLED_DY", 1)     # first stack's pool backward inside its weight-gradient kernel
        monkeypatch.setattr(models, "WGRAD_BATCH_LAUNCH", 1)  # one weight-gradient launch per stack's blocks ...
        acts_a = a.encode(x, train=True)
        saved = {k: acts_a[k].clone() for k in ("q0_0_in", "a0_0", "q0_1_in", "a0_1", "in1", "q1_0_in", "a1_0", "q1_1_in", "a1_1", "in2", "idx2",
                                                "q2_0_in", "a2_0", "q2_1_in", "a2_1", "flat")}
        a.ppo_minibatch(x, actions, pac, logp, adv, ret)
        monkeypatch.setattr(models, "FUSE_STACK_TAIL", 0)
        monkeypatch.setattr(models, "WGRAD_POOLED_DY", 0)
        monkeypatch.setattr(models, "WGRAD_BATCH_LAUNCH", 0)  # ... against one per convolution
        acts_b = b.encode(x, train=True)
        for k, v in saved.items():
            assert torch.equal(v, acts_b[k]), (B, k)
        b.ppo_minibatch(x, actions, pac, logp, adv, ret)
        torch.cuda.synchronize()
        # Bit-identical everywhere except the block convolutions' weight / bias gradients: a batched launch gives each
        # problem a quarter of the workgroups (one wave of workgroups for the whole batch), so its slabs partition the
        # (image, band) items differently from a per-convolution launch — the same products in another summation
        # order.  Both orders are fixed (deterministic); they agree to float32 round-off.
        assert float(a.grad.abs().sum()) > 0, B
        for name in a.grads:
            ga, gb = a.grads[name], b.grads[name]
            if ".blocks." in name or name.startswith("encoder.stacks.2.firstconv"):
                # (the last stack's first convolution rides in the 21x21 blocks' launch as its fifth problem: WGRAD_RIDE)
                assert float((ga - gb).abs().max()) <= 2e-6 * max(float(gb.abs().max()), 1e-30), (B, name)
            else:
                assert torch.equal(ga, gb), (B, name)
        a.ppo_minibatch(x, actions, pac, logp, adv, ret)
        again = a.grad.clone()
        a.ppo_minibatch(x, actions, pac, logp, adv, ret)
        torch.cuda.synchronize()
        assert torch.equal(a.grad, again), "the batched weight-gradient launch is not deterministic"
        assert {("bwd", 0), ("bwd", 1), ("full_bwd", 2)} <= set(a._tail_ptrs), "the fused backward did not engage"


def test_optimiser_step_keeps_the_packed_convolution_weights_fresh(gold, monkeypatch):
    """ppo_adam_step_scatter_f32 writes every updated convolution weight into the kernels' pre-packed MFMA operand
    layouts as well (forward, and flipped / transposed for backward-data), so no re-pack launch runs per step: after a
    few steps the packed buffer must be, bit for bit, what ppo_conv3x3_pack_weights_f32 makes of the parameters."""
    g, meta = gold
    monkeypatch.setattr(models, "ADAM_SCATTER", 1)  # opt-in path (default off: measured slower than the re-pack launch)
    net = make_net(meta)
    assert net._scatter_table() is not None
    table, n_conv = net._scatter_table()
    t = table.cpu().numpy()
    n_weights = sum(int(np.prod(v["shape"])) for k, v in meta["params"].items() if k.startswith("encoder.stacks") and k.endswith("weight"))
    assert int((t[:, 0] >= 0).sum()) == n_weights and int((t[:, 1] >= 0).sum()) == n_weights - 16 * 4 * 9  # no transposed first conv
    x = torch.from_numpy(g["mb0_prev_state"]).cuda()
    B = x.shape[0]
    for _ in range(3):
        out = net.forward(x)
        net.ppo_minibatch(x, torch.zeros(B, dtype=torch.int32, device="cuda"), out["log_policy"][:, 0].contiguous(),
                          out["log_policy"].clone(), torch.ones(B, device="cuda"), torch.zeros(B, 1, device="cuda"))
        net.adam_step()
    torch.cuda.synchronize()
    assert not net._packed_dirty
    kept = net._packed.clone()
    net._packed.zero_()
    net.mark_weights_changed()
    net._refresh_packed()
    torch.cuda.synchronize()
    assert torch.equal(kept, net._packed)


@pytest.mark.parametrize("B", [128, 100, 8, 1])
def test_two_workgroups_per_image_chain_launch_is_bit_identical(gold, monkeypatch, B):
    """Inference batches of a rollout group (<= 128 images) run the chained 21x21 -> 11x11 launch with every image on
    TWO workgroups that split the output channels and exchange halves per layer (stack_chain_split_kernel).  Same K
    order and epilogue arithmetic per output element, so the heads must be bit-identical to the one-workgroup-per-image
    launch - over repeated launches (the kernel advances its own launch counter), for batches that do not fill the
    pairing groups of 8, and with no partner ever missing.  (The net's own first-use check of the split form - it keeps
    the one-workgroup launch if the bits differ - must have passed.)"""
    g, meta = gold
    rng = np.random.default_rng(B)
    x = torch.from_numpy(rng.integers(0, 256, size=(B, *meta["input_dims"]), dtype=np.uint8)).cuda()
    x2 = torch.from_numpy(rng.integers(0, 256, size=(B, *meta["input_dims"]), dtype=np.uint8)).cuda()
    outs = {}
    for split in (0, 1):
        monkeypatch.setattr(models, "CHAIN_SPLIT", split)
        net = make_net(meta)
        calls = []
        orig = net._call
        net._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
        res = []
        for inp in (x, x2, x):
            # chain_split: the Runner's pipelined rollout passes this; other forwards keep one workgroup per image
            o = net.heads(net.encode(inp, False, chain_split=True), "i")  # the whole head row: raw_policy, value and the rest
            res.append((o[:, :net.n_actions].clone(), o[:, net.n_actions:].clone()))
        torch.cuda.synchronize()
        assert ("ppo_impala_stack_chain_split_forward_f32" in calls) == bool(split)
        assert not net.chain_split_error()
        # the first split launch checks itself against the one-workgroup form and would fall back on a mismatch:
        # on this hardware it must not have
        assert net._chain_split_usable is (True if split else None)
        outs[split] = res
    for (p0, v0), (p1, v1) in zip(outs[0], outs[1]):
        assert torch.equal(p0, p1) and torch.equal(v0, v1)
    assert torch.equal(outs[1][0][0], outs[1][2][0]) and not torch.equal(outs[1][0][0], outs[1][1][0])


def test_first_layer_kernel_choice_does_not_change_a_bit_of_the_network(gold):
    """ppo_conv1_pool_form: the uint8 first layer through the LDS kernel (1) or pooled out of the MFMA accumulators (0,
    csrc/conv1_pool.hip) - inference forward, training forward + PPO minibatch gradients (the kernel's argmax feeds the
    first layer's weight gradient) and the parameters after an Adam step must agree bit for bit: it is a speed switch."""
    from ppo_amd import _lib
    g, meta = gold
    lib = _lib.load()
    d = {k: g[f"mb0_{k}"] for k in ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns")}
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(0, 256, size=(128, *meta["input_dims"]), dtype=np.uint8)).cuda()
    before = lib.ppo_conv1_pool_form(-1)
    res = {}
    try:
        for form in (1, 0):
            lib.ppo_conv1_pool_form(form)
            net = make_net(meta)
            o = net.forward(x)
            stats = net.ppo_minibatch(
                torch.from_numpy(d["prev_state"]).cuda(), torch.from_numpy(d["actions"].astype(np.int32)).cuda(),
                torch.from_numpy(d["log_pac"]).cuda(), torch.from_numpy(d["log_policy"]).cuda(),
                torch.from_numpy(d["advantages"]).cuda(), torch.from_numpy(d["returns"]).cuda(),
                eps_clip=meta["ppo_epsilon"], ent_coef=meta["entropy_bonus"], vf_coef=meta["ppo_vf_coef"], loss_scale=1.0)
            grad = net.grad.clone()
            net.adam_step()
            torch.cuda.synchronize()
            res[form] = (o["raw_policy"].clone(), o["value"].clone(), stats.clone(), grad, net.flat.clone())
    finally:
        lib.ppo_conv1_pool_form(before)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert float(res[0][3].abs().max()) > 0
