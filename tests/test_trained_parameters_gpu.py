"""GPU: every network path with parameters as training leaves them - every bias and log_std non-zero.

The initialisers of ppo_amd/models.py zero every bias and log_std, and every other network-level test builds its net from
them (or from fixtures drawn by them), so a bias read at the wrong channel offset, from the wrong layer, twice or not at
all inside a fused launch - or two same-shaped bias pointers exchanged in a pointer table - passes those tests.  Here each
net gets oracle/trained_params.perturbed_state_dict (biases N(0, 0.1), log_std N(0, 0.3)) through its public
load_state_dict and is held to the bars the project already holds the same quantities to with zero biases:

  a. IMPALA inference, every launch form: bit-identical head rows across forms, the four-convolution form within 1e-4 of
     float64 (oracle/model_torch.forward); each form's own entry point must have run (recorded through net._call).
  b. IMPALA training forward + backward (defaults / everything fused / nothing fused): saved maps bit-identical, every
     gradient within 1e-5 of its largest entry of float64 autograd with the kinks shared (forward_shared_kinks).
  c. Nature: head rows 1e-4, gradients at the bars of tests/test_nature_gpu.py against float64 autograd.
  d. MLP, fused and op-by-op: every head 1e-4 of float64 at batches 1, 7, 130; each training phase fused against
     op-by-op at 2e-5, the discrete PPO phase against float64 at 2e-5; log_std's gradient follows log_std.
  e. --precision=medium: head rows within 1e-4 of float64 and not the exact path's bits.
  f. TVFModel.adjust_value_scale against rl/models.py:630-651.

tests/test_bias_sensitivity_cpu.py shows in float64 that every single-tensor bias fault moves the head row by more than
100 of the 1e-4 bars, so none of them can hide under the tolerance here.

Every comparison against float64 prints a TRAINED_ERR line (case, quantity, measured error, bar).  Worst values measured
on an MI355X (profiles/trained_parameters_accuracy.md):
    a. IMPALA inference head row          5.8e-7   bar 1e-4
    b. IMPALA training gradients          7.7e-7   bar 1e-5
    c. Nature head row                    1.8e-7   bar 1e-4
       Nature gradients, convolutions     5.1e-7   bar 1e-4
       Nature gradients, linear + heads   2.9e-7   bar 1e-5
    d. MLP heads                          5.0e-7   bar 1e-4
       MLP discrete PPO gradients         1.3e-6   bar 2e-5
    e. --precision=medium head row        7.8e-6   bar 1e-4
    f. adjust_value_scale, outputs        4.1e-7   bar 1e-6
No defect was found: every bar holds with two decades to spare.  No case needed another seed for a ReLU near-tie (the
Nature cases re-decide their ReLUs in float64; the smallest pre-activation, relative to its layer's largest, is printed
with them: 5.0e-6 at 84x84, 1.3e-5 at 36x36 - far above float32 round-off of the sums that make it).

That these tests can fail was checked once with a scratch build whose bias_r in csrc/stack_fused.hip is forced to zero,
loaded through PPO_AMD_LIB: all four inference cases (fused forms 0.026 - 0.051 away from the four convolutions, where
they must be bit-identical), the "defaults" and "all-fused" training cases of both geometries (first gradient
6.1e-3 / 2.5e-2 against the 1e-5 bar), both plan-agreement cases (saved map a1_0) and the medium-precision case (its
exact-path row 0.26 against 1e-4) turn red."""
import contextlib
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import model_torch as R  # noqa: E402
from oracle import trained_params as T  # noqa: E402
from ppo_amd import _lib, models  # noqa: E402

SEED = 21  # of the perturbation (the seed tests/test_bias_sensitivity_cpu.py checks)
GEOMETRIES = {"84x84": ((4, 84, 84), 6), "64x64": ((3, 64, 64), 15)}


@contextlib.contextmanager
def switches(**values):
    """The launch-path switches of ppo_amd.models (module globals, read when a net is built or runs) set for a block."""
    before = {k: getattr(models, k) for k in values}
    try:
        for k, v in values.items():
            setattr(models, k, v)
        yield
    finally:
        for k, v in before.items():
            setattr(models, k, v)


def record_calls(net):
    """[(entry point, args)] of everything the net launches through _call from now on."""
    calls, orig = [], net._call

    def call(fn, *a):
        calls.append((fn, a))
        return orig(fn, *a)

    net._call = call
    return calls


def names_of(calls):
    return [fn for fn, _a in calls]


def rel_err(a, ref):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else a
    ref = ref.detach().cpu().numpy() if hasattr(ref, "detach") else ref
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a.reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-30))


def report(case, quantity, err, bar):
    print(f"TRAINED_ERR {case} {quantity} err={err:.3e} bar={bar:.0e}")
    return err


# ---------------------------------------------------------------------------------------------- IMPALA
def impala_net(geom, precision="high"):
    dims, nA = GEOMETRIES[geom]
    torch.manual_seed(11)
    return models.DualHeadNet("impala", dims, nA, hidden_units=256, head_scale=0.1, head_bias=True, device="cuda",
                              precision=precision)


@functools.lru_cache(maxsize=None)
def impala_parameters(geom):
    """The perturbed parameters every IMPALA net of this file loads (CPU tensors)."""
    with switches(PACKED_WEIGHTS=0):  # (only its state_dict is wanted)
        sd = T.perturbed_state_dict(impala_net(geom).state_dict(), SEED)
    for name in T.bias_names(sd):
        assert bool((sd[name] != 0).all()), name
    return sd


@functools.lru_cache(maxsize=None)
def impala_inputs(geom, B):
    dims, _nA = GEOMETRIES[geom]
    return torch.from_numpy(np.random.default_rng(100 + B).integers(0, 256, size=(B, *dims), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def impala_float64_row(geom, B):
    with torch.no_grad():
        return T.head_row(R.forward(T.as_double(impala_parameters(geom)), impala_inputs(geom, B).double() / 255.0))


def tail_channels(calls):
    """Channel counts of the fused residual-block launches (..., B, channels, h, w)."""
    return [a[-3] for fn, a in calls if fn == "ppo_impala_stack_tail_forward_f32"]


FUSED = ("ppo_impala_stack_", "ppo_conv3x3_block_forward")


def ran(name):
    return lambda c, geom: name in names_of(c)


def _four_convolutions(c, geom):
    n = names_of(c)
    return n.count("ppo_conv3x3_forward_packed_f32") == 12 and not any(f.startswith(FUSED) for f in n)


def _chain_split(c, geom):
    # the two-workgroup form exists for the 32-channel 21x21 -> 11x11 chain only (the 84x84 net); the 64x64 net
    # keeps the one-workgroup chain with chain_split=True
    want = "ppo_impala_stack_chain_split_forward_f32" if geom == "84x84" else "ppo_impala_stack_chain_forward_f32"
    return want in names_of(c)


def _one_workgroup_chain(c, geom):
    n = names_of(c)
    return "ppo_impala_stack_chain_forward_f32" in n and "ppo_impala_stack_chain_split_forward_f32" not in n


def _whole_stack(c, geom):
    n = names_of(c)
    return "ppo_impala_stack_full_forward_f32" in n and tail_channels(c) == [32] and not any("chain" in f for f in n)


def _tails(c, geom):
    n = names_of(c)
    return tail_channels(c) == [32, 32] and not any("chain" in f or "stack_full" in f for f in n)


def _blocks(c, geom):
    n = names_of(c)
    return n.count("ppo_conv3x3_block_forward_packed_f32") >= 2 and not any(f.startswith("ppo_impala_stack_") for f in n)


def _defaults(c, geom):
    n = names_of(c)  # (at these batches the 16-channel stack runs one launch per residual block)
    return "ppo_impala_stack_chain_forward_f32" in n and n.count("ppo_conv3x3_block_forward_packed_f32") == 2


def _stack16(c, geom):
    return 16 in tail_channels(c) and "ppo_conv3x3_block_forward_packed_f32" not in names_of(c)


def _no_block_launch(c, geom):
    n = names_of(c)
    return "ppo_impala_stack_chain_forward_f32" in n and n.count("ppo_conv3x3_forward_packed_f32") == 4 \
        and "ppo_conv3x3_block_forward_packed_f32" not in n and 16 not in tail_channels(c)


def _unpacked(c, geom):
    n = names_of(c)
    return n.count("ppo_conv3x3_forward_f32") == 12 and n.count("ppo_conv3x3_pool_forward_f32") == 3 \
        and not any("packed" in f or f.startswith(FUSED) for f in n)


def _separate_pool(c, geom):
    n = names_of(c)
    return n.count("ppo_maxpool3x3s2_forward_f32") == 2 and not any("conv3x3_pool_forward" in f for f in n)


# name -> (module switches, encode's chain_split, first-layer form or None, "the kernel this plan is about ran")
INFERENCE_PLANS = {
    "four-convolutions": (dict(FUSE_STACK_TAIL=0, FUSE_BLOCK=0), False, None, _four_convolutions),
    "defaults": ({}, False, None, _defaults),
    "chain-split": ({}, True, None, _chain_split),
    "CHAIN_SPLIT=0": (dict(CHAIN_SPLIT=0), True, None, _one_workgroup_chain),
    "FUSE_STACK_CHAIN=0": (dict(FUSE_STACK_CHAIN=0), False, None, _whole_stack),
    "FUSE_STACK_FULL=0": (dict(FUSE_STACK_FULL=0), False, None, _tails),
    "FUSE_STACK_TAIL=0": (dict(FUSE_STACK_TAIL=0), False, None, _blocks),
    # the 16-channel row-shifted form at a small batch, against the block launches (defaults) and the four convolutions
    "FUSE_STACK16_MIN_BATCH=1": (dict(FUSE_STACK16_MIN_BATCH=1), False, None, _stack16),
    "FUSE_BLOCK=0": (dict(FUSE_BLOCK=0), False, None, _no_block_launch),
    "PACKED_WEIGHTS=0": (dict(PACKED_WEIGHTS=0), False, None, _unpacked),
    "FUSE_POOL_STACKS=0": (dict(FUSE_POOL_STACKS=0), False, None, _separate_pool),  # (the last stack pools inside its launch)
    "conv1_pool_form=0": ({}, False, 0, ran("ppo_conv3x3_pool_forward_packed_f32")),
    "conv1_pool_form=1": ({}, False, 1, ran("ppo_conv3x3_pool_forward_packed_f32")),
}


def run_inference_plan(geom, x, plan):
    sw, allow_split, form, engaged = INFERENCE_PLANS[plan]
    lib = _lib.load()
    before = lib.ppo_conv1_pool_form(-1)
    try:
        if form is not None:
            lib.ppo_conv1_pool_form(form)
            assert lib.ppo_conv1_pool_form(-1) == form
        with switches(**sw):
            net = impala_net(geom)
            net.load_state_dict(impala_parameters(geom))
            calls = record_calls(net)
            row = net.heads(net.encode(x, False, chain_split=allow_split), "i").clone()
            # the recorded launch list, with its cached pointers
            replayed = net.heads(net.encode(x, False, chain_split=allow_split), "i").clone()
            torch.cuda.synchronize()
    finally:
        lib.ppo_conv1_pool_form(before)
    assert engaged(calls, geom), (plan, names_of(calls))
    assert torch.equal(row, replayed), plan
    if allow_split:
        assert not net.chain_split_error(), plan
        if geom == "84x84" and models.CHAIN_SPLIT and "CHAIN_SPLIT" not in sw:
            assert net._chain_split_usable is True, "the split launch did not reproduce the one-workgroup launch"
    return row


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_impala_inference_every_launch_form(geom, B):
    """3a.  Every fused entry point documents "same bits as the convolutions it replaces" (include/ppo_amd.h): with
    non-zero biases in all sixteen encoder tensors that covers each form's bias reads - channel offset, layer, once."""
    x = impala_inputs(geom, B).cuda()
    rows = {plan: run_inference_plan(geom, x, plan) for plan in INFERENCE_PLANS}
    base = rows["four-convolutions"]
    err = report(f"impala-{geom}-B{B}", "head_row", rel_err(base, impala_float64_row(geom, B)), 1e-4)
    assert err < 1e-4, err
    different = [plan for plan, row in rows.items() if not torch.equal(row, base)]
    assert not different, {plan: float((rows[plan] - base).abs().max()) for plan in different}


SAVED = ("q0_0_in", "a0_0", "q0_1_in", "a0_1", "in1", "q1_0_in", "a1_0", "q1_1_in", "a1_1", "in2", "idx2",
         "q2_0_in", "a2_0", "q2_1_in", "a2_1", "flat", "idx0", "idx1", "h")


def _default_training(c):
    n = names_of(c)
    return "ppo_impala_stack_chain_forward_f32" in n and n.count("ppo_impala_stack_tail_backward_f32") == 3 \
        and "ppo_impala_stack_full_backward_f32" not in n and 16 not in tail_channels(c)


def _all_fused_training(c):
    n = names_of(c)
    return "ppo_impala_stack_chain_forward_f32" in n and 16 in tail_channels(c) \
        and "ppo_impala_stack_full_backward_f32" in n and n.count("ppo_impala_stack_tail_backward_f32") == 2


def _unfused_training(c):
    n = names_of(c)
    return not any(f.startswith("ppo_impala_stack_") for f in n) and n.count("ppo_maxpool3x3s2_backward_f32") == 3 \
        and "ppo_conv3x3_backward_weight_slabs_f32" in n and not any("slabs_batch" in f or "slabs_pooled" in f for f in n)


TRAINING_PLANS = {
    "defaults": ({}, _default_training),
    "all-fused": (dict(FUSE_STACK_FULL_BWD=1, FUSE_STACK_TAIL_BWD=7, FUSE_STACK16_MIN_BATCH=1), _all_fused_training),
    "all-unfused": (dict(FUSE_STACK_TAIL=0, WGRAD_POOLED_DY=0, WGRAD_BATCH_LAUNCH=0), _unfused_training),
}


@functools.lru_cache(maxsize=None)
def training_batch(geom):
    """B = 5: observations, actions, old log-policy (the net's own, disturbed: most ratios inside the clip range),
    advantages, returns.  Device tensors shared by the plans."""
    _dims, nA = GEOMETRIES[geom]
    B = 5
    x = impala_inputs(geom, B).cuda()
    net = impala_net(geom)
    net.load_state_dict(impala_parameters(geom))
    g = torch.Generator(device="cuda").manual_seed(7)
    raw = net.forward(x)["raw_policy"].clone()
    old_lp = torch.log_softmax(raw + 0.1 * torch.randn(B, nA, device="cuda", generator=g), dim=1).contiguous()
    actions = torch.randint(0, nA, (B,), dtype=torch.int32, device="cuda", generator=g)
    pac = old_lp.gather(1, actions.long()[:, None])[:, 0].contiguous()
    adv = torch.randn(B, device="cuda", generator=g)
    ret = torch.randn(B, 1, device="cuda", generator=g)
    return x, actions, pac, old_lp, adv, ret


@functools.lru_cache(maxsize=None)
def training_result(geom, plan):
    sw, engaged = TRAINING_PLANS[plan]
    x, actions, pac, old_lp, adv, ret = training_batch(geom)
    with switches(**sw):
        net = impala_net(geom)
        net.load_state_dict(impala_parameters(geom))
        calls = record_calls(net)
        acts = net.encode(x, train=True)
        saved = {k: acts[k].clone() for k in SAVED}
        stats = net.ppo_minibatch(x, actions, pac, old_lp, adv, ret, eps_clip=0.2, ent_coef=0.01, vf_coef=0.5, loss_scale=1.0).clone()
        torch.cuda.synchronize()
        grads = {k: v.clone() for k, v in net.grads.items()}
        acts = net.encode(x, train=True)  # same buffers, same values: the kinks of the pass that made the gradients
        for k, v in saved.items():
            assert torch.equal(acts[k], v), k
    # float64 autograd of the function the HIP forward evaluated (its own ReLU masks and max-pool taps)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in net.params.items()}
    out = R.forward_shared_kinks(sd, x.double() / 255.0, acts)
    R.ppo_loss(out, actions.long(), pac.double(), adv.double(), ret.double()).backward()
    errs = {}
    for name, p in sd.items():
        if p.grad is None:
            assert float(grads[name].abs().max()) == 0.0, name
            continue
        errs[name] = report(f"impala-{geom}-train-{plan}", f"grad:{name}", rel_err(grads[name], p.grad), 1e-5)
    return dict(saved=saved, grads=grads, stats=stats, calls=calls, errs=errs, engaged=engaged(calls))


@pytest.mark.parametrize("plan", list(TRAINING_PLANS))
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_impala_training_gradients_match_float64_given_shared_kinks(geom, plan):
    """3b, the method and bar of test_model_gpu.py::test_backward_is_exact_given_shared_kinks.  The gradients flow
    through maps that the training forms of the fused launches wrote (a0 / q0 / a1 carry each layer's bias)."""
    r = training_result(geom, plan)
    assert r["engaged"], (plan, names_of(r["calls"]))
    assert len(r["errs"]) == 36  # all but the advantage head and log_std, which do not enter the loss
    for name, e in r["errs"].items():
        assert e < 1e-5, (name, e)


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_impala_training_plans_agree_bit_for_bit(geom):
    base = training_result(geom, "all-unfused")
    for plan in ("defaults", "all-fused"):
        r = training_result(geom, plan)
        for k, v in base["saved"].items():
            assert torch.equal(v, r["saved"][k]), (plan, k)
        assert torch.equal(base["stats"], r["stats"]), plan
        for name, gb in base["grads"].items():
            ga = r["grads"][name]
            if ".blocks." in name or name.startswith("encoder.stacks.2.firstconv"):
                # batched weight-gradient launches sum the same products in another (fixed) order: see
                # test_model_gpu.py::test_fused_stack_tail_is_bit_identical_to_four_convolutions
                assert float((ga - gb).abs().max()) <= 2e-6 * max(float(gb.abs().max()), 1e-30), (plan, name)
            else:
                assert torch.equal(ga, gb), (plan, name)


def test_medium_precision_reads_the_same_biases():
    """3e.  The split-bf16 launches take their own bias pointer table (models._build_split_bf16)."""
    geom, B = "84x84", 9
    x = impala_inputs(geom, B).cuda()
    rows = {}
    for precision in ("high", "medium"):
        net = impala_net(geom, precision)
        net.load_state_dict(impala_parameters(geom))
        calls = record_calls(net)
        rows[precision] = net.forward(x)["_heads"].clone()
        torch.cuda.synchronize()
        assert (names_of(calls).count("ppo_impala_stack_tail_forward_bf16x3") == 3) == (precision == "medium")
        assert any("bf16x3" in f and "conv3x3" in f for f in names_of(calls)) == (precision == "medium")
        err = report(f"impala-{geom}-B{B}-{precision}", "head_row", rel_err(rows[precision], impala_float64_row(geom, B)), 1e-4)
        assert err < 1e-4, (precision, err)
    assert not torch.equal(rows["high"], rows["medium"])


# ---------------------------------------------------------------------------------------------- Nature
def nature_bar(name):
    return 1e-4 if name.startswith("encoder.conv") else 1e-5


@pytest.mark.parametrize("dims,hidden,B", [((4, 84, 84), 512, 3), ((4, 36, 36), 64, 1)], ids=["84x84-B3", "36x36-B1"])
def test_nature_forward_and_gradients_match_float64(dims, hidden, B):
    """3c.  ReLUs are re-decided in float64 here; the smallest |pre-activation| relative to its layer's largest is
    printed (RELU_MARGIN) so that a near-tie would be seen for what it is."""
    nA = 6
    torch.manual_seed(11)
    net = models.DualHeadNet("nature", dims, nA, hidden_units=hidden, head_scale=0.1, head_bias=True, device="cuda")
    cpu = T.perturbed_state_dict(net.state_dict(), SEED)
    net.load_state_dict(cpu)
    calls = record_calls(net)
    rng = np.random.default_rng(5 + B)
    x = torch.from_numpy(rng.integers(0, 256, size=(B, *dims), dtype=np.uint8))
    case = f"nature-{dims[1]}x{dims[2]}-B{B}"
    sd = T.as_double(cpu, requires_grad=True)
    o = T.nature_forward(sd, x.double() / 255.0)
    for _ in range(2):  # the second forward replays the recorded launch list
        row = net.forward(x.cuda())["_heads"].clone()
        assert report(case, "head_row", rel_err(row, o), 1e-4) < 1e-4
    assert names_of(calls).count("ppo_conv2d_strided_forward_f32") == 3
    with torch.no_grad():
        h, margin = x.double() / 255.0, 1.0
        for name, stride in (("conv1", 4), ("conv2", 2), ("conv3", 1)):
            pre = torch.nn.functional.conv2d(h, sd[f"encoder.{name}.weight"], sd[f"encoder.{name}.bias"], stride=stride)
            margin, h = min(margin, float(pre.abs().min() / pre.abs().max())), torch.relu(pre)
        pre = torch.nn.functional.linear(h.reshape(B, -1), sd["encoder.fc.weight"], sd["encoder.fc.bias"])
        margin = min(margin, float(pre.abs().min() / pre.abs().max()))
    print(f"RELU_MARGIN {case} {margin:.2e}")
    # one PPO minibatch
    actions = torch.from_numpy(rng.integers(0, nA, size=(B,)).astype(np.int64))
    old_lp = torch.log_softmax(o.detach()[:, :nA].float() + torch.from_numpy(rng.normal(size=(B, nA)).astype(np.float32)) * 0.1, dim=1)
    pac = old_lp[torch.arange(B), actions].contiguous()
    adv = torch.from_numpy(rng.normal(size=(B,)).astype(np.float32))
    ret = torch.from_numpy(rng.normal(size=(B, 1)).astype(np.float32))
    net.ppo_minibatch(x.cuda(), actions.int().cuda(), pac.cuda(), old_lp.cuda(), adv.cuda(), ret.cuda(), eps_clip=0.2, ent_coef=0.01,
                      vf_coef=0.5, loss_scale=1.0)
    torch.cuda.synchronize()
    out = {"raw_policy": o[:, :nA], "log_policy": torch.log_softmax(o[:, :nA], dim=1), "value": o[:, nA:nA + 1]}
    R.ppo_loss(out, actions, pac.double(), adv.double(), ret.double()).backward()
    worst = {}
    for name, p in sd.items():
        if p.grad is None or float(p.grad.abs().max()) == 0.0:  # the advantage head and log_std do not enter the loss
            assert float(net.grads[name].abs().max()) == 0.0, name
            continue
        worst[name] = report(case, f"grad:{name}", rel_err(net.grads[name], p.grad), nature_bar(name))
    assert len(worst) == 12
    for name, e in worst.items():
        assert e < nature_bar(name), (name, e, margin)


# ---------------------------------------------------------------------------------------------- MLP
# the shapes of the three reference variants of tests/test_variants_gpu.py (tanh, relu, and the Humanoid-sized one)
MLP_VARIANTS = {
    "mlp_disc": dict(input_dims=(4,), n_actions=2, hidden=64, activation="relu", n_tvf=0, gaussian=False),
    "mlp_gauss_tvf": dict(input_dims=(11,), n_actions=3, hidden=64, activation="tanh", n_tvf=8, gaussian=True),
    "humanoid": dict(input_dims=(377,), n_actions=17, hidden=256, activation="tanh", n_tvf=128, gaussian=True),
}


def mlp_model(tag, fuse):
    v = MLP_VARIANTS[tag]
    horizons = list(range(1, v["n_tvf"] + 1)) if v["n_tvf"] else None
    with switches(FUSE_MLP=fuse):
        torch.manual_seed(7)
        model = models.TVFModel("mlp", input_dims=v["input_dims"], actions=v["n_actions"], device="cuda", architecture="dual",
                                hidden_units=v["hidden"], encoder_activation_fn=v["activation"], head_scale=0.1, head_bias=True,
                                tvf_fixed_head_horizons=horizons, tvf_fixed_head_weights=[1.0] * v["n_tvf"] if horizons else None)
    assert model.policy_net.mlp_fused == bool(fuse) and model.value_net.mlp_fused == bool(fuse)
    return model


@functools.lru_cache(maxsize=None)
def mlp_parameters(tag):
    """(policy net's, value net's) perturbed parameters, CPU tensors."""
    model = mlp_model(tag, 0)
    return (T.perturbed_state_dict(model.policy_net.state_dict(), SEED), T.perturbed_state_dict(model.value_net.state_dict(), SEED + 1))


def load_mlp(model, tag):
    pol, val = mlp_parameters(tag)
    model.policy_net.load_state_dict(pol)
    model.value_net.load_state_dict(val)
    return model


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused-mlp", "op-by-op"])
@pytest.mark.parametrize("tag", list(MLP_VARIANTS))
def test_mlp_heads_match_float64(tag, fuse):
    """3d, forward.  Batches 1, 7 and 130: a single row, a ragged 16-row tile, and more tiles than one wave takes in one
    go plus a ragged last one - the fused kernel's bias quads travel in a prefetch ring from tile to tile."""
    v = MLP_VARIANTS[tag]
    model = load_mlp(mlp_model(tag, fuse), tag)
    net = model.policy_net
    calls = record_calls(net)
    sd = T.as_double(mlp_parameters(tag)[0])
    for B in (1, 7, 130):
        x = torch.randn(B, *v["input_dims"], generator=torch.Generator().manual_seed(B))
        with torch.no_grad():
            want = R.mlp_forward(sd, x.double(), v["activation"])
        with switches(FUSE_MLP=fuse):
            got = net.forward(x.cuda())
            torch.cuda.synchronize()
        for k in ("raw_policy", "value", "advantage") + (("tvf_value",) if v["n_tvf"] else ()):
            err = report(f"{tag}-{'fused' if fuse else 'op-by-op'}-B{B}", k, rel_err(got[k], want[k]), 1e-4)
            assert err < 1e-4, (B, k, err)
    assert ("ppo_mlp_forward_f32" in names_of(calls)) == bool(fuse)


def stats_close(a, b, tol, what):
    a, b = a.double(), b.double()
    scale = b.abs().amax(dim=0).clamp_min(1e-6)
    err = ((a - b).abs().amax(dim=0) / scale).max()
    assert float(err) <= tol, f"{what}: statistics differ by {float(err):.3e} of their column's largest entry"


def grads_close(fused, plain, tol, what):
    assert float(plain.grad.abs().max()) > 0, what
    for name, gp in plain.grads.items():
        gf = fused.grads[name]
        scale = float(gp.abs().max())
        if scale == 0.0:
            assert float(gf.abs().max()) == 0.0, (what, name)
            continue
        err = float((gf - gp).abs().max()) / scale
        assert err <= tol, f"{what}: grad {name} differs by {err:.3e} of its largest entry"


@pytest.mark.parametrize("tag", list(MLP_VARIANTS))
def test_mlp_training_phases_fused_against_op_by_op(tag):
    """3d, training: the three launches of the fused path (csrc/mlp_fused.hip) against the op-by-op path on the same
    perturbed parameters - every phase the variant has, flat gradient and per-sample statistics at 2e-5 (the tolerance
    of test_variants_gpu.py::check_grads); the discrete PPO phase also against float64 autograd; log_std's gradient must
    be non-zero and follow a rotation of log_std."""
    v = MLP_VARIANTS[tag]
    B, nA, K = 37, v["n_actions"], v["n_tvf"]
    fused, plain = load_mlp(mlp_model(tag, 1), tag), load_mlp(mlp_model(tag, 0), tag)
    fused_calls = record_calls(fused.policy_net)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, *v["input_dims"], generator=g)
    adv = torch.randn(B, generator=g).cuda()
    ret = torch.randn(B, 1, generator=g).cuda()
    pol_sd = T.as_double(mlp_parameters(tag)[0], requires_grad=True)
    out64 = R.mlp_forward(pol_sd, x.double(), v["activation"])
    mu = out64["raw_policy"].detach().float()
    xd = x.cuda()

    def both(method, net_name, *args, **kw):
        res = []
        for model, fuse in ((fused, 1), (plain, 0)):
            net = getattr(model, net_name)
            net.grad.zero_()
            with switches(FUSE_MLP=fuse):
                res.append(getattr(net, method)(*args, **kw).clone())
            torch.cuda.synchronize()
        what = f"{tag} {method}"
        stats_close(res[0], res[1], 2e-5, what)
        grads_close(getattr(fused, net_name), getattr(plain, net_name), 2e-5, what)
        return res[0]

    if v["gaussian"]:
        log_std = mlp_parameters(tag)[0]["log_std"]
        actions = (mu + torch.exp(log_std) * torch.randn(B, nA, generator=g)).contiguous()
        old_pac = (torch.distributions.Normal(mu, torch.exp(log_std)).log_prob(actions) + 0.1 * torch.randn(B, nA, generator=g)).contiguous()
        both("gaussian_minibatch", "policy_net", xd, actions.cuda(), old_pac.cuda(), adv, None, eps_clip=0.2)
        first = {name: (m.policy_net.grads["log_std"].clone(), m.policy_net.grad.clone()) for name, m in (("fused", fused), ("plain", plain))}
        assert float(first["fused"][0].abs().min()) > 0 and float(first["plain"][0].abs().min()) > 0
        # the same minibatch with log_std rotated by one action: sigma_a moves to another column of the actions
        rolled = dict(mlp_parameters(tag)[0], log_std=torch.roll(log_std, 1))
        for name, model, fuse in (("fused", fused, 1), ("plain", plain, 0)):
            net = model.policy_net
            net.load_state_dict(rolled)
            with switches(FUSE_MLP=fuse):
                net.gaussian_minibatch(xd, actions.cuda(), old_pac.cuda(), adv, None, eps_clip=0.2)
            torch.cuda.synchronize()
            assert not torch.equal(net.grads["log_std"], first[name][0]), name
            assert not torch.equal(net.grads["log_std"], torch.roll(first[name][0], 1)), name
            net.load_state_dict(mlp_parameters(tag)[0])
        grads_close(fused.policy_net, plain.policy_net, 2e-5, f"{tag} gaussian_minibatch, log_std rotated and restored")
    else:
        actions = torch.randint(0, nA, (B,), generator=g)
        old_lp = torch.log_softmax(mu + 0.1 * torch.randn(B, nA, generator=g), dim=1).contiguous()
        pac = old_lp[torch.arange(B), actions].contiguous()
        both("ppo_minibatch", "policy_net", xd, actions.int().cuda(), pac.cuda(), old_lp.cuda(), adv, None, eps_clip=0.2, ent_coef=0.01,
             vf_coef=0.0)
        out64["log_policy"] = torch.log_softmax(out64["raw_policy"], dim=1)
        R.ppo_loss(out64, actions, pac.double(), adv.cpu().double(), torch.zeros(B, 1, dtype=torch.float64), vf_coef=0.0).backward()
        for name, net in (("fused", fused.policy_net), ("op-by-op", plain.policy_net)):
            n_checked = 0
            for pname, p in pol_sd.items():
                if p.grad is None or float(p.grad.abs().max()) == 0.0:
                    assert float(net.grads[pname].abs().max()) == 0.0, pname
                    continue
                n_checked += 1
                err = report(f"{tag}-{name}-ppo", f"grad:{pname}", rel_err(net.grads[pname], p.grad), 2e-5)
                assert err < 2e-5, (name, pname, err)
            assert n_checked == 6  # fc1, fc2, policy head: weights and biases (vf_coef = 0 leaves the value head out)
    # value phase
    kw = dict(returns=ret, vf_coef=0.5)
    if K:
        kw.update(tvf_returns=torch.randn(B, K, generator=g).cuda(), tvf_weights=(0.5 + torch.rand(K, generator=g)).cuda(), tvf_coef=1.0)
    both("value_minibatch", "value_net", xd, **kw)
    # distillation phase
    if v["gaussian"]:
        both("distil_minibatch", "policy_net", xd, torch.randn(B, K, generator=g).cuda(), (mu + 0.1 * torch.randn(B, nA, generator=g)).cuda(),
             beta=1.0, use_tvf=True, weights=(0.5 + torch.rand(K, generator=g)).cuda(), gaussian=True)
    else:
        both("distil_minibatch", "policy_net", xd, torch.randn(B, generator=g).cuda(),
             torch.log_softmax(mu + 0.1 * torch.randn(B, nA, generator=g), dim=1).contiguous().cuda(), beta=1.0)
    assert names_of(fused_calls).count("ppo_mlp_train_f32") >= 2


# ---------------------------------------------------------------------------------------------- adjust_value_scale
def _scale_model(kind):
    if kind == "mlp-dual":
        return load_mlp(mlp_model("mlp_gauss_tvf", 1), "mlp_gauss_tvf"), torch.randn(9, 11, generator=torch.Generator().manual_seed(1)).cuda()
    torch.manual_seed(11)
    model = models.TVFModel("impala", input_dims=(4, 84, 84), actions=6, device="cuda", architecture="single", hidden_units=256,
                            head_scale=0.1, head_bias=True, tvf_fixed_head_horizons=[1, 10, 100, 1000], tvf_fixed_head_weights=[1.0] * 4)
    model.policy_net.load_state_dict(T.perturbed_state_dict(model.policy_net.state_dict(), SEED))
    return model, impala_inputs("84x84", 9).cuda()


@pytest.mark.parametrize("kind", ["mlp-dual", "impala-single"])
def test_adjust_value_scale(kind):
    """3f.  rl/models.py:630-651: weights AND biases of the value head (process_value) and of the TVF head (process_tvf)
    times the factor, in the policy net and the value net, or in the value net alone (value_net_only; the policy net of
    a single model, which is its value net) - and nothing else.  A bias left unscaled shows only when it is non-zero."""
    f = 0.37
    model, x = _scale_model(kind)
    nets = {"policy_net": model.policy_net} if kind == "impala-single" else {"policy_net": model.policy_net, "value_net": model.value_net}
    assert all(float(net.params[h + ".bias"].abs().min()) > 0 for net in nets.values() for h in ("value_head", "tvf_head"))

    def outputs():
        out = {k: v.clone() for k, v in model.forward(x, output="full").items()}
        torch.cuda.synchronize()
        return out

    def snapshot():
        return {(n, k): v.clone() for n, net in nets.items() for k, v in net.params.items()}

    def check_touched(before, touched):
        """touched: {(net, head)}; every other parameter must keep its bits."""
        for (n, k), was in before.items():
            now = nets[n].params[k]
            if (n, k.rsplit(".", 1)[0]) in touched:
                assert torch.equal(now, was * f), (n, k)
                assert not torch.equal(now, was), (n, k)
            else:
                assert torch.equal(now, was), (n, k)

    out0, p0 = outputs(), snapshot()
    model.adjust_value_scale(f)
    check_touched(p0, {(n, h) for n in nets for h in ("value_head", "tvf_head")})
    out1 = outputs()
    scaled = [k for k in out0 if k.endswith("value") and "raw" not in k]
    assert any("tvf_value" in k for k in scaled) and any(k.endswith("_value") and "tvf" not in k for k in scaled)
    for k in out0:
        if k in scaled:
            err = rel_err(out1[k], out0[k].double() * f)
            print(f"VALUE_SCALE {kind} {k} err={err:.3e} bar=1e-06")
            assert err <= 1e-6, (k, err)
        elif "raw_policy" in k or "log_policy" in k or "advantage" in k:
            assert torch.equal(out1[k], out0[k]), k
    # the switches, each from the state the call before left
    p1 = snapshot()
    model.adjust_value_scale(f, process_value=False)
    check_touched(p1, {(n, "tvf_head") for n in nets})
    p2 = snapshot()
    model.adjust_value_scale(f, process_tvf=False)
    check_touched(p2, {(n, "value_head") for n in nets})
    p3 = snapshot()
    model.adjust_value_scale(f, value_net_only=True)
    only = "policy_net" if kind == "impala-single" else "value_net"  # a single model's value net IS its policy net
    check_touched(p3, {(only, "value_head"), (only, "tvf_head")})
    p4 = snapshot()
    model.adjust_value_scale(f, process_value=False, process_tvf=False)
    check_touched(p4, set())
