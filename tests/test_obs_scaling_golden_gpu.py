"""GPU: TVFModel(observation_scaling=centered|unit) end to end.

Against tests/golden/obs_scaling_golden.npz (the reference's TVFModel on CPU, tests/golden/make_obs_scaling_golden.py):
the product loads the reference's weights and reproduces log_policy / value of a uint8 batch at the forward bar of
tests/test_model_gpu.py (1e-4 of the tensor's largest value) - the Nature encoder on (4, 36, 36) (strided kernels), IMPALA
on (3, 16, 16) (the generic 3x3 kernels) and IMPALA behind the observation normaliser.  The specialised first layer,
which no fixture of that size reaches: a (4, 84, 84) IMPALA net in each mode against the same net fed the pre-scaled
float32 batch, forward and one PPO minibatch's gradients.  And a Runner built the way train.py builds it under
--observation_scaling=unit: a rollout and train() through the indexed uint8 first layer, finite losses."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import obs_scaling_torch as O  # noqa: E402
from ppo_amd import models  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return (np.load(os.path.join(golden_dir, "obs_scaling_golden.npz")),
            json.load(open(os.path.join(golden_dir, "obs_scaling_golden.json"))))


def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("tag", ["nature", "impala", "impala_norm"])
def test_forward_matches_the_reference(gold, tag, scaling):
    g, meta = gold
    m = meta["models"][tag]
    model = models.TVFModel(m["encoder"], input_dims=tuple(m["input_dims"]), actions=meta["n_actions"], device="cuda",
                            architecture="single", hidden_units=meta["hidden_units"], head_scale=meta["head_scale"],
                            head_bias=meta["head_bias"], observation_normalization=m["observation_normalization"],
                            norm_eps=meta.get("norm_eps", 1e-5), observation_scaling=scaling)
    assert model.observation_scaling == model.policy_net.observation_scaling == scaling
    assert model.policy_net.u8_mode == O.IN_MODE[scaling]
    names = meta["models"][m["weights"]]["state_dict"]
    model.load_state_dict({f"policy_net.{n}": g[f"{m['weights']}.{n}"] for n in names})
    if m["observation_normalization"]:
        assert model.obs_norm.observation_scaling == scaling and model.obs_norm.u8_prep == O.OBS_PREP[scaling]
        model.obs_norm.load_state_dict({"mean": g[f"{tag}_{scaling}_obs_mean"], "var": g[f"{tag}_{scaling}_obs_var"],
                                        "count": float(g[f"{tag}_{scaling}_obs_count"])})
    out = model.forward(torch.from_numpy(g[f"{tag}_x"]).cuda(), output="policy")
    torch.cuda.synchronize()
    for k in ("log_policy", "value"):
        err = rel_err(out[k].cpu().numpy(), g[f"{tag}_{scaling}_{k}"])
        print(f"OBS_SCALING_GOLDEN {tag} {scaling} {k} rel_err={err:.3e}")
        assert err < 1e-4, (k, err)
    # and the scaling matters: the other mode's answer is far outside the bar (not behind the normaliser, which undoes
    # the factor 6 between the two up to its epsilon)
    other = "unit" if scaling == "centered" else "centered"
    if not m["observation_normalization"]:
        assert rel_err(out["log_policy"].cpu().numpy(), g[f"{tag}_{other}_log_policy"]) > 1e-3


@pytest.mark.parametrize("scaling", O.SIGNED)
def test_nature_split_pairs_keep_their_split_launches(gold, scaling):
    """--precision=medium: the pairs of models.NATURE_SPLIT run as split-bf16 launches in the new modes too - conv1's
    forward and weight gradient read the bytes with the model's mode - and the forward stays at the bar
    tests/test_nature_bf16x3_gpu.py holds the split forward to (1e-4)."""
    g, meta = gold
    m = meta["models"]["nature"]
    net = models.DualHeadNet("nature", tuple(m["input_dims"]), meta["n_actions"], hidden_units=meta["hidden_units"],
                             head_scale=meta["head_scale"], head_bias=meta["head_bias"], device="cuda", precision="medium",
                             observation_scaling=scaling)
    net.load_state_dict({n: g[f"nature.{n}"] for n in m["state_dict"]})
    net.use_plans = False  # every launch through _call, the inference forward's too
    calls = []
    orig = net._call
    net._call = lambda fn, *a: (calls.append((fn, a)), orig(fn, *a))[1]
    x = torch.from_numpy(g["nature_x"]).cuda()
    out = {k: v.clone() for k, v in net.forward(x).items() if k in ("log_policy", "value")}
    B = x.shape[0]
    actions = torch.zeros(B, dtype=torch.int32, device="cuda")
    stats = net.ppo_minibatch(x, actions, out["log_policy"][:, 0].contiguous(), out["log_policy"].clone(),
                              torch.ones(B, device="cuda"), torch.zeros(B, 1, device="cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and torch.isfinite(net.grad).all()
    for k in ("log_policy", "value"):
        assert rel_err(out[k].cpu().numpy(), g[f"nature_{scaling}_{k}"]) < 1e-4, k
    strided = [(fn, a) for fn, a in calls if fn.startswith("ppo_conv2d_strided_")]
    for layer, conv_pass in models.NATURE_SPLIT:
        assert any(fn == f"ppo_conv2d_strided_{conv_pass}_bf16x3" for fn, _a in strided), (layer, conv_pass)
    assert sum(fn.endswith("bf16x3") for fn, _a in strided) >= len(models.NATURE_SPLIT)
    # the launches that read the observations carry the model's mode (second argument), the others PPO_IN_NONE
    modes = {a[1] for fn, a in strided if "backward_data" not in fn and a[0] == x.data_ptr()}
    assert modes == {O.IN_MODE[scaling]}
    assert {a[1] for fn, a in strided if "backward_data" not in fn and a[0] != x.data_ptr()} == {0}


@pytest.mark.parametrize("scaling", O.SIGNED)
def test_normaliser_statistics_follow_the_prepared_observation(gold, scaling):
    """Three updates of the product's normaliser on the batches the fixture's generator drew give the reference's running
    statistics (to the float32 rounding of a batch mean the reference itself has: csrc/obs_norm.hip)."""
    g, meta = gold
    dims = tuple(meta["models"]["impala_norm"]["input_dims"])
    rng = np.random.default_rng(meta["seed"] + len("impala_norm"))
    x = rng.integers(0, 256, size=(8, *dims), dtype=np.uint8)
    x[0, :, 0, :] = 0
    assert np.array_equal(x, g["impala_norm_x"]), "this NumPy draws other batches than the generator's"
    norm = models.ObsNormalizer(dims, "cuda", norm_eps=meta["norm_eps"], observation_scaling=scaling)
    for _ in range(3):
        norm.update(torch.from_numpy(rng.integers(0, 256, size=(8, *dims), dtype=np.uint8)).cuda())
    sd = norm.state_dict()
    assert sd["count"] == pytest.approx(float(g[f"impala_norm_{scaling}_obs_count"]), rel=1e-12)
    span = {"centered": 1.0, "unit": 6.0}[scaling]
    assert np.abs(sd["mean"].numpy().reshape(dims) - g[f"impala_norm_{scaling}_obs_mean"]).max() < 1e-6 * span
    assert np.abs(sd["var"].numpy().reshape(dims) - g[f"impala_norm_{scaling}_obs_var"]).max() < 1e-6 * span * span


@pytest.mark.parametrize("scaling", O.SIGNED)
def test_specialised_first_layer_against_the_prescaled_float_batch(scaling):
    """IMPALA on (4, 84, 84): the fused conv + pool launch reads the bytes in the new mode; the same net fed
    prep(x) as float32 reads them with PPO_IN_NONE.  Same weights, same arithmetic behind the load."""
    torch.manual_seed(3)
    net = models.DualHeadNet("impala", (4, 84, 84), 6, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda",
                             observation_scaling=scaling)
    assert not net.generic_convs, "the north-star net keeps its specialised kernels"
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, size=(5, 4, 84, 84), dtype=np.uint8)
    x[0] = 0
    x[1, :, :3] = 0
    xu = torch.from_numpy(x)
    got = {k: v.clone() for k, v in net.forward(xu.cuda()).items() if k in ("log_policy", "value")}
    ref = {k: v.clone() for k, v in net.forward(O.prep(xu, scaling).cuda()).items() if k in ("log_policy", "value")}
    torch.cuda.synchronize()
    for k in got:
        err = rel_err(got[k].cpu().numpy(), ref[k].cpu().numpy())
        print(f"OBS_SCALING_84 {scaling} {k} rel_err={err:.3e}")
        assert err < 1e-4, (k, err)
    scaled = models.DualHeadNet("impala", (4, 84, 84), 6, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda")
    scaled.load_state_dict(net.state_dict())
    assert rel_err(scaled.forward(xu.cuda())["log_policy"].cpu().numpy(), ref["log_policy"].cpu().numpy()) > 1e-3
    # one PPO minibatch each way: the first layer's weight gradient comes from the pooled-gradient launch reading the bytes
    # in the new mode, resp. the float batch; the gradient bar of tests/test_model_gpu.py (1e-4 of the tensor's maximum)
    B = x.shape[0]
    actions = torch.from_numpy(rng.integers(0, 6, size=(B,)).astype(np.int32)).cuda()
    lp = got["log_policy"]
    old_pac = lp[torch.arange(B), actions.long()].contiguous()
    adv = torch.from_numpy(rng.normal(size=(B,)).astype(np.float32)).cuda()
    ret = torch.from_numpy(rng.normal(size=(B, 1)).astype(np.float32)).cuda()
    grads = []
    for batch in (xu.cuda(), O.prep(xu, scaling).cuda()):
        stats = net.ppo_minibatch(batch, actions, old_pac, lp.clone(), adv, ret)
        torch.cuda.synchronize()
        assert torch.isfinite(stats).all()
        grads.append({n: t.clone() for n, t in net.grads.items()})
    for n in ("encoder.stacks.0.firstconv.weight", "encoder.stacks.0.firstconv.bias", "policy_head.weight"):
        err = rel_err(grads[0][n].cpu().numpy(), grads[1][n].cpu().numpy())
        print(f"OBS_SCALING_84 {scaling} grad {n} rel_err={err:.3e}")
        assert float(grads[1][n].abs().max()) > 0 and err < 1e-4, (n, err)


def test_float_observations_ignore_the_flag():
    torch.manual_seed(3)
    a = models.DualHeadNet("impala", (4, 84, 84), 6, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda")
    b = models.DualHeadNet("impala", (4, 84, 84), 6, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda",
                           observation_scaling="unit")
    b.load_state_dict(a.state_dict())
    x = torch.rand(3, 4, 84, 84, device="cuda")
    assert torch.equal(a.forward(x)["log_policy"], b.forward(x)["log_policy"])


def test_runner_trains_under_unit_scaling(tmp_path):
    import train
    from ppo_amd import envs, logger, rollout
    from ppo_amd.config import args
    args.setup(["--agents=8", "--n_steps=8", "--model_architecture=single", "--model_encoder=impala", "--env_type=synthetic",
                "--env_synthetic_shape=4,84,84", "--env_embed_time=False", "--seed=4", "--policy_opt_mini_batch_size=32",
                "--policy_opt_epochs=1", "--env_warmup_period=5", "--experiment_name=exp", "--run_name=obs_scaling",
                "--model_hidden_units=64", "--observation_scaling=unit", "--device=cuda",
                f"--output_folder={tmp_path}"])
    try:
        torch.manual_seed(1)
        np.random.seed(9)
        log = logger.Logger(quiet=True)
        model = train.make_model(log)
        assert model.observation_scaling == "unit" and model.policy_net.u8_mode == O.IN_MODE["unit"]
        r = rollout.Runner(model, log)
        r.vec_env = envs.create_envs_classic()
        r.reset()
        start = r.net.flat.clone()
        r.generate_rollout()
        r.calculate_returns()
        r.train()
        torch.cuda.synchronize()
        net = r.net
        assert torch.isfinite(net.flat).all() and torch.isfinite(net.grad).all() and not torch.equal(net.flat, start)
        stat_rows = [t for (bname, _shape, _dt), t in net._bufs.items() if bname.startswith("stat_rows_")]
        assert stat_rows and all(torch.isfinite(t).all() for t in stat_rows), "a minibatch's loss statistics are not finite"
        assert net.takes_obs_index(r.all_obs), "the minibatches read the uint8 rollout buffer through the index"
        name = "encoder.stacks.0.firstconv.weight"
        o, shape = net._offsets[name]
        n = int(np.prod(shape))
        assert not torch.equal(net.flat[o:o + n], start[o:o + n]), f"{name} did not move"
    finally:
        args.setup([])
