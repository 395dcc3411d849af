"""GPU: TVFModel(use_rnd=True) - prediction_net / target_net on the HIP kernels - against tests/golden/rnd_golden.npz (the
reference's RND path on CPU, tests/golden/make_rnd_golden.py).

The model is built from the fixture's seed (tests/test_rnd_cpu.py checks that the seed gives the reference's initial
weights) and given the fixture's observation-normaliser state.  Bars: rnd_error within 1e-4 of its max;
the loss of one train_rnd_minibatch within 2e-6, the dense layers' gradients within 1e-5 and the convolutions' within 1e-4
of each tensor's max; the predictor after one optimiser step within 2e-6.  The fixture's seed leaves every leaky-ReLU /
ReLU pre-activation at least 1e-5 from zero, so nothing is excluded.  Tensors the fixture stores as every k-th row are
compared on those rows and on the float64 sum and sum of squares of the whole tensor.

The functional test: 200 predictor steps on 8 fixed observations bring their mean error below a tenth of where it
started, while 8 observations the predictor never saw keep a larger error than the trained ones."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import _lib, models  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "rnd_golden.npz")), json.load(open(os.path.join(golden_dir, "rnd_golden.json")))


def make_model(meta, g=None, architecture="single"):
    torch.manual_seed(meta["seed"])
    model = models.TVFModel(encoder="nature", input_dims=tuple(meta["input_dims"]), actions=meta["n_actions"], device="cuda",
                            architecture=architecture, hidden_units=meta["hidden_units"], use_rnd=True,
                            observation_normalization=True, head_scale=meta["head_scale"], head_bias=meta["head_bias"],
                            value_head_names=("ext", "int"))
    if g is not None:
        model.obs_norm.load_state_dict({"mean": g["obs_mean"], "var": g["obs_var"], "count": float(g["obs_count"])})
    return model


def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def compare_stored(g, meta, key, got, bar, absolute=False):
    """`got` (whole tensor) against the fixture's rows of it; returns the error measured."""
    got = np.asarray(got, np.float64)
    stride = meta["row_stride"][key]
    ref = g[key].astype(np.float64)
    e = np.abs(got[::stride] - ref).max() / (1.0 if absolute else max(np.abs(ref).max(), 1e-30))
    if stride > 1:
        s, q = g["whole_" + key]
        assert abs(got.sum() - s) <= 1e-4 * max(np.sqrt(q), 1e-30), key       # a sum of n terms of rms sqrt(q / n)
        assert abs((got ** 2).sum() - q) <= 1e-4 * q, key
    print(f"RND_MODEL {key} err={e:.3e} bar={bar:.0e}")
    return e


def test_state_dict_and_ownership(gold):
    g, meta = gold
    model = make_model(meta)
    keys = list(model.state_dict().keys())
    rnd_keys = [f"{net}.{n}" for net in ("prediction_net", "target_net") for n in meta["param_names"][net]]
    assert keys[-len(rnd_keys):] == rnd_keys
    assert not [k for k in keys[:-len(rnd_keys)] if "prediction_net" in k or "target_net" in k]
    assert model.policy_net.vh == 2 and model.policy_net.value_head_names == ["ext", "int"]
    assert model.target_net.grad is None and model.target_net.grads is None   # the target is never given a gradient
    assert list(model.prediction_net.grads) == meta["param_names"]["prediction_net"]
    # off: no RND keys, no RND objects
    torch.manual_seed(meta["seed"])
    plain = models.TVFModel(encoder="nature", input_dims=tuple(meta["input_dims"]), actions=meta["n_actions"], device="cuda",
                            architecture="single", hidden_units=meta["hidden_units"], observation_normalization=True,
                            head_scale=meta["head_scale"], head_bias=meta["head_bias"], value_head_names=("ext", "int"))
    assert list(plain.state_dict().keys()) == keys[:-len(rnd_keys)] and plain.rnd is None
    with pytest.raises(_lib.PpoAmdError):
        plain.rnd_prediction_error(torch.zeros((1, *meta["input_dims"]), dtype=torch.uint8))
    # a state_dict round trip restores both nets
    other = make_model(dict(meta, seed=meta["seed"] + 1))
    assert not torch.equal(other.prediction_net.flat, model.prediction_net.flat)
    other.load_state_dict(model.state_dict())
    assert torch.equal(other.prediction_net.flat, model.prediction_net.flat)
    assert torch.equal(other.target_net.flat, model.target_net.flat)


def test_rnd_error_matches_reference(gold):
    g, meta = gold
    model = make_model(meta, g)
    x = torch.from_numpy(g["fwd_x"]).cuda()
    err = model.rnd_prediction_error(g["fwd_x"])
    assert err.shape == (8,) and err.dtype == torch.float32
    e = rel_err(err.cpu().numpy(), g["fwd_rnd_error"])
    print(f"RND_MODEL fwd_rnd_error err={e:.3e}")
    assert e <= 1e-4
    out = model.forward(x, output="policy", include_rnd=True)
    assert torch.equal(out["rnd_error"], err) and "log_policy" in out and out["value"].shape == (8, 2)
    assert "rnd_error" not in model.forward(x, output="policy")
    # float observations take the same path as uint8 ones
    errf = model.rnd_prediction_error(x.float() / 255.0)
    assert rel_err(errf.cpu().numpy(), g["fwd_rnd_error"]) <= 1e-4
    # the indexed form reads the rows it is told to
    index = torch.tensor([7, 0, 0, 3], dtype=torch.int32, device="cuda")
    assert torch.equal(model.rnd.prediction_error(x, index=index), err[index.long()])
    # and the strided form writes one column of a [B, 3] buffer
    wide = torch.full((8, 3), -1.0, device="cuda")
    model.rnd.prediction_error(x, err=wide[:, 1], err_stride=3)
    assert torch.equal(wide[:, 1], err) and bool((wide[:, ::2] == -1.0).all())


def test_train_minibatch_and_optimizer_step_match_reference(gold):
    g, meta = gold
    assert meta["margin"] >= 1e-5
    model = make_model(meta, g)
    rnd = model.rnd
    target_before = model.target_net.flat.clone()
    x = torch.from_numpy(g["mb_x"]).cuda()
    stats = torch.zeros(_lib.PPO_RND_STATS, device="cuda")
    err = rnd.train_minibatch(x, loss_scale=1.0, stats=stats)
    torch.cuda.synchronize()
    s = stats.cpu().numpy().astype(np.float64)
    loss = float(g["mb_loss"])
    print(f"RND_MODEL loss={err.double().mean().item():.9f} stats_loss={s[0] / 8:.9f} ref={loss:.9f}")
    assert abs(err.double().mean().item() - loss) <= 2e-6 * max(1.0, abs(loss))
    assert abs(s[0] / 8 - loss) <= 2e-6 * max(1.0, abs(loss))
    feat = g["mb_feat"]  # mean, var over the batch axis averaged over features, max |.| (rl/models.py:732-734)
    assert s[4] == 1.0
    assert abs(s[1] - feat[0]) <= 1e-5 and abs(s[2] - feat[1]) <= 1e-4 * feat[1] and abs(s[3] - feat[2]) <= 1e-4 * feat[2]
    assert meta["grad_none"] == ["target_net." + n for n in meta["param_names"]["target_net"]]
    worst = {}
    for name in meta["param_names"]["prediction_net"]:
        bar = 1e-4 if name.startswith("conv") else 1e-5
        worst[name] = (compare_stored(g, meta, "grad_" + name, rnd.prediction_net.grads[name].cpu().numpy(), bar), bar)
    for name, (e, bar) in worst.items():
        assert e <= bar, (name, e)

    gn = torch.zeros(1, device="cuda")
    opt = meta["opt"]
    assert opt["grad_clip_mode"] == "global_norm"
    rnd.adam_step(lr=opt["lr"], beta1=opt["betas"][0], beta2=opt["betas"][1], eps=opt["eps"], max_grad_norm=opt["max_grad_norm"],
                  grad_norm_out=gn)
    torch.cuda.synchronize()
    assert abs(gn.item() - float(g["step_grad_norm"])) <= 1e-5 * float(g["step_grad_norm"])
    worst = {name: compare_stored(g, meta, "step_" + name, rnd.prediction_net.params[name].cpu().numpy(), 2e-6, absolute=True)
             for name in meta["param_names"]["prediction_net"]}
    for name, e in worst.items():
        assert e <= 2e-6, (name, e)
    assert torch.equal(model.target_net.flat, target_before)


def test_indexed_minibatch_equals_the_gathered_one(gold):
    """train_minibatch(x, index) reads its rows out of the whole batch: same bits as the gathered copy."""
    g, meta = gold
    model = make_model(meta, g)
    rnd = model.rnd
    whole = torch.from_numpy(np.concatenate([g["mb_x"], g["fwd_x"]])).cuda()
    index = torch.tensor([15, 3, 3, 8, 0], dtype=torch.int32, device="cuda")
    rnd.train_minibatch(whole[index.long()].contiguous(), loss_scale=0.5)
    want = rnd.prediction_net.grad.clone()
    rnd.prediction_net.grad.fill_(float("nan"))
    rnd.train_minibatch(whole, index=index, loss_scale=0.5)
    assert torch.equal(rnd.prediction_net.grad, want)


def test_predictor_learns_the_batch_it_is_shown(gold):
    """200 minibatches on 8 fixed observations: their mean error falls below a tenth of its initial value, and 8 fresh
    observations keep a larger error than the trained ones."""
    g, meta = gold
    model = make_model(meta, g)
    rnd = model.rnd
    seen, fresh = torch.from_numpy(g["mb_x"]).cuda(), torch.from_numpy(g["fwd_x"]).cuda()
    first = rnd.prediction_error(seen).mean().item()
    opt = meta["opt"]
    for _ in range(200):
        rnd.train_minibatch(seen)
        rnd.adam_step(lr=opt["lr"], beta1=opt["betas"][0], beta2=opt["betas"][1], eps=opt["eps"], max_grad_norm=opt["max_grad_norm"])
    last, other = rnd.prediction_error(seen).mean().item(), rnd.prediction_error(fresh).mean().item()
    print(f"RND_MODEL functional first={first:.4e} after_200={last:.4e} fresh={other:.4e}")
    assert np.isfinite(last) and last < 0.1 * first
    assert other > last


def test_dual_architecture_builds_and_runs(gold):
    """The RND networks beside two DualHeadNets: drawn after both (so other weights than the fixture's), same plumbing."""
    g, meta = gold
    model = make_model(meta, g, architecture="dual")
    x = torch.from_numpy(g["fwd_x"]).cuda()
    out = model.forward(x, include_rnd=True)
    err = out["rnd_error"].cpu().numpy()
    assert err.shape == (8,) and np.isfinite(err).all() and (err > 0).all()
    assert out["value"].shape == (8, 2) and out["log_policy"].shape == (8, meta["n_actions"])
    keys = list(model.state_dict().keys())
    assert [k.split(".")[0] for k in keys if k.split(".")[0] != "policy_net"][0] == "value_net" and keys[-1] == "target_net.out.bias"
