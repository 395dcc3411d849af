"""GPU: Runner.train_distil_minibatch under the distillation switches beyond the default against the reference's own
results (tests/golden/distil_golden.npz, recorded by make_distil_golden.py from the reference's
Runner.train_distil_minibatch on CPU, rl/rollout.py:1331-1449): loss, loss_std and every policy_net gradient of one
minibatch of 32, on the fused MLP launches.

Bars: those tests/test_variants_gpu.py applies to the distil phase of the default switches - the loss to 2e-6 (of
max(1, |loss|)), gradients to 2e-5 of the tensor's largest entry, parameters the reference leaves without a gradient exact
zeros; loss_std to that file's bar for a loss's standard deviation, 1e-5."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import logger, models, rollout  # noqa: E402
from ppo_amd.config import args  # noqa: E402

HERE = os.path.dirname(__file__)
GOLD = np.load(os.path.join(HERE, "golden", "distil_golden.npz"))
META = json.load(open(os.path.join(HERE, "golden", "distil_golden.json")))
COMBOS = ["logit_l1", "policy_clipped", "kl_huber", "huber0", "advantage", "return", "tvf_heads3"]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_runner(tag):
    m = META[tag]
    MB = META["minibatch"]
    args.setup(["--model_encoder=mlp", "--env_type=synthetic", "--seed=7", "--disable_logging=True", "--device=cuda",
                "--model_architecture=dual", f"--agents={MB}", "--n_steps=4", f"--distil_opt_mini_batch_size={MB}",
                f"--distil_beta={m['distil_beta']}", *m["flags"]])
    assert args._ignored == []
    assert (args.distil.loss, args.distil.value_loss, args.distil.target) == (m["distil_loss"], m["distil_value_loss"],
                                                                               m["distil_target"])
    assert (args.distil.delta, args.distil.l1_scale, args.distil.max_heads) == (m["distil_delta"], m["distil_l1_scale"],
                                                                                 m["distil_max_heads"])
    tvf = f"{tag}_tvf_horizons" in GOLD
    torch.manual_seed(7)
    model = models.TVFModel(
        "mlp", input_dims=tuple(META["input_dims"]), actions=META["n_actions"], device="cuda", architecture="dual",
        hidden_units=META["hidden"], encoder_activation_fn="relu", head_scale=m["head_scale"], head_bias=m["head_bias"],
        tvf_fixed_head_horizons=list(GOLD[f"{tag}_tvf_horizons"]) if tvf else None,
        tvf_fixed_head_weights=list(GOLD[f"{tag}_tvf_weights"]) if tvf else None, value_head_names=("ext",))
    pol = model.policy_net
    assert pol.mlp_fused
    # the net the recorded gradients belong to (the orthogonal initialiser's last bits depend on the host)
    pol.load_state_dict({name: torch.from_numpy(GOLD[f"init_{m['init']}_{name}"]) for name in pol.state_dict()})
    return rollout.Runner(model, logger.Logger(quiet=True)), m


@pytest.mark.parametrize("tag", COMBOS)
def test_minibatch_equals_the_reference_s(tag):
    r, m = make_runner(tag)
    pol = r.policy_net
    data = {k: cuda(GOLD[f"{tag}_{k}"]) for k in ("prev_state", "distil_targets", "old_raw_policy", "old_log_policy",
                                                  "distil_actions")}
    pol.grad.zero_()
    res = r.train_distil_minibatch(data, loss_scale=1.0)
    torch.cuda.synchronize()
    want = GOLD[f"{tag}_result"]
    print(f"{tag}: loss {res['loss']:.9g} (reference {want[0]:.9g}), loss_std {res['loss_std']:.9g} ({want[1]:.9g})")
    assert abs(res["loss"] - want[0]) < 2e-6 * max(1, abs(want[0]))
    assert abs(res["loss_std"] - want[1]) < 1e-5 * max(1, abs(want[1]))
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
    assert seen >= 6
    if tag == "tvf_heads3":  # heads outside even_sample_down(range(8), 3) = [0, 3, 7]: no gradient
        g = pol.grads["tvf_head.weight"].cpu().numpy()
        assert float(np.abs(g[[1, 2, 4, 5, 6]]).max()) == 0.0
        assert all(float(np.abs(g[k]).max()) > 0 for k in (0, 3, 7))
