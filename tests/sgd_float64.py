"""float64 reference, float32 comparison evaluation and its wrong variants for the SGD step (csrc/optim.hip:
ppo_sgd_step_f32, ppo_sgd_step_presummed_f32): clip_grad_norm_ followed by torch.optim.SGD.step without momentum, weight
decay or dampening (rl/rollout.py:137-138, :1287-1321).  The data regimes, the max_norm kinds, the bars (MULTIPLE = 4
over plain float32 torch on the CPU against float64, never below 2^-23 of the local scale) and the guarded buffers are
those of tests/policy_optim_float64.py; w's local scale is Adam's: ulp(w) + |dw| per element, the norm's is itself.
tests/test_sgd_float64_gpu.py compares the kernels with these; tests/test_sgd_float64_cpu.py checks, without a GPU, that
the bars reject the wrong variants."""
import math

import numpy as np
import torch

import policy_optim_float64 as R

SGD_LR = 2.5e-4
SGD_VARIANTS = ("no_grad_div", "norm_undivided", "clip_no_1e-6", "plus", "lr_in_norm")


def sgd_ref(w, gs, max_norm, grad_div, lr=SGD_LR, sumsq=None):
    """float64, free-running over len(gs) steps from the float32 w: norm = sqrt(sum g^2) / grad_div, clip = min(1,
    max_norm / (norm + 1e-6)) when max_norm > 0 else 1, w <- w - lr g (clip / grad_div).  lr enters at the float32 value
    the kernel receives; max_norm and grad_div are float32 already.  sumsq: the sum of squares to take for the norm (the
    presummed entry point).  -> one dict per step: w, norm, dw, w_scale."""
    lr_ = float(np.float32(lr))
    w = np.asarray(w, np.float64).copy()
    max_norm, grad_div = float(max_norm), float(grad_div)
    out = []
    for g in gs:
        g = np.asarray(g, np.float64)
        tot = float(sumsq) if sumsq is not None else math.fsum((g * g).tolist())
        norm = math.sqrt(tot) / grad_div
        clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
        dw = -lr_ * (g * (clip / grad_div))
        w = w + dw
        out.append({"w": w.copy(), "norm": norm, "dw": dw,
                    "w_scale": np.spacing(np.abs(w).astype(np.float32)).astype(np.float64) + np.abs(dw)})
    return out


def sgd_f32(w, gs, max_norm, grad_div, lr=SGD_LR, variant=None):
    """Plain float32 torch on the CPU, the operations of clip_grad_norm_ and torch.optim.SGD.step on a gradient that was
    divided by grad_div first.  Wrong variants: 'no_grad_div' (the gradient is never divided), 'norm_undivided' (the clip
    is formed from sqrt(sum g^2) without / grad_div; the update and the reported norm are right otherwise),
    'clip_no_1e-6' (max_norm / norm), 'plus' (w + lr g), 'lr_in_norm' (the reported norm is multiplied by lr)."""
    assert variant is None or variant in SGD_VARIANTS, variant
    w = torch.from_numpy(np.array(w, np.float32))
    lr32 = float(np.float32(lr))  # a Python scalar enters a float32 torch operation at its float32 value
    out = []
    for g in gs:
        raw = torch.from_numpy(np.asarray(g, np.float32))
        g = raw if variant == "no_grad_div" else raw / np.float32(grad_div)
        norm = torch.linalg.vector_norm(g)
        clip_norm = torch.linalg.vector_norm(raw) if variant == "norm_undivided" else norm
        if max_norm > 0:
            coef = np.float32(max_norm) / (clip_norm + (0.0 if variant == "clip_no_1e-6" else np.float32(1e-6)))
            g = g * torch.clamp(coef, max=1.0)
        w = w + lr32 * g if variant == "plus" else w - lr32 * g
        reported = float(norm * lr32) if variant == "lr_in_norm" else float(norm)
        out.append({"w": w.numpy().copy(), "norm": reported})
    return out


def sgd_errs(got, ref):
    """got / ref: per-step dicts -> max over the steps of the relative errors of w and the norm."""
    e = {"w": 0.0, "norm": 0.0}
    for a, r in zip(got, ref):
        e["w"] = max(e["w"], R.rel_err(a["w"], r["w"], r["w_scale"]))
        if a.get("norm") is not None:
            e["norm"] = max(e["norm"], R.rel_err(a["norm"], r["norm"], r["norm"] if r["norm"] > 0 else 1.0))
    return e


def sgd_inputs(n, regime, w_zero, seed=0, n_steps=3):
    """float32 numpy w and n_steps gradients: the Adam data set's, without its moments."""
    w, _m, _v, gs = R.adam_inputs(n, regime, w_zero, seed=seed, n_steps=n_steps)
    return w, gs
