"""Simple noise scale — host mirror of the reference's rl/sns.py (McCandlish et al. 2018, arXiv:1812.06162): the
critical batch size of an update phase from two gradient norms, |G_small|^2 (the mean over b_big / b_small backward
passes of b_small rows) and |G_big|^2 (of their mean).

What changed relative to the reference, and why:
  * the reference reads a norm back per parameter tensor per pass (`utils.calc_norm`, rl/utils.py:146-161) and adds the
    gradients tensor by tensor (rl/sns.py:149-178).  Here every backward pass overwrites the flat `net.grad`, so one
    launch per pass (ppo_grad_noise_pass_f32) adds it into a second flat buffer and leaves the pass's sum of squares on
    the device; ppo_grad_noise_finish_f64 delivers all of them in ONE device->host copy per estimate;
  * `get_ema_constant` takes the runner: the reference calls it without one (rl/sns.py:60, 62) and `--sns_smoothing_mode=ema`,
    its default, raises AttributeError there.  The evident intent is built;
  * `--sns_labels` may be the default list or a string (the reference applies ast.literal_eval to its default list and
    raises ValueError); the smoothing horizons parse as float;
  * the estimate's passes do not draw torch.bernoulli for `--tvf_horizon_dropout`: the dropout counter advances instead.
The float64 host arithmetic, the `noise_stats` keys, the log keys and the np.random draws are the reference's.
"""
import math
import time as clock
from collections import deque

import numpy as np
import torch

from . import _lib
from .config import args
from .value_quality import even_sample_down


def get_ema_constant(runner, required_horizon, updates_every: int = 1):
    """EMA coefficient that matches a horizon given in environment interactions when updates are applied every
    `updates_every` rollouts (rl/sns.py:18-27)."""
    if required_horizon == 0:
        return 0
    updates_every_steps = (updates_every * runner.N * runner.A)
    ema_horizon = required_horizon / updates_every_steps
    return 1 - (1 / ema_horizon)


def history_length(runner) -> int:
    """Length of the `avg` mode's history (rl/sns.py:53-55)."""
    history_frames = int(args.sns.smoothing_horizon_avg)
    ideal_updates_length = history_frames / (runner.N * runner.A)
    return int(max(10, math.ceil(ideal_updates_length / args.sns.period)))


def _dictionary_ema(d: dict, key: str, target, alpha: float):
    """rl/utils.py:135-143 (linear form): the first value is taken as it is."""
    value_1 = d.get(key, target)
    d[key] = alpha * value_1 + (1 - alpha) * target
    return d[key]


def process_noise_scale(runner, g_b_small_squared: float, g_b_big_squared: float, label: str, verbose: bool = True,
                        b_small: int = None, b_big: int = None):
    """Logs noise levels from the two squared gradient norms (rl/sns.py:29-106), float64 expression for expression."""
    b_small = b_small or args.sns.b_small
    b_big = b_big or args.sns.b_big

    est_s = (g_b_small_squared - g_b_big_squared) / (1 / b_small - 1 / b_big)
    est_g2 = (b_big * g_b_big_squared - b_small * g_b_small_squared) / (b_big - b_small)

    stats = runner.noise_stats
    if args.sns.smoothing_mode == "avg":
        for var_name, var_value in zip(["s", "g2"], [est_s, est_g2]):
            if f"{label}_{var_name}_history" not in stats:
                stats[f"{label}_{var_name}_history"] = deque(maxlen=history_length(runner))
            stats[f"{label}_{var_name}_history"].append(var_value)
            stats[f"{label}_{var_name}"] = np.mean(stats[f"{label}_{var_name}_history"])
    elif args.sns.smoothing_mode == "ema":
        ema_s = get_ema_constant(runner, args.sns.smoothing_horizon_s, args.sns.period)
        g2_horizon = args.sns.smoothing_horizon_policy if label == "policy" else args.sns.smoothing_horizon_g2
        ema_g2 = get_ema_constant(runner, g2_horizon, args.sns.period)
        _dictionary_ema(stats, f"{label}_s", est_s, ema_s)
        _dictionary_ema(stats, f"{label}_g2", est_g2, ema_g2)
    else:
        raise ValueError(f"Invalid smoothing mode {args.sns.smoothing_mode}.")

    smooth_s = float(stats[f"{label}_s"])
    smooth_g2 = float(stats[f"{label}_g2"])

    # the g2 estimate is frequently negative: the *smoothed* g2 is clipped to epsilon so the ratio keeps its sign
    epsilon = 1e-4
    ratio = smooth_s / (max(0.0, smooth_g2) + epsilon)

    stats[f"{label}_ratio"] = ratio
    if "head" in label:
        # keep track of which heads we have results for
        try:
            idx = int(label.split("_")[-1])
            if "active_heads" not in stats:
                stats["active_heads"] = set()
            stats["active_heads"].add(idx)
        except ValueError:
            pass

    log = runner.log
    log.watch(f"sns_{label}_smooth_s", smooth_s, display_precision=0, display_width=0, display_name=f"sns_{label}_s")
    log.watch(f"sns_{label}_smooth_g2", smooth_g2, display_precision=0, display_width=0, display_name=f"sns_{label}_g2")
    log.watch(f"sns_{label}_s", est_s, display_precision=0, display_width=0)
    log.watch(f"sns_{label}_g2", est_g2, display_precision=0, display_width=0)
    log.watch(f"sns_{label}_b", ratio, display_precision=0, display_width=0)
    log.watch(f"sns_{label}", np.clip(ratio, 0, float("inf")) ** 0.5, display_precision=0,
              display_width=8 if verbose else 0)
    return stats[f"{label}_ratio"]


def wants_noise_estimate(runner, label: str) -> bool:
    """Whether `label` wants a noise update on this step (rl/sns.py:284-296)."""
    if not args.sns.enabled:
        return False
    if runner.batch_counter % args.sns.period != args.sns.period - 1:
        return False  # only evaluate every so often
    return label.lower() in args.sns.label_list()


# ---------------------------------------------------------------------- the device half
def _scratch(net, n: int, passes: int, lib):
    """(acc [n] float32, workspace, out [passes + 1] float64) on net.grad's device; kept in the net's scratch memory
    where it has one.  Nothing here exists before the first estimate."""
    ws_doubles = int(lib.ppo_grad_noise_workspace_bytes(passes)) // 8
    if hasattr(net, "_buf"):
        return (net._buf("grad_noise_acc", (n,)), net._buf("grad_noise_ws", (ws_doubles,), torch.float64),
                net._buf("grad_noise_out", (passes + 1,), torch.float64))
    dev = net.grad.device
    return (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(ws_doubles, dtype=torch.float64, device=dev),
            torch.empty(passes + 1, dtype=torch.float64, device=dev))


def gradient_norms(net, sample: np.ndarray, step, b_small: int):
    """(|G_small|^2, |G_big|^2) over the rows `sample` (rl/sns.py:149-178): pass i runs `step(index)` - a backward pass
    that leaves its gradient in the flat float32 device buffer `net.grad` - on sample[i * b_small:(i + 1) * b_small]
    (an int32 device vector; the sample is uploaded once), then one launch adds the gradient into the running sum and
    takes its sum of squares.  No host sync until the one copy at the end.  Afterwards net.grad is zero; the
    data-parallel early-bucket hook is parked meanwhile and comes back on every exit path."""
    lib = _lib.load()
    grad = net.grad
    if grad.dtype != torch.float32 or not grad.is_contiguous() or grad.dim() != 1:
        raise ValueError("net.grad must be a flat contiguous float32 device tensor")
    assert len(sample) % b_small == 0, "b_small must divide b_big"
    m = len(sample) // b_small
    n = grad.numel()
    acc, ws, out = _scratch(net, n, m, lib)
    sample_dev = torch.from_numpy(np.ascontiguousarray(sample, dtype=np.int32)).to(grad.device, non_blocking=True)
    hook = getattr(net, "grad_ready_hook", None)
    if hook is not None:
        net.grad_ready_hook = None  # only an optimiser step's gradient may leave
    try:
        for i in range(m):
            step(sample_dev[i * b_small:(i + 1) * b_small])
            rc = lib.ppo_grad_noise_pass_f32(grad.data_ptr(), acc.data_ptr(), n, i, m, ws.data_ptr(), _lib.current_stream())
            if rc != 0:
                _lib.check(rc, "ppo_grad_noise_pass_f32")
        rc = lib.ppo_grad_noise_finish_f64(acc.data_ptr(), n, m, m, ws.data_ptr(), out.data_ptr(), _lib.current_stream())
        if rc != 0:
            _lib.check(rc, "ppo_grad_noise_finish_f64")
        sums = out.cpu().numpy()  # the one device->host copy of an estimate
    finally:
        if hook is not None:
            net.grad_ready_hook = hook
        grad.zero_()  # optimizer.zero_grad (rl/sns.py:176)
        if hasattr(net, "_presummed"):
            net._presummed = 0  # the last pass's sums of g^2 belong to no optimiser step
    return float(np.mean(sums[:m])), float(sums[m] / (m * m))


def estimate_noise_scale(runner, rows: int, step, net, label: str, verbose: bool = True):
    """Estimates the critical batch size of one phase from a small and a large batch (rl/sns.py:109-179).  `rows`: size
    of the phase's batch; `step(index)`: the phase's own minibatch step with loss_scale 1 on the rows `index`; `net`:
    anything with a flat float32 device `.grad` that `step` fills.  The per-sample statistics of the passes are
    dropped, as the reference mutes its logger."""
    b_small = args.sns.b_small
    # always the full batch for policy (it is required to get the precision needed)
    b_big = runner.N * runner.A if label == "policy" else args.sns.b_big
    if b_big > rows:
        raise ValueError(f"Can not take {b_big} samples from a batch of {rows}")
    sample = np.random.choice(rows, b_big, replace=False)  # resamples and shuffles (same draws as choice(range(rows)))
    assert b_big % b_small == 0, "b_small must divide b_big"
    g_small, g_big = gradient_norms(net, sample, step, b_small)
    return process_noise_scale(runner, g_small, g_big, label, verbose, b_big=b_big)


def log_accumulated_gradient_norms(runner, make_step, net):
    """Per-horizon estimates of the value net (rl/sns.py:299-328, 182-226): for each of up to --sns_max_heads heads a
    fresh sample, passes of the TVF loss alone on heads 0..head (`make_step(head)` -> step(index)), label
    acc_head_<head>, quiet display."""
    required_heads = even_sample_down(range(len(runner.tvf_horizons)), args.sns.max_heads)
    start_time = clock.time()
    n_rows = runner.N * runner.A
    for head_id in required_heads:
        if args.sns.b_big > n_rows:
            raise ValueError(f"Can not take {args.sns.b_big} samples from rollout of size {runner.N}x{runner.A}")
        # a different sample for each head; sampled even when all rows are needed, to shuffle the order
        sample = np.random.choice(n_rows, args.sns.b_big, replace=False)
        g_small, g_big = gradient_norms(net, sample, make_step(head_id), args.sns.b_small)
        process_noise_scale(runner, g_small, g_big, label=f"acc_head_{head_id}", verbose=False)
    s = clock.time() - start_time
    runner.log.watch_mean("t_s_heads", s / args.sns.period)


def log_fake_accumulated_gradient_norms(runner, d: int):
    """--sns_fake_noise (rl/sns.py:229-282): estimates of synthetic gradients of `d` parameters whose noise grows with
    the head's horizon - a unit signal on the first dimension plus np.random.randn noise.  Host NumPy throughout, the
    reference's draws and its float32 / float64 arithmetic."""
    required_heads = even_sample_down(range(len(runner.tvf_horizons)), args.sns.max_heads)
    b_small, b_big = args.sns.b_small, args.sns.b_big
    # a NumPy integer as in the reference (a sum of np.prod): renorm_factor is then a NumPy float64 scalar, and under
    # NumPy 2 promotion `grad *= renorm_factor` multiplies in float64 before rounding to float32
    d = np.int64(d)
    mini_batches = b_big // b_small
    for required_head in required_heads:
        small_norms_sqr = []
        big_grad = 0
        for i in range(mini_batches):
            # no fake noise on the final horizon... half the noise as decreasing signal, half as increasing noise
            target_noise_level = runner.tvf_horizons[abs(required_head)] / 10
            if target_noise_level > 0:
                noise_level = math.sqrt(target_noise_level)
                signal_level = 1 / math.sqrt(target_noise_level)
            else:
                noise_level = target_noise_level
                signal_level = 1
            grad = np.random.randn(d).astype(np.float32)
            norm2 = d ** 0.5
            renorm_factor = noise_level / norm2 / math.sqrt(b_small)
            grad *= renorm_factor
            grad[0] += signal_level  # the true signal is a unit vector on the first dimension
            small_norms_sqr.append(np.linalg.norm(grad, ord=2) ** 2)
            if i == 0:
                big_grad = grad.copy()
            else:
                big_grad += grad
        g_small_sqr = float(np.mean(small_norms_sqr))
        g_big_sqr = (np.linalg.norm(big_grad, ord=2) / mini_batches) ** 2
        process_noise_scale(runner, g_small_sqr, g_big_sqr, label=f"fake_head_{required_head}", verbose=False)


# ---------------------------------------------------------------------- checkpoints
def noise_stats_to_plain(stats: dict) -> dict:
    """`noise_stats` as plain data: floats, the `avg` histories as lists, active_heads as a sorted list."""
    out = {}
    for k, v in stats.items():
        if isinstance(v, deque):
            out[k] = [float(x) for x in v]
        elif isinstance(v, (set, frozenset)):
            out[k] = sorted(int(x) for x in v)
        else:
            out[k] = float(v)
    return out


def noise_stats_from_plain(plain: dict, runner) -> dict:
    """The inverse: histories become deques again, their maxlen recomputed from the run's flags."""
    out = {}
    for k, v in (plain or {}).items():
        if k == "active_heads":
            out[k] = set(int(x) for x in v)
        elif k.endswith("_history"):
            out[k] = deque((float(x) for x in v), maxlen=history_length(runner))
        else:
            out[k] = float(v)
    return out
