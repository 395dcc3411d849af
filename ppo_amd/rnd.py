"""Random Network Distillation networks on the HIP kernels - host mirror of the reference's RNDTarget / RNDPredictor
(rl/models.py:216-298) and of TVFModel.rnd_prediction_error (:712-738).

Both networks read the last channel of the normalised observation, (1, H, W): three strided convolutions with
F.leaky_relu(., 0.2) behind each (csrc/conv_strided.hip, the leaky entry points), then `out` (the target) or `fc1`, `fc2`,
`out` with a ReLU between them (the predictor) on ppo_gemm_f32.  The intrinsic reward is the mean squared difference of the
two outputs (csrc/rnd.hip).  Only the predictor trains: it owns a flat parameter buffer, a flat gradient buffer and Adam
moments; the target has parameters and nothing else.
"""
from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from . import _lib

IN_NONE = _lib.PPO_IN_NONE
SLOPE = 0.2      # rl/models.py:250-252, 291-293
FEATURES = 512   # hidden_units default of both classes; the predictor's fc1 / fc2 are 512 wide whatever it is
WEIGHT_SCALE = np.sqrt(2) * 1.3  # rl/models.py:243, 285
LAYERS = (("conv1", 32, 8, 4), ("conv2", 64, 4, 2), ("conv3", 64, 3, 1))  # rl/models.py:228-230
_ALIGN = 4  # floats: every parameter starts on a 16-byte boundary


def _p(t):
    return None if t is None else t.data_ptr()


def rnd_geometry(input_dims):
    """(name, cin, cout, kernel, stride, h, w, ho, wo) of the three convolutions on one channel of input_dims, and the flat
    width behind them."""
    _c, h, w = (int(d) for d in input_dims)
    c, layers = 1, []
    for name, cout, k, s in LAYERS:
        if h < k or w < k:
            raise ValueError(f"input_dims={tuple(input_dims)} is too small for the RND networks ({name}: {k}x{k} on {h}x{w})")
        ho, wo = (h - k) // s + 1, (w - k) // s + 1
        layers.append((name, c, cout, k, s, h, w, ho, wo))
        c, h, w = cout, ho, wo
    return layers, c * h * w


def _scaled(module):
    """scale_weights(weight_scale=sqrt(2) * 1.3, bias_scale=0) on one child (rl/models.py:902-905)."""
    with torch.no_grad():
        module.weight.data *= WEIGHT_SCALE
        module.bias.data *= 0.0
    return module.weight.data, module.bias.data


def init_rnd_parameters(input_dims, hidden_units: int = FEATURES):
    """Initial parameters of (prediction_net, target_net) as CPU tensors under the reference's names, drawn from torch's
    global CPU generator in the reference's construction order - the predictor, then the target (rl/models.py:621-622),
    each: three nn.Conv2d, then its nn.Linear layers, then scale_weights - so that a TVFModel built under the same
    torch.manual_seed holds the reference's initial weights exactly (TVFModel draws policy_net and value_net first)."""
    layers, flat = rnd_geometry(input_dims)
    nets = []
    for dense in ((("fc1", flat, 512), ("fc2", 512, 512), ("out", 512, hidden_units)), (("out", flat, hidden_units),)):
        mods = [(name, torch.nn.Conv2d(cin, cout, kernel_size=(k, k), stride=(s, s))) for name, cin, cout, k, s, *_r in layers]
        mods += [(name, torch.nn.Linear(fin, fout)) for name, fin, fout in dense]
        init = OrderedDict()
        for name, m in mods:
            init[f"{name}.weight"], init[f"{name}.bias"] = _scaled(m)
        nets.append(init)
    return nets[0], nets[1]


class _Params:
    """One net's parameters in a flat device buffer, with views under the reference's names."""

    def __init__(self, init, device, with_grad):
        offs, total = OrderedDict(), 0
        for name, t in init.items():
            offs[name] = (total, tuple(t.shape))
            total += (t.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        flat = torch.zeros(total, dtype=torch.float32)
        for name, t in init.items():
            flat[offs[name][0]:offs[name][0] + t.numel()] = t.reshape(-1)
        self.flat = flat.to(device)
        self.offsets = offs
        self.params = self._views(self.flat)
        self.grad = torch.zeros_like(self.flat) if with_grad else None
        self.grads = self._views(self.grad) if with_grad else None

    def _views(self, flat):
        return OrderedDict((n, flat[o:o + int(np.prod(s))].view(s)) for n, (o, s) in self.offsets.items())

    def state_dict(self):
        return OrderedDict((n, t.clone()) for n, t in self.params.items())

    def load_state_dict(self, sd, strict=True):
        missing = [n for n in self.params if n not in sd]
        if strict and (missing or [n for n in sd if n not in self.params]):
            raise KeyError(f"state_dict mismatch: missing {missing}, unexpected {[n for n in sd if n not in self.params]}")
        for n, t in sd.items():
            if n in self.params:
                self.params[n].copy_(torch.as_tensor(t).to(self.flat.device, torch.float32).reshape(self.params[n].shape))


class RNDNets:
    """prediction_net and target_net of a TVFModel(use_rnd=True).  `obs_norm` is the model's ObsNormalizer: its float32
    constants normalise the channel the networks read."""

    def __init__(self, input_dims, obs_norm, device, hidden_units: int = FEATURES):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.input_dims = tuple(int(d) for d in input_dims)
        self.obs_norm = obs_norm
        self.F = int(hidden_units)
        self.layers, self.flat_width = rnd_geometry(self.input_dims)
        for _name, cin, cout, k, s, h, w, _ho, _wo in self.layers:
            if not self.lib.ppo_conv2d_strided_supported(cin, cout, k, k, s, h, w):
                raise _lib.PpoAmdError(f"no strided-convolution kernel for {cin}->{cout} {k}x{k}/{s} on {h}x{w}")
        pred, target = init_rnd_parameters(self.input_dims, self.F)
        self.prediction_net = _Params(pred, self.device, with_grad=True)
        self.target_net = _Params(target, self.device, with_grad=False)
        self.exp_avg = self.exp_avg_sq = None
        self.adam_steps = 0
        self._bufs = {}
        # what Runner._run_epochs / optimizer_step ask of the net behind an optimiser (DualHeadNet's interface)
        self.grad = self.prediction_net.grad
        self.grad_ready_hook = None
        self._presummed = 0

    # ------------------------------------------------------------------ scratch memory, launches
    def _buf(self, name, shape, dtype=torch.float32):
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.empty(shape, dtype=dtype, device=self.device)
        return t

    def _call(self, fn_name, *args):
        rc = getattr(self.lib, fn_name)(*args, _lib.current_stream())
        if rc != 0:
            _lib.check(rc, fn_name)

    def _linear(self, net, x, k, wname, out, relu_x, tag):
        w = net.params[wname + ".weight"]
        B, n = x.shape[0], w.shape[0]
        ws_bytes = self.lib.ppo_gemm_workspace_bytes(B, n, k)
        ws = self._buf("gemm_ws" + tag, ((ws_bytes + 3) // 4,))
        self._call("ppo_gemm_f32", _p(x), k, 1, relu_x, _p(w), 1, k, 0, _p(net.params[wname + ".bias"]), None, _p(out), n, B,
                   n, k, _p(ws), ws_bytes)

    def _linear_backward(self, x, k, wname, dy, dx, relu_x, mask):
        """dW = dy^T @ f(x), db = colsum(dy), dx = (dy @ W) * [mask > 0] (DualHeadNet._linear_backward)."""
        net = self.prediction_net
        w = net.params[wname + ".weight"]
        B, n = dy.shape[0], w.shape[0]
        self._call("ppo_gemm_f32", _p(dy), 1, n, 0, _p(x), k, 1, relu_x, None, None, _p(net.grads[wname + ".weight"]), k, n, k,
                   B, None, 0)
        self._call("ppo_colsum_f32", _p(dy), B, n, n, _p(net.grads[wname + ".bias"]), 0)
        self._call("ppo_gemm_f32", _p(dy), n, 1, 0, _p(w), k, 1, 0, None, _p(mask), _p(dx), k, B, k, n, None, 0)

    # ------------------------------------------------------------------ forward
    def normalised_channel(self, x, index: Optional[torch.Tensor], B, tag):
        """clamp((prep(x)[row, -1] - mu) / (std + eps), -5, 5) as [B, 1, H, W] (rl/models.py:719-723), row b of the result
        read at x[index[b]] when an index is given.  prep: the normaliser's --observation_scaling for uint8 input."""
        C, H, W = self.input_dims
        if tuple(x.shape[1:]) != self.input_dims or x.dtype not in (torch.uint8, torch.float32) or not x.is_contiguous() \
                or x.device != self.obs_norm.device:
            raise ValueError(f"expected a contiguous uint8/float32 [B, {self.input_dims}] tensor on {self.obs_norm.device}")
        if index is not None and (index.dtype != torch.int32 or index.numel() != B or not index.is_contiguous()):
            raise ValueError("index must be a contiguous int32 tensor with one entry per row")
        n = self.obs_norm
        out = self._buf(tag + "xn", (B, 1, H, W))
        self._call("ppo_obs_normalize_channel_f32", _p(x), n.u8_prep if x.dtype == torch.uint8 else 0, _p(index), _p(n.mu), _p(n.std),
                   n.norm_eps, _p(out), B, C, H, W, C - 1)
        return out

    def _features(self, net, xn, tag, predictor):
        """RNDTarget.forward / RNDPredictor.forward (rl/models.py:245-255, 287-298); returns the saved tensors."""
        B = xn.shape[0]
        acts, cur = {"x": xn}, xn
        for name, cin, cout, k, s, h, w, ho, wo in self.layers:
            y = self._buf(f"{tag}{name}", (B, cout, ho, wo))
            self._call("ppo_conv2d_strided_forward_leaky_f32", _p(cur), IN_NONE, _p(net.params[f"{name}.weight"]),
                       _p(net.params[f"{name}.bias"]), _p(y), SLOPE, B, cin, h, w, cout, k, k, s)
            acts[name] = cur = y
        flat = cur.view(B, self.flat_width)
        out = self._buf(tag + "out", (B, self.F))
        if predictor:
            h1, h2 = self._buf(tag + "h1", (B, 512)), self._buf(tag + "h2", (B, 512))
            self._linear(net, flat, self.flat_width, "fc1", h1, 0, tag)
            self._linear(net, h1, 512, "fc2", h2, 1, tag)  # the ReLU behind fc1 / fc2 is applied on the next layer's load
            self._linear(net, h2, 512, "out", out, 1, tag)
            acts["h1"], acts["h2"] = h1, h2
        else:
            self._linear(net, flat, self.flat_width, "out", out, 0, tag)
        acts["flat"], acts["out"] = flat, out
        return acts

    def prediction_error(self, x, index=None, rows=None, err=None, err_stride=1, tag="i", already_normed=False):
        """errors[b] = mean_j (target(x_b) - predictor(x_b))^2 (rl/models.py:736) of `rows` observations (default: all of
        x; with an index: x[index[b]]), written to err[b * err_stride] (default: a fresh [rows] tensor).  No host read.
        `already_normed`: x is the float32 output of the normaliser (rl/models.py:716-718); its last channel is read."""
        B = int(rows if rows is not None else (index.numel() if index is not None else x.shape[0]))
        if already_normed:
            if index is not None or x.dtype != torch.float32 or tuple(x.shape[1:]) != self.input_dims:
                raise ValueError(f"an already normalised input is a float32 [B, {self.input_dims}] tensor, read without index")
            xn = self._buf(tag + "xn", (B, 1, *self.input_dims[1:]))
            xn.copy_(x[:B, -1:])
        else:
            xn = self.normalised_channel(x, index, B, tag)
        t = self._features(self.target_net, xn, tag + "t_", False)
        p = self._features(self.prediction_net, xn, tag + "p_", True)
        if err is None:
            err, err_stride = torch.empty(B, dtype=torch.float32, device=self.device), 1
        self._call("ppo_rnd_error_f32", _p(p["out"]), _p(t["out"]), B, self.F, _p(err), err_stride, None, 0.0, None)
        return err

    # ------------------------------------------------------------------ training
    def train_minibatch(self, x, index=None, loss_scale: float = 1.0, stats: Optional[torch.Tensor] = None):
        """Runner.train_rnd_minibatch (rl/rollout.py:1804-1821): the gradient of loss_scale * mean_b error(x_b) w.r.t. every
        predictor parameter, written to prediction_net.grads (overwritten, as every backward here).  `stats` (device float
        [PPO_RND_STATS]) takes the sums behind loss_rnd / feat_mean / feat_var / feat_max.  Returns the per-row errors."""
        B = int(index.numel() if index is not None else x.shape[0])
        xn = self.normalised_channel(x, index, B, "t")
        t = self._features(self.target_net, xn, "tt_", False)
        p = self._features(self.prediction_net, xn, "tp_", True)
        err, dout = self._buf("terr", (B,)), self._buf("tdout", (B, self.F))
        self._call("ppo_rnd_error_f32", _p(p["out"]), _p(t["out"]), B, self.F, _p(err), 1, _p(dout), float(loss_scale) / B,
                   _p(stats))
        dh2, dh1 = self._buf("tdh2", (B, 512)), self._buf("tdh1", (B, 512))
        g = self._buf("tg_conv3", tuple(p["conv3"].shape))
        self._linear_backward(p["h2"], 512, "out", dout, dh2, 1, p["h2"])
        self._linear_backward(p["h1"], 512, "fc2", dh2, dh1, 1, p["h1"])
        self._linear_backward(p["flat"], self.flat_width, "fc1", dh1, g.view(B, self.flat_width), 0, None)
        net = self.prediction_net
        for li in (2, 1, 0):  # g: the gradient w.r.t. layer li's leaky output, gated by that output itself
            name, cin, cout, k, s, h, w, _ho, _wo = self.layers[li]
            src = p[self.layers[li - 1][0]] if li else xn
            geom = (B, cin, h, w, cout, k, k, s)
            nbytes = int(self.lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
            ws = self._buf("twgrad_ws_" + name, ((nbytes + 3) // 4,))
            self._call("ppo_conv2d_strided_backward_weight_leaky_f32", _p(src), IN_NONE, _p(g), _p(p[name]),
                       _p(net.grads[f"{name}.weight"]), _p(net.grads[f"{name}.bias"]), _p(ws), nbytes, SLOPE, *geom)
            if li:
                gx = self._buf("tg_" + self.layers[li - 1][0], tuple(src.shape))
                self._call("ppo_conv2d_strided_backward_data_leaky_f32", _p(g), _p(p[name]), _p(net.params[f"{name}.weight"]),
                           _p(gx), SLOPE, *geom)
                g = gx
        return err

    def takes_obs_index(self, obs) -> bool:
        """The channel-normalise launch reads its rows through the minibatch index: no observation row is copied."""
        return True

    def adam_step(self, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=20.0, grad_div=1.0,
                  grad_norm_out: Optional[torch.Tensor] = None, state=None):
        """Runner.optimizer_step(rnd_optimizer) (rl/rollout.py:1287-1321): clip_grad_norm_ + torch.optim.Adam.step over the
        predictor's flat buffer.  `grad_div`: the data-parallel world size - the gradient arrives summed over ranks and the
        kernel divides it before the clip, as for the other nets."""
        if state is not None:
            raise NotImplementedError("the RND predictor has one set of Adam moments")
        self._presummed = 0
        net = self.prediction_net
        if self.exp_avg is None:
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(net.flat), torch.zeros_like(net.flat)
        self.adam_steps += 1
        nbytes = int(self.lib.ppo_adam_workspace_bytes())
        ws = self._buf("adam_ws", ((nbytes + 3) // 4,))
        self._call("ppo_adam_step_f32", _p(net.flat), _p(net.grad), _p(self.exp_avg), _p(self.exp_avg_sq), net.flat.numel(),
                   self.adam_steps, float(lr), float(beta1), float(beta2), float(eps), float(max_grad_norm), float(grad_div), _p(ws),
                   _p(grad_norm_out))

    def sgd_step(self, lr=2.5e-4, max_grad_norm=20.0, grad_div=1.0, grad_norm_out: Optional[torch.Tensor] = None):
        """Runner.optimizer_step(rnd_optimizer) under --rnd_opt_optimizer=sgd (rl/rollout.py:137-138, :1287-1321):
        clip_grad_norm_ + torch.optim.SGD.step over the predictor's flat buffer; no moments, no step count."""
        self._presummed = 0
        net = self.prediction_net
        nbytes = int(self.lib.ppo_adam_workspace_bytes())
        ws = self._buf("adam_ws", ((nbytes + 3) // 4,))
        self._call("ppo_sgd_step_f32", _p(net.flat), _p(net.grad), net.flat.numel(), float(lr), float(max_grad_norm),
                   float(grad_div), _p(ws), _p(grad_norm_out))

    def parameter_count(self):
        return len(self.prediction_net.offsets)

    # ------------------------------------------------------------------ optimiser state (checkpoints)
    def optimizer_state_dict(self, cfg=None):
        """`torch.optim.Adam(prediction_net.parameters()).state_dict()` layout, as DualHeadNet.adam_state_dict writes it
        for the other optimisers (rl/rollout.py:416-417).  Every predictor parameter has a gradient from the first step
        on, so every one has an entry once the optimiser has stepped."""
        net, state = self.prediction_net, {}
        if self.exp_avg is not None and self.adam_steps > 0:
            for i, (name, (o, shape)) in enumerate(net.offsets.items()):
                n = int(np.prod(shape))
                state[i] = {"step": torch.tensor(float(self.adam_steps), dtype=torch.float32),
                            "exp_avg": self.exp_avg[o:o + n].view(shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + n].view(shape).clone()}
        group = {"lr": float(cfg.lr) if cfg is not None else 0.0,
                 "betas": (float(cfg.adam_beta1), float(cfg.adam_beta2)) if cfg is not None else (0.9, 0.999),
                 "eps": float(cfg.adam_epsilon) if cfg is not None else 1e-8, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "params": list(range(len(net.offsets)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        net, state = self.prediction_net, sd.get("state") or {}
        if not state:
            self.exp_avg = self.exp_avg_sq = None
            self.adam_steps = 0
            return
        names = list(net.offsets)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(net.flat), torch.zeros_like(net.flat)
        for key, st in state.items():
            o, shape = net.offsets[names[int(key)]]
            n = int(np.prod(shape))
            self.exp_avg[o:o + n].copy_(torch.as_tensor(st["exp_avg"]).reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(torch.as_tensor(st["exp_avg_sq"]).reshape(-1))
            self.adam_steps = max(self.adam_steps, int(float(st["step"])))
