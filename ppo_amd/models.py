"""Policy/value networks on hand-written HIP kernels — host mirror of the reference's
rl/models.py (TVFModel :511-856, DualHeadNet :304-508, ImpalaCNN :54-99, StandardMLP :148-169) and
rl/impala.py.

The network's arithmetic runs entirely in libppo_amd.so (f32-MFMA convolutions and GEMMs,
fused load transforms, fused losses, fused Adam); this module owns the memory plan and the
call order.  Parameters of one net live in ONE flat float32 device buffer (so the optimiser step
and the RCCL gradient all-reduce are single launches) and are exposed under the reference's
``state_dict`` names, so reference checkpoints load unchanged.

torch is used for device memory, views and (on the CPU, at construction only) the reference's
parameter initialisers; no torch operator is on the forward/backward path.
"""
import contextlib
import ctypes
import functools
import math
import os
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .rnd import RNDNets, init_rnd_parameters  # noqa: F401  (init_rnd_parameters: the RND half of init_parameters)

IN_NONE, IN_RELU, IN_U8 = _lib.PPO_IN_NONE, _lib.PPO_IN_RELU, _lib.PPO_IN_U8
# --observation_scaling (rl/models.py:846-855): how a uint8 observation becomes the network's input.  Per value, the
# in_mode of the convolution launches that read the bytes and the `is_u8` code of the ppo_obs_* launches.  Float32
# observations are used as they are whatever the value, as in the reference.
OBSERVATION_SCALINGS = {"scaled": (_lib.PPO_IN_U8, _lib.PPO_OBS_U8), "centered": (_lib.PPO_IN_U8_CENTERED, _lib.PPO_OBS_U8_CENTERED),
                        "unit": (_lib.PPO_IN_U8_UNIT, _lib.PPO_OBS_U8_UNIT)}
U8_MODES = frozenset(m for m, _ in OBSERVATION_SCALINGS.values())


def check_observation_scaling(observation_scaling):
    """The reference's refusal (rl/models.py:855)."""
    if observation_scaling not in OBSERVATION_SCALINGS:
        raise ValueError(f"Invalid observation_scaling mode {observation_scaling}")
    return observation_scaling
_ALIGN = 4  # floats: every parameter starts on a 16-byte boundary
# bit i set: stack i runs its first convolution fused with the max-pool (bit-identical either way; the choice is
# a measured one)
FUSE_POOL_STACKS = int(os.environ.get("PPO_AMD_FUSE_POOL", "7"))
# (Every convolution's weight gradient is formed as slabs in a workspace of its own, and one launch at the end of the
# backward pass reduces the slabs of all layers.)  The four block convolutions of a stack share a geometry: their weight
# gradients go out as ONE launch (4 x the workgroups, one ramp and one tail) once the stack's backward-data pass is through.
WGRAD_BATCH_LAUNCH = int(os.environ.get("PPO_AMD_WGRAD_BATCH_LAUNCH", "1"))
# The first stack's max-pool backward is folded into its first convolution's weight-gradient kernel (the only reader of
# that 84x84 gradient map: nothing back-propagates into the observations).  Measured: the max-pool backward launch
# (37 us) goes, the weight-gradient kernel grows by ~20 us (it gathers (argmax, g) pairs instead of streaming the map in
# by LDS-DMA): -15 us per step net and a 115 MB tensor less.
WGRAD_POOLED_DY = int(os.environ.get("PPO_AMD_WGRAD_POOLED_DY", "1"))
# a stack's first convolution whose geometry equals the PREVIOUS stack's block convolutions (32 -> 32 at 21x21 for the 84x84
# net) has its weight gradient formed by that stack's batched launch, as a fifth problem read without the ReLU
# (ppo_conv3x3_backward_weight_slabs_batch_mixed_f32): one launch less per backward pass (11 - 14 us of fixed cost)
WGRAD_RIDE = int(os.environ.get("PPO_AMD_WGRAD_RIDE", "1"))
# --precision=medium|low only: weight gradients of the 16- and 32-channel float layers as split-bf16 products too
# (csrc/wgrad_bf16x3.hip; 0 keeps them on the exact float32 kernel while the residual blocks stay split).
SPLIT_WGRAD = int(os.environ.get("PPO_AMD_SPLIT_WGRAD", "1"))
# likewise the stack-first convolutions (forward: split convolution, with the max-pool inside the launch where that
# geometry has a kernel and as a launch of its own elsewhere, instead of the fused float32 conv + pool kernel;
# backward-data): csrc/conv_bf16x3.hip
SPLIT_CONV = int(os.environ.get("PPO_AMD_SPLIT_CONV", "1"))
# convolutions read their MFMA A operand from a pre-packed copy of the weights, refreshed by one launch after every
# optimiser step (0 = every kernel stages the raw tensor through LDS itself); bit-identical either way
PACKED_WEIGHTS = int(os.environ.get("PPO_AMD_PACKED_WEIGHTS", "1"))
# the optimiser step writes the updated convolution weights into their packed layouts too (no re-pack launch per step).
# Measured and NOT kept (0): 1.118 ms per training step against 1.094 with the separate 5 us pack launch - 2 x 98 k
# scattered 4-byte writes from the first hundred workgroups of the Adam launch cost more than the coalesced re-pack
ADAM_SCATTER = int(os.environ.get("PPO_AMD_ADAM_SCATTER", "0"))
# The two residual blocks of a stack as one launch with the image resident in LDS (csrc/stack_fused.hip), where the
# geometry has a kernel (32 channels at 11x11) and the packed weights exist; 0 = four convolution launches.
FUSE_STACK_TAIL = int(os.environ.get("PPO_AMD_FUSE_STACK_TAIL", "1"))
# A whole stack (first convolution + max-pool + both blocks) in one launch where its input map and pre-pool map fit LDS
# together (32 channels at 21x21 -> 11x11, i.e. the last stack of the 84x84 net); 0 = conv+pool launch, then the tail.
FUSE_STACK_FULL = int(os.environ.get("PPO_AMD_FUSE_STACK_FULL", "1"))
# ... with the previous stack's residual blocks chained in front of it (that stack's output stays in LDS).
FUSE_STACK_CHAIN = int(os.environ.get("PPO_AMD_FUSE_STACK_CHAIN", "1"))
# inference batches of at most CHAIN_SPLIT_MAX_BATCH images (a rollout group) run the chained launch with every image
# on TWO workgroups (output channels split, halves exchanged per layer): same bits, the whole chip instead of half of it.
# Alone, a 128-image forward takes 0.258 ms against 0.282 (the launch 104 us against 128).  In the two-group rollout an
# env step is one group's forward latency plus its host leg, so the shorter launch pays even though it spends 1.6 x
# the CU time: variants alternated rollout by rollout in one process (tools/rollout_ab.py; separate processes differ by
# more than the effect) 0.4846 -> 0.4649 ms per env step, 0.4584 with the action step inside the heads launch as well.
# A partner that never arrives sets an error word which the Runner checks after every rollout (chain_split_error) and
# answers by dropping to the one-workgroup launch and redoing the rollout (Runner.generate_rollout).  Only a forward called
# with `encode(..., chain_split=True)` (the Runner's pipelined rollout passes it, and checks) takes the split launch:
# evaluation, greedy and generic-rollout forwards, whose callers never look at the error word, keep the one-workgroup launch.
CHAIN_SPLIT = int(os.environ.get("PPO_AMD_CHAIN_SPLIT", "1"))
CHAIN_SPLIT_MAX_BATCH = 128
# ... and its backward-data pass (blocks + max-pool backward + transposed first convolution) likewise.  Off by default:
# bit-identical, and on its own it has not been measured faster than the launches it replaces (see
# profiles/chain_backward.md for the single-stream figures); the chained form below is what runs at training batches.
FUSE_STACK_FULL_BWD = int(os.environ.get("PPO_AMD_FUSE_STACK_FULL_BWD", "0"))
# ... and the same for their backward-data chain, as a bit mask over the stacks (per 256-sample step, same box:
# 1.476 ms with mask 0, 1.450 with 4 (11x11), 1.404 with 2 (21x21), 1.408 with 6).
FUSE_STACK_TAIL_BWD = int(os.environ.get("PPO_AMD_FUSE_STACK_TAIL_BWD", "7"))
# The backward-data pass of the last stack AND of the previous stack's blocks as one launch
# (ppo_impala_stack_chain_backward_f32, the mirror of the chained forward: the gradient of the previous stack's output
# stays in LDS) instead of four: tail at 11x11, max-pool backward, transposed first convolution, tail at 21x21.  Same
# bits.  One workgroup per image, so small batches idle the chip and keep the four launches: the chained launch runs
# from FUSE_CHAIN_BWD_MIN_BATCH images up (interleaved A/B, profiles/chain_backward.md: 1.0841 -> 1.0676 ms per
# minibatch of 256, a tie at 128, 11 us slower at 64).
FUSE_CHAIN_BWD_MIN_BATCH = 192
# The 16-channel stack's blocks (42x42 / 32x32: the map fills most of a CU's LDS) as the in-place, row-shifted form of the
# same kernel family (csrc/stack_fused.hip stack_shift_kernel) instead of four convolution launches.  One 16-wave workgroup per
# image and per CU, two wave groups half a band apart (one in its K loop while the other runs its epilogue): measured at
# batch 256 forward 0.398 -> 0.393 ms, training step 1.219 -> 1.186 ms with the backward-data form too (bit 0 of the mask
# above).  At 128 images (a rollout group) it leaves half the chip idle (0.296 -> 0.325 ms), so batches below
# FUSE_STACK16_MIN_BATCH keep the four launches.  Same bits either way.
FUSE_STACK16_MIN_BATCH = int(os.environ.get("PPO_AMD_FUSE_STACK16_MIN_BATCH", "192"))
# Below that batch an inference forward runs each 16-channel residual block as one launch (csrc/conv3x3_block.hip: band by
# band, the intermediate map in LDS) instead of two convolution launches: a 128-image group is launch-cost-bound there.
FUSE_BLOCK = int(os.environ.get("PPO_AMD_FUSE_BLOCK", "1"))
# MLP nets (encoder "mlp": the continuous-control and classic configs) run as fused launches (csrc/mlp_fused.hip): one
# per inference forward, three per training minibatch (rows kernel: forward + loss + backward-data; weight gradients +
# statistics; Adam) instead of ~14 launches of 8 - 20 us each.  0 = the op-by-op path (same arithmetic per element up to
# float32 summation order; tests/test_variants_gpu.py runs both against the reference's fixtures).
FUSE_MLP = int(os.environ.get("PPO_AMD_FUSE_MLP", "1"))
# uint8 image minibatches are read out of the whole rollout batch through the permutation by the first convolution (and by
# its weight gradient) instead of being gathered into a second buffer by a launch of its own (0 = gather first)
GATHER_IN_CONV = int(os.environ.get("PPO_AMD_GATHER_IN_CONV", "1"))
# --precision=medium|low with the nature encoder: the (layer, pass) pairs that run as split-bf16 launches (csrc/
# conv_strided_bf16x3.hip) instead of the exact float32 ones.  A pair is listed only where tools/nature_split_ab.py
# measured the split launch faster than the exact one by more than the block-to-block spread at n = 128 and n = 256
# (the table: profiles/nature_kernels.md "Timing").
# The weight gradients of conv2 and conv3 are not listed: split / exact 0.98 - 1.01, inside the spread.
NATURE_SPLIT = frozenset({
    ("conv1", "forward"), ("conv1", "backward_weight"),
    ("conv2", "forward"), ("conv2", "backward_data"),
    ("conv3", "forward"), ("conv3", "backward_data"),
})
HEAD_NAMES = ("policy_head", "value_head", "advantage_head", "tvf_head")
BN_EPS, BN_MOMENTUM = 1e-5, 0.1  # nn.BatchNorm2d's defaults, which rl/impala.py:64-65 takes


def _p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def _conv_names(si, reverse=False, firstconv=False, n_block=2):
    """Parameter names of stack si's block convolutions in forward order (block 0: conv0, conv1; block 1: ...), with
    `firstconv` behind the stack's first convolution.  `reverse`: the order the backward pass processes them in."""
    names = [f"encoder.stacks.{si}.blocks.{bi}.conv{ci}" for bi in range(n_block) for ci in range(2)]
    if firstconv:
        names.insert(0, f"encoder.stacks.{si}.firstconv")
    return tuple(reversed(names)) if reverse else tuple(names)


def _save_block_maps(acts, si, p, a0, q0, a1):
    """What the backward pass (and tools/debug_backward.py) reads of a two-block stack: per block its input and the
    map between its convolutions."""
    acts[f"q{si}_0_in"], acts[f"a{si}_0"], acts[f"q{si}_1_in"], acts[f"a{si}_1"] = p, a0, q0, a1


def _block_wgrad_problems(si, maps, g, grads):
    """The weight-gradient problems [(input, output gradient, parameter name)] of a two-block stack in processing
    order: `maps` and `grads` as _block_grads returns them, g the gradient of the stack's output."""
    p_in, a0, q0, a1 = maps
    da1, g1, da0, _g0 = grads
    b1c1, b1c0, b0c1, b0c0 = _conv_names(si, reverse=True)
    return [(a1, g, b1c1), (q0, da1, b1c0), (a0, g1, b0c1), (p_in, da0, b0c0)]


# ----------------------------------------------------------------------------------------------
# parameter initialisation (host, CPU): the reference's initialisers in the reference's draw order
# ----------------------------------------------------------------------------------------------
def _normed_conv(cin, cout, scale=1.0):
    """rl/tensor_utilities.py:58-67 NormedConv2d: nn.Conv2d init, each filter L2-normalised * scale, zero bias."""
    m = torch.nn.Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        m.weight.data *= scale / m.weight.norm(dim=(1, 2, 3), p=2, keepdim=True)
        m.bias.data *= 0
    return m.weight.data, m.bias.data


def _normed_linear(fin, fout, scale=1.0):
    """rl/tensor_utilities.py:40-56 NormedLinear."""
    m = torch.nn.Linear(fin, fout)
    with torch.no_grad():
        m.weight.data *= scale / m.weight.norm(dim=1, p=2, keepdim=True)
        m.bias.data *= 0
    return m.weight.data, m.bias.data


def _custom_linear(fin, fout, scale=1.0, bias=True):
    """rl/tensor_utilities.py:69-86 CustomLinear(weight_init='orthogonal'): zero bias, orthogonal weight."""
    m = torch.nn.Linear(fin, fout, bias=bias)
    with torch.no_grad():
        if m.bias is not None:
            m.bias.data *= 0
        torch.nn.init.orthogonal_(m.weight.data, gain=scale)
    return m.weight.data, (m.bias.data if bias else None)


def _custom_conv(cin, cout, kernel, stride, scale=1.0):
    """rl/tensor_utilities.py:69-94 CustomConv2d(weight_init='orthogonal'): nn.Conv2d init (its draws are consumed),
    zero bias, then an orthogonal weight."""
    m = torch.nn.Conv2d(cin, cout, kernel_size=(kernel, kernel), stride=(stride, stride))
    with torch.no_grad():
        m.bias.data *= 0
        torch.nn.init.orthogonal_(m.weight.data, gain=scale)
    return m.weight.data, m.bias.data


class ImpalaSpec:
    """Static geometry of the IMPALA encoder (rl/models.py:54-99, rl/impala.py:85-123)."""
    kind = "impala"

    def __init__(self, input_dims, channels=(16, 32, 32), n_block=2, hidden_units=256, down_sample="pool",
                 batch_norm=False):
        if down_sample not in ("pool", "stride", "none"):
            raise ValueError(f"Invalid down_sample mode {down_sample}")  # rl/impala.py:123
        if batch_norm:
            # the spec is the static geometry, which batch norm does not change: the layers are DualHeadNet's
            raise NotImplementedError("batch_norm is not an argument of ImpalaSpec: pass batch_norm=True to DualHeadNet "
                                      "(or in --model_encoder_args), which builds the batch-norm layers itself")
        c, h, w = input_dims
        self.input_dims = tuple(input_dims)
        self.channels = tuple(channels)
        self.n_block = n_block
        self.hidden_units = hidden_units
        # how a stack shrinks its map (rl/impala.py:96-123): 'pool' - first convolution at stride 1, then max-pool 3x3 /
        # stride 2 / padding 1; 'stride' - first convolution at stride 2, no pool; 'none' - stride 1, no pool
        self.down_sample = down_sample
        self.stacks = []  # (cin, cout, h_in, w_in, h_out, w_out)
        for cout in channels:
            # floor((h + 2 - 3) / 2) + 1 == (h + 1) // 2 for the pool and for the strided convolution alike
            ho, wo = (h, w) if down_sample == "none" else ((h + 1) // 2, (w + 1) // 2)
            self.stacks.append((c, cout, h, w, ho, wo))
            c, h, w = cout, ho, wo
        self.out_shape = (c, h, w)
        self.flat = c * h * w


class NatureSpec:
    """Static geometry of the Nature-CNN encoder (rl/models.py:101-145): conv 8x8 stride 4, conv 4x4 stride 2, conv 3x3
    stride 1, no padding, base_channels / 2x / 2x channels, a ReLU behind each, then a linear layer to hidden_units."""
    kind = "nature"

    def __init__(self, input_dims, hidden_units=512, base_channels=32):
        if len(input_dims) != 3:
            raise ValueError(f"the nature encoder takes [C, H, W] observations, got input_dims={input_dims}")
        c, h, w = (int(d) for d in input_dims)
        self.input_dims = (c, h, w)
        self.hidden_units = hidden_units
        self.base_channels = base_channels
        self.layers = []  # (name, cin, cout, kernel, stride, h_in, w_in, h_out, w_out)
        for name, cout, k, s in (("conv1", base_channels, 8, 4), ("conv2", 2 * base_channels, 4, 2),
                                 ("conv3", 2 * base_channels, 3, 1)):
            if h < k or w < k:
                raise ValueError(f"input_dims={tuple(input_dims)} is too small for the nature encoder ({name}: {k}x{k} on {h}x{w})")
            ho, wo = (h - k) // s + 1, (w - k) // s + 1
            self.layers.append((name, c, cout, k, s, h, w, ho, wo))
            c, h, w = cout, ho, wo
        self.out_shape = (c, h, w)
        self.flat = c * h * w


class RtgSpec:
    """Static geometry of the RTG encoder (rl/models.py:172-213, RTG_LSTM - a plain CNN despite its name): conv 4x4
    stride 2 without padding to 32 channels, then two 3x3 padding-1 convolutions (32 -> 64, 64 -> 64), each followed by
    F.relu(max_pool2d(., 2, 2)) - the pool floors, so an odd last row or column is dropped - then a linear layer to
    hidden_units.  Every other encoder argument is accepted and ignored, as the reference's **ignore_args does."""
    kind = "rtg"

    def __init__(self, input_dims, hidden_units=512, **ignored):
        if len(input_dims) != 3:
            raise ValueError(f"the rtg encoder takes [C, H, W] observations, got input_dims={input_dims}")
        c, h, w = (int(d) for d in input_dims)
        if h < 18 or w < 18:  # 18 -> 8 -> 4 -> 4 -> 2 -> 2 -> 1: three pools still leave one pixel
            raise ValueError(f"input_dims={tuple(input_dims)} is too small for the rtg encoder (each side at least 18)")
        if hidden_units < 1:
            raise ValueError(f"the rtg encoder needs hidden_units >= 1, got {hidden_units}")
        self.input_dims = (c, h, w)
        self.hidden_units = hidden_units
        # (name, cin, cout, kernel, stride, padding, h_in, w_in, h_conv, w_conv, h_pooled, w_pooled)
        self.layers = []
        for name, cout, k, s, p in (("conv1", 32, 4, 2, 0), ("conv2", 64, 3, 1, 1), ("conv3", 64, 3, 1, 1)):
            hc, wc = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            self.layers.append((name, c, cout, k, s, p, h, w, hc, wc, hc // 2, wc // 2))
            c, h, w = cout, hc // 2, wc // 2
        self.pool_shapes = [(cout, hc, wc) for _n, _ci, cout, _k, _s, _p, _h, _w, hc, wc, _hp, _wp in self.layers]
        self.out_shape = (c, h, w)
        self.flat = c * h * w


class MLPSpec:
    """StandardMLP (rl/models.py:148-169): fc1 -> tanh -> fc2 on a flat float observation."""
    kind = "mlp"

    def __init__(self, input_dims, hidden_units=64):
        if len(input_dims) != 1:
            raise ValueError(f"the mlp encoder takes flat observations, got input_dims={input_dims}")
        self.input_dims = tuple(input_dims)
        self.in_features = int(input_dims[0])
        self.hidden_units = hidden_units


def init_encoder_parameters(spec, batch_norm=False):
    """Encoder parameters as CPU tensors, drawn from torch's global CPU generator in the reference's
    construction order (impala: rl/models.py:73-84, rl/impala.py:60-62, 96-100; mlp: rl/models.py:157-161;
    nature: rl/models.py:114-125; rtg: rl/models.py:183-194).  `batch_norm` (impala): every residual block also has
    bn0 / bn1 (rl/impala.py:63-65) behind its convolutions, as the reference's named_parameters() lists them - weight
    (gamma) ones, bias (beta) zeros; nn.BatchNorm2d draws nothing, so every other tensor is what it is without."""
    init = OrderedDict()
    if spec.kind == "rtg":
        # plain nn.Conv2d / nn.Linear: torch's default initialisation (kaiming_uniform_(a=sqrt(5)) weights, uniform
        # non-zero biases), tensors taken unchanged
        for name, cin, cout, k, s, p, *_r in spec.layers:
            m = torch.nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p)
            init[f"encoder.{name}.weight"], init[f"encoder.{name}.bias"] = m.weight.data, m.bias.data
        m = torch.nn.Linear(spec.flat, spec.hidden_units)
        init["encoder.fc.weight"], init["encoder.fc.bias"] = m.weight.data, m.bias.data
        return init
    if spec.kind == "nature":
        for name, cin, cout, k, s, *_r in spec.layers:
            w, b = _custom_conv(cin, cout, k, s, scale=1.414)
            init[f"encoder.{name}.weight"], init[f"encoder.{name}.bias"] = w, b
        w, b = _custom_linear(spec.flat, spec.hidden_units, scale=1.414)
        init["encoder.fc.weight"], init["encoder.fc.bias"] = w, b
        return init
    if spec.kind == "mlp":
        w, b = _custom_linear(spec.in_features, spec.hidden_units, scale=torch.nn.init.calculate_gain("tanh"))
        init["encoder.fc1.weight"], init["encoder.fc1.bias"] = w, b
        w, b = _custom_linear(spec.hidden_units, spec.hidden_units, scale=1.414)
        init["encoder.fc2.weight"], init["encoder.fc2.bias"] = w, b
        return init
    s_stack = 1 / math.sqrt(len(spec.channels))  # rl/models.py:75
    for si, (cin, cout, *_r) in enumerate(spec.stacks):
        w, b = _normed_conv(cin, cout)  # firstconv: scale 1 (rl/impala.py:96)
        init[f"encoder.stacks.{si}.firstconv.weight"], init[f"encoder.stacks.{si}.firstconv.bias"] = w, b
        s_block = math.sqrt(s_stack / math.sqrt(spec.n_block))  # rl/impala.py:60,97
        for bi in range(spec.n_block):
            for cname in ("conv0", "conv1"):
                w, b = _normed_conv(cout, cout, scale=s_block)
                init[f"encoder.stacks.{si}.blocks.{bi}.{cname}.weight"] = w
                init[f"encoder.stacks.{si}.blocks.{bi}.{cname}.bias"] = b
            for bname in (("bn0", "bn1") if batch_norm else ()):
                init[f"encoder.stacks.{si}.blocks.{bi}.{bname}.weight"] = torch.ones(cout)
                init[f"encoder.stacks.{si}.blocks.{bi}.{bname}.bias"] = torch.zeros(cout)
    w, b = _normed_linear(spec.flat, spec.hidden_units, scale=1.414)  # rl/models.py:84
    init["encoder.dense.weight"], init["encoder.dense.bias"] = w, b
    return init


def init_parameters(spec, n_actions: int, vh: int, head_scale: float, head_bias: bool, n_tvf: int = 0,
                    batch_norm: bool = False):
    """Initial parameters of DualHeadNet as CPU tensors in the reference's construction order
    (rl/models.py:348-384: encoder, policy / value / advantage heads, log_std, then the TVF head), so
    that the same ``torch.manual_seed`` reproduces the reference's initial weights exactly.
    Keys are the reference's names relative to ``policy_net``."""
    init = init_encoder_parameters(spec, batch_norm=batch_norm)
    heads = [("policy_head", n_actions), ("value_head", vh), ("advantage_head", n_actions)]
    if n_tvf:
        heads.append(("tvf_head", n_tvf * vh))
    for name, rows in heads:
        w, b = _custom_linear(spec.hidden_units, rows, scale=head_scale, bias=head_bias)
        init[f"{name}.weight"] = w
        if head_bias:
            init[f"{name}.bias"] = b
    init["log_std"] = torch.zeros(n_actions)  # rl/models.py:368 (no random draw, so its position is free)
    return init


BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def is_bn_buffer(name: str) -> bool:
    return name.rsplit(".", 1)[-1] in BN_BUFFERS


def state_dict_names(init_names, batch_norm: bool = False):
    """The keys of the reference module's state_dict() for the names init_parameters returns: log_std first (a parameter
    of the net itself, ahead of its sub-modules), then construction order, with nn.BatchNorm2d's buffers behind their
    layer's weight and bias.  Without the buffers (is_bn_buffer) it is the order of named_parameters(), which the integer
    keys of torch.optim.Adam's state dict index."""
    names = []
    for n in ["log_std"] + [n for n in init_names if n != "log_std"]:
        names.append(n)
        if batch_norm and n.endswith(".bias") and n.split(".")[-2] in ("bn0", "bn1"):
            names += [n[:-len("bias")] + b for b in BN_BUFFERS]
    return names


def init_impala_parameters(spec: ImpalaSpec, n_actions: int, vh: int, head_scale: float, head_bias: bool):
    return init_parameters(spec, n_actions, vh, head_scale, head_bias)


def tvf_feature_mask(K: int, H: int, sparsity: float, window: int) -> torch.Tensor:
    """The scaled mask [K, H] of rl/models.py:386-421 (CPU tensor): `sparsity` keeps each (head, feature) with probability
    1 - sparsity and scales the kept ones by sqrt(1 / keep) - drawn from a CPU generator seeded 99, i.e. what the reference
    draws on --device=cpu (torch's CPU generators give the same stream only on hosts that take the same vector code path);
    `window` gives head k the features [left_k, right_k), the window sliding from the first to the last feature with k,
    scaled by sqrt(H / window)."""
    mask = torch.ones([K, H], dtype=torch.float32)
    if sparsity > 0:
        keep_prob = 1 - sparsity
        g = torch.Generator(device="cpu")
        g.manual_seed(99)
        scaled = torch.bernoulli(mask * keep_prob, generator=g) * math.sqrt(1 / keep_prob)
    if window > 0:
        assert sparsity <= 0, "sparsity and feature window not supported together"
        first_right, last_left = window, H - window
        for head in range(K):
            factor = head / (K - 1)
            left = int(0 * (1 - factor) + last_left * factor)
            right = int(first_right * (1 - factor) + H * factor)
            mask[head, :left] = 0
            mask[head, right:] = 0
        scaled = mask * ((1 / math.sqrt(window)) / (1 / math.sqrt(H)))
    return scaled


def plan_input_keys(kind):
    """Entries of encode()'s result that alias the input tensor."""
    return ("x", "in0") if kind == "impala" else ("x",)


class AdamState:
    """Adam moments + step count over a net's flat parameter buffer."""

    def __init__(self):
        self.exp_avg = self.exp_avg_sq = None
        self.step = 0

    def ensure(self, flat):
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(flat)
            self.exp_avg_sq = torch.zeros_like(flat)


def sgd_state_dict(n_parameters: int, lr: float):
    """`torch.optim.SGD(params, lr=lr).state_dict()` of n_parameters parameters (rl/rollout.py:137-138, :412-421): an
    empty `state` and one param group with the installed torch's own keys and defaults, taken from a throw-away optimiser
    on the CPU so that the layout follows torch and not a list written here."""
    params = [torch.zeros(1, requires_grad=True) for _ in range(int(n_parameters))]
    return torch.optim.SGD(params, lr=float(lr)).state_dict()


def optimizer_layout_kind(sd):
    """'adam', 'sgd' or None (cannot tell) for an optimiser state dict: torch's Adam groups carry `betas`, its SGD groups
    `momentum`; the layouts earlier versions of this package wrote (whole `flat` moments; name-keyed moments without
    param groups) are Adam's."""
    groups = sd.get("param_groups") or []
    if "flat" in sd or any("betas" in g for g in groups):
        return "adam"
    if any("momentum" in g for g in groups):
        return "sgd"
    if any(isinstance(st, dict) and "exp_avg" in st for st in (sd.get("state") or {}).values()):
        return "adam"
    return None


def check_optimizer_layout(sd, kind):
    """Refuse a state dict of the other optimiser kind.  Stricter than torch, on purpose: torch.optim.SGD would load an
    Adam dict (and the reverse) and carry on with the wrong hyper-parameters."""
    found = optimizer_layout_kind(sd)
    if found is not None and found != kind:
        raise ValueError(f"optimizer state dict has the {found} layout but this optimizer is {kind}: the checkpoint was "
                         f"written with --*_opt_optimizer={found}")


class ObsNormalizer:
    """Device-resident form of the reference's observation normaliser (rl/models.py:615-617, 661-694):
    `obs_rms` (utils.RunningMeanStd: float64 mean / var per feature, scalar count) plus the float32 constants
    `_mu` / `_std`.  One instance is shared by the policy and value nets of a TVFModel; each net applies it in
    `encode`.  Data-parallel ranks all-reduce the batch moments, so every rank holds the same statistics."""

    def __init__(self, input_dims, device, norm_eps: float = 1e-5, frozen: bool = False, epsilon: float = 1e-4,
                 observation_scaling: str = "scaled"):
        # what a uint8 batch is before it is normalised: prep_for_model's output (rl/models.py:846-855)
        self.observation_scaling = check_observation_scaling(observation_scaling)
        self.u8_prep = OBSERVATION_SCALINGS[observation_scaling][1]
        self.input_dims = tuple(int(d) for d in input_dims)
        self.F = int(np.prod(self.input_dims))
        self.device = torch.device(device)
        self.norm_eps, self.frozen = float(norm_eps), bool(frozen)
        self.mean = torch.zeros(self.F, dtype=torch.float64, device=self.device)
        self.var = torch.ones(self.F, dtype=torch.float64, device=self.device)
        self.count = float(epsilon)
        self.mu = torch.zeros(self.F, dtype=torch.float32, device=self.device)
        self.std = torch.ones(self.F, dtype=torch.float32, device=self.device)
        self._moments = torch.empty(2 * self.F, dtype=torch.float64, device=self.device)
        self.device = self.mean.device  # 'cuda' -> 'cuda:0', comparable with tensors' devices
        self.lib = _lib.load()

    def _call(self, fn_name, *args):
        rc = getattr(self.lib, fn_name)(*args, _lib.current_stream())
        if rc != 0:
            _lib.check(rc, fn_name)

    def _check(self, x):
        if tuple(x.shape[1:]) != self.input_dims or x.dtype not in (torch.uint8, torch.float32) \
                or not x.is_contiguous() or x.device != self.device:
            raise ValueError(f"expected a contiguous uint8/float32 [B, {self.input_dims}] tensor on {self.device}")

    def update(self, x: torch.Tensor):
        """perform_normalization(..., update_normalization=True)'s statistics update (rl/models.py:681-687)."""
        if self.frozen or x.shape[0] == 0:
            return
        self._check(x)
        from . import parallel
        self._call("ppo_obs_moments_f64", _p(x), self.u8_prep if x.dtype == torch.uint8 else 0, x.shape[0], self.F,
                   _p(self._moments))
        n = x.shape[0]
        if parallel.world_size() > 1:
            parallel.allreduce_sum_(self._moments)
            n *= parallel.world_size()
        self._call("ppo_obs_rms_update_f64", _p(self._moments), float(n), self.count, _p(self.mean), _p(self.var),
                   _p(self.mu), _p(self.std), self.F)
        self.count += n

    def apply(self, x: torch.Tensor, out: torch.Tensor):
        self._check(x)
        self._call("ppo_obs_normalize_f32", _p(x), self.u8_prep if x.dtype == torch.uint8 else 0, _p(self.mu), _p(self.std),
                   self.norm_eps, _p(out), x.shape[0], self.F)
        return out

    def state_dict(self):
        return {"mean": self.mean.cpu(), "var": self.var.cpu(), "count": float(self.count)}

    def load_state_dict(self, sd):
        self.mean.copy_(torch.as_tensor(sd["mean"], dtype=torch.float64).reshape(self.F))
        self.var.copy_(torch.as_tensor(sd["var"], dtype=torch.float64).reshape(self.F))
        self.count = float(sd["count"])
        self.mu.copy_(self.mean.float())                # refresh_normalization_constants, rl/models.py:661-663
        self.std.copy_(self.var.float().sqrt())


class DualHeadNet:
    """One encoder + policy / value / advantage (/ TVF) heads (reference: rl/models.py:304-508), HIP-backed.

    Encoders: ``impala`` (3x3 conv stacks, uint8 or float images; encoder arguments ``channels``, ``n_block`` and
    ``down_sample`` = 'pool' | 'stride' | 'none', see ImpalaSpec, and ``batch_norm``: bn0 / bn1 in every residual block,
    op-by-op launches in exact float32, the mode switched by train() / eval() - see `training`), ``nature`` (three strided convolutions and a linear
    layer, uint8 or float images; op-by-op launches, the convolution passes listed in NATURE_SPLIT as split-bf16 launches
    under `precision` low | medium and everything in exact float32 under high), ``rtg`` (a 4x4 stride-2 and
    two 3x3 convolutions, each behind a fused 2x2 max-pool + ReLU launch, and a linear layer, torch's default
    initialisation; uint8 or float images of at least 18x18, every encoder argument ignored; op-by-op in exact float32
    whatever `precision`) and ``mlp`` (flat float observations);
    encoder activation ``relu`` (fused into the head GEMM's operand load) or ``tanh``.  All heads are ONE
    [nh, hidden] matrix so a forward is one GEMM: columns [policy nA | value VH | advantage nA | tvf K*VH].
    ``observation_scaling`` (scaled | centered | unit, rl/models.py:846-855) picks the input mode of every launch that
    reads uint8 observations (`u8_mode`); the launches themselves - fused, indexed, split - are the same in all three.
    """

    def __init__(self, encoder: str, input_dims, n_actions: int, hidden_units: int = 256,
                 activation_fn: str = "relu", tvf_fixed_head_horizons=None, tvf_feature_sparsity: float = 0.0,
                 tvf_feature_window: int = -1, head_scale: float = 1.0, value_head_names=("ext",),
                 head_bias: bool = False, device="cuda", precision: str = "high", observation_scaling: str = "scaled",
                 **encoder_args):
        encoder = encoder.lower()
        # the in_mode of every launch that reads uint8 observations (float32 ones are read with IN_NONE whatever it says)
        self.observation_scaling = check_observation_scaling(observation_scaling)
        self.u8_mode = OBSERVATION_SCALINGS[observation_scaling][0]
        if precision not in ("low", "medium", "high"):
            raise ValueError(f"Invalid precision mode {precision}")
        if encoder not in ("impala", "mlp", "nature", "rtg"):
            raise NotImplementedError(f"encoder '{encoder}' has no HIP path (impala | nature | rtg | mlp)")
        if activation_fn not in ("relu", "tanh"):
            raise ValueError(f"Invalid activation function {activation_fn}")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PpoAmdError(f"device '{device}': the HIP path runs on the GPU only")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # batch_norm=True (impala only): bn0 / bn1 in every residual block (rl/impala.py:63-76), see _encode_impala_bn
        self.batch_norm = bool(encoder_args.pop("batch_norm", False)) if encoder == "impala" else False
        # nn.Module.training.  Only a batch-norm net reads it: set, an inference forward normalises with the statistics of
        # its own batch and updates the running ones (the rollout, rl/rollout.py:712); cleared, every forward uses the
        # running statistics (rl/rollout.py:927, 1192, 2228).  Not encode()'s `train` argument - see there.
        self.training = True
        if encoder == "impala":
            self.spec = ImpalaSpec(input_dims, hidden_units=hidden_units, **encoder_args)
        elif encoder == "nature":
            self.spec = NatureSpec(input_dims, hidden_units=hidden_units, **encoder_args)
            for _name, cin, cout, k, s, h, w, _ho, _wo in self.spec.layers:
                if not self.lib.ppo_conv2d_strided_supported(cin, cout, k, k, s, h, w):
                    raise _lib.PpoAmdError(f"no strided-convolution kernel for {cin}->{cout} {k}x{k}/{s} on {h}x{w}")
        elif encoder == "rtg":
            self.spec = RtgSpec(input_dims, hidden_units=hidden_units, **encoder_args)
            for _name, cin, cout, k, s, p, h, w, *_r in self.spec.layers:
                if p == 0 and not self.lib.ppo_conv2d_strided_supported(cin, cout, k, k, s, h, w):
                    raise _lib.PpoAmdError(f"no strided-convolution kernel for {cin}->{cout} {k}x{k}/{s} on {h}x{w}")
                if p == 1 and not self.lib.ppo_conv3x3_any_supported(cin, cout, h, w):
                    raise _lib.PpoAmdError(f"no 3x3 convolution kernel for {cin}->{cout} on {h}x{w}")
        else:
            self.spec = MLPSpec(input_dims, hidden_units=hidden_units, **encoder_args)
        self.encoder_kind = encoder
        self.encoder_activation_fn = activation_fn
        self.n_actions = n_actions
        self.hidden_units = hidden_units
        self.value_head_names = list(value_head_names)
        self.vh = len(self.value_head_names)
        self.head_bias = head_bias
        self.tvf_fixed_head_horizons = None if tvf_fixed_head_horizons is None else list(tvf_fixed_head_horizons)
        self.K = 0 if tvf_fixed_head_horizons is None else len(tvf_fixed_head_horizons)
        # fused head columns
        self.col_policy, self.col_value = 0, n_actions
        self.col_advantage = n_actions + self.vh
        self.col_tvf = 2 * n_actions + self.vh
        self.nh = self.col_tvf + self.K * self.vh
        self._build_parameters(head_scale)
        self.tvf_feature_sparsity, self.tvf_feature_window = tvf_feature_sparsity, tvf_feature_window
        self.tvf_features_mask = None
        self._build_tvf_feature_mask()
        self._bufs: Dict[tuple, torch.Tensor] = {}
        self._rec = None   # launch recorder (see encode)
        self._chain_split_usable = None  # decided at the first split launch (see _chain_split_first_use)
        self._tail_ptrs = {}  # pointer arrays of the fused stack kernels, by stack index or (form, stack index): _packed_ptrs
        self.obs_norm = None  # shared ObsNormalizer (set by TVFModel when observation_normalization is on)
        self.grad_ready_hook = None  # callable(stream), see _backward_impala (data-parallel gradient buckets)
        self._split_ws = {}  # workspaces of the two-workgroups-per-image chain launch
        self._plans = {}   # (tag, batch, dtype, chain_split[, training: batch-norm nets]) -> recorded inference launch list
        self.use_plans = True  # False: every inference launch goes through _call (bench.py's per-kernel table brackets it)
        self._find_generic_convs()
        self._build_packed_weights()
        self._build_split_bf16(precision)
        self._build_mlp_fused()
        self._adam_step = 0
        self.exp_avg = None
        self.exp_avg_sq = None

    @property
    def use_tvf(self):
        return self.K > 0

    # ------------------------------------------------------------------ parameters
    def _build_parameters(self, head_scale):
        sp = self.spec
        init = init_parameters(sp, self.n_actions, self.vh, head_scale, self.head_bias, self.K, batch_norm=self.batch_norm)
        # nn.BatchNorm2d's buffers, outside the flat parameter buffer (no optimiser, gradient or reducer sees them):
        # name -> tensor in state_dict order, behind their layer's weight and bias
        self.buffers = OrderedDict()
        for name in state_dict_names(init.keys(), self.batch_norm):
            if is_bn_buffer(name):
                c = init[name.rsplit(".", 1)[0] + ".bias"].numel()
                self.buffers[name] = (torch.zeros((), dtype=torch.int64, device=self.device) if name.endswith("tracked")
                                      else torch.full((c,), float(name.endswith("var")), dtype=torch.float32, device=self.device))
        # physical order: encoder..., then the head weights contiguous (one [nh, hidden] matrix),
        # then the head biases contiguous, then log_std
        head_names = [n for n in HEAD_NAMES if f"{n}.weight" in init]
        order = [(n, t) for n, t in init.items() if n.startswith("encoder.")]
        order += [(f"{n}.weight", init[f"{n}.weight"]) for n in head_names]
        if self.head_bias:
            order += [(f"{n}.bias", init[f"{n}.bias"]) for n in head_names]
        order += [("log_std", init["log_std"])]

        offs, total = OrderedDict(), 0
        for name, t in order:
            offs[name] = (total, tuple(t.shape))
            n = t.numel()
            # head weights / biases must stay contiguous: no padding inside those groups
            contiguous_group = name.endswith("_head.weight") or name.endswith("_head.bias")
            total += n if contiguous_group else (n + _ALIGN - 1) // _ALIGN * _ALIGN
        total = (total + _ALIGN - 1) // _ALIGN * _ALIGN
        self.n_params_padded = total
        flat = torch.zeros(total, dtype=torch.float32)
        for name, t in order:
            o, shape = offs[name]
            flat[o:o + t.numel()] = t.reshape(-1)
        self.flat = flat.to(self.device)
        self.grad = torch.zeros_like(self.flat)
        self._offsets = offs
        self._state_order = list(init.keys())
        self.params = OrderedDict((name, self.flat[o:o + int(np.prod(shape))].view(shape)) for name, (o, shape) in offs.items())
        self.grads = OrderedDict((name, self.grad[o:o + int(np.prod(shape))].view(shape)) for name, (o, shape) in offs.items())
        o = offs["policy_head.weight"][0]
        self.w_heads = self.flat[o:o + self.nh * sp.hidden_units].view(self.nh, sp.hidden_units)
        self.g_w_heads = self.grad[o:o + self.nh * sp.hidden_units].view(self.nh, sp.hidden_units)
        if self.head_bias:
            o = offs["policy_head.bias"][0]
            self.b_heads = self.flat[o:o + self.nh]
            self.g_b_heads = self.grad[o:o + self.nh]
        else:
            self.b_heads = self.g_b_heads = None

    def _build_split_bf16(self, precision):
        """--precision=low|medium (rl train.py:166-178 lets cuDNN use TF32 there).  nature: the convolution passes listed in
        NATURE_SPLIT run as split-bf16 launches (csrc/conv_strided_bf16x3.hip), which split their float32 operands
        themselves - no buffers, no packing jobs.  impala (two blocks, no batch norm): the residual blocks of the 32-channel
        stacks run as split-bf16 launches (csrc/stack_bf16x3.hip: three bf16 MFMAs per product, float32 accumulation,
        ~16-bit products; forward and backward-data).  `high` - the default of this class, of bench.py and of every
        parity test - is exact float32 everywhere.  Buffers: per such stack the forward and the transposed packing of
        its four block convolutions, refreshed by ONE launch behind the float32 re-pack."""
        self.precision = precision
        self.split_bf16, self._pk16, self._split_jobs, self._split_conv_jobs = False, {}, None, None
        self._nature_split = NATURE_SPLIT if precision != "high" and self.encoder_kind == "nature" else frozenset()
        self.split_bf16 = bool(self._nature_split)
        if precision == "high" or self.encoder_kind != "impala" or self.spec.n_block != 2 or self.batch_norm:
            return  # (a batch-norm net runs op by op in exact float32 whatever `precision`, like rtg)
        jobs = []
        nbytes = int(self.lib.ppo_impala_stack_tail_bf16x3_packed_bytes())
        for si, (_cin, cout, _h, _w, ho, wo) in enumerate(self.spec.stacks):
            if not self.lib.ppo_impala_stack_tail_bf16x3_supported(cout, ho, wo) \
                    or _conv_names(si)[0] in self._generic:
                continue
            for tr in (0, 1):  # the transposed packing in the backward pass's processing order
                buf = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
                self._pk16[(si, tr)] = buf
                ws = [self.params[n + ".weight"].data_ptr() for n in _conv_names(si, reverse=bool(tr))]
                jobs.append(_lib.SplitPackJob((ctypes.c_void_p * 4)(*ws), buf.data_ptr(), cout, tr))
            self._pk16[(si, "bias")] = (ctypes.c_void_p * 4)(*[self.params[n + ".bias"].data_ptr() for n in _conv_names(si)])
        if jobs:
            self._split_jobs = (_lib.SplitPackJob * len(jobs))(*jobs)
            self.split_bf16 = True
            self._packed_dirty = True
        # the stack-first convolutions that are not part of a chain (csrc/conv_bf16x3.hip): forward and backward-data
        cjobs = []
        self._split_conv_jobs = None
        for si, (cin, cout, h, w, _ho, _wo) in enumerate(self.spec.stacks):
            if not (self.split_bf16 and SPLIT_CONV and si > 0 and cin in (16, 32) and cout in (16, 32)) \
                    or self.spec.down_sample != "pool":  # (without the max-pool the first convolutions stay exact float32)
                continue
            wname = f"encoder.stacks.{si}.firstconv"
            if wname in self._generic:
                continue
            nb = int(self.lib.ppo_conv3x3_bf16x3_packed_bytes(cin, cout))
            for tr, (ci_op, co_op) in ((0, (cin, cout)), (1, (cout, cin))):
                if not self.lib.ppo_conv3x3_bf16x3_supported(ci_op, co_op, h, w):
                    continue
                buf = torch.zeros(nb, dtype=torch.uint8, device=self.device)
                self._pk16[(wname, tr)] = buf
                cjobs.append(_lib.ConvPackJob(self.params[wname + ".weight"].data_ptr(), buf.data_ptr(), cin, cout, tr))
        if cjobs:
            self._split_conv_jobs = (_lib.ConvPackJob * len(cjobs))(*cjobs)

    def _build_mlp_fused(self):
        """The pointer tables of the fused MLP launches (the flat buffers never move)."""
        self.mlp_fused, self._presummed = False, 0
        sp = self.spec
        if not FUSE_MLP or self.encoder_kind != "mlp" or \
                not self.lib.ppo_mlp_supported(sp.in_features, sp.hidden_units, self.nh):
            return
        P, G = self.params, self.grads
        self._mlp_net = _lib.MlpNet(
            w1=_p(P["encoder.fc1.weight"]), b1=_p(P["encoder.fc1.bias"]), w2=_p(P["encoder.fc2.weight"]),
            b2=_p(P["encoder.fc2.bias"]), wh=_p(self.w_heads), bh=_p(self.b_heads), F=sp.in_features, H=sp.hidden_units,
            NH=self.nh, act=1 if self.encoder_activation_fn == "tanh" else 2)
        self._mlp_grads = _lib.MlpGrads(
            dw1=_p(G["encoder.fc1.weight"]), db1=_p(G["encoder.fc1.bias"]), dw2=_p(G["encoder.fc2.weight"]),
            db2=_p(G["encoder.fc2.bias"]), dwh=_p(self.g_w_heads), dbh=_p(self.g_b_heads), dlog_std=_p(G["log_std"]),
            n_log_std=self.n_actions)
        self._mlp_loss = _lib.MlpLoss()
        self._mlp_npart = ctypes.c_int(0)
        self.mlp_fused = True

    def _mlp_train(self, kind, prev_state, index, stats, n_stats, stat_sums, stat_accumulate, *, obs_indexed=False,
                   **fields):
        """Forward + loss `kind` + backward of one minibatch through the fused launches; the gradients land in
        self.grad, the per-workgroup sums of g^2 in the optimiser's workspace (adam_step picks them up).
        obs_indexed: prev_state is the array `index` points into (sample b is its row index[b]), see ppo_minibatch."""
        B = self._minibatch_rows(prev_state, index, obs_indexed)
        x = prev_state
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("the mlp encoder takes contiguous float32 observations")
        x_indexed = int(x.shape[0]) if obs_indexed else 0  # rows of the array the index points into
        if self.obs_norm is not None:
            if x_indexed:
                raise ValueError("observation normalisation needs the gathered minibatch")
            xn = self._buf("txn", tuple(x.shape))
            self._call("ppo_obs_normalize_f32", _p(x), 0, _p(self.obs_norm.mu), _p(self.obs_norm.std),
                       self.obs_norm.norm_eps, _p(xn), x.shape[0], self.obs_norm.F)
            x = xn
        L = self._mlp_loss
        L.kind, L.stats = kind, _p(stats)
        for k, v in fields.items():
            setattr(L, k, v)
        H = self.hidden_units
        ws = self._buf("mlp_ws", (int(self.lib.ppo_mlp_train_workspace_floats(B, self.spec.in_features, H, self.nh)),))
        partials = self._ws("adam_ws", self.lib.ppo_adam_workspace_bytes())
        self._call("ppo_mlp_train_f32", _p(x), ctypes.addressof(self._mlp_net), ctypes.addressof(self._mlp_grads), _p(index),
                   x_indexed, B, ctypes.addressof(L), _p(ws), None, _p(stat_sums), n_stats, 1 if stat_accumulate else 0,
                   _p(partials), ctypes.addressof(self._mlp_npart))
        self._presummed = self._mlp_npart.value
        return stats

    def _build_tvf_feature_mask(self):
        """rl/models.py:386-421: a static mask [K, hidden] over the TVF head's weights - `tvf_feature_sparsity` zeroes a
        random share of each head's features (the kept ones scaled by sqrt(1 / keep)), `tvf_feature_window` gives head k
        a window of that many features sliding from the first to the last with k (scaled by sqrt(hidden / window)).
        The initial weights are multiplied by the scaled mask; the 0 / 1 mask stays and is re-applied after every
        optimiser step (mask_feature_weights).  The random mask comes from a CPU generator seeded 99, i.e. what the
        reference draws on --device=cpu (on a GPU it seeds that device's generator: another stream, same law)."""
        if not self.use_tvf or (self.tvf_feature_sparsity <= 0 and self.tvf_feature_window <= 0):
            return
        if self.vh != 1:  # the reference's [K, hidden] mask broadcasts against [K * vh, hidden] only then
            raise ValueError("TVF feature masks need a single value head")
        scaled = tvf_feature_mask(self.K, self.hidden_units, self.tvf_feature_sparsity, self.tvf_feature_window)
        w = self.params["tvf_head.weight"]
        w.mul_(scaled.to(self.device))
        self.tvf_features_mask = torch.gt(scaled, 0).to(torch.uint8).to(self.device).contiguous()

    def mask_feature_weights(self):
        """rl/models.py:425-427; the reference calls it before every forward that evaluates the TVF head (:494-497),
        here it follows whatever wrote the weights (optimiser step, load_state_dict): the same weights at every use."""
        if self.tvf_features_mask is not None:
            w = self.params["tvf_head.weight"]
            self._call("ppo_mask_mul_f32", _p(w), _p(self.tvf_features_mask), w.numel())

    @property
    def early_grad_offset(self) -> int:
        """Offset in the flat gradient from which everything (dense layer, heads, log_std) is written by the first
        launches of a backward pass; [0, offset) are the convolution gradients, final only at its end."""
        return self._offsets["encoder.dense.weight"][0] if self.encoder_kind == "impala" else 0

    def n_parameters(self) -> int:
        return sum(int(np.prod(s)) for _, s in self._offsets.values())

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """Reference key names (policy_net.<these>), tensors are views into the flat buffer - and, on a batch-norm net,
        the layers' buffers (running_mean, running_var, num_batches_tracked) behind each layer's weight and bias, where
        nn.Module.state_dict() puts them."""
        return OrderedDict((n, self.params[n] if n in self.params else self.buffers[n])
                           for n in state_dict_names(self._state_order, self.batch_norm))

    def train(self, mode: bool = True):
        """nn.Module.train: see `training` (__init__)."""
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    # ------------------------------------------------------------------ convolutions without a specialised kernel
    def _find_generic_convs(self):
        """`generic_convs`: the IMPALA convolutions, by parameter name, that the specialised kernels (csrc/conv3x3.hip,
        csrc/conv3x3_wgrad.hip: the layers of the (16, 32, 32) stacks on 84x84 and 64x64 observations) have no
        instantiation for - another --env_resolution / --env_color_mode / --env_frame_stack / --env_synthetic_shape, or
        other `channels` / `n_block` encoder arguments.  Their forward, backward-data and weight-gradient launches are
        the generic ppo_conv3x3_any_* ones, in exact float32 whatever `precision`.  Decided per convolution, by asking
        the specialised dispatchers' own probes: a net keeps every specialised and fused launch its other layers
        qualify for (a (12, 84, 84) net moves its first convolution only).  A generic convolution has no packed
        weights, which is also what keeps the fused stack / block launches - all of them read packed weights - off it.
        down_sample='stride' lists every stack's first convolution (its kernels are ppo_conv3x3s2_any_*);
        down_sample='none' probes the blocks at the un-halved map, which is what `stacks` holds then."""
        self.generic_convs, self._probes = [], {}
        if self.encoder_kind == "impala":
            lib, sp = self.lib, self.spec

            def specialised(modes, cin, cout, h, w, data_grad):
                return all(lib.ppo_conv3x3_forward_supported(m, cin, cout, h, w)
                           and lib.ppo_conv3x3_backward_weight_supported(m, cin, cout, h, w) for m in modes) \
                    and (not data_grad or lib.ppo_conv3x3_backward_data_supported(cin, cout, h, w))

            for si, (cin, cout, h, w, ho, wo) in enumerate(sp.stacks):
                # the observations arrive as uint8 or (normalised, or float environments) as float32; nothing
                # back-propagates into them
                if sp.down_sample == "stride":
                    # the stride-2 first convolution has the generic ppo_conv3x3s2_any_* kernels only: no packed weights,
                    # no split-bf16 packing and no fused launch that contains it
                    self.generic_convs.append(f"encoder.stacks.{si}.firstconv")
                    if not lib.ppo_conv3x3s2_any_supported(cin, cout, h, w):
                        raise _lib.PpoAmdError(f"no 3x3 stride-2 convolution kernel for {cin}->{cout} on {h}x{w}")
                elif not specialised((self.u8_mode, IN_NONE) if si == 0 else (IN_NONE,), cin, cout, h, w, si > 0):
                    self.generic_convs.append(f"encoder.stacks.{si}.firstconv")
                    if not lib.ppo_conv3x3_any_supported(cin, cout, h, w):
                        raise _lib.PpoAmdError(f"no 3x3 convolution kernel for {cin}->{cout} on {h}x{w}")
                if not specialised((IN_RELU,), cout, cout, ho, wo, True):
                    self.generic_convs += _conv_names(si, n_block=sp.n_block)
                    if not lib.ppo_conv3x3_any_supported(cout, cout, ho, wo):
                        raise _lib.PpoAmdError(f"no 3x3 convolution kernel for {cout}->{cout} on {ho}x{wo}")
        self._generic = frozenset(self.generic_convs)

    def _probe(self, fn_name, *args) -> bool:
        """A *_supported probe of the library, asked once per argument list."""
        key = (fn_name, args)
        ok = self._probes.get(key)
        if ok is None:
            ok = self._probes[key] = bool(getattr(self.lib, fn_name)(*args))
        return ok

    # ------------------------------------------------------------------ pre-packed convolution weights
    def _build_packed_weights(self):
        """One buffer with, per convolution, the forward kernels' A operand and the backward-data kernels' (flipped,
        transposed) one in per-lane order, plus the job table of the launch that refreshes all of them."""
        self._pk, self._pack_table, self._packed_dirty, self._scatter = {}, None, False, None
        if not PACKED_WEIGHTS or self.encoder_kind != "impala":
            return
        jobs, total = [], 0
        for name, w in self.params.items():
            if not (name.startswith("encoder.stacks.") and name.endswith(".weight")) or name[:-len(".weight")] in self._generic \
                    or w.dim() != 4:
                continue  # (the generic kernels read the raw tensor; a batch-norm layer's weight is no convolution's)
            cout, cin = int(w.shape[0]), int(w.shape[1])
            for transposed in (0, 1):
                if transposed and name == "encoder.stacks.0.firstconv.weight":
                    continue  # nothing back-propagates into the observations
                n = int(self.lib.ppo_conv3x3_packed_floats(cin, cout, transposed))
                jobs.append((name[:-len(".weight")], transposed, cin, cout, total, n))
                total += n
        if not jobs:
            return
        self._packed = torch.zeros(total, dtype=torch.float32, device=self.device)
        table = (_lib.PackJob * len(jobs))()
        for k, (wname, transposed, cin, cout, off, n) in enumerate(jobs):
            view = self._packed[off:off + n]
            self._pk[(wname, transposed)] = view
            table[k] = _lib.PackJob(_p(self.params[wname + ".weight"]), _p(view), cin, cout, transposed)
        self._pack_table = table
        self._packed_dirty = True

    def _scatter_table(self):
        """[n_conv, 2] int32 (device): for every element of the flat buffer's convolution head the one or two slots of
        the packed buffer that hold it (-1: none - biases, alignment padding), so that the optimiser step can refresh
        the packed operands itself (ppo_adam_step_scatter_f32).  Found by packing a buffer of element numbers once."""
        if self._scatter is None and self._pack_table is not None:
            n_conv = int(self.early_grad_offset)
            keep = self.flat[:n_conv].clone()
            self.flat[:n_conv] = torch.arange(1, n_conv + 1, dtype=torch.float32, device=self.device)  # exact below 2^24
            self._packed_dirty = True
            self._refresh_packed()
            slots = self._packed.cpu().numpy().astype(np.int64)
            self.flat[:n_conv] = keep
            self._packed_dirty = True
            self._refresh_packed()
            pos = np.flatnonzero(slots > 0)
            src = slots[pos] - 1
            order = np.argsort(src, kind="stable")
            src, pos = src[order], pos[order]
            first = np.r_[True, src[1:] != src[:-1]]
            second = ~first
            assert not (second[1:] & second[:-1]).any(), "a weight sits in more than two packed slots"
            table = np.full((n_conv, 2), -1, np.int32)
            table[src[first], 0] = pos[first]
            table[src[second], 1] = pos[second]
            self._scatter = (torch.from_numpy(table).to(self.device), n_conv)
        return self._scatter

    def mark_weights_changed(self):
        """Call after writing convolution weights other than through adam_step / load_state_dict."""
        self._packed_dirty = self._pack_table is not None or getattr(self, "_split_jobs", None) is not None

    def _refresh_packed(self):
        if self._packed_dirty:
            self._packed_dirty = False
            with self._unrecorded():  # never part of a recorded forward: the refresh is conditional
                if self._pack_table is not None:
                    self._call("ppo_conv3x3_pack_weights_f32", ctypes.addressof(self._pack_table), len(self._pack_table))
                if self._split_jobs is not None:
                    self._call("ppo_impala_stack_tail_pack_bf16x3_jobs", ctypes.addressof(self._split_jobs), len(self._split_jobs))
                    if self._split_conv_jobs is not None:
                        self._call("ppo_conv3x3_pack_bf16x3_jobs", ctypes.addressof(self._split_conv_jobs), len(self._split_conv_jobs))

    def load_state_dict(self, sd, strict=True):
        self.mark_weights_changed()
        missing = [n for n in (*self.params, *self.buffers) if n not in sd]
        unexpected = [n for n in sd if n not in self.params and n not in self.buffers]
        if strict and (missing or unexpected):
            raise KeyError(f"state_dict mismatch: missing {missing}, unexpected {unexpected}")
        with torch.no_grad():
            for n, t in sd.items():
                if n in self.params:
                    self.params[n].copy_(torch.as_tensor(t).to(self.device, torch.float32).reshape(self.params[n].shape))
                elif n in self.buffers:  # in place: recorded launch plans hold their addresses
                    b = self.buffers[n]
                    b.copy_(torch.as_tensor(t).to(self.device, b.dtype).reshape(b.shape))
        self.mask_feature_weights()

    # ------------------------------------------------------------------ scratch memory
    def _buf(self, name, shape, dtype=torch.float32):
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t

    def _ws(self, name, nbytes):
        return self._buf(name, ((nbytes + 3) // 4,), torch.float32)

    def _call(self, fn_name, *args):
        fn = getattr(self.lib, fn_name)
        if self._rec is not None:
            self._rec.append((fn, fn_name, args))
        rc = fn(*args, _lib.current_stream())
        if rc != 0:
            _lib.check(rc, fn_name)

    @contextlib.contextmanager
    def _unrecorded(self):
        """Launches made inside are kept out of the launch list that encode() is recording, if it is recording one;
        yields that list (or None) for the caller to append what a replay should launch instead."""
        rec, self._rec = self._rec, None
        try:
            yield rec
        finally:
            self._rec = rec

    def _linear(self, x, k, wname, out, relu_x=0, tag=""):
        """out[B, n] = f(x)[B, k] @ W[n, k]^T + b  (torch.nn.Linear).  `tag` keys the split-K workspace, so
        forwards that run concurrently on different streams do not share it."""
        w = self.params[wname + ".weight"]
        B, n = x.shape[0], w.shape[0]
        ws_bytes = self.lib.ppo_gemm_workspace_bytes(B, n, k)
        ws = self._ws("gemm_ws" + tag, ws_bytes)
        self._call("ppo_gemm_f32", _p(x), k, 1, relu_x, _p(w), 1, k, 0, _p(self.params[wname + ".bias"]), None,
                   _p(out), n, B, n, k, _p(ws), ws_bytes)

    def _linear_backward(self, x, k, wname, dy, dx, relu_x=0, mask=None, acc=0, bias_done=False):
        """dW = dy^T @ f(x), db = colsum(dy), dx = (dy @ W) [* (mask > 0)]  (dx nullable).  `bias_done`: an earlier
        launch has written db already."""
        w = self.params[wname + ".weight"]
        B, n = dy.shape[0], w.shape[0]
        self._call("ppo_gemm_f32", _p(dy), 1, n, 0, _p(x), k, 1, relu_x, None, None,
                   _p(self.grads[wname + ".weight"]), k, n, k, B, None, 0)
        if not bias_done:
            self._call("ppo_colsum_f32", _p(dy), B, n, n, _p(self.grads[wname + ".bias"]), acc)
        if dx is not None:
            self._call("ppo_gemm_f32", _p(dy), n, 1, 0, _p(w), k, 1, 0, None, _p(mask), _p(dx), k, B, k, n, None, 0)

    # ------------------------------------------------------------------ forward
    def _conv(self, x, mode, wname, out, residual, n, cin, cout, h, w):
        if wname in self._generic:
            self._call("ppo_conv3x3_any_forward_f32", _p(x), mode, _p(self.params[wname + ".weight"]),
                       _p(self.params[wname + ".bias"]), _p(residual), _p(out), n, cin, cout, h, w)
            return
        pk = self._pk.get((wname, 0))
        if pk is not None:
            self._call("ppo_conv3x3_forward_packed_f32", _p(x), mode, _p(pk), _p(self.params[wname + ".bias"]),
                       _p(residual), _p(out), n, cin, cout, h, w)
            return
        self._call("ppo_conv3x3_forward_f32", _p(x), mode, _p(self.params[wname + ".weight"]),
                   _p(self.params[wname + ".bias"]), _p(residual), _p(out), n, cin, cout, h, w)

    def encode(self, x: torch.Tensor, train: bool, tag: Optional[str] = None, *, index=None, tail=None, chain_split=False):
        """x: [B, *input_dims] uint8 (scaled /255 on load; impala only) or float32.  Returns the dict of
        saved tensors; 'h' is the encoder output before the encoder activation, 'hact' its tanh when the
        activation is tanh.  `tag` names the scratch-buffer set ("t" training, "i" inference by default);
        forwards that overlap on different streams use different tags.
        `index`: [B] int32 (device), a training forward only: sample b is x[index[b]] and B = len(index), on a net
        that can read its observations through it (takes_obs_index); anything else raises ValueError.
        `tail`: the arguments that ride on the dense + heads launch (_dense_heads) behind the ones every form of it
        takes.  Training: those of the discrete PPO loss on the finished head row, ppo_dense_heads_loss_forward_f32's
        (n_actions, n_value_heads, actions, old_log_pac, old_log_policy, advantages, returns, eps_clip, ent_coef, vf_coef,
        grad_scale, dheads, stats, index).  Inference: those of the rollout's action step, ppo_dense_heads_act_forward_f32's
        (n_actions, temperature, seed, offset, log_policy, actions, log_pac, raw_policy, values, n_value_heads).  The
        result's 'tail_taken' says whether a launch took them (always a bool; False without a tail, and on a net that has
        no such launch): if not, the caller launches the loss or the action step itself.
        `chain_split`: an inference forward may take the two-workgroups-per-image chained launch (CHAIN_SPLIT); the
        caller checks chain_split_error() afterwards."""
        sp = self.spec
        tag = tag or ("t" if train else "i")
        self._refresh_packed()
        if tuple(x.shape[1:]) != sp.input_dims:
            raise ValueError(f"expected input [B, {sp.input_dims}], got {tuple(x.shape)}")
        if x.dtype not in (torch.uint8, torch.float32) or not x.is_contiguous() or x.device != self.device:
            raise ValueError("input must be a contiguous uint8/float32 tensor on the model's device")
        if index is not None and not (train and self.takes_obs_index(x)):
            raise ValueError("index: a training forward only, on a net that reads observations through it (takes_obs_index)")
        # Inference forwards (the rollout: 2 x 257 per iteration, with the host on the critical path) replay a
        # recorded launch list: every pointer and size of a (tag, batch) forward is fixed — scratch buffers
        # persist, parameters are views of one flat buffer — except the input, which is patched in.  That cuts
        # the per-launch Python work to the ctypes call itself.
        key = (tag, x.shape[0], x.dtype, chain_split)
        if self.batch_norm:
            # Two flags meet here.  `train` (this call): keep the maps for a backward pass.  `self.training` (the net, as
            # nn.Module's): normalise with batch statistics and update the running ones.  A batch-norm net records its
            # two modes as different plans - they are different launches - and a replayed batch-statistics plan updates
            # the running statistics exactly as the recorded one did: the launches write them.
            if train and self.training:
                raise RuntimeError("a training forward of a batch-norm net in training mode: back-propagation through "
                                   "batch statistics is not built (and the reference never runs it) - call eval() first")
            key += (self.training,)
        plan = None if train or not self.use_plans else self._plans.get(key)
        if plan is not None:
            calls, acts, x_slots, heads_at = plan
            taken = tail is not None and heads_at is not None
            if taken:
                # the rollout's action step rides on the dense + heads launch: the recorded plain form gives way to the
                # action form with this env step's tail
                calls = list(calls)
                calls[heads_at] = (self.lib.ppo_dense_heads_act_forward_f32, "ppo_dense_heads_act_forward_f32",
                                   (*calls[heads_at][2], *tail))
            st, xp = _lib.current_stream(), x.data_ptr()
            for k, (fn, fn_name, args) in enumerate(calls):
                rc = fn(xp, *args[1:], st) if k in x_slots else fn(*args, st)
                if rc != 0:
                    _lib.check(rc, fn_name)
            out = dict(acts, tail_taken=taken)
            if self.obs_norm is None:
                for name in plan_input_keys(self.encoder_kind):
                    out[name] = x
            return out
        if not train and self.use_plans:
            self._rec = []
        try:
            x_in = x
            if self.obs_norm is not None:
                # clamp((x - mu) / (std + eps), -5, 5) ahead of the network (rl/models.py:783-784); the net then
                # sees a float32 input, which is also what its backward reads
                x_in = self._buf(tag + "xn", tuple(x.shape))
                self._call("ppo_obs_normalize_f32", _p(x), self.obs_norm.u8_prep if x.dtype == torch.uint8 else 0, _p(self.obs_norm.mu),
                           _p(self.obs_norm.std), self.obs_norm.norm_eps, _p(x_in), x.shape[0], self.obs_norm.F)
            acts = (self._encode_mlp(x_in, train, tag) if self.encoder_kind == "mlp"
                    else self._encode_nature(x_in, train, tag, tail) if self.encoder_kind == "nature"
                    else self._encode_rtg(x_in, train, tag, tail) if self.encoder_kind == "rtg"
                    else self._encode_impala_bn(x_in, train, tag, tail) if self.batch_norm
                    else self._encode_impala(x_in, train, tag, index, tail, chain_split))
            acts.setdefault("tail_taken", False)  # (no dense + heads launch on this path)
            if self.encoder_activation_fn == "tanh" and "heads" not in acts:
                h = acts["h"]
                hact = self._buf(tag + "hact", tuple(h.shape))
                self._call("ppo_tanh_forward_f32", _p(h), _p(hact), h.numel())
                acts["hact"] = hact
            if self._rec is not None:
                xp = x.data_ptr()
                x_slots = frozenset(k for k, (_f, _n, a) in enumerate(self._rec) if a and a[0] == xp)
                # where a replay with a tail puts the action form (the plain form is what _dense_heads records)
                heads_at = next((k for k, (_f, n, _a) in enumerate(self._rec) if n == "ppo_dense_heads_forward_f32"), None)
                self._plans[key] = (self._rec, {k: v for k, v in acts.items() if v is not x}, x_slots, heads_at)
        finally:
            self._rec = None
        return acts

    def _encode_mlp(self, x, train, tag):
        if x.dtype != torch.float32:
            raise ValueError("the mlp encoder takes float32 observations")
        sp, B = self.spec, x.shape[0]
        if self.mlp_fused and not train:
            # the whole net in one launch: heads, and the encoder output before / after its activation
            o = self._buf(f"{tag}heads", (B, self.nh))
            h = self._buf(f"{tag}h", (B, sp.hidden_units))
            hact = self._buf(f"{tag}hact", (B, sp.hidden_units))
            self._call("ppo_mlp_forward_f32", _p(x), ctypes.addressof(self._mlp_net), None, B, _p(o), _p(h), _p(hact))
            return {"x": x, "h": h, "hact": hact, "heads": o}
        z1 = self._buf(f"{tag}z1", (B, sp.hidden_units))
        self._linear(x, sp.in_features, "encoder.fc1", z1, tag=tag)
        a1 = self._buf(f"{tag}a1", (B, sp.hidden_units))
        self._call("ppo_tanh_forward_f32", _p(z1), _p(a1), z1.numel())
        h = self._buf(f"{tag}h", (B, sp.hidden_units))
        self._linear(a1, sp.hidden_units, "encoder.fc2", h, tag=tag)
        return {"x": x, "a1": a1, "h": h}

    def _nature_conv(self, layer, conv_pass):
        """The entry point of one pass of a Nature layer: split-bf16 for the pairs of NATURE_SPLIT under precision
        low | medium, else exact float32."""
        return f"ppo_conv2d_strided_{conv_pass}_" + ("bf16x3" if (layer, conv_pass) in self._nature_split else "f32")

    def _encode_nature(self, x, train, tag, tail):
        """NatureCNN.forward (rl/models.py:130-145), one launch per layer: three strided convolutions with the ReLU in
        their stores (exact float32, or split-bf16 where _nature_conv says so), then the linear layer - with the heads
        (and the action step or the PPO loss) in the same call when the encoder activation is relu, as behind the
        IMPALA encoder."""
        sp, B = self.spec, x.shape[0]
        acts = {"x": x}
        cur, mode = x, (self.u8_mode if x.dtype == torch.uint8 else IN_NONE)
        for name, cin, cout, k, s, h, w, ho, wo in sp.layers:
            y = self._buf(f"{tag}{name}", (B, cout, ho, wo))
            self._call(self._nature_conv(name, "forward"), _p(cur), mode, _p(self.params[f"encoder.{name}.weight"]),
                       _p(self.params[f"encoder.{name}.bias"]), _p(y), 1, B, cin, h, w, cout, k, k, s)
            acts[name] = y
            cur, mode = y, IN_NONE
        # conv3's output is already through its ReLU
        return self._dense_heads(cur.view(B, sp.flat), 0, "encoder.fc", tag, train, acts, tail)

    def _encode_rtg(self, x, train, tag, tail):
        """RTG_LSTM.forward (rl/models.py:198-213), op by op: per layer the convolution without an activation (conv1 on the
        strided kernel, conv2 and conv3 on the generic 3x3 one) and one launch for F.relu(max_pool2d(., 2, 2)), which in
        a training forward also records the gate byte its backward reads; then the linear layer with the heads (and the
        action step or the PPO loss) as behind the nature encoder.  Seven launches."""
        sp, B = self.spec, x.shape[0]
        acts = {"x": x}
        cur, mode = x, (self.u8_mode if x.dtype == torch.uint8 else IN_NONE)
        for name, cin, cout, k, s, p, h, w, hc, wc, hp, wp in sp.layers:
            y = self._buf(f"{tag}{name}", (B, cout, hc, wc))
            wt, bias = self.params[f"encoder.{name}.weight"], self.params[f"encoder.{name}.bias"]
            if p == 0:
                self._call("ppo_conv2d_strided_forward_f32", _p(cur), mode, _p(wt), _p(bias), _p(y), 0, B, cin, h, w, cout,
                           k, k, s)
            else:
                self._call("ppo_conv3x3_any_forward_f32", _p(cur), mode, _p(wt), _p(bias), None, _p(y), B, cin, cout, h, w)
            q = self._buf(f"{tag}{name}_pool", (B, cout, hp, wp))
            gate = self._buf(f"{tag}{name}_gate", (B, cout, hp, wp), torch.uint8) if train else None
            self._call("ppo_maxpool2x2_relu_forward_f32", _p(y), _p(q), _p(gate), B, cout, hc, wc)
            acts[name], acts[name + "_gate"] = q, gate
            cur, mode = q, IN_NONE
        # the last pooled map is already through its ReLU
        return self._dense_heads(cur.view(B, sp.flat), 0, "encoder.fc", tag, train, acts, tail)

    def _batchnorm(self, x, base, z, tag, n, c, h, w):
        """z = bn(x) for layer `base` (…blocks.k.bn0 | bn1; nn.BatchNorm2d defaults, rl/impala.py:63-76) WITHOUT the ReLU -
        the next convolution reads z with IN_RELU.  In training mode two launches that use this batch's statistics and
        update the layer's buffers, otherwise one launch on the running statistics."""
        gamma, beta = self.params[base + ".weight"], self.params[base + ".bias"]
        rm, rv = self.buffers[base + ".running_mean"], self.buffers[base + ".running_var"]
        if self.training:
            nbytes = int(self.lib.ppo_batchnorm_workspace_bytes(c))
            ws = self._buf(f"{tag}bn_ws", ((nbytes + 7) // 8,), torch.float64)
            self._call("ppo_batchnorm_batch_forward_f32", _p(x), _p(gamma), _p(beta), _p(rm), _p(rv),
                       _p(self.buffers[base + ".num_batches_tracked"]), _p(z), None, None, _p(ws), nbytes, n, c, h, w,
                       BN_EPS, BN_MOMENTUM)
        else:
            self._call("ppo_batchnorm_running_forward_f32", _p(x), _p(gamma), _p(beta), _p(rm), _p(rv), _p(z), n, c, h, w, BN_EPS)

    def _encode_impala_bn(self, x, train, tag, tail):
        """The IMPALA encoder with batch_norm=True (rl/impala.py:67-108), op by op in exact float32: per stack the first
        convolution with its pool or stride through the single-operation entry points, then per residual block
        z0 = bn0(q); a = conv0(relu(z0)); z1 = bn1(a); q' = q + conv1(relu(z1)) as batch-norm launch, convolution,
        batch-norm launch, convolution with the skip as residual.  No whole-stack, block-fused or split-bf16 launch."""
        sp, B = self.spec, x.shape[0]
        acts = {"x": x}
        cur, cur_mode = x, (self.u8_mode if x.dtype == torch.uint8 else IN_NONE)
        for si, (cin, cout, h, w, ho, wo) in enumerate(sp.stacks):
            wname = f"encoder.stacks.{si}.firstconv"
            p = self._buf(f"{tag}p{si}", (B, cout, ho, wo))
            idx = None
            if sp.down_sample == "pool":
                idx = self._buf(f"{tag}idx{si}", (B, cout, ho, wo), torch.uint8) if train else None
                c = self._buf(f"{tag}c{si}", (B, cout, h, w))
                self._conv(cur, cur_mode, wname, c, None, B, cin, cout, h, w)
                self._call("ppo_maxpool3x3s2_forward_f32", _p(c), _p(p), _p(idx), B, cout, h, w)
            elif sp.down_sample == "stride":
                self._call("ppo_conv3x3s2_any_forward_f32", _p(cur), cur_mode, _p(self.params[wname + ".weight"]),
                           _p(self.params[wname + ".bias"]), None, _p(p), B, cin, cout, h, w)
            else:
                self._conv(cur, cur_mode, wname, p, None, B, cin, cout, h, w)
            acts[f"in{si}"], acts[f"idx{si}"] = cur, idx
            q = p
            for bi in range(sp.n_block):
                base = f"encoder.stacks.{si}.blocks.{bi}"
                z0, a, z1, qn = (self._buf(f"{tag}{k}{si}_{bi}", (B, cout, ho, wo)) for k in ("z0_", "a", "z1_", "q"))
                self._batchnorm(q, base + ".bn0", z0, tag, B, cout, ho, wo)
                self._conv(z0, IN_RELU, base + ".conv0", a, None, B, cout, cout, ho, wo)
                self._batchnorm(a, base + ".bn1", z1, tag, B, cout, ho, wo)
                self._conv(z1, IN_RELU, base + ".conv1", qn, q, B, cout, cout, ho, wo)
                acts[f"q{si}_{bi}_in"], acts[f"z0_{si}_{bi}"], acts[f"a{si}_{bi}"], acts[f"z1_{si}_{bi}"] = q, z0, a, z1
                q = qn
            cur, cur_mode = q, IN_NONE
        return self._dense_heads(cur.view(B, sp.flat), 1, "encoder.dense", tag, train, acts, tail)

    def _dense_heads(self, flat, relu_x, wname, tag, train, acts, tail):
        """The encoder's last linear layer `wname` on relu(flat) (relu_x = 1) or flat (0), and - where the encoder
        activation is relu - the fused heads behind it in the same launch (the K-slice reduction of the dense product and
        the heads share it; heads() hands the result out).  That launch also takes `tail` (see encode): the discrete PPO
        loss on the finished head row (a training forward: no loss launch) or the rollout's action step (an inference
        forward).  Fills acts' 'flat', 'h', 'tail_taken' and, with the fused launch, 'heads'."""
        sp, B = self.spec, flat.shape[0]
        h = self._buf(f"{tag}h", (B, sp.hidden_units))
        fused = self.encoder_activation_fn == "relu"
        if fused:
            o = self._buf(f"{tag}heads", (B, self.nh))
            ws_bytes = self.lib.ppo_gemm_workspace_bytes(B, sp.hidden_units, sp.flat)
            ws = self._ws("gemm_ws" + tag, ws_bytes)
            args = (_p(flat), relu_x, _p(self.params[wname + ".weight"]), _p(self.params[wname + ".bias"]), _p(self.w_heads),
                    _p(self.b_heads), 1, _p(h), _p(o), B, sp.flat, sp.hidden_units, self.nh, _p(ws), ws_bytes)
            if tail is None:
                self._call("ppo_dense_heads_forward_f32", *args)
            elif train:
                self._call("ppo_dense_heads_loss_forward_f32", *args, *tail)
            else:
                # the recorded launch list keeps the plain form: its replay adds the tail of its own env step (see encode)
                with self._unrecorded() as rec:
                    self._call("ppo_dense_heads_act_forward_f32", *args, *tail)
                if rec is not None:
                    rec.append((self.lib.ppo_dense_heads_forward_f32, "ppo_dense_heads_forward_f32", args))
            acts["heads"] = o
        else:
            self._linear(flat, sp.flat, wname, h, relu_x=relu_x, tag=tag)
        acts["flat"], acts["h"], acts["tail_taken"] = flat, h, fused and tail is not None
        return acts

    def _packed_ptrs(self, key, names, transposed, biases=False, split=None):
        """The host array of the packed-weight pointers (forward operands, or the transposed ones of backward-data) of
        the convolutions `names`, cached in _tail_ptrs[key]: packed buffers and parameter views keep their addresses
        for the life of the net.  `biases`: (that array, the array of their bias pointers); `split`: two arrays, of the
        first `split` names and of the rest.  None - and nothing cached - while a packed view is missing."""
        cached = self._tail_ptrs.get(key)
        if cached is None:
            pks = [self._pk.get((n, transposed)) for n in names]
            if any(pk is None for pk in pks):
                return None
            ptrs = [pk.data_ptr() for pk in pks]
            if split:
                cached = ((ctypes.c_void_p * split)(*ptrs[:split]), (ctypes.c_void_p * (len(ptrs) - split))(*ptrs[split:]))
            else:
                cached = (ctypes.c_void_p * len(ptrs))(*ptrs)
            if biases:
                cached = (cached, (ctypes.c_void_p * len(names))(*[self.params[n + ".bias"].data_ptr() for n in names]))
            self._tail_ptrs[key] = cached
        return cached

    def _stack_full_ptrs(self, si, cin, cout, h, w):
        """Host arrays of the five packed-weight / bias pointers (firstconv + the four block convolutions) of stack
        si for the whole-stack kernel, or None when it does not apply."""
        if not (FUSE_STACK_FULL and FUSE_STACK_TAIL) or self.spec.n_block != 2 or cin != cout \
                or not self.lib.ppo_impala_stack_full_supported(cout, h, w) or self.split_bf16 \
                or self.spec.down_sample != "pool":
            return None  # (split mode: the blocks of the 32-channel stacks have their own launches; the kernel pools)
        return self._packed_ptrs(("full", si), _conv_names(si, firstconv=True), 0, biases=True)

    def _stack_tail_ptrs(self, si, cout, ho, wo, batch=1 << 30):
        """Host arrays of the four packed-weight / bias pointers of stack si's residual blocks for the fused
        kernel, or None when it does not apply."""
        if not FUSE_STACK_TAIL or self.spec.n_block != 2 or not self.lib.ppo_impala_stack_tail_supported(cout, ho, wo) \
                or (cout == 16 and batch < FUSE_STACK16_MIN_BATCH):
            return None
        return self._packed_ptrs(si, _conv_names(si), 0, biases=True)

    def _chain_split_ws(self, tag, B, c, h, w):
        """Exchange slots + flags + control words of ppo_impala_stack_chain_split_forward_f32: zeroed ONCE (the flag
        values only ever grow, the kernel advances its own launch counter), one per scratch-buffer set."""
        key = (tag, B, c, h, w)
        ws = self._split_ws.get(key)
        if ws is None:
            n = int(self.lib.ppo_impala_stack_chain_split_workspace_bytes(B, c, h, w))
            ws = torch.zeros(n, dtype=torch.uint8, device=self.device)
            self._split_ws[key] = ws
        return ws

    def chain_split_error(self) -> bool:
        """True if any split launch saw a workgroup whose partner never arrived (word 2 of the control words).
        One device -> host copy however many workspaces there are."""
        if not self._split_ws:
            return False
        words = torch.stack([ws[-16:].view(torch.int32)[2] for ws in self._split_ws.values()])
        return bool(words.any().item())

    def chain_split_armed(self) -> bool:
        """Whether a forward with chain_split=True may take the split launch (so its caller has to check for errors)."""
        return bool(CHAIN_SPLIT) and self.encoder_kind == "impala" and not self.batch_norm \
            and self._chain_split_usable is not False

    def chain_split_disable(self):
        """After an error: the one-workgroup launch from now on.  Clears the error (and fault-injection) words and
        forgets every recorded launch list that holds the split launch."""
        self._chain_split_usable = False
        for ws in self._split_ws.values():
            ws[-16:].view(torch.int32)[2:4].zero_()
        self._plans = {k: v for k, v in self._plans.items()
                       if all(name != "ppo_impala_stack_chain_split_forward_f32" for _f, name, _a in v[0])}

    def chain_split_inject_fault(self):
        """Tests only: from the next split launch on, the second workgroup of every pair withholds its flags (control
        word 3, csrc/stack_fused.hip), i.e. the first one times out exactly as if its partner had never been dispatched."""
        for ws in self._split_ws.values():
            ws[-16:].view(torch.int32)[3] = 1

    def _encode_impala(self, x, train, tag, index, tail, chain_split):
        sp = self.spec
        B = x.shape[0] if index is None else int(index.shape[0])
        acts = {"x": x, "in0_index": index}
        cur, cur_mode = x, (self.u8_mode if x.dtype == torch.uint8 else IN_NONE)
        pending = None  # (pooled map, pointer arrays, output buffers) of a stack whose blocks the next launch runs
        pool = sp.down_sample == "pool"
        for si, (cin, cout, h, w, ho, wo) in enumerate(sp.stacks):
            p = self._buf(f"{tag}p{si}", (B, cout, ho, wo))
            idx = self._buf(f"{tag}idx{si}", (B, cout, ho, wo), torch.uint8) if train and pool else None
            wname = f"encoder.stacks.{si}.firstconv"
            acts[f"in{si}"], acts[f"idx{si}"] = cur, idx
            full = self._stack_full_ptrs(si, cin, cout, h, w) if cur_mode == IN_NONE else None
            if full is not None:
                a0, q0, a1, q1 = self._block_maps(tag, si, B)
                outs = (_p(p) if train else None, _p(idx), _p(a0) if train else None, _p(q0) if train else None,
                        _p(a1) if train else None, _p(q1), B, cout, h, w)
                if pending is None:
                    launch = ("ppo_impala_stack_full_forward_f32", _p(cur), full[0], full[1], *outs)
                else:
                    # the previous stack's blocks run inside the same launch, on its pooled map
                    p_prev, ptrs_prev, (pa0, pq0, pa1, pq1) = pending
                    pending = None
                    launch = ("ppo_impala_stack_chain_forward_f32", _p(p_prev), ptrs_prev[0], ptrs_prev[1],
                              _p(pa0) if train else None, _p(pq0) if train else None, _p(pa1) if train else None,
                              _p(pq1) if train else None, full[0], full[1], *outs)
                    if not train and CHAIN_SPLIT and chain_split and self._chain_split_usable is not False \
                            and B <= CHAIN_SPLIT_MAX_BATCH and (cout, h, w) == (32, 21, 21):
                        # a rollout group (at most half as many images as CUs): every image on two workgroups that split
                        # the output channels of the 21x21 convolutions and exchange halves (bit-identical, ~0.7 x the time)
                        ws = self._chain_split_ws(tag, B, cout, h, w)
                        two_wg = ("ppo_impala_stack_chain_split_forward_f32", _p(p_prev), ptrs_prev[0], ptrs_prev[1],
                                  full[0], full[1], _p(q1), _p(ws), ws.numel(), B, cout, h, w)
                        if self._chain_split_usable is None:
                            # the check ran both forms and q1 holds the chosen one's result: a replay launches that one
                            name, *args = self._chain_split_first_use(two_wg, launch, q1)
                            if self._rec is not None:
                                self._rec.append((getattr(self.lib, name), name, tuple(args)))
                            launch = None
                        else:
                            launch = two_wg
                if launch is not None:
                    self._call(*launch)
                _save_block_maps(acts, si, p, a0, q0, a1)
                cur, cur_mode = q1, IN_NONE
                continue
            if not pool:
                # down_sample 'stride' | 'none' (rl/impala.py:96, 102-105): no max-pool, the first convolution - exact
                # float32 at stride 2, or whatever _conv picks at stride 1 - writes the stack's map itself
                if sp.down_sample == "stride":
                    self._call("ppo_conv3x3s2_any_forward_f32", _p(cur), cur_mode, _p(self.params[wname + ".weight"]),
                               _p(self.params[wname + ".bias"]), None, _p(p), B, cin, cout, h, w)
                else:
                    self._conv(cur, cur_mode, wname, p, None, B, cin, cout, h, w)
            elif self.split_bf16 and (wname, 0) in self._pk16 and cur_mode not in U8_MODES and cur.dtype == torch.float32:
                # --precision=low|medium: the stack-first convolution as split-bf16 products, with the max-pool inside the
                # launch or behind it
                if self.lib.ppo_conv3x3_pool_bf16x3_supported(cin, cout, h, w):
                    self._call("ppo_conv3x3_pool_bf16x3", _p(cur), int(cur_mode == IN_RELU), _p(self._pk16[(wname, 0)]),
                               _p(self.params[wname + ".bias"]), _p(p), _p(idx), B, cin, cout, h, w)
                else:
                    c = self._buf(f"{tag}c{si}", (B, cout, h, w))
                    self._call("ppo_conv3x3_bf16x3", _p(cur), int(cur_mode == IN_RELU), _p(self._pk16[(wname, 0)]),
                               _p(self.params[wname + ".bias"]), _p(c), B, cin, cout, h, w)
                    self._call("ppo_maxpool3x3s2_forward_f32", _p(c), _p(p), _p(idx), B, cout, h, w)
            elif FUSE_POOL_STACKS >> si & 1 and wname not in self._generic \
                    and self._probe("ppo_conv3x3_pool_forward_supported", int(cur_mode), cin, cout, h, w):
                # stack-first convolution + max-pool, fused: the pre-pool map never reaches HBM
                pk = self._pk.get((wname, 0))
                if si == 0 and index is not None:
                    # the minibatch's rows of the whole batch, through the permutation: no gather launch, no second copy
                    self._call("ppo_conv3x3_pool_forward_packed_indexed_f32", _p(cur), _p(index), cur_mode, _p(pk),
                               _p(self.params[wname + ".bias"]), _p(p), _p(idx), B, cin, cout, h, w)
                else:
                    self._call("ppo_conv3x3_pool_forward_f32" if pk is None else "ppo_conv3x3_pool_forward_packed_f32",
                               _p(cur), cur_mode, _p(self.params[wname + ".weight"] if pk is None else pk),
                               _p(self.params[wname + ".bias"]), _p(p), _p(idx), B, cin, cout, h, w)
            else:
                c = self._buf(f"{tag}c{si}", (B, cout, h, w))
                self._conv(cur, cur_mode, wname, c, None, B, cin, cout, h, w)
                self._call("ppo_maxpool3x3s2_forward_f32", _p(c), _p(p), _p(idx), B, cout, h, w)
            split = self.split_bf16 and (si, 0) in self._pk16
            tail_ptrs = None if split else self._stack_tail_ptrs(si, cout, ho, wo, B)
            if split or tail_ptrs is not None:
                a0, q0, a1, q1 = self._block_maps(tag, si, B)
                _save_block_maps(acts, si, p, a0, q0, a1)
                cur, cur_mode = q1, IN_NONE
            if split:
                # --precision=low|medium: this stack's residual blocks as the split-bf16 launch
                if train and cout == 16:  # (measured: 82 -> 61 us for the 16-channel backward chain; nothing at 32 channels)
                    # the backward chain's gates as sign maps (1 byte per 4 elements instead of 4 float32 maps read for a sign)
                    sg = [self._buf(f"{tag}sg{si}_{k}", (B, cout // 4, ho, wo), torch.uint8) for k in range(4)]
                    acts[f"signs{si}"] = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in sg])
                    self._call("ppo_impala_stack_tail_forward_signs_bf16x3", _p(p), _p(self._pk16[(si, 0)]), self._pk16[(si, "bias")],
                               _p(a0), _p(q0), _p(a1), _p(q1), acts[f"signs{si}"], B, cout, ho, wo)
                else:
                    self._call("ppo_impala_stack_tail_forward_bf16x3", _p(p), _p(self._pk16[(si, 0)]), self._pk16[(si, "bias")],
                               _p(a0) if train else None, _p(q0) if train else None, _p(a1) if train else None, _p(q1), B, cout,
                               ho, wo)
                continue
            if tail_ptrs is not None:
                nxt = sp.stacks[si + 1] if si + 1 < len(sp.stacks) else None
                if FUSE_STACK_CHAIN and nxt is not None and (nxt[0], nxt[2], nxt[3]) == (cout, ho, wo) \
                        and self._stack_full_ptrs(si + 1, nxt[0], nxt[1], nxt[2], nxt[3]) is not None:
                    # the next stack's launch takes these blocks along (their output stays in LDS on the way)
                    pending = (p, tail_ptrs, (a0, q0, a1, q1))
                    continue
                # inference needs only the stack's output; training keeps the maps the backward pass reads
                # (the 16-channel form re-reads q0 for its second block's skip connection: it is written in inference too)
                self._call("ppo_impala_stack_tail_forward_f32", _p(p), tail_ptrs[0], tail_ptrs[1], _p(a0) if train else None,
                           _p(q0) if (train or cout == 16) else None, _p(a1) if train else None, _p(q1), B, cout, ho, wo)
                continue
            q = p
            for bi in range(sp.n_block):
                a = self._buf(f"{tag}a{si}_{bi}", (B, cout, ho, wo))
                qn = self._buf(f"{tag}q{si}_{bi}", (B, cout, ho, wo))
                base = f"encoder.stacks.{si}.blocks.{bi}"
                pk0, pk1 = self._pk.get((base + ".conv0", 0)), self._pk.get((base + ".conv1", 0))
                if not train and FUSE_BLOCK and pk0 is not None and pk1 is not None \
                        and self.lib.ppo_conv3x3_block_supported(cout, ho, wo):
                    # inference below the whole-stack kernel's batch: both convolutions of the block in one launch
                    self._call("ppo_conv3x3_block_forward_packed_f32", _p(q), _p(pk0), _p(self.params[base + ".conv0.bias"]),
                               _p(pk1), _p(self.params[base + ".conv1.bias"]), _p(qn), B, cout, ho, wo)
                    q = qn
                    continue
                self._conv(q, IN_RELU, base + ".conv0", a, None, B, cout, cout, ho, wo)
                self._conv(a, IN_RELU, base + ".conv1", qn, q, B, cout, cout, ho, wo)
                acts[f"q{si}_{bi}_in"], acts[f"a{si}_{bi}"] = q, a
                q = qn
            cur, cur_mode = q, IN_NONE
        return self._dense_heads(cur.view(B, sp.flat), 1, "encoder.dense", tag, train, acts, tail)

    def _block_maps(self, tag, si, B):
        """The buffers (a0, q0, a1, q1) of stack si's two residual blocks in scratch-buffer set `tag`: per block the map
        between its convolutions and its output."""
        _cin, cout, _h, _w, ho, wo = self.spec.stacks[si]
        shape = (B, cout, ho, wo)
        return (self._buf(f"{tag}a{si}_0", shape), self._buf(f"{tag}q{si}_0", shape),
                self._buf(f"{tag}a{si}_1", shape), self._buf(f"{tag}q{si}_1", shape))

    def _chain_split_first_use(self, split, chain, q1):
        """First split launch on this device.  The exchange goes through the L2 the two workgroups of a pair share, which
        rests on workgroups b and b ^ 8 landing on one XCD: both forms - (entry point, *arguments) each - run once on this
        batch, outside any recorded launch list, and if the bits of their output q1 differ (another partition mode,
        another dispatch order) the one-workgroup form stays for the life of the net.  Returns the chosen form; q1
        holds its result."""
        with self._unrecorded():
            self._call(*split)
            got = q1.clone()
            self._call(*chain)
            self._chain_split_usable = bool(torch.equal(got, q1)) and not self.chain_split_error()
        if not self._chain_split_usable:
            import warnings
            warnings.warn("the two-workgroups-per-image chain launch does not reproduce the one-workgroup "
                          "launch on this device; using the latter (PPO_AMD_CHAIN_SPLIT=0 silences this)")
        return split if self._chain_split_usable else chain

    def heads(self, acts, tag="i"):
        """[B, nh] = act(h) @ [policy | value | advantage | tvf]^T (+ bias)  (rl/models.py:467-506).
        `acts` is encode()'s dict (or, for relu nets, the pre-activation tensor h itself)."""
        if isinstance(acts, dict):
            if "heads" in acts:  # computed with the dense layer (encode, IMPALA / relu)
                return acts["heads"]
            h = acts.get("hact", acts["h"])
        else:
            h = acts
            if self.encoder_activation_fn == "tanh":
                raise ValueError("pass encode()'s dict: the tanh activation is computed there")
        B = h.shape[0]
        o = self._buf(f"{tag}heads", (B, self.nh))
        relu = 1 if self.encoder_activation_fn == "relu" else 0
        self._call("ppo_gemm_f32", _p(h), self.hidden_units, 1, relu, _p(self.w_heads), 1, self.hidden_units, 0,
                   _p(self.b_heads), None, _p(o), self.nh, B, self.nh, self.hidden_units, None, 0)
        return o

    def forward(self, x, policy_temperature: float = 1.0, train: bool = False, exclude_value=False,
                exclude_policy=False, exclude_tvf=False, include_features=False,
                required_tvf_heads=None) -> Dict[str, torch.Tensor]:
        """Same result keys as the reference's DualHeadNet.forward (rl/models.py:433-508).  Value-like
        entries are views of the fused head row (strided, not copies)."""
        acts = self.encode(x, train)
        o = self.heads(acts, "t" if train else "i")
        B, nA = o.shape[0], self.n_actions
        result = {}
        if include_features:
            result["raw_features"] = acts["h"]
            result["features"] = acts["hact"] if "hact" in acts else torch.relu(acts["h"])
        if not exclude_policy:
            logp = self._buf("log_policy", (B, nA))
            result["raw_policy"] = o[:, :nA]
            if nA > 32:
                pass  # wide gaussian policies have no log_softmax (rl/rollout.py uses raw_policy only)
            elif policy_temperature > 0:
                self._call("ppo_policy_act_f32", _p(o), B, self.nh, nA, float(policy_temperature), None, 0, 0, 1,
                           _p(logp), None, None, None, None, self.vh)
                result["log_policy"] = logp
            else:
                # greedy / blended policy (rl/models.py:475-485): tiny [B, nA] tensors, composed from the
                # HIP log-softmax and argmax
                act = self._buf("greedy_actions", (B,), torch.int32)
                self._call("ppo_policy_act_f32", _p(o), B, self.nh, nA, 1.0, None, 0, 0, 1, _p(logp), _p(act), None,
                           None, None, self.vh)
                argmax_policy = torch.zeros_like(logp)
                argmax_policy[torch.arange(B, device=self.device), act.long()] = 1.0
                eps = 1 + policy_temperature
                result["log_policy"] = torch.log(eps * argmax_policy + (1 - eps) * torch.exp(logp) + 1e-8)
                result["argmax_policy"] = argmax_policy
        if not exclude_value:
            result["value"] = o[:, self.col_value:self.col_value + self.vh]
            if self.use_tvf and not exclude_tvf:
                tvf = o[:, self.col_tvf:].view(B, self.K, self.vh)
                result["tvf_value"] = tvf if required_tvf_heads is None else tvf[:, required_tvf_heads]
        result["advantage"] = o[:, self.col_advantage:self.col_advantage + nA]
        result["_heads"], result["_acts"] = o, acts
        return result

    # ------------------------------------------------------------------ backward
    def backward(self, acts, dheads: torch.Tensor):
        """Back-propagate d loss / d heads through heads and encoder into self.grad, which it overwrites (the Runner sums
        the passes of a minibatch split into micro-batches)."""
        sp = self.spec
        B = dheads.shape[0]
        H = sp.hidden_units
        h = acts["h"]
        relu = self.encoder_activation_fn == "relu"
        hin = h if relu else acts["hact"]
        # heads: dW = dheads^T @ act(h); db = colsum(dheads); dh = (dheads @ W) * act'(h)
        dh = self._buf("dh", (B, H))
        # one launch: dh, the heads' weight / bias gradients and - when dh is final (relu) - the dense layer's bias
        # gradient, which is the column sum of dh
        dense_bias_done = bool(relu and self.encoder_kind == "impala" and self.nh <= 16)
        if self.nh <= 16:
            self._call("ppo_heads_backward_f32", _p(dheads), _p(hin), 1 if relu else 0, _p(h) if relu else None, _p(self.w_heads),
                       _p(dh), _p(self.g_w_heads), _p(self.g_b_heads) if self.head_bias else None,
                       _p(self.grads["encoder.dense.bias"]) if dense_bias_done else None, B, H, self.nh)
        else:
            self._call("ppo_gemm_f32", _p(dheads), 1, self.nh, 0, _p(hin), H, 1, 1 if relu else 0, None, None,
                       _p(self.g_w_heads), H, self.nh, H, B, None, 0)
            if self.head_bias:
                self._call("ppo_colsum_f32", _p(dheads), B, self.nh, self.nh, _p(self.g_b_heads), 0)
            self._call("ppo_gemm_f32", _p(dheads), self.nh, 1, 0, _p(self.w_heads), H, 1, 0, None, _p(h) if relu else None,
                       _p(dh), H, B, H, self.nh, None, 0)
        if not relu:
            self._call("ppo_tanh_backward_f32", _p(dh), _p(hin), _p(dh), dh.numel())
        if self.encoder_kind == "mlp":
            self._backward_mlp(acts, dh)
        elif self.encoder_kind == "nature":
            self._backward_nature(acts, dh)
        elif self.encoder_kind == "rtg":
            self._backward_rtg(acts, dh)
        elif self.batch_norm:
            self._backward_impala_bn(acts, dh, dense_bias_done)
        else:
            self._backward_impala(acts, dh, dense_bias_done)

    def _backward_mlp(self, acts, dh):
        sp = self.spec
        B, H = dh.shape
        da1 = self._buf("da1", (B, H))
        self._linear_backward(acts["a1"], H, "encoder.fc2", dh, da1)
        self._call("ppo_tanh_backward_f32", _p(da1), _p(acts["a1"]), _p(da1), da1.numel())
        self._linear_backward(acts["x"], sp.in_features, "encoder.fc1", da1, None)

    def _backward_nature(self, acts, dh):
        """Backward through the Nature encoder, one launch per gradient: the linear layer (its data gradient gated by
        conv3's output, i.e. already through conv3's ReLU), then weight and data gradients of conv3 and conv2 and the
        weight gradient of conv1 - nothing back-propagates into the observations.  Each strided-convolution launch
        takes the gradient w.r.t. its layer's post-ReLU output and gates it by that output itself; the passes listed
        in NATURE_SPLIT are split-bf16 launches under precision low | medium (same arguments, same workspace)."""
        sp = self.spec
        B = dh.shape[0]
        x, flat = acts["x"], acts["flat"]
        g = self._buf("ng_conv3", tuple(acts["conv3"].shape))
        self._linear_backward(flat, sp.flat, "encoder.fc", dh, g.view(B, sp.flat), mask=flat)
        gate = None  # conv3's gate is in g already
        for li in (2, 1, 0):
            name, cin, cout, k, s, h, w, _ho, _wo = sp.layers[li]
            src = acts[sp.layers[li - 1][0]] if li else x
            mode = self.u8_mode if src.dtype == torch.uint8 else IN_NONE
            geom = (B, cin, h, w, cout, k, k, s)
            nbytes = int(self.lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
            ws = self._ws("nwgrad_ws_" + name, nbytes)
            self._call(self._nature_conv(name, "backward_weight"), _p(src), mode, _p(g), _p(gate),
                       _p(self.grads[f"encoder.{name}.weight"]), _p(self.grads[f"encoder.{name}.bias"]), _p(ws), nbytes, *geom)
            if li:
                gx = self._buf("ng_" + sp.layers[li - 1][0], tuple(src.shape))
                self._call(self._nature_conv(name, "backward_data"), _p(g), _p(gate), _p(self.params[f"encoder.{name}.weight"]),
                           _p(gx), *geom)
                g, gate = gx, src
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(torch.cuda.current_stream())

    def _backward_rtg(self, acts, dh):
        """Backward through the RTG encoder, one launch per gradient: the linear layer (its data gradient unmasked - the
        pool backward applies the gate, which holds the ReLU's decision too), then per layer from the last the pool +
        ReLU backward into the pre-pool map, the weight and bias gradient, and the data gradient where a layer lies
        below - nothing back-propagates into the observations."""
        sp = self.spec
        B = dh.shape[0]
        x, flat = acts["x"], acts["flat"]
        g = self._buf("rg_conv3_pool", tuple(acts["conv3"].shape))
        self._linear_backward(flat, sp.flat, "encoder.fc", dh, g.view(B, sp.flat))
        for li in (2, 1, 0):
            name, cin, cout, k, s, p, h, w, hc, wc, _hp, _wp = sp.layers[li]
            src = acts[sp.layers[li - 1][0]] if li else x
            mode = self.u8_mode if src.dtype == torch.uint8 else IN_NONE
            dy = self._buf("rg_" + name, (B, cout, hc, wc))
            self._call("ppo_maxpool2x2_relu_backward_f32", _p(g), _p(acts[name + "_gate"]), _p(dy), B, cout, hc, wc)
            dw, db = self.grads[f"encoder.{name}.weight"], self.grads[f"encoder.{name}.bias"]
            if p == 0:
                geom = (B, cin, h, w, cout, k, k, s)
                nbytes = int(self.lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
                ws = self._ws("rwgrad_ws_" + name, nbytes)
                self._call("ppo_conv2d_strided_backward_weight_f32", _p(src), mode, _p(dy), None, _p(dw), _p(db), _p(ws),
                           nbytes, *geom)
            else:
                nbytes = int(self.lib.ppo_conv3x3_any_wgrad_workspace_bytes(B, cin, cout, h, w))
                ws = self._ws("rwgrad_ws_" + name, nbytes)
                self._call("ppo_conv3x3_any_backward_weight_f32", _p(src), mode, _p(dy), _p(dw), _p(db), _p(ws), nbytes,
                           B, cin, cout, h, w, 0)
            if li:
                gx = self._buf("rg_" + sp.layers[li - 1][0] + "_pool", tuple(src.shape))
                self._call("ppo_conv3x3_any_backward_data_f32", _p(dy), _p(self.params[f"encoder.{name}.weight"]), None, None,
                           _p(gx), B, cin, cout, h, w)
                g = gx
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(torch.cuda.current_stream())

    def _backward_impala_bn(self, acts, dh, dense_bias_done=False):
        """Backward through the batch-norm IMPALA encoder (eval mode: every bn is a per-channel affine map of constants
        s = gamma / sqrt(running_var + eps), t = beta - running_mean * s), one launch per gradient.  Per block, from
        g = d loss / d (block output), with out = q + conv1(relu(z1)), z1 = bn1(a), a = conv0(relu(z0)), z0 = bn0(q):
        conv1's weight gradient, its data gradient gated by z1, bn1's backward (dgamma, dbeta, da), conv0's weight
        gradient, its data gradient gated by z0, and bn0's backward, which takes g - the skip - as its residual.  Then
        the max-pool backward (down_sample 'pool') and the stack's first convolution."""
        sp, lib = self.spec, self.lib
        B = dh.shape[0]
        flat = acts["flat"]
        c_last, h_last, w_last = sp.out_shape
        g = self._buf(f"g{len(sp.stacks) - 1}_top", (B, c_last, h_last, w_last))
        self._linear_backward(flat, sp.flat, "encoder.dense", dh, g, relu_x=1, mask=flat, bias_done=dense_bias_done)
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(torch.cuda.current_stream())

        def wgrad(x, mode, dy, wname, cin, cout, hh, ww):
            dw, db = self.grads[wname + ".weight"], self.grads[wname + ".bias"]
            if wname in self._generic:
                nbytes = int(lib.ppo_conv3x3_any_wgrad_workspace_bytes(B, cin, cout, hh, ww))
                fn = "ppo_conv3x3_any_backward_weight_f32"
            else:
                nbytes = int(lib.ppo_conv3x3_wgrad_workspace_bytes(cin, cout))
                fn = "ppo_conv3x3_backward_weight_f32"
            ws = self._ws("wgrad_ws_" + wname, nbytes)
            self._call(fn, _p(x), mode, _p(dy), _p(dw), _p(db), _p(ws), nbytes, B, cin, cout, hh, ww, 0)

        def bn_backward(dz, x, residual, base, dx, c, hh, ww):
            nbytes = int(lib.ppo_batchnorm_workspace_bytes(c))
            ws = self._buf("bn_bwd_ws", ((nbytes + 7) // 8,), torch.float64)
            self._call("ppo_batchnorm_running_backward_f32", _p(dz), _p(x), _p(residual), _p(self.params[base + ".weight"]),
                       _p(self.buffers[base + ".running_mean"]), _p(self.buffers[base + ".running_var"]), _p(dx),
                       _p(self.grads[base + ".weight"]), _p(self.grads[base + ".bias"]), _p(ws), nbytes, B, c, hh, ww,
                       BN_EPS, 0)

        for si in reversed(range(len(sp.stacks))):
            cin, cout, hh, ww, ho, wo = sp.stacks[si]
            fc = f"encoder.stacks.{si}.firstconv"
            shape = (B, cout, ho, wo)
            for bi in reversed(range(sp.n_block)):
                base = f"encoder.stacks.{si}.blocks.{bi}"
                q_in, z0, a, z1 = (acts[f"{k}{si}_{bi}{s}"] for k, s in (("q", "_in"), ("z0_", ""), ("a", ""), ("z1_", "")))
                wgrad(z1, IN_RELU, g, base + ".conv1", cout, cout, ho, wo)
                dz1 = self._buf(f"g{si}_{bi}_dz1", shape)
                self._call(self._bwd_data_fn(base + ".conv1"), _p(g), _p(self._bwd_w(base + ".conv1")), _p(z1), None, _p(dz1),
                           B, cout, cout, ho, wo)
                da = self._buf(f"g{si}_{bi}_da", shape)
                bn_backward(dz1, a, None, base + ".bn1", da, cout, ho, wo)
                wgrad(z0, IN_RELU, da, base + ".conv0", cout, cout, ho, wo)
                dz0 = self._buf(f"g{si}_{bi}_dz0", shape)
                self._call(self._bwd_data_fn(base + ".conv0"), _p(da), _p(self._bwd_w(base + ".conv0")), _p(z0), None, _p(dz0),
                           B, cout, cout, ho, wo)
                gn = self._buf(f"g{si}_{bi}_in", shape)
                bn_backward(dz0, q_in, g, base + ".bn0", gn, cout, ho, wo)
                g = gn
            x_in = acts[f"in{si}"]
            mode = IN_NONE if si > 0 else (self.u8_mode if x_in.dtype == torch.uint8 else IN_NONE)
            g_prev = self._buf(f"g{si - 1}_top", (B, cin, hh, ww)) if si > 0 else None
            if sp.down_sample == "stride":
                nbytes = int(lib.ppo_conv3x3s2_any_wgrad_workspace_bytes(B, cin, cout, hh, ww))
                ws = self._ws("wgrad_ws_" + fc, nbytes)
                self._call("ppo_conv3x3s2_any_backward_weight_f32", _p(x_in), mode, _p(g), _p(self.grads[fc + ".weight"]),
                           _p(self.grads[fc + ".bias"]), _p(ws), nbytes, B, cin, cout, hh, ww, 0)
                if si > 0:
                    self._call("ppo_conv3x3s2_any_backward_data_f32", _p(g), _p(self.params[fc + ".weight"]), None, None,
                               _p(g_prev), B, cin, cout, hh, ww)
            else:
                dc = g
                if sp.down_sample == "pool":
                    dc = self._buf(f"g{si}_dc", (B, cout, hh, ww))
                    self._call("ppo_maxpool3x3s2_backward_f32", _p(g), _p(acts[f"idx{si}"]), _p(dc), B, cout, hh, ww)
                wgrad(x_in, mode, dc, fc, cin, cout, hh, ww)
                if si > 0:
                    self._call(self._bwd_data_fn(fc), _p(dc), _p(self._bwd_w(fc)), None, None, _p(g_prev), B, cin, cout, hh, ww)
            g = g_prev

    def _backward_impala(self, acts, dh, dense_bias_done=False):
        """Backward through the encoder, every launch on the current stream: the dense layer, then stack by stack from
        the last one the backward-data chain of the blocks (one fused launch where the geometry has a kernel), max-pool
        backward and the transposed first convolution.  Weight gradients are formed as slabs, each layer in a workspace
        of its own - the block convolutions of a stack in one launch behind that stack's backward-data chain - and one
        launch at the end of the pass reduces the slabs of all layers into self.grad.  Every gradient tensor has its own
        buffer within a pass.  `dense_bias_done`: the heads launch wrote encoder.dense.bias's gradient already."""
        sp, lib = self.spec, self.lib
        B, H = dh.shape
        flat = acts["flat"]
        # dense: dW = dh^T @ relu(flat); db = colsum(dh); dflat = (dh @ W) * (flat > 0)
        c_last, h_last, w_last = sp.out_shape
        g = self._buf(f"g{len(sp.stacks) - 1}_top", (B, c_last, h_last, w_last))
        self._linear_backward(flat, sp.flat, "encoder.dense", dh, g, relu_x=1, mask=flat, bias_done=dense_bias_done)
        if self.grad_ready_hook is not None:
            # dense + head gradients (the tail of the flat buffer from `early_grad_offset` on) are final once the
            # launches queued so far on this stream have run: a data-parallel reducer ships them under the rest
            self.grad_ready_hook(torch.cuda.current_stream())

        jobs = []  # deferred slab reductions: one launch for all layers at the end of the pass

        def split_wgrad(mode, cin, cout, hh, ww):
            """--precision=medium|low: this layer's weight gradient as split-bf16 products (csrc/wgrad_bf16x3.hip)."""
            return self.split_bf16 and SPLIT_WGRAD and mode in (IN_NONE, IN_RELU) \
                and lib.ppo_conv3x3_backward_weight_bf16x3_supported(cin, cout, hh, ww)

        def slab_launch(args_, n_slabs, layers, cin, cout):
            """One slab launch for layers = [(wname, its workspace)]; the kernel reports the slab count through n_slabs."""
            self._call(*args_)
            for wname, ws in layers:
                jobs.append(_lib.WgradJob(_p(ws), _p(self.grads[wname + ".weight"]), _p(self.grads[wname + ".bias"]),
                                          n_slabs.value, cin, cout, 0))

        def wgrad(x, mode, dy, wname, n, cin, cout, hh, ww, argmax=None):
            """argmax given: dy is the POOLED gradient and the kernel forms max-pool backward itself."""
            if wname in self._generic:
                # no specialised kernel: the generic one, slabs reduced by a launch of its own straight into self.grad
                nbytes = int(lib.ppo_conv3x3_any_wgrad_workspace_bytes(n, cin, cout, hh, ww))
                ws = self._ws("wgrad_ws_" + wname, nbytes)
                self._call("ppo_conv3x3_any_backward_weight_f32", _p(x), mode, _p(dy), _p(self.grads[wname + ".weight"]),
                           _p(self.grads[wname + ".bias"]), _p(ws), nbytes, n, cin, cout, hh, ww, 0)
                return
            nbytes = lib.ppo_conv3x3_wgrad_workspace_bytes(cin, cout)
            ws = self._ws("wgrad_ws_" + wname, nbytes)  # per layer: the slabs live until the batched reduction
            n_slabs = ctypes.c_int(0)
            if argmax is not None and acts.get("in0_index") is not None and wname == "encoder.stacks.0.firstconv":
                args_ = ("ppo_conv3x3_backward_weight_slabs_pooled_indexed_f32", _p(x), _p(acts["in0_index"]), mode, _p(dy),
                         _p(argmax), _p(ws), nbytes, n, cin, cout, hh, ww, ctypes.addressof(n_slabs))
            elif argmax is not None:
                args_ = ("ppo_conv3x3_backward_weight_slabs_pooled_f32", _p(x), mode, _p(dy), _p(argmax), _p(ws),
                         nbytes, n, cin, cout, hh, ww, ctypes.addressof(n_slabs))
            elif split_wgrad(mode, cin, cout, hh, ww):
                keep = ((ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int * 1)(int(mode == IN_RELU)),
                        (ctypes.c_void_p * 1)(dy.data_ptr()), (ctypes.c_void_p * 1)(ws.data_ptr()))
                args_ = ("ppo_conv3x3_backward_weight_slabs_batch_bf16x3", keep[0], keep[1], keep[2], keep[3], nbytes, 1, n,
                         cin, cout, hh, ww, ctypes.addressof(n_slabs))
            else:
                args_ = ("ppo_conv3x3_backward_weight_slabs_f32", _p(x), mode, _p(dy), _p(ws), nbytes, n, cin, cout,
                         hh, ww, ctypes.addressof(n_slabs))
            slab_launch(args_, n_slabs, [(wname, ws)], cin, cout)

        carry = []  # [(x, dy, wname, n, c, hh, ww)]: a first convolution waiting for the next batched launch of its geometry

        def flush_carry():
            while carry:
                x, dy, wname, n, c, hh, ww = carry.pop()
                wgrad(x, IN_NONE, dy, wname, n, c, c, hh, ww)

        def wgrad_blocks(problems, n, c, hh, ww):
            """Weight gradients of a stack's block convolutions, problems = [(x, dy, wname)] (all IN_RELU, c -> c)."""
            if not WGRAD_BATCH_LAUNCH or len(problems) > 4 or problems[0][2] in self._generic:
                flush_carry()
                for x, dy, wname in problems:
                    wgrad(x, IN_RELU, dy, wname, n, c, c, hh, ww)
                return
            relu = [1] * len(problems)
            if carry and carry[-1][3:] == (n, c, hh, ww):
                x, dy, wname = carry.pop()[:3]
                problems = list(problems) + [(x, dy, wname)]
                relu.append(0)  # the stack-first convolution read its input raw
            flush_carry()
            nbytes = lib.ppo_conv3x3_wgrad_workspace_bytes(c, c)
            wss = [self._ws("wgrad_ws_" + wname, nbytes) for _x, _dy, wname in problems]
            k = len(problems)
            n_slabs = ctypes.c_int(0)
            ins = (ctypes.c_void_p * k)(*[x.data_ptr() for x, _d, _w in problems])
            dys = (ctypes.c_void_p * k)(*[dy.data_ptr() for _x, dy, _w in problems])
            wsp = (ctypes.c_void_p * k)(*[ws.data_ptr() for ws in wss])
            if split_wgrad(IN_RELU, c, c, hh, ww):
                args_ = ("ppo_conv3x3_backward_weight_slabs_batch_bf16x3", ins, (ctypes.c_int * k)(*relu), dys, wsp, nbytes, k, n,
                         c, c, hh, ww, ctypes.addressof(n_slabs))
            elif k > 4:
                args_ = ("ppo_conv3x3_backward_weight_slabs_batch_mixed_f32", ins, (ctypes.c_int * k)(*relu), dys, wsp, nbytes, k, n,
                         c, c, hh, ww, ctypes.addressof(n_slabs))
            else:
                args_ = ("ppo_conv3x3_backward_weight_slabs_batch_f32", ins, IN_RELU, dys, wsp, nbytes, k, n, c, c, hh, ww,
                         ctypes.addressof(n_slabs))
            slab_launch(args_, n_slabs, [(wname, ws) for (_x, _dy, wname), ws in zip(problems, wss)], c, c)

        chained = None  # (si, maps, grads): stack si's blocks went through the chained launch of stack si + 1
        for si in reversed(range(len(sp.stacks))):
            cin, cout, hh, ww, ho, wo = sp.stacks[si]
            fc = f"encoder.stacks.{si}.firstconv"
            chain_w = self._stack_chain_bwd_ptrs(si, B) if chained is None else None
            if chain_w is not None:
                # this stack's backward-data pass and the previous stack's blocks in one launch; the weight-gradient
                # launches are those of the separate launches, reading the same buffers
                maps, masks, grads = self._block_grads(acts, si, B)
                pmaps, pmasks, pgrads = self._block_grads(acts, si - 1, B)
                da1, g1, da0, g0 = grads
                pda1, pg1, pda0, pg0 = pgrads
                dc = self._buf(f"g{si}_dc", (B, cout, hh, ww))
                g_prev = self._buf(f"g{si - 1}_top", (B, cin, hh, ww))
                self._call("ppo_impala_stack_chain_backward_f32", _p(g), chain_w[0], masks, _p(acts[f"idx{si}"]), _p(da1),
                           _p(g1), _p(da0), _p(g0), _p(dc), _p(g_prev), chain_w[1], pmasks, _p(pda1), _p(pg1), _p(pda0),
                           _p(pg0), B, cout, hh, ww)
                wgrad_blocks(_block_wgrad_problems(si, maps, g, grads), B, cout, ho, wo)
                if self._first_wgrad_rides(si):
                    carry.append((acts[f"in{si}"], dc, fc, B, cin, hh, ww))
                else:
                    wgrad(acts[f"in{si}"], IN_NONE, dc, fc, B, cin, cout, hh, ww)
                g = g_prev
                chained = (si - 1, pmaps, pgrads)
                continue
            # blocks + max-pool backward + transposed first convolution of the stack in one launch, ...
            full_w = self._stack_full_bwd_ptrs(si, cin, cout, hh, ww) if si > 0 else None
            # ... or the four backward-data convolutions of the stack's blocks in one launch (csrc/stack_fused.hip), ...
            tail_w = self._stack_tail_bwd_ptrs(si, cout, ho, wo) if full_w is None else None
            # ... which in split mode is the gated transposed chain of this stack's blocks as the split-bf16 launch
            split = full_w is None and self.split_bf16 and (si, 1) in self._pk16
            fused = full_w is not None or tail_w is not None or split
            if chained is not None and chained[0] == si:
                # the chained launch above ran this stack's blocks: their weight gradients, then the pool and first conv
                fused, full_w = True, None
                _si, maps, grads = chained
                wgrad_blocks(_block_wgrad_problems(si, maps, g, grads), B, cout, ho, wo)
                g = grads[3]
            elif fused:
                maps, masks, grads = self._block_grads(acts, si, B)
                da1, g1, da0, g0 = grads
                if full_w is not None:
                    dc = self._buf(f"g{si}_dc", (B, cout, hh, ww))
                    g_prev = self._buf(f"g{si - 1}_top", (B, cin, hh, ww))
                    self._call("ppo_impala_stack_full_backward_f32", _p(g), full_w, masks, _p(acts[f"idx{si}"]), _p(da1), _p(g1),
                               _p(da0), _p(g0), _p(dc), _p(g_prev), B, cout, hh, ww)
                elif split and acts.get(f"signs{si}") is not None:
                    self._call("ppo_impala_stack_tail_backward_signs_bf16x3", _p(g), _p(self._pk16[(si, 1)]), acts[f"signs{si}"],
                               _p(da1), _p(g1), _p(da0), _p(g0), B, cout, ho, wo)
                elif split:
                    self._call("ppo_impala_stack_tail_backward_bf16x3", _p(g), _p(self._pk16[(si, 1)]), masks, _p(da1), _p(g1),
                               _p(da0), _p(g0), B, cout, ho, wo)
                else:
                    self._call("ppo_impala_stack_tail_backward_f32", _p(g), tail_w, masks, _p(da1), _p(g1), _p(da0), _p(g0),
                               B, cout, ho, wo)
                wgrad_blocks(_block_wgrad_problems(si, maps, g, grads), B, cout, ho, wo)
                if full_w is not None:
                    wgrad(acts[f"in{si}"], IN_NONE, dc, fc, B, cin, cout, hh, ww)
                    g = g_prev
                    continue
                g = g0
            defer = WGRAD_BATCH_LAUNCH and sp.n_block * 2 <= 4
            problems = []
            for bi in (() if fused else reversed(range(sp.n_block))):
                base = f"encoder.stacks.{si}.blocks.{bi}"
                q_in, a = acts[f"q{si}_{bi}_in"], acts[f"a{si}_{bi}"]
                # g = d loss / d (block output);  block: out = q_in + conv1(relu(conv0(relu(q_in))))
                if defer:
                    problems.append((a, g, base + ".conv1"))
                else:
                    wgrad(a, IN_RELU, g, base + ".conv1", B, cout, cout, ho, wo)
                da = self._buf(f"g{si}_{bi}_da", (B, cout, ho, wo))
                self._call(self._bwd_data_fn(base + ".conv1"), _p(g), _p(self._bwd_w(base + ".conv1")), _p(a), None,
                           _p(da), B, cout, cout, ho, wo)
                if defer:
                    problems.append((q_in, da, base + ".conv0"))
                else:
                    wgrad(q_in, IN_RELU, da, base + ".conv0", B, cout, cout, ho, wo)
                gn = self._buf(f"g{si}_{bi}_in", (B, cout, ho, wo))
                self._call(self._bwd_data_fn(base + ".conv0"), _p(da), _p(self._bwd_w(base + ".conv0")), _p(q_in),
                           _p(g), _p(gn), B, cout, cout, ho, wo)
                g = gn
            if problems:
                wgrad_blocks(problems, B, cout, ho, wo)
            # max-pool backward, then the stack's first convolution
            x_in = acts[f"in{si}"]
            mode = IN_NONE if si > 0 else (self.u8_mode if x_in.dtype == torch.uint8 else IN_NONE)
            if sp.down_sample != "pool":
                # no max-pool: g is the gradient of the first convolution's output
                g_prev = self._buf(f"g{si - 1}_top", (B, cin, hh, ww)) if si > 0 else None
                if sp.down_sample == "stride":
                    nbytes = int(lib.ppo_conv3x3s2_any_wgrad_workspace_bytes(B, cin, cout, hh, ww))
                    ws = self._ws("wgrad_ws_" + fc, nbytes)
                    self._call("ppo_conv3x3s2_any_backward_weight_f32", _p(x_in), mode, _p(g), _p(self.grads[fc + ".weight"]),
                               _p(self.grads[fc + ".bias"]), _p(ws), nbytes, B, cin, cout, hh, ww, 0)
                    if si > 0:
                        self._call("ppo_conv3x3s2_any_backward_data_f32", _p(g), _p(self.params[fc + ".weight"]), None, None,
                                   _p(g_prev), B, cin, cout, hh, ww)
                else:
                    wgrad(x_in, mode, g, fc, B, cin, cout, hh, ww)
                    if si > 0:
                        self._call(self._bwd_data_fn(fc), _p(g), _p(self._bwd_w(fc)), None, None, _p(g_prev), B, cin, cout,
                                   hh, ww)
                g = g_prev
                continue
            if si == 0 and WGRAD_POOLED_DY and fc not in self._generic \
                    and lib.ppo_conv3x3_backward_weight_pooled_supported(cin, cout, hh, ww):
                # nothing else reads this stack's pre-pool gradient: the weight-gradient kernel forms it band by band
                wgrad(x_in, mode, g, fc, B, cin, cout, hh, ww, argmax=acts[f"idx{si}"])
                continue
            dc = self._buf(f"g{si}_dc", (B, cout, hh, ww))
            self._call("ppo_maxpool3x3s2_backward_f32", _p(g), _p(acts[f"idx{si}"]), _p(dc), B, cout, hh, ww)
            if self._first_wgrad_rides(si):
                carry.append((x_in, dc, fc, B, cin, hh, ww))
            else:
                wgrad(x_in, mode, dc, fc, B, cin, cout, hh, ww)
            if si > 0:
                g = self._buf(f"g{si - 1}_top", (B, cin, hh, ww))
                if self.split_bf16 and (fc, 1) in self._pk16:
                    self._call("ppo_conv3x3_bf16x3", _p(dc), 0, _p(self._pk16[(fc, 1)]), None, _p(g), B, cout, cin, hh, ww)
                else:
                    self._call(self._bwd_data_fn(fc), _p(dc), _p(self._bwd_w(fc)),
                               None, None, _p(g), B, cin, cout, hh, ww)
        flush_carry()
        if jobs:
            table = (_lib.WgradJob * len(jobs))(*jobs)
            self._call("ppo_conv3x3_wgrad_reduce_f32", ctypes.addressof(table), len(jobs))

    def _block_grads(self, acts, si, B):
        """What the backward-data pass of stack si's two residual blocks works on: the saved maps (p_in, a0, q0, a1), the
        host array of their addresses in processing order (each gradient is gated by the sign of the map its convolution
        read) and the gradient buffers (da1, g1, da0, g0) - per block, from the last, the gradient of the map between
        its convolutions and of its input."""
        _cin, cout, _h, _w, ho, wo = self.spec.stacks[si]
        shape = (B, cout, ho, wo)
        p_in, a0, q0, a1 = acts[f"q{si}_0_in"], acts[f"a{si}_0"], acts[f"q{si}_1_in"], acts[f"a{si}_1"]
        masks = (ctypes.c_void_p * 4)(a1.data_ptr(), q0.data_ptr(), a0.data_ptr(), p_in.data_ptr())
        return (p_in, a0, q0, a1), masks, (self._buf(f"g{si}_1_da", shape), self._buf(f"g{si}_1_in", shape),
                                           self._buf(f"g{si}_0_da", shape), self._buf(f"g{si}_0_in", shape))

    def _first_wgrad_rides(self, si) -> bool:
        """Whether the weight gradient of stack si's first convolution waits for stack si - 1's batched launch, as its
        fifth problem (WGRAD_RIDE): a c -> c convolution with a specialised kernel, on the geometry of that stack's four
        block convolutions.  (Its input is read raw: below the first stack no convolution reads uint8.)"""
        sp = self.spec
        if not (WGRAD_RIDE and WGRAD_BATCH_LAUNCH) or si < 1 or sp.n_block != 2 or sp.down_sample != "pool":
            return False
        cin, cout, hh, ww, _ho, _wo = sp.stacks[si]
        return cin == cout and f"encoder.stacks.{si}.firstconv" not in self._generic \
            and sp.stacks[si - 1][1] == cin and tuple(sp.stacks[si - 1][4:6]) == (hh, ww)

    def _stack_full_bwd_ptrs(self, si, cin, cout, h, w):
        """Host array of the five backward-data packed weights of stack si in processing order (block1.conv1,
        block1.conv0, block0.conv1, block0.conv0, firstconv), or None when the whole-stack kernel does not apply."""
        if not (FUSE_STACK_FULL_BWD and FUSE_STACK_TAIL) or self.spec.n_block != 2 or cin != cout \
                or not self.lib.ppo_impala_stack_full_supported(cout, h, w) or self.spec.down_sample != "pool":
            return None  # (the kernel reads the max-pool's argmax)
        return self._packed_ptrs(("full_bwd", si), _conv_names(si, reverse=True, firstconv=True), 1)

    def _stack_chain_bwd_ptrs(self, si, batch):
        """(the five backward-data packed weights of stack si, the four of stack si - 1's blocks) as host arrays in
        processing order, or None when ppo_impala_stack_chain_backward_f32 does not apply: exact float32 only, two blocks
        per stack, both stacks of one channel count at a geometry the whole-stack kernels have, and a batch that fills
        the chip (one workgroup per image)."""
        if si < 1 or self.split_bf16 or batch < FUSE_CHAIN_BWD_MIN_BATCH or self.spec.n_block != 2 \
                or self.spec.down_sample != "pool" \
                or not (FUSE_STACK_TAIL and FUSE_STACK_TAIL_BWD >> si & 1 and FUSE_STACK_TAIL_BWD >> (si - 1) & 1):
            return None
        cin, cout, h, w, _ho, _wo = self.spec.stacks[si]
        if cin != cout or self.spec.stacks[si - 1][1] != cin or tuple(self.spec.stacks[si - 1][4:6]) != (h, w) \
                or not self.lib.ppo_impala_stack_full_supported(cout, h, w):
            return None
        names = _conv_names(si, reverse=True, firstconv=True) + _conv_names(si - 1, reverse=True)
        return self._packed_ptrs(("chain_bwd", si), names, 1, split=5)

    def _stack_tail_bwd_ptrs(self, si, cout, ho, wo):
        """Host array of the four backward-data packed weights of stack si's blocks in processing order
        (block1.conv1, block1.conv0, block0.conv1, block0.conv0), or None when the fused kernel does not apply."""
        if not (FUSE_STACK_TAIL and FUSE_STACK_TAIL_BWD >> si & 1) or self.spec.n_block != 2 \
                or not self.lib.ppo_impala_stack_tail_supported(cout, ho, wo):
            return None
        return self._packed_ptrs(("bwd", si), _conv_names(si, reverse=True), 1)

    def _bwd_data_fn(self, wname):
        if wname in self._generic:
            return "ppo_conv3x3_any_backward_data_f32"
        return "ppo_conv3x3_backward_data_packed_f32" if (wname, 1) in self._pk else "ppo_conv3x3_backward_data_f32"

    def _bwd_w(self, wname):
        return self._pk.get((wname, 1), self.params[wname + ".weight"])

    # ------------------------------------------------------------------ minibatch losses + optimiser
    def takes_obs_index(self, obs) -> bool:
        """Whether a training minibatch can read its observations out of the whole batch through the permutation
        (ppo_conv3x3_pool_forward_packed_indexed_f32 + the indexed first-layer weight gradient) instead of from a
        gathered copy: uint8 images into the fused first convolution + max-pool, the pooled-gradient weight-gradient form.
        IMPALA only, and only where the first convolution has its specialised kernels (the generic ones take the gathered
        minibatch): the nature, rtg and mlp op-by-op paths take the gathered minibatch."""
        if self.encoder_kind != "impala" or self.batch_norm or "encoder.stacks.0.firstconv" in self._generic \
                or obs.dtype != torch.uint8 \
                or self.obs_norm is not None or not GATHER_IN_CONV or self.spec.down_sample != "pool":
            return False
        cin, cout, h, w, _ho, _wo = self.spec.stacks[0]
        return bool(FUSE_POOL_STACKS & 1) and self._pk.get(("encoder.stacks.0.firstconv", 0)) is not None \
            and bool(WGRAD_POOLED_DY) \
            and bool(self.lib.ppo_conv3x3_backward_weight_pooled_supported(cin, cout, h, w))

    @staticmethod
    def _minibatch_rows(prev_state, index, obs_indexed) -> int:
        """The number of samples of a training minibatch, after checking that prev_state is what obs_indexed says."""
        if obs_indexed:
            if index is None:
                raise ValueError("obs_indexed=True needs the index that prev_state is read through")
            return int(index.shape[0])
        B = int(prev_state.shape[0])
        if index is not None and int(index.shape[0]) != B:
            raise ValueError(f"prev_state holds {B} rows for a minibatch of {int(index.shape[0])}: pass the gathered "
                             "minibatch, or the array the index points into with obs_indexed=True")
        return B

    def _train_forward(self, prev_state, index=None, obs_indexed=False, tail=None):
        self._minibatch_rows(prev_state, index, obs_indexed)
        if obs_indexed and not self.takes_obs_index(prev_state):
            raise ValueError("this net needs the gathered minibatch of observations (takes_obs_index is False)")
        acts = self.encode(prev_state, train=True, index=index if obs_indexed else None, tail=tail)
        o = self.heads(acts, "t")
        B = o.shape[0]
        return acts, o, B, self._buf("dheads", (B, self.nh))

    def ppo_minibatch(self, prev_state, actions, old_log_pac, old_log_policy, advantages, returns,
                      eps_clip=0.2, ent_coef=0.01, vf_coef=0.5, loss_scale=1.0, index=None, stat_sums=None,
                      stat_accumulate=False, obs_indexed=False, side_target_logp=None, side_penalty=None):
        """Forward, fused PPO loss, backward: gradients of mean(-gain)*loss_scale land in self.grad
        (Runner.train_policy_minibatch, rl/rollout.py:1610-1771; discrete actions).  vf_coef = 0 (and
        returns None) leaves the value head out, as the dual architecture's policy phase does (:1744).
        The per-sample arrays are either minibatch-sized or, with ``index`` ([B] int32), whole-batch arrays read at
        index[b].  What prev_state holds is said by ``obs_indexed``, never inferred from its shape:
        False - exactly the minibatch's rows, in order (already gathered); ``index`` then applies to the per-sample
        arrays only, and a prev_state whose row count is not B raises ValueError.
        True - the array ``index`` points into: sample b is prev_state[index[b]] and B = len(index), whatever
        prev_state.shape[0] is (B included).  Needs ``index``, and a net that can read through it (takes_obs_index,
        or the fused MLP path without observation normalisation); anything else raises ValueError.
        Returns the per-sample statistics tensor [B, 8] (device).  MLP nets on the fused path (mlp_fused) also take
        ``stat_sums``, a device row that receives the column sums of the statistics.
        ``side_target_logp`` ([n_actions] float32 log-probabilities): SIDE (rl/rollout.py:1662-1679) - the entropy bonus
        becomes -ent_coef * (KL(new || target) - H); ``side_penalty`` ([B] float32, optional) receives that penalty per
        sample.  The loss then runs as a launch of its own (ppo_ppo_loss_side_f32), not on the dense + heads launch."""
        if side_target_logp is not None:
            self._check_policy_rows("side_target_logp", side_target_logp, None)
        elif side_penalty is not None:
            raise ValueError("side_penalty without side_target_logp")
        if self.mlp_fused:
            B = self._minibatch_rows(prev_state, index, obs_indexed)
            return self._mlp_train(
                _lib.MLP_LOSS_PPO, prev_state, index, self._buf("loss_stats", (B, 8)), 8, stat_sums, stat_accumulate,
                obs_indexed=obs_indexed, grad_scale=float(loss_scale) / B, n_actions=self.n_actions,
                n_value_heads=self.vh if returns is not None else 0,
                returns=_p(returns), vf_coef=float(vf_coef), actions_i=_p(actions), old_log_pac=_p(old_log_pac),
                old_log_policy=_p(old_log_policy), advantages=_p(advantages), eps_clip=float(eps_clip), ent_coef=float(ent_coef),
                side_target_logp=_p(side_target_logp), side_penalty=_p(side_penalty))
        B = self._minibatch_rows(prev_state, index, obs_indexed)
        stats = self._buf("loss_stats", (B, 8))
        vh = self.vh if returns is not None else 0
        loss_args = (self.n_actions, vh, _p(actions), _p(old_log_pac), _p(old_log_policy), _p(advantages), _p(returns),
                     float(eps_clip), float(ent_coef), float(vf_coef), float(loss_scale) / B,
                     _p(self._buf("dheads", (B, self.nh))), _p(stats), _p(index))
        # the loss rides on the dense + heads launch of the training forward where that launch exists (_dense_heads: image
        # encoders with relu; ppo_dense_heads_loss_forward_f32, bit-identical, one latency-bound launch less per minibatch)
        if side_target_logp is not None:
            acts, o, B, dheads = self._train_forward(prev_state, index, obs_indexed)
            self._call("ppo_ppo_loss_side_f32", _p(o), B, self.nh, *loss_args, _p(side_target_logp), _p(side_penalty))
            self.backward(acts, dheads)
            return stats
        acts, o, B, dheads = self._train_forward(prev_state, index, obs_indexed, tail=loss_args)
        if not acts["tail_taken"]:
            self._call("ppo_ppo_loss_f32", _p(o), B, self.nh, *loss_args)
        self.backward(acts, dheads)
        return stats

    def _check_policy_rows(self, name, t, rows):
        """A [rows, n_actions] (rows None: [n_actions]) contiguous float32 device array of a discrete policy."""
        if self.n_actions > 32:
            raise ValueError(f"{name}: discrete policies only (at most 32 actions, this net has {self.n_actions})")
        want = (self.n_actions,) if rows is None else (rows, self.n_actions)
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != want:
            raise ValueError(f"{name} must be a contiguous float32 {list(want)} tensor, got {t.dtype} {list(t.shape)}")

    def policy_kl_minibatch(self, prev_state, old_log_policy, penalty_scale, loss_scale=1.0, index=None, obs_indexed=False,
                            stat_sums=None, stat_accumulate=False):
        """The global KL pass (rl/rollout.py:1723-1738): training forward over a chunk of the global states, KL(new || old)
        per state against old_log_policy [B, n_actions] (row b belongs to state b of the chunk: ``index`` applies to
        prev_state alone), backward: the gradient of penalty_scale * loss_scale * sum_b kl_b lands in self.grad.  The
        caller folds the reference's divisor in: penalty_scale = penalty / (S * n_actions) for a sample of S states.
        prev_state, ``index`` and ``obs_indexed`` as in ppo_minibatch.  Returns kl_b [B, 1] (device); MLP nets on the
        fused path also take ``stat_sums``, a one-element device row that receives (or is added) their sum."""
        B = self._minibatch_rows(prev_state, index, obs_indexed)
        self._check_policy_rows("old_log_policy", old_log_policy, B)
        scale = float(penalty_scale) * float(loss_scale)
        kl = self._buf("kl_rows", (B, 1))
        if self.mlp_fused:
            return self._mlp_train(_lib.MLP_LOSS_POLICY_KL, prev_state, index, kl, 1, stat_sums, stat_accumulate,
                                   obs_indexed=obs_indexed, grad_scale=scale, n_actions=self.n_actions,
                                   old_log_policy=_p(old_log_policy))
        acts, o, B, dheads = self._train_forward(prev_state, index, obs_indexed)
        self._call("ppo_policy_kl_loss_f32", _p(o), B, self.nh, self.n_actions, _p(old_log_policy), scale, _p(dheads), _p(kl))
        self.backward(acts, dheads)
        return kl

    def policy_kl_rows(self, prev_state, old_log_policy, index=None, obs_indexed=False):
        """kl_b [B, 1] of policy_kl_minibatch without its backward pass (--gkl_penalty=0: the statistic alone); self.grad
        and the optimiser's sums of g^2 stay as they are."""
        B = self._minibatch_rows(prev_state, index, obs_indexed)
        self._check_policy_rows("old_log_policy", old_log_policy, B)
        kl = self._buf("kl_rows", (B, 1))
        if self.mlp_fused:
            x = prev_state
            if x.dtype != torch.float32 or not x.is_contiguous():
                raise ValueError("the mlp encoder takes contiguous float32 observations")
            if self.obs_norm is not None:  # as _mlp_train
                if obs_indexed:
                    raise ValueError("observation normalisation needs the gathered minibatch")
                xn = self._buf("txn", tuple(x.shape))
                self._call("ppo_obs_normalize_f32", _p(x), 0, _p(self.obs_norm.mu), _p(self.obs_norm.std),
                           self.obs_norm.norm_eps, _p(xn), x.shape[0], self.obs_norm.F)
                x = xn
            o = self._buf("klheads", (B, self.nh))
            self._call("ppo_mlp_forward_f32", _p(x), ctypes.addressof(self._mlp_net), _p(index) if obs_indexed else None,
                       B, _p(o), None, None)
        else:
            _acts, o, B, _dheads = self._train_forward(prev_state, index, obs_indexed)
        self._call("ppo_policy_kl_loss_f32", _p(o), B, self.nh, self.n_actions, _p(old_log_policy), 0.0,
                   _p(self._buf("kl_dheads", (B, self.nh))), _p(kl))
        return kl

    def gaussian_minibatch(self, prev_state, actions, old_log_pac, advantages, returns, eps_clip=0.2, vf_coef=0.5,
                           loss_scale=1.0, index=None, stat_sums=None, stat_accumulate=False, obs_indexed=False):
        """As ppo_minibatch for gaussian policies (rl/rollout.py:1693-1704); also fills log_std's gradient.
        prev_state, ``index`` and ``obs_indexed`` as in ppo_minibatch."""
        if self.mlp_fused:
            B = self._minibatch_rows(prev_state, index, obs_indexed)
            return self._mlp_train(
                _lib.MLP_LOSS_GAUSSIAN, prev_state, index, self._buf("loss_stats", (B, 8)), 8, stat_sums, stat_accumulate,
                obs_indexed=obs_indexed, grad_scale=float(loss_scale) / B, n_actions=self.n_actions,
                n_value_heads=self.vh if returns is not None else 0,
                returns=_p(returns), vf_coef=float(vf_coef), actions_f=_p(actions), old_log_pac=_p(old_log_pac),
                advantages=_p(advantages), log_std=_p(self.params["log_std"]), eps_clip=float(eps_clip),
                dlog_std_rows=_p(self._buf("dlog_std_rows", (B, self.n_actions))))
        acts, o, B, dheads = self._train_forward(prev_state, index, obs_indexed)
        stats = self._buf("loss_stats", (B, 8))
        rows = self._buf("dlog_std_rows", (B, self.n_actions))
        vh = self.vh if returns is not None else 0
        self._call("ppo_gaussian_loss_f32", _p(o), B, self.nh, self.n_actions, vh, _p(actions), _p(old_log_pac),
                   _p(advantages), _p(returns), _p(self.params["log_std"]), float(eps_clip), float(vf_coef),
                   float(loss_scale) / B, _p(dheads), _p(rows), _p(stats), _p(index))
        # log_std's gradient first: it sits in the early data-parallel bucket, which leaves during the backward pass
        self._call("ppo_colsum_f32", _p(rows), B, self.n_actions, self.n_actions, _p(self.grads["log_std"]), 0)
        self.backward(acts, dheads)
        return stats

    def value_minibatch(self, prev_state, returns=None, tvf_returns=None, tvf_weights=None, vf_coef=0.5,
                        tvf_coef=1.0, loss_scale=1.0, index=None, tvf_keep_prob=1.0, dropout_seed=0, dropout_offset=0,
                        stat_sums=None, stat_accumulate=False, obs_indexed=False):
        """Value phase (Runner.train_value_minibatch, rl/rollout.py:1513-1567; TVF loss rl/tvf.py:32-77, with
        horizon dropout when tvf_keep_prob < 1: :64-69).  prev_state, ``index`` and ``obs_indexed`` as in
        ppo_minibatch."""
        if self.mlp_fused:
            B = self._minibatch_rows(prev_state, index, obs_indexed)
            return self._mlp_train(
                _lib.MLP_LOSS_VALUE, prev_state, index, self._buf("value_stats", (B, 4)), 4, stat_sums, stat_accumulate,
                obs_indexed=obs_indexed, grad_scale=float(loss_scale) / B, value_col=self.col_value,
                n_value_heads=self.vh if returns is not None else 0,
                returns=_p(returns), vf_coef=float(vf_coef), tvf_col=self.col_tvf if self.K else 0,
                n_tvf=self.K if tvf_returns is not None else 0, tvf_stride=max(self.vh, 1), tvf_returns=_p(tvf_returns),
                tvf_weights=_p(tvf_weights), tvf_coef=float(tvf_coef), tvf_keep_prob=float(tvf_keep_prob),
                seed=int(dropout_seed) & (2**64 - 1), offset=int(dropout_offset) & (2**64 - 1))
        acts, o, B, dheads = self._train_forward(prev_state, index, obs_indexed)
        stats = self._buf("value_stats", (B, 4))
        self._call("ppo_value_loss_f32", _p(o), B, self.nh, self.col_value, self.vh if returns is not None else 0,
                   _p(returns), float(vf_coef), self.col_tvf if self.K else 0, self.K if tvf_returns is not None else 0,
                   max(self.vh, 1), _p(tvf_returns), _p(tvf_weights), float(tvf_coef), float(loss_scale) / B, _p(dheads),
                   _p(stats), _p(index), float(tvf_keep_prob), int(dropout_seed) & (2**64 - 1),
                   int(dropout_offset) & (2**64 - 1))
        self.backward(acts, dheads)
        return stats

    def distil_minibatch(self, prev_state, targets, old_policy, beta=1.0, use_tvf=False, weights=None, gaussian=False,
                         loss_scale=1.0, index=None, stat_sums=None, stat_accumulate=False, obs_indexed=False,
                         policy_loss="kl_policy", value_loss="mse", delta=0.0, l1_scale=0.0, pred_actions=None,
                         head_subset=None):
        """Distillation phase (Runner.train_distil_minibatch, rl/rollout.py:1331-1449): targets [*] against the
        ext value head, or [*, K] against the TVF heads' ext column (use_tvf).  prev_state, ``index`` and
        ``obs_indexed`` as in ppo_minibatch.  policy_loss / value_loss (+ delta, l1_scale): --distil_loss /
        --distil_value_loss by name; pred_actions [*] int32: the prediction is the advantage head's entry for that
        action (targets "return" / "advantage", :1364-1368); head_subset: the TVF heads that take part
        (--distil_max_heads), ``weights`` then being w_k on them and 0 elsewhere."""
        col, n_pred, stride = (self.col_tvf, self.K, self.vh) if use_tvf else (self.col_value, 1, 1)
        if pred_actions is not None:
            if use_tvf:
                raise ValueError("pred_actions: a scalar target against the advantage head, not the TVF heads")
            if pred_actions.dtype != torch.int32 or not pred_actions.is_contiguous():
                raise ValueError("pred_actions must be contiguous int32")
            col = self.col_advantage
        n_active = 0
        if head_subset is not None:
            if not use_tvf or weights is None:
                raise ValueError("head_subset: a subset of the TVF heads, with their weights")
            n_active = len(head_subset)
        try:
            pl, vl = _lib.DISTIL_POLICY_LOSSES[policy_loss], _lib.DISTIL_VALUE_LOSSES[value_loss]
        except KeyError as e:
            raise ValueError(f"Invalid distil loss {e.args[0]}") from None
        if self.mlp_fused:
            B = self._minibatch_rows(prev_state, index, obs_indexed)
            return self._mlp_train(
                _lib.MLP_LOSS_DISTIL, prev_state, index, self._buf("distil_stats", (B, 4)), 4, stat_sums, stat_accumulate,
                obs_indexed=obs_indexed, grad_scale=float(loss_scale) / B, n_actions=self.n_actions, pred_col=col,
                n_pred=n_pred, pred_stride=stride,
                vector_targets=1 if use_tvf else 0, targets=_p(targets), weights=_p(weights), old_policy=_p(old_policy),
                log_std=_p(self.params["log_std"]) if gaussian else None, beta=float(beta),
                distil_policy_loss=pl, distil_value_loss=vl, distil_delta=float(delta), distil_l1_scale=float(l1_scale),
                pred_actions=_p(pred_actions), n_active=n_active)
        acts, o, B, dheads = self._train_forward(prev_state, index, obs_indexed)
        stats = self._buf("distil_stats", (B, 4))
        self._call("ppo_distil_loss_modes_f32", _p(o), B, self.nh, self.n_actions, col, n_pred, stride, 1 if use_tvf else 0,
                   _p(targets), _p(weights), _p(old_policy), _p(self.params["log_std"]) if gaussian else None,
                   float(beta), float(loss_scale) / B, _p(dheads), _p(stats), _p(index), pl, vl, float(delta),
                   float(l1_scale), _p(pred_actions), n_active)
        self.backward(acts, dheads)
        return stats

    def last_dheads(self, B):
        """d loss / d heads [B, nh] of the last training minibatch (a view of scratch memory, for tests and diagnostics):
        the fused MLP path keeps it at the end of its workspace, the op-by-op path in its own buffer."""
        if self.mlp_fused:
            ws = self._buf("mlp_ws", (int(self.lib.ppo_mlp_train_workspace_floats(B, self.spec.in_features, self.hidden_units,
                                                                                   self.nh)),))
            return ws[4 * B * self.hidden_units:4 * B * self.hidden_units + B * self.nh].view(B, self.nh)
        return self._buf("dheads", (B, self.nh))

    def zero_untouched_grads(self):
        """log_std only receives gradient from the gaussian policy loss; every other parameter is overwritten
        by each backward.  Called by phases that do not touch log_std so a stale gradient never leaks."""
        self.grads["log_std"].zero_()

    def adam_step(self, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=20.0, grad_div=1.0,
                  grad_norm_out: Optional[torch.Tensor] = None, state: Optional["AdamState"] = None):
        """clip_grad_norm_ + torch.optim.Adam.step over the flat buffer (rl/rollout.py:1287-1321).
        `state`: a separate set of Adam moments over the same parameters (the reference's distil optimiser,
        rl/rollout.py:136-141); default is the net's own."""
        ws = self._ws("adam_ws", self.lib.ppo_adam_workspace_bytes())
        scatter = self._scatter_table() if ADAM_SCATTER else None
        if scatter is None:
            self.mark_weights_changed()
        elif self._packed_dirty:
            self._refresh_packed()  # weights written by hand since the last step: start from a consistent packed copy
        if state is not None:
            state.ensure(self.flat)
            state.step += 1
            m, v, step = state.exp_avg, state.exp_avg_sq, state.step
        else:
            if self.exp_avg is None:
                self.exp_avg = torch.zeros_like(self.flat)
                self.exp_avg_sq = torch.zeros_like(self.flat)
            self._adam_step += 1
            m, v, step = self.exp_avg, self.exp_avg_sq, self._adam_step
        n_part, self._presummed = self._presummed, 0
        args = (_p(self.flat), _p(self.grad), _p(m), _p(v), self.flat.numel(), step, float(lr), float(beta1), float(beta2),
                float(eps), float(max_grad_norm), float(grad_div), _p(ws))
        if n_part and scatter is None and grad_div == 1.0:
            # the launch that wrote the gradients left the per-workgroup sums of g^2 in the workspace (fused MLP path)
            self._call("ppo_adam_step_presummed_f32", *args, n_part, _p(grad_norm_out))
        elif scatter is not None:
            # the step also refreshes the convolution kernels' packed operands: no re-pack launch before the next forward
            self._call("ppo_adam_step_scatter_f32", *args, _p(grad_norm_out), _p(scatter[0]), scatter[1], _p(self._packed))
        else:
            self._call("ppo_adam_step_f32", *args, _p(grad_norm_out))
        self.mask_feature_weights()

    def sgd_step(self, lr=2.5e-4, max_grad_norm=20.0, grad_div=1.0, grad_norm_out: Optional[torch.Tensor] = None):
        """clip_grad_norm_ + torch.optim.SGD.step (no momentum, weight decay or dampening) over the flat buffer
        (rl/rollout.py:137-138, :1287-1321).  Everything adam_step does around its launch, without moments or a step
        count.  There is no scatter form: under PPO_AMD_ADAM_SCATTER too the weights are marked changed and the ordinary
        re-pack follows before the next forward."""
        ws = self._ws("adam_ws", self.lib.ppo_adam_workspace_bytes())
        self.mark_weights_changed()
        n_part, self._presummed = self._presummed, 0
        args = (_p(self.flat), _p(self.grad), self.flat.numel(), float(lr), float(max_grad_norm), float(grad_div))
        if n_part and grad_div == 1.0:
            # the launch that wrote the gradients left the per-workgroup sums of g^2 in the workspace (fused MLP path)
            self._call("ppo_sgd_step_presummed_f32", *args, _p(ws), n_part, _p(grad_norm_out))
        else:
            self._call("ppo_sgd_step_f32", *args, _p(ws), _p(grad_norm_out))
        self.mask_feature_weights()

    # ------------------------------------------------------------------ optimiser state (checkpoints)
    def parameter_order(self):
        """Parameter names in the order of the reference module's `.parameters()` (= its state_dict order): the
        integer keys of torch.optim.Adam.state_dict()['state'] index this list."""
        return [n for n in self.state_dict().keys() if n not in self.buffers]  # (buffers are no parameters)

    def parameter_count(self):
        return len(self.parameter_order())

    def adam_state_dict(self, exp_avg, exp_avg_sq, step, cfg=None):
        """The layout of `torch.optim.Adam(net.parameters()).state_dict()` — what the reference stores per optimiser
        (rl/rollout.py:412-421): {'state': {i: {'step': f32 scalar tensor, 'exp_avg', 'exp_avg_sq'}}, 'param_groups':
        [{'lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'foreach', 'capturable', 'params': [0..n)}]},
        i = index into `parameter_order()`.  torch creates a parameter's entry at the first step that sees a gradient
        for it, so parameters whose gradient was never non-zero (the reference leaves them at grad=None) have none."""
        names = self.parameter_order()
        state = {}
        if exp_avg is not None and step > 0:
            touched = {}
            for i, name in enumerate(names):
                o, shape = self._offsets[name]
                n = int(np.prod(shape))
                touched[i] = (exp_avg_sq[o:o + n], exp_avg[o:o + n], shape)
            flags = torch.stack([(v != 0).any() | (m != 0).any() for v, m, _ in touched.values()]).cpu().tolist()
            for (i, (v, m, shape)), hit in zip(touched.items(), flags):
                if hit:
                    state[i] = {"step": torch.tensor(float(step), dtype=torch.float32),
                                "exp_avg": m.view(shape).clone(), "exp_avg_sq": v.view(shape).clone()}
        group = {"lr": float(cfg.lr) if cfg is not None else 0.0,
                 "betas": (float(cfg.adam_beta1), float(cfg.adam_beta2)) if cfg is not None else (0.9, 0.999),
                 "eps": float(cfg.adam_epsilon) if cfg is not None else 1e-8, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "params": list(range(len(names)))}
        return {"state": state, "param_groups": [group]}

    def read_adam_state_dict(self, sd):
        """(exp_avg, exp_avg_sq, step) flat buffers from a torch.optim.Adam-layout dict (see adam_state_dict) or from
        the two layouts earlier versions of this package wrote (name-keyed per-parameter moments; whole flat buffers).
        (None, None, 0) when the optimiser had not stepped."""
        if "flat" in sd:  # round <= 2: separate flat state of the distil optimiser
            return (sd["flat"]["exp_avg"].to(self.device).clone(), sd["flat"]["exp_avg_sq"].to(self.device).clone(),
                    int(sd["step"]))
        state = sd.get("state") or {}
        if not state:
            return None, None, int(sd.get("step", 0)) if not isinstance(sd.get("step"), torch.Tensor) else 0
        names = self.parameter_order()
        m, v, step = torch.zeros_like(self.flat), torch.zeros_like(self.flat), int(sd.get("step", 0) or 0)
        for key, st in state.items():
            name = names[int(key)] if not isinstance(key, str) or key.isdigit() else key
            o, shape = self._offsets[name]
            n = int(np.prod(shape))
            m[o:o + n].copy_(torch.as_tensor(st["exp_avg"]).reshape(-1))
            v[o:o + n].copy_(torch.as_tensor(st["exp_avg_sq"]).reshape(-1))
            if "step" in st:
                step = max(step, int(float(st["step"])))
        return m, v, step

    def optimizer_state_dict(self, cfg=None):
        return self.adam_state_dict(self.exp_avg, self.exp_avg_sq, self._adam_step, cfg)

    def load_optimizer_state_dict(self, sd):
        self.exp_avg, self.exp_avg_sq, self._adam_step = self.read_adam_state_dict(sd)


class TVFModel:
    """Host mirror of the reference's TVFModel (rl/models.py:511-856): owns `policy_net` and `value_net`
    (the same object for `architecture='single'`, two nets for 'dual'), exposes
    `forward(x, output=..., policy_temperature=...) -> dict` with the reference's routing and key aliasing
    (:790-821) and a `state_dict` with the reference's `policy_net.` / `value_net.` prefixes.  With `use_rnd` it also owns
    `prediction_net` / `target_net` (ppo_amd/rnd.py; `rnd_prediction_error`, `forward(include_rnd=True)`, two more
    `state_dict` prefixes); without it nothing of that exists."""

    def __init__(self, encoder: str, encoder_args=None, input_dims=(4, 84, 84), actions: int = 6, device="cuda",
                 architecture: str = "dual", dtype=torch.float32, use_rnd: bool = False, hidden_units: int = 512,
                 encoder_activation_fn: str = "relu", observation_normalization=False,
                 freeze_observation_normalization=False, tvf_fixed_head_horizons=None, tvf_fixed_head_weights=None,
                 tvf_feature_sparsity: float = 0.0, tvf_feature_window: int = -1, head_scale: float = 1.0,
                 value_head_names=("ext",), norm_eps: float = 1e-5, head_bias: bool = False,
                 observation_scaling: str = "scaled", precision: str = "high"):
        if architecture not in ("single", "dual"):
            raise Exception("Invalid architecture, use [dual|single]")
        if use_rnd:
            assert 'int' in value_head_names, "RND requires int value head."  # rl/models.py:585
            assert observation_normalization, "rnd requires observation normalization."  # rl/models.py:620
            if tvf_fixed_head_horizons is not None:
                raise NotImplementedError("RND together with TVF heads is not built (the reference trains TVF on 'ext' only)")
        if dtype != torch.float32:
            raise ValueError("the reference path is float32 (rl/models.py:31-32)")
        self.observation_scaling = check_observation_scaling(observation_scaling)
        if isinstance(encoder_args, str):
            import ast
            encoder_args = ast.literal_eval(encoder_args)
        self.input_dims = tuple(input_dims)
        self.actions = actions
        self.dtype = dtype
        self.architecture = architecture
        self.encoder_name = encoder
        self.tvf_fixed_head_horizons = tvf_fixed_head_horizons
        self.tvf_fixed_head_weights = tvf_fixed_head_weights
        if architecture == "single":
            self.name = "PPO-" + encoder
        else:
            self.name = ("TVF-" if tvf_fixed_head_horizons is not None else "DNA-") + encoder

        def make_net():
            return DualHeadNet(encoder, input_dims, actions, hidden_units=hidden_units,
                               activation_fn=encoder_activation_fn, tvf_fixed_head_horizons=tvf_fixed_head_horizons,
                               tvf_feature_sparsity=tvf_feature_sparsity, tvf_feature_window=tvf_feature_window,
                               head_scale=head_scale, value_head_names=value_head_names, head_bias=head_bias,
                               device=device, precision=precision, observation_scaling=observation_scaling,
                               **(encoder_args or {}))

        self.policy_net = make_net()
        self.value_net = make_net() if architecture == "dual" else self.policy_net
        self.device = self.policy_net.device
        self.observation_normalization = bool(observation_normalization)
        self.obs_norm = None
        if self.observation_normalization:
            self.obs_norm = ObsNormalizer(self.input_dims, self.device, norm_eps=norm_eps,
                                          frozen=freeze_observation_normalization, observation_scaling=observation_scaling)
            self.policy_net.obs_norm = self.value_net.obs_norm = self.obs_norm
        self.use_rnd = bool(use_rnd)
        self.rnd = None
        if self.use_rnd:
            # drawn after policy_net / value_net, as the reference's constructor does (rl/models.py:619-622)
            self.rnd = RNDNets(self.input_dims, self.obs_norm, self.device)
            self.prediction_net, self.target_net = self.rnd.prediction_net, self.rnd.target_net

    def train(self, mode: bool = True):
        """nn.Module.train for both nets (rl/rollout.py:712).  Only batch-norm nets read the flag (DualHeadNet.training)."""
        self.policy_net.train(mode)
        self.value_net.train(mode)
        return self

    def eval(self):
        return self.train(False)

    @property
    def batch_norm(self) -> bool:
        return self.policy_net.batch_norm

    def model_size(self, trainable_only: bool = True):
        n = self.policy_net.n_parameters()
        return n if self.architecture == "single" else n + self.value_net.n_parameters()

    def prep_for_model(self, x):
        """rl/models.py:824-856: accept ndarray or tensor, uint8 or float; the scaling itself (`observation_scaling`:
        x/255, x/255 - 0.5 or (x/255 - 0.5) * 6) is fused into the load of the kernels that read the bytes - the first
        convolution, the normaliser, the RND input, the hash input.  Float input is used as it is."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        if x.dtype not in (torch.uint8, torch.float32):
            raise AssertionError("Invalid dtype {}".format(x.dtype))
        if tuple(x.shape[1:]) != self.input_dims:
            raise AssertionError("Invalid dims, expected {} but found {}".format((None, *self.input_dims), tuple(x.shape)))
        return x.to(self.device, non_blocking=True).contiguous()

    def forward(self, x, output: str = "default", policy_temperature: float = 1.0, include_rnd=False,
                include_features=False, update_normalization=False, **kwargs):
        assert output in ["default", "full", "policy", "value"]
        x = self.prep_for_model(x)
        if update_normalization and self.obs_norm is not None:
            self.obs_norm.update(x)
        net_args = dict(policy_temperature=policy_temperature, include_features=include_features, **kwargs)
        if include_rnd:
            rnd_error = self.rnd_prediction_error(x)  # rl/models.py:786-787

        def public(d):
            return {k: (v.clone() if self.architecture == "dual" else v) for k, v in d.items() if not k.startswith("_")}

        result = {"rnd_error": rnd_error} if include_rnd else {}
        if self.architecture == "single":
            for k, v in public(self.policy_net.forward(x, **net_args)).items():
                result["policy_" + k] = v
                result["value_" + k] = v
                result[k] = v
            return result
        # dual: head rows live in per-net scratch that the next forward of that net reuses, so results are
        # cloned (small [B, heads] tensors)
        if output == "full":
            for k, v in public(self.policy_net.forward(x, **net_args)).items():
                result["policy_" + k] = v
            for k, v in public(self.value_net.forward(x, **net_args)).items():
                result["value_" + k] = v
            return result
        if output in ("default", "policy"):
            result.update(public(self.policy_net.forward(x, **net_args, exclude_value=output == "default")))
        if output in ("default", "value"):
            result.update(public(self.value_net.forward(x, **net_args, exclude_policy=output == "default")))
        return result

    __call__ = forward

    def log_policy(self, x):
        return self.forward(x, output="policy")["log_policy"].detach().cpu().numpy()

    @property
    def obs_rms(self):
        """The reference's `model.obs_rms` (utils.RunningMeanStd) as host arrays: mean / var [*input_dims] float64
        and the scalar count."""
        import types
        n = self.obs_norm
        return types.SimpleNamespace(mean=n.mean.cpu().numpy().reshape(self.input_dims),
                                     var=n.var.cpu().numpy().reshape(self.input_dims), count=n.count)

    def perform_normalization(self, x, update_normalization: bool = False):
        """rl/models.py:666-694 on a prepared batch; returns the normalised float32 tensor."""
        x = self.prep_for_model(x)
        if update_normalization:
            self.obs_norm.update(x)
        return self.obs_norm.apply(x, torch.empty(x.shape, dtype=torch.float32, device=self.device))

    def rnd_prediction_error(self, x, already_normed=False):
        """rl/models.py:712-738: the prediction error [B] (device) of observations - ndarray or tensor, uint8 or float32;
        with `already_normed` the float32 output of `perform_normalization`, whose last channel is read as it is."""
        if not self.use_rnd:
            raise _lib.PpoAmdError("rnd_prediction_error needs TVFModel(use_rnd=True)")
        if already_normed:
            x = torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous()
            return self.rnd.prediction_error(x, already_normed=True)
        return self.rnd.prediction_error(self.prep_for_model(x))

    def adjust_value_scale(self, factor: float, process_value=True, process_tvf=True, value_net_only=False):
        """rl/models.py:630-651: scale value predictions by scaling the value / TVF head weights and biases."""
        nets = [self.value_net] if value_net_only else ([self.policy_net] if self.architecture == "single" else
                                                        [self.policy_net, self.value_net])
        for net in nets:
            names = (["value_head"] if process_value else []) + (["tvf_head"] if process_tvf and net.use_tvf else [])
            for n in names:
                net.params[n + ".weight"].mul_(factor)
                if net.head_bias:
                    net.params[n + ".bias"].mul_(factor)

    def state_dict(self):
        sd = OrderedDict()
        for prefix, net in (("policy_net.", self.policy_net), ("value_net.", self.value_net)):
            for k, v in net.state_dict().items():
                sd[prefix + k] = v
        if self.use_rnd:
            for prefix, net in (("prediction_net.", self.prediction_net), ("target_net.", self.target_net)):
                for k, v in net.state_dict().items():
                    sd[prefix + k] = v
        return sd

    def load_state_dict(self, sd, strict=True):
        pol = {k[len("policy_net."):]: v for k, v in sd.items() if k.startswith("policy_net.")}
        self.policy_net.load_state_dict(pol, strict=strict)
        if self.architecture == "dual":
            val = {k[len("value_net."):]: v for k, v in sd.items() if k.startswith("value_net.")}
            self.value_net.load_state_dict(val, strict=strict)
        if self.use_rnd:
            for prefix, net in (("prediction_net.", self.prediction_net), ("target_net.", self.target_net)):
                net.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=strict)
