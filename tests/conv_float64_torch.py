"""Test helper (no test in here): the exact-float32 3x3 / stride 1 / padding 1 convolutions of csrc/conv3x3.hip and
csrc/conv3x3_wgrad.hip - forward, backward-data, weight gradient, forward fused with the max-pool - as plain torch
contractions in float64, with the magnitude map `A` of every output element (the same contraction on absolute values,
plus |bias|, |residual|, |dres|), and two comparison evaluations of the same contraction on the CPU: plain float32, and
an emulated split (each operand as bf16 hi + lo, keeping hi.hi + hi.lo + lo.hi) that stands in for "a reduced-precision
path was taken".

Also the cases at which tests/test_conv_float64_gpu.py calls the kernels and tests/test_conv_float64_cpu.py checks the
input conditions: the 14 geometries of dispatch_conv, the modes each entry point admits there, the data sets, the batch
sizes that wrap the persistent item loops, and the per-element bar.

A case is (ck, cm, h, w) as dispatch_conv sees it: ck channels are contracted over, cm are produced.  For the forward,
the fused pool and the weight gradient that is (cin, cout); backward-data contracts over the forward's output channels,
so its case (ck, cm) is the entry point's (cin = cm, cout = ck)."""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

NONE, RELU, U8 = 0, 1, 2  # PPO_IN_* (include/ppo_amd.h)
U = 2.0 ** -24            # unit roundoff of float32

CASES = [(4, 16, 84, 84), (5, 16, 84, 84), (3, 16, 64, 64), (4, 16, 64, 64), (16, 32, 42, 42), (16, 32, 32, 32),
         (32, 16, 42, 42), (32, 16, 32, 32), (16, 16, 42, 42), (16, 16, 32, 32), (32, 32, 21, 21), (32, 32, 16, 16),
         (32, 32, 11, 11), (32, 32, 8, 8)]
DATA_SETS = ("plain", "ranged")

# Per map side, the constants the wrapping batch sizes follow from.  They restate, and must be kept in step with:
#   conv  (TR, NW): PPO_CONV_CASE(.., TR, MT, NW) in dispatch_conv, csrc/conv3x3.hip - rows per band, waves per workgroup;
#                   launch_conv_impl starts min(256 * min(occupancy, 24 / NW), n * NBANDS) workgroups
#   pool  PR:       PPO_CP_CASE(.., PR, MT, NW) in dispatch_conv_pool, csrc/conv3x3.hip - pooled rows per band;
#                   launch_conv_pool_impl starts min(256 * min(occupancy, 3), n * NBANDS) workgroups
#   wgrad TR:       PPO_WGRAD_CASE(.., TR) in dispatch_wgrad, csrc/conv3x3_wgrad.hip - rows per band; launch_wgrad starts
#                   min(256 * PPO_TUNE_WGRAD_PERCU, kWgradMaxSlabs, n * NBANDS) <= 512 workgroups, one slab each
TILING = {
    #side  conv (TR, NW)   pool PR   wgrad TR
    84: dict(conv=(12, 8), pool=3, wgrad=6),
    64: dict(conv=(16, 8), pool=4, wgrad=8),
    42: dict(conv=(6, 8), pool=4, wgrad=7),
    32: dict(conv=(8, 8), pool=4, wgrad=8),
    21: dict(conv=(6, 4), pool=6, wgrad=7),
    16: dict(conv=(8, 4), pool=8, wgrad=8),
    11: dict(conv=(11, 4), pool=None, wgrad=11),
    8: dict(conv=(8, 4), pool=None, wgrad=8),
}
CONV_MAX_WG_PER_CU_WAVES = 24  # launch_conv_impl: at most 24 / NW workgroups per CU
POOL_MAX_WG_PER_CU = 3         # launch_conv_pool_impl
WGRAD_MAX_GRID = 512           # 256 * PPO_TUNE_WGRAD_PERCU = kWgradMaxSlabs
N_CUS = 256


def case_id(case):
    return "x".join(str(v) for v in case)


def nbands(op, side):
    """Bands (items per image) of the kernel family `op` in "conv" | "pool" | "wgrad" on a side x side map."""
    t = TILING[side]
    if op == "conv":
        return -(-side // t["conv"][0])
    if op == "pool":
        return -(-((side + 1) // 2) // t["pool"])
    return -(-side // t["wgrad"])


def wrapping_n(op, side):
    """The smallest batch at which the persistent loop of `op` must wrap: more items than the largest grid the launch
    can start - whatever occupancy the runtime reports - and, for the double-buffered conv / pool loops, a number of
    items that is no multiple of 256, so that the last pass is a partial one at every grid the launch can choose."""
    nb = nbands(op, side)
    if op == "wgrad":
        return WGRAD_MAX_GRID // nb + 1
    cap = N_CUS * (CONV_MAX_WG_PER_CU_WAVES // TILING[side]["conv"][1] if op == "conv" else POOL_MAX_WG_PER_CU)
    n = cap // nb + 1
    while (n * nb) % N_CUS == 0:
        n += 1
    return n


def first_layer(case):
    return case[0] <= 5


def table(case):
    """What dispatch_conv / dispatch_conv_pool / dispatch_wgrad admit at a case, read off their case lists."""
    ck, cm, h, w = case
    if first_layer(case):
        return dict(forward=(NONE, U8), backward_data=False, backward_weight=(NONE, U8), pool=(NONE, U8))
    if ck < cm:    # the channel-changing stack-first convolution
        return dict(forward=(NONE,), backward_data=False, backward_weight=(NONE,), pool=(NONE,))
    if ck > cm:    # its backward-data
        return dict(forward=(), backward_data=True, backward_weight=(), pool=())
    first_of_stack = ck == 32 and h in (21, 16)
    return dict(forward=(NONE, RELU), backward_data=True, backward_weight=(NONE, RELU) if first_of_stack else (RELU,),
                pool=(NONE,) if first_of_stack else ())


def probed(lib, case):
    ck, cm, h, w = case
    modes = (NONE, RELU, U8)
    return dict(forward=tuple(m for m in modes if lib.ppo_conv3x3_forward_supported(m, ck, cm, h, w)),
                backward_data=bool(lib.ppo_conv3x3_backward_data_supported(cm, ck, h, w)),
                backward_weight=tuple(m for m in modes if lib.ppo_conv3x3_backward_weight_supported(m, ck, cm, h, w)),
                pool=tuple(m for m in modes if lib.ppo_conv3x3_pool_forward_supported(m, ck, cm, h, w)))


@functools.lru_cache(maxsize=None)
def admitted(case):
    """dict(forward: modes, backward_data: bool, backward_weight: modes, pool: modes) - from the library's probes (host
    functions: no GPU needed) where it loads, from the table otherwise; tests/test_conv_float64_cpu.py holds one to the
    other."""
    try:
        from ppo_amd import _lib
        return probed(_lib.load(), case)
    except Exception:  # not built on this host
        return table(case)


# ------------------------------------------------------------------------------------------------------- the data sets
def _gen(case, n, data, op):
    return torch.Generator().manual_seed(zlib.crc32(repr((case, n, data, op)).encode()) % (1 << 31))


def _pow2(count, g):
    return torch.exp2(torch.randint(-12, 13, (count,), generator=g).float())


def _sparse(t, g, signed_zero):
    """About 30 % exact zeros; with signed_zero a third of them are -0.0."""
    r = torch.rand(t.shape, generator=g)
    t = torch.where(r < 0.3, torch.zeros_like(t), t)
    if signed_zero:
        t = torch.where(r < 0.1, torch.full_like(t, -0.0), t)
    return t


@functools.lru_cache(maxsize=3)
def forward_inputs(case, n, data):
    """float32 x [n,ck,h,w], w [cm,ck,3,3], b [cm], res [n,cm,h,w] and, for a first-layer case, uint8 xu.
    `ranged`: x scaled by a power of two per input channel, w / b / res by one per filter, x about 30 % exact zeros
    (some of them -0.0, next to the negatives randn brings: ReLU-mode inputs)."""
    ck, cm, h, w = case
    g = _gen(case, n, data, "forward")
    x = torch.randn(n, ck, h, w, generator=g)
    wt = torch.randn(cm, ck, 3, 3, generator=g) / math.sqrt(9 * ck)
    b = torch.randn(cm, generator=g) * 0.5 + 0.25
    res = torch.randn(n, cm, h, w, generator=g)
    r = {}
    if data == "integers":
        x = torch.randint(-2, 3, (n, ck, h, w), generator=g).float()
        wt = torch.randint(-2, 3, (cm, ck, 3, 3), generator=g).float()
        b = torch.randint(-5, 6, (cm,), generator=g).float()
        res = torch.randint(-2, 3, (n, cm, h, w), generator=g).float()
    elif data == "ranged":
        sx, sw = _pow2(ck, g), _pow2(cm, g)
        x = _sparse(x, g, True) * sx[None, :, None, None]
        wt, b, res = wt * sw[:, None, None, None], b * sw, res * sw[None, :, None, None]
    if first_layer(case):
        xu = torch.randint(0, 256, (n, ck, h, w), generator=g, dtype=torch.uint8)
        if data == "ranged":
            xu = torch.where(torch.rand(xu.shape, generator=g) < 0.3, torch.zeros_like(xu), xu)
        r["xu"] = xu
    r.update(x=x, w=wt, b=b, res=res)
    return r


@functools.lru_cache(maxsize=3)
def backward_data_inputs(case, n, data):
    """float32 dy [n,ck,h,w], w [ck,cm,3,3] (the forward's weight: cout = ck), relu_src and dres [n,cm,h,w].
    `ranged`: dy and w scaled by a power of two per dy channel / per filter, relu_src and dres per dx channel."""
    ck, cm, h, w = case
    g = _gen(case, n, data, "backward_data")
    dy = torch.randn(n, ck, h, w, generator=g)
    wt = torch.randn(ck, cm, 3, 3, generator=g) / math.sqrt(9 * cm)
    src = torch.randn(n, cm, h, w, generator=g)
    dres = torch.randn(n, cm, h, w, generator=g)
    if data == "integers":
        dy = torch.randint(-2, 3, (n, ck, h, w), generator=g).float()
        wt = torch.randint(-2, 3, (ck, cm, 3, 3), generator=g).float()
        src = torch.randint(-2, 3, (n, cm, h, w), generator=g).float()
        dres = torch.randint(-2, 3, (n, cm, h, w), generator=g).float()
    elif data == "ranged":
        sd, sw, sx = _pow2(ck, g), _pow2(ck, g), _pow2(cm, g)
        dy = _sparse(dy, g, False) * sd[None, :, None, None]
        wt = wt * sw[:, None, None, None]
        src = _sparse(src, g, True) * sx[None, :, None, None]
        # (of the order of the products that reach the channel, so that the bar is not dres's alone)
        dres = dres * sx[None, :, None, None]
    return dict(dy=dy, w=wt, relu_src=src, dres=dres)


@functools.lru_cache(maxsize=3)
def backward_weight_inputs(case, n, data):
    """float32 x [n,ck,h,w] (+ uint8 xu for a first-layer case) and dy [n,cm,h,w].  `ranged`: x scaled per input
    channel, dy per channel; x about 30 % exact zeros."""
    ck, cm, h, w = case
    g = _gen(case, n, data, "backward_weight")
    x = torch.randn(n, ck, h, w, generator=g)
    dy = torch.randn(n, cm, h, w, generator=g)
    r = {}
    if data == "integers":
        x = torch.randint(-2, 3, (n, ck, h, w), generator=g).float()
        dy = torch.randint(-2, 3, (n, cm, h, w), generator=g).float()
    elif data == "ranged":
        sx, sd = _pow2(ck, g), _pow2(cm, g)
        x = _sparse(x, g, True) * sx[None, :, None, None]
        dy = dy * sd[None, :, None, None]
    if first_layer(case):
        xu = torch.randint(0, 256, (n, ck, h, w), generator=g, dtype=torch.uint8)
        if data == "ranged":
            xu = torch.where(torch.rand(xu.shape, generator=g) < 0.3, torch.zeros_like(xu), xu)
        r["xu"] = xu
    r.update(x=x, dy=dy)
    return r


def loaded(inp, mode):
    """The float32 operand the kernel contracts: f(in) of include/ppo_amd.h.  Every f is exact in float32 but the
    uint8 quotient, which is the correctly rounded x / 255 (test_uint8_scaling_is_the_exact_quotient_for_all_256_values)."""
    if mode == U8:
        return inp["xu"].float() / 255.0
    return torch.relu(inp["x"]) if mode == RELU else inp["x"]


# ---------------------------------------------------------------------------------------------------- the evaluations
def split_bf16(t):
    hi = t.bfloat16().float()
    return hi, (t - hi).bfloat16().float()


def contract(op, a, b, how):
    """One of the three contractions on float32 operands, as a float64 tensor.
    op: "forward" conv2d(a = x, b = w) | "backward_data" conv_transpose2d(a = dy, b = w) | "backward_weight"
    conv2d_weight(a = x, b = dy).  how: "f64" | "abs" (float64, on absolute values) | "f32" (plain float32 torch) |
    "split" (float32 torch on bf16 hi / lo parts: hi.hi + hi.lo + lo.hi)."""
    def run(p, q):
        if op == "forward":
            return F.conv2d(p, q, None, padding=1)
        if op == "backward_data":
            return F.conv_transpose2d(p, q, None, padding=1)
        return torch.nn.grad.conv2d_weight(p, (q.shape[1], p.shape[1], 3, 3), q, padding=1)
    if how == "f64":
        return run(a.double(), b.double())
    if how == "abs":
        return run(a.double().abs(), b.double().abs())
    if how == "f32":
        return run(a, b).double()
    assert how == "split"
    (ah, al), (bh, bl) = split_bf16(a), split_bf16(b)
    return ((run(ah, bh) + run(ah, bl)) + run(al, bh)).double()


def _ch(v):
    return v[None, :, None, None]


def forward_eval(xin, w, b, res, how):
    """conv3x3(xin) + b + res (b, res nullable) -> float64 [n,cm,h,w]; how as in contract (the epilogue in float32 for
    "f32" and "split").  `xin` is loaded(inp, mode)."""
    y = contract("forward", xin, w, how)
    if how in ("f32", "split"):
        y = y.float()
        if b is not None:
            y = y + _ch(b)
        if res is not None:
            y = y + res
        return y.double()
    absf = torch.abs if how == "abs" else (lambda t: t)
    if b is not None:
        y = y + _ch(absf(b.double()))
    if res is not None:
        y = y + absf(res.double())
    return y


def backward_data_eval(dy, w, relu_src, dres, how):
    """conv3x3^T(dy) * (relu_src > 0) + dres (relu_src, dres nullable) -> float64 [n,cm,h,w]."""
    y = contract("backward_data", dy, w, how)
    if relu_src is not None:
        y = y * (relu_src > 0).to(y.dtype)
    if dres is not None:
        if how in ("f32", "split"):
            y = (y.float() + dres).double()
        else:
            y = y + (dres.double().abs() if how == "abs" else dres.double())
    return y


def backward_weight_eval(xin, dy, how):
    """(dw [cm,ck,3,3], db [cm]) in float64; for "split" db is the float32 sum (one operand: nothing to split)."""
    dw = contract("backward_weight", xin, dy, how)
    if how == "f64":
        db = dy.double().sum((0, 2, 3))
    elif how == "abs":
        db = dy.double().abs().sum((0, 2, 3))
    else:
        db = dy.sum((0, 2, 3)).double()
    return dw, db


# ------------------------------------------------------------------------------------------------------------ the bar
def sum_length(op, case, n):
    """K of the bar: 9 ck for forward and backward-data (ck = cin, resp. the entry point's cout), n h w for dw / db."""
    ck, cm, h, w = case
    return n * h * w if op == "backward_weight" else 9 * ck


def bar_factor(K):
    """| got - ref | <= bar_factor(K) * A per element.  (K + 3) u bounds, to first order and for any summation order, K
    individually rounded float32 products-and-adds plus the bias, the residual and the final store; the factor 2 covers
    the MFMA's unspecified internal rounding."""
    return 2.0 * (K + 3) * U


def err_stats(got, ref, A, K):
    """-> (max e/A, rms e/A, elements over the bar) with e = |got - ref|, over every element."""
    e = (got.double() - ref).abs()
    bad = int((e > bar_factor(K) * A).sum())
    q = e / A.clamp_min(1e-300)
    return float(q.max()), float(q.pow(2).mean().sqrt()), bad


# The (case id, n) at which the weight gradient carries the aggregate bar: where tests/test_conv_float64_cpu.py finds the
# emulated split at least 10 x worse than plain float32 in rms(e/A) on both data sets (it prints every ratio and asserts
# these).  At long sums accumulation rounding swamps the split's truncation and there is nothing to tell apart.  Listed are
# the cases measured at 14 x or more, so that another CPU's float32 summation order does not move one across the line;
# the others (3 x at 84x84, 6 x to 13 x at 64x64 / 42x42 / 32x32 with n = 3) keep the per-element bar and the integers.
WGRAD_AGGREGATE = {("4x16x64x64", 1), ("16x32x32x32", 1), ("16x16x42x42", 1), ("16x16x42x42", 3), ("16x16x32x32", 1),
                   ("16x16x32x32", 3), ("32x32x21x21", 1), ("32x32x16x16", 1), ("32x32x11x11", 1), ("32x32x11x11", 3),
                   ("32x32x8x8", 1), ("32x32x8x8", 3)}


def integer_bound(op, case, n):
    """The largest |partial sum| the `integers` set can reach: operands in [-2, 2], bias in [-5, 5], residual / dres
    in [-2, 2]."""
    return 4 * sum_length(op, case, n) + 5 + 2
