"""Test helper (no test in here): the per-element bar of the split-bf16 strided convolutions (csrc/
conv_strided_bf16x3.hip) and an emulation of their arithmetic in torch, on the cases of tests/test_conv_strided_gpu.py.

The bar, derived.  x = hi + lo + r with hi = bf16(x), lo = bf16(x - hi): |r| <= 2^-17 |x| and |lo| <= 2^-8 |x|.  The
kernel keeps hi.hi + hi.lo + lo.hi of a product a b, so it drops a_lo b_lo + a_hi-or-lo r_b + r_a b: at most
(2^-16 + 2 * 2^-17) |a b| = 2^-15 |a b| to first order.  Products of bf16 values are exact in float32, and what remains is
float32 summation, bounded like the exact kernels' by bar_factor of tests/conv_float64_torch.py with one more term (the
three partial products of a K tile add one rounding).  Per element, with u = 2^-24, K the sum length and A the same
operation on the absolute values of the operands in float64:

    |got - ref64| <= (2^-15 + 2 (K + 4) u) * A
"""
import functools

import torch
import torch.nn.functional as F

from test_conv_strided_gpu import CASES, reference

U = 2.0 ** -24
PASSES = ("forward", "backward_data", "backward_weight", "bias")


def bar_factor(K):
    return 2.0 ** -15 + 2.0 * (K + 4) * U


def geometry(name):
    n, cin, h, w, cout, kh, kw, stride, u8 = CASES[name]
    return n, cin, h, w, cout, kh, kw, stride, u8, (h - kh) // stride + 1, (w - kw) // stride + 1


def sum_length(name, op):
    n, cin, _h, _w, cout, kh, kw, _s, _u8, ho, wo = geometry(name)
    return {"forward": cin * kh * kw, "backward_data": cout * kh * kw}.get(op, n * ho * wo)


def operands(name):
    """The float32 operands the launches contract: x (uint8 as x / 255), w, b and the gated gradient g."""
    r = reference(name)
    u8 = CASES[name][8]
    x = r["raw"].float() / 255.0 if u8 else r["raw"]
    g = torch.where(r["gate"] > 0, r["dy"], torch.zeros_like(r["dy"]))
    return x, r["w"], r["b"], g


def contract(name, op, a, b):
    """One contraction of case `name` on tensors a, b of any float dtype.
    forward: conv2d(a = x, b = w); backward_data: its input gradient (a = g, b = w); backward_weight: its weight
    gradient (a = x, b = g); bias: the sum of a b = g over (n, oy, ox), a the scalar 1 (the kernel's row of ones)."""
    n, cin, h, w, cout, kh, kw, stride, *_ = geometry(name)
    if op == "forward":
        return F.conv2d(a, b, None, stride=stride)
    if op == "backward_data":
        return torch.nn.grad.conv2d_input((n, cin, h, w), b, a, stride=stride)
    if op == "backward_weight":
        return torch.nn.grad.conv2d_weight(a, (cout, cin, kh, kw), b, stride=stride)
    return (a * b).sum(dim=(0, 2, 3))


def pass_operands(name, op):
    x, w, _b, g = operands(name)
    return {"forward": (x, w), "backward_data": (g, w), "backward_weight": (x, g), "bias": (torch.ones(()), g)}[op]


@functools.lru_cache(maxsize=None)
def magnitude(name, op):
    """A: the contraction on absolute values in float64 (the forward's with |bias| added)."""
    a, b = pass_operands(name, op)
    A = contract(name, op, a.double().abs(), b.double().abs())
    if op == "forward":
        A = A + reference(name)["b"].double().abs()[None, :, None, None]
    return A


@functools.lru_cache(maxsize=None)
def exact(name, op):
    """The float64 result on the float32 operands (the forward's before the ReLU, with the bias)."""
    a, b = pass_operands(name, op)
    y = contract(name, op, a.double(), b.double())
    if op == "forward":
        y = y + reference(name)["b"].double()[None, :, None, None]
    return y


def bar(name, op):
    return bar_factor(sum_length(name, op)) * magnitude(name, op)


def split(t):
    """(hi, lo) as float64 tensors: hi = bf16(x), lo = bf16(x - hi), the kernel's expression."""
    hi = t.bfloat16().float()
    return hi.double(), (t - hi).bfloat16().double()


def emulated(name, op, terms=("hh", "hl", "lh")):
    """The split arithmetic with exact (float64) summation: the listed partial products of (a_hi + a_lo)(b_hi + b_lo)."""
    a, b = pass_operands(name, op)
    (ah, al), (bh, bl) = split(a), split(b)
    parts = {"hh": (ah, bh), "hl": (ah, bl), "lh": (al, bh)}
    y = sum(contract(name, op, *parts[t]) for t in terms)
    if op == "forward":
        y = y + reference(name)["b"].double()[None, :, None, None]
    return y


def worst_ratio(got, name, op):
    """max over elements of |got - exact| / bar (<= 1: inside the bar)."""
    e = (got.double() - exact(name, op)).abs()
    return float((e / bar(name, op).clamp_min(1e-300)).max())


def split_ratio(got, name, op):
    """max over elements of |got - exact| / (2^-15 A): the share of the split term of the bar that is used."""
    e = (got.double() - exact(name, op)).abs()
    return float((e / (2.0 ** -15 * magnitude(name, op)).clamp_min(1e-300)).max())
