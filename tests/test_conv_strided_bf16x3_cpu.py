"""CPU: the split-bf16 strided convolutions (csrc/conv_strided_bf16x3.hip) without a GPU - the ABI, the argument
validation (every rejected call returns its `_f32` twin's code and message before anything is launched) and the
arithmetic the per-element bar of tests/conv_strided_split_torch.py is derived for.

The emulation (each operand as bf16 hi + lo in torch, partial products summed in float64) on the ten cases of
tests/test_conv_strided_gpu.py, every pass: the three-term form hi.hi + hi.lo + lo.hi uses at most 0.79 of the
2^-15 A split term (n1_conv3 backward-weight, a single product per element); with either cross term left out the whole
bar - float32 summation term included - is missed on every case and pass (the bias sum aside, whose other operand is
the constant 1 with lo = 0): by 2.3 x at the least (n1_conv3 forward without hi.lo; conv1_f32 backward-weight 2.4 x,
where K = 1200 makes the summation term the larger one) and by up to 120 x."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

import conv_strided_split_torch as S  # noqa: E402
from test_conv_strided_gpu import CASES  # noqa: E402

INVALID = -1
NAMES = ("ppo_conv2d_strided_forward_bf16x3", "ppo_conv2d_strided_backward_data_bf16x3",
         "ppo_conv2d_strided_backward_weight_bf16x3")


def test_entry_points_are_declared_and_exported(hip_lib):
    from ppo_amd import _lib
    for name in NAMES:
        twin = name.replace("bf16x3", "f32")
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]
        assert hasattr(hip_lib, name)


def _both(hip_lib, kind, *args):
    """(code, message) of the split entry point and of its _f32 twin, the twin's name replaced by the split one's."""
    res = []
    for suffix in ("bf16x3", "f32"):
        name = f"ppo_conv2d_strided_{kind}_{suffix}"
        rc = getattr(hip_lib, name)(*args, None)
        res.append((rc, (hip_lib.ppo_last_error() or b"").replace(name.encode(), b"@")))
    return res


def test_validation_is_the_f32_twins(hip_lib):
    """Null pointer, bad in_mode, unsupported geometry, n = 0 and a short workspace: rejected before any launch (the
    pointers are host memory no kernel could read), with the twin's code and message."""
    from ppo_amd import _lib
    host = ctypes.create_string_buffer(64)
    p = ctypes.addressof(host)
    good = (2, 2, 9, 9, 1, 3, 3, 2)       # cout1
    bad = (2, 4, 7, 84, 32, 8, 8, 4)      # window taller than the image
    empty = (0, 2, 9, 9, 1, 3, 3, 2)
    nbytes = int(hip_lib.ppo_conv2d_strided_wgrad_workspace_bytes(*good))
    assert nbytes > 0
    checks = [
        ("forward", (None, 0, p, p, p, 1, *good), b"null pointer"),
        ("forward", (p, 0, p, p, None, 1, *good), b"null pointer"),
        ("forward", (p, _lib.PPO_IN_RELU, p, p, p, 1, *good), b"in_mode"),
        ("forward", (p, 0, p, p, p, 1, *bad), b"unsupported geometry"),
        ("forward", (p, 0, p, p, p, 1, *empty), b"n=0"),
        ("backward_data", (p, p, None, p, *good), b"null pointer"),
        ("backward_data", (p, p, p, p, *bad), b"unsupported geometry"),
        ("backward_data", (p, p, p, p, *empty), b"n=0"),
        ("backward_weight", (p, 0, p, None, p, p, None, nbytes, *good), b"null pointer"),
        ("backward_weight", (p, _lib.PPO_IN_RELU, p, None, p, p, p, nbytes, *good), b"in_mode"),
        ("backward_weight", (p, 0, p, None, p, p, p, nbytes - 4, *good), b"workspace"),
        ("backward_weight", (p, 0, p, None, p, p, p, nbytes, *bad), b"unsupported geometry"),
        ("backward_weight", (p, 0, p, None, p, p, p, nbytes, *empty), b"n=0"),
    ]
    for kind, args, text in checks:
        (rc, msg), (rc32, msg32) = _both(hip_lib, kind, *args)
        assert rc == rc32 == INVALID, (kind, text, rc, rc32)
        assert msg == msg32 and text in msg and msg.startswith(b"@:"), (kind, msg, msg32)


def test_split_of_every_operand_obeys_the_bounds_the_bar_uses():
    """|x - hi - lo| <= 2^-17 |x| and |lo| <= 2^-8 |x| on every operand of every case."""
    for name in CASES:
        for t in S.operands(name):
            hi, lo = S.split(t)
            x = t.double()
            assert bool(((x - hi - lo).abs() <= 2.0 ** -17 * x.abs()).all()), name
            assert bool((lo.abs() <= 2.0 ** -8 * x.abs()).all()), name


@pytest.mark.parametrize("name", list(CASES))
def test_three_terms_hold_the_bar_and_two_do_not(name):
    u8 = CASES[name][8]
    for op in S.PASSES:
        if op == "backward_data" and u8:
            continue  # nothing back-propagates into uint8 observations
        three = S.emulated(name, op)
        used, share = S.worst_ratio(three, name, op), S.split_ratio(three, name, op)
        print(f"SPLIT_EMU {name} {op} K={S.sum_length(name, op)} three_terms: {used:.3f} of the bar, {share:.3f} of 2^-15 A")
        assert share <= 1.0 and used <= 1.0, (name, op, used, share)
        if op == "bias":
            continue  # the other operand is the constant 1: lo = 0, a cross term less changes nothing it could show
        for terms in (("hh", "hl"), ("hh", "lh")):
            over = S.worst_ratio(S.emulated(name, op, terms), name, op)
            print(f"SPLIT_EMU {name} {op} {'+'.join(terms)}: {over:.1f} x the bar")
            assert over > 1.0, (name, op, terms, over)
