"""The fused-stack, residual-block and weight-gradient entry points without a GPU: which geometries their probes report, and
what the launch entry points reject before any HIP call, in which order.

No call here may pass validation: every one is an empty (or negative) batch, or has a null or misaligned argument, or a
geometry that the family's probe rejects (`call` refuses anything else).  Geometries a probe accepts are given to probes
only.  The pointer tables are real ctypes arrays, which the host code reads; their elements and every tensor argument are
one made-up aligned address that nothing follows.

Two entry points differ from the common order (batch, null pointers, alignment, geometry last) and are pinned as they are:
`ppo_impala_stack_chain_split_forward_f32` looks at the geometry before its workspace and layer tables, so its table
checks cannot be reached from here; the weight-gradient entry points reject an empty batch.
"""
import ctypes
import itertools

import pytest

ALIGN, INVALID, OK = -3, -1, 0
IN_NONE, IN_RELU, IN_U8 = 0, 1, 2
P = 0x1000  # a non-null 16-byte aligned pointer that is never followed
OFF = P + 4  # 4-byte aligned, not 16

CHANNELS, CINS, SIDES = (8, 16, 32, 64), (3, 4, 5, 16), (8, 11, 16, 21, 32, 42, 64, 84)
TAIL = {(16, 42, 42), (16, 32, 32), (32, 21, 21), (32, 11, 11), (32, 16, 16), (32, 8, 8)}
SUPPORTED = {
    "ppo_impala_stack_tail_supported": TAIL,
    "ppo_impala_stack_full_supported": {(32, 21, 21), (32, 16, 16)},
    "ppo_impala_stack_tail_bf16x3_supported": TAIL,
    "ppo_conv3x3_block_supported": {(16, 42, 42), (16, 32, 32)},
    # (cin, cout, h, w): the observation convolution, whose gradient arrives pooled
    "ppo_conv3x3_backward_weight_pooled_supported": {(4, 16, 84, 84), (5, 16, 84, 84), (3, 16, 64, 64), (4, 16, 64, 64)},
}
NO_KERNEL = [(32, 42, 42), (16, 21, 21), (64, 21, 21), (32, 21, 16)]  # (channels, h, w)
NO_WGRAD_KERNEL = [(7, 16, 30, 30), (32, 32, 21, 16), (16, 16, 21, 21), (4, 16, 84, 64)]  # (cin, cout, h, w)


@pytest.mark.parametrize("probe", sorted(SUPPORTED))
def test_supported_geometries(hip_lib, probe):
    fn = getattr(hip_lib, probe)
    first = (CINS, CHANNELS) if probe == "ppo_conv3x3_backward_weight_pooled_supported" else (CHANNELS,)
    got = {g for g in itertools.product(*first, SIDES, SIDES) if fn(*g)}
    assert got == SUPPORTED[probe]


# ---- the entry points that take (..., n_images, channels, h, w, stream)
# Argument kinds: T a required tensor, O a nullable one, M a required one with a message of its own, PACKED one packed
# weight buffer (16-byte aligned), W<n> a table of n packed-weight pointers, B<n> its companion table (biases, masks or sign
# maps, every element required), S4 a table whose elements are not looked at, NBYTES a size_t that is always large enough.
def entry(probe, args, **extra):
    return dict(probe=probe, args=args.split(), **extra)


FOUR_MAPS = b"the backward pass writes all four gradient maps"
ENTRIES = {
    "ppo_impala_stack_tail_forward_f32": entry("ppo_impala_stack_tail_supported", "in:T w:W4 bias:B4 a0:O q0:O a1:O q1:T"),
    "ppo_impala_stack_tail_backward_f32": entry("ppo_impala_stack_tail_supported", "g:T w:W4 mask:B4 da1:T g1:T da0:T g0:T"),
    "ppo_impala_stack_full_forward_f32": entry("ppo_impala_stack_full_supported",
                                               "in:T w:W5 bias:B5 pooled:O argmax:O a0:O q0:O a1:O q1:T"),
    "ppo_impala_stack_chain_forward_f32": entry("ppo_impala_stack_full_supported",
                                                "in:T pre_w:W4 pre_bias:B4 pre_a0:O pre_q0:O pre_a1:O pre_q1:O w:W5 bias:B5 "
                                                "pooled:O argmax:O a0:O q0:O a1:O q1:T"),
    "ppo_impala_stack_full_backward_f32": entry("ppo_impala_stack_full_supported",
                                                "g:T w:W5 mask:B4 argmax:T da1:T g1:T da0:T g0:T dc:T g_prev:T"),
    "ppo_impala_stack_chain_backward_f32": entry("ppo_impala_stack_full_supported",
                                                 "g:T w:W5 mask:B4 argmax:T da1:T g1:T da0:T g0:T dc:T g_prev:T post_w:W4 "
                                                 "post_mask:B4 post_da1:T post_g1:T post_da0:T post_g0:T"),
    # its one geometry is among those of the whole-stack probe; the geometry is looked at before the tables
    "ppo_impala_stack_chain_split_forward_f32": entry("ppo_impala_stack_full_supported",
                                                      "in:T pre_w:W4 pre_bias:B4 w:W5 bias:B5 q1:T workspace:T bytes:NBYTES",
                                                      geometry_before_tables=True),
    "ppo_impala_stack_tail_forward_bf16x3": entry("ppo_impala_stack_tail_bf16x3_supported",
                                                  "in:T packed:PACKED bias:B4 a0:O q0:O a1:O q1:T", misaligned=INVALID),
    "ppo_impala_stack_tail_backward_bf16x3": entry("ppo_impala_stack_tail_bf16x3_supported",
                                                   "g:T packed:PACKED mask:B4 da1:M g1:M da0:M g0:T", misaligned=INVALID),
    "ppo_impala_stack_tail_forward_signs_bf16x3": entry("ppo_impala_stack_tail_bf16x3_supported",
                                                        "in:T packed:PACKED bias:B4 a0:O q0:O a1:O q1:T signs:S4",
                                                        misaligned=INVALID),
    "ppo_impala_stack_tail_backward_signs_bf16x3": entry("ppo_impala_stack_tail_bf16x3_supported",
                                                         "g:T packed:PACKED signs:B4 da1:M g1:M da0:M g0:T", misaligned=INVALID),
    "ppo_conv3x3_block_forward_packed_f32": entry("ppo_conv3x3_block_supported",
                                                  "in:T packed0:PACKED bias0:T packed1:PACKED bias1:T out:T", misaligned=ALIGN),
}
STACK_ENTRIES = sorted(ENTRIES)


def table(n, **elements):
    """n pointers P as a ctypes array; table(4, at=1, value=None) has a null element 1."""
    values = [P] * n
    if elements:
        values[elements["at"]] = elements["value"]
    return (ctypes.c_void_p * n)(*values)


def default(kind):
    if kind[0] in "WBS":
        return table(int(kind[1:]))
    return 1 << 40 if kind == "NBYTES" else P


def call(lib, name, n=1, geometry=NO_KERNEL[-1], **override):
    """One call of entry point `name`: the named arguments replaced, everything else valid but for the geometry."""
    spec = ENTRIES[name]
    assert not getattr(lib, spec["probe"])(*geometry), "a geometry with a kernel goes to the probes only"
    values = {a.split(":")[0]: default(a.split(":")[1]) for a in spec["args"]}
    assert set(override) <= set(values), override
    values.update(override)
    return getattr(lib, name)(*values.values(), n, *geometry, None)


def args_of(name, *kinds):
    return [a.split(":") for a in ENTRIES[name]["args"] if a.split(":")[1][0] in kinds]


@pytest.mark.parametrize("name", STACK_ENTRIES)
def test_batch_size_comes_first(hip_lib, name):
    first = ENTRIES[name]["args"][0].split(":")[0]
    assert call(hip_lib, name, n=-1) == INVALID
    assert call(hip_lib, name, n=0) == OK
    assert call(hip_lib, name, n=0, **{first: None}) == OK  # before any pointer is looked at
    for geometry in NO_KERNEL:
        assert call(hip_lib, name, n=0, geometry=geometry) == OK  # and before the geometry


@pytest.mark.parametrize("name", STACK_ENTRIES)
def test_null_pointers(hip_lib, name):
    for arg, kind in args_of(name, "T", "M", "P", "W", "B", "S"):
        assert call(hip_lib, name, **{arg: None}) == INVALID, arg
        assert (FOUR_MAPS if kind == "M" else b"null") in hip_lib.ppo_last_error(), arg


@pytest.mark.parametrize("name", STACK_ENTRIES)
def test_null_table_elements(hip_lib, name):
    for arg, kind in args_of(name, "W", "B"):
        n = int(kind[1:])
        for at in (0, n - 1):
            assert call(hip_lib, name, **{arg: table(n, at=at, value=None)}) == INVALID, (arg, at)
            text = hip_lib.ppo_last_error()
            if ENTRIES[name].get("geometry_before_tables"):
                assert b"no kernel" in text
            else:
                assert b"null" in text and b"of layer %d" % at in text, (arg, at)


@pytest.mark.parametrize("name", STACK_ENTRIES)
def test_packed_weights_are_16_byte_aligned(hip_lib, name):
    for arg, kind in args_of(name, "W"):
        n = int(kind[1:])
        for at in (0, n - 1):
            rc = call(hip_lib, name, **{arg: table(n, at=at, value=OFF)})
            if ENTRIES[name].get("geometry_before_tables"):
                assert rc == INVALID and b"no kernel" in hip_lib.ppo_last_error()
            else:
                assert rc == ALIGN, (arg, at)
                assert b"packed weights must be 16-byte aligned" in hip_lib.ppo_last_error()
    for arg, _ in args_of(name, "P"):
        # the split-bf16 entry points report their one packed buffer with the null pointers
        assert call(hip_lib, name, **{arg: OFF}) == ENTRIES[name]["misaligned"], arg
        assert b"aligned" in hip_lib.ppo_last_error()


@pytest.mark.parametrize("name", STACK_ENTRIES)
def test_geometry_comes_last(hip_lib, name):
    for geometry in NO_KERNEL:
        assert call(hip_lib, name, geometry=geometry) == INVALID, geometry
        assert b"%s: no kernel for %d channels at %dx%d" % (name.encode(), *geometry) == hip_lib.ppo_last_error()


def test_full_backward_argmax_alignment(hip_lib):
    for name in ("ppo_impala_stack_full_backward_f32", "ppo_impala_stack_chain_backward_f32"):
        assert call(hip_lib, name, argmax=P + 1) == ALIGN
        assert b"argmax must be 4-byte aligned" in hip_lib.ppo_last_error()
        assert call(hip_lib, name, argmax=P + 1, w=table(5, at=0, value=None)) == ALIGN  # before the tables


def test_tail_forward_input_alignment(hip_lib):
    assert call(hip_lib, "ppo_impala_stack_tail_forward_f32", **{"in": P + 2}) == ALIGN
    assert b"input must be 4-byte aligned" in hip_lib.ppo_last_error()


def test_16_channel_tail_extras(hip_lib):
    fwd, bwd, geometry = "ppo_impala_stack_tail_forward_f32", "ppo_impala_stack_tail_backward_f32", (16, 21, 21)
    assert call(hip_lib, fwd, geometry=geometry, q0=None) == INVALID
    assert b"ppo_impala_stack_tail_forward_f32: the 16-channel form needs q0 (its second block re-reads it)" == hip_lib.ppo_last_error()
    assert call(hip_lib, fwd, geometry=(32, 42, 42), q0=None) == INVALID  # 32 channels: q0 is optional
    assert b"no kernel" in hip_lib.ppo_last_error()
    for arg in ("in", "a0", "q0", "a1", "q1"):
        assert call(hip_lib, fwd, geometry=geometry, **{arg: OFF}) == ALIGN, arg
        assert b"the 16-channel form needs 16-byte aligned maps" in hip_lib.ppo_last_error()
        assert call(hip_lib, fwd, geometry=(32, 42, 42), **{arg: OFF}) == INVALID, arg
    for a0, a1 in ((None, P), (P, None), (None, None)):  # nullable maps need no alignment
        assert call(hip_lib, fwd, geometry=geometry, a0=a0, a1=a1) == INVALID
        assert b"no kernel" in hip_lib.ppo_last_error()
    for arg in ("g", "da1", "g1", "da0", "g0"):
        assert call(hip_lib, bwd, geometry=geometry, **{arg: OFF}) == ALIGN, arg
        assert b"ppo_impala_stack_tail_backward_f32: the 16-channel form needs 16-byte aligned maps" == hip_lib.ppo_last_error()
    for at in range(4):
        assert call(hip_lib, bwd, geometry=geometry, mask=table(4, at=at, value=OFF)) == ALIGN, at
        assert call(hip_lib, bwd, geometry=(32, 42, 42), mask=table(4, at=at, value=OFF)) == INVALID, at


def test_chain_split_workspace(hip_lib):
    name = "ppo_impala_stack_chain_split_forward_f32"
    bytes_ = hip_lib.ppo_impala_stack_chain_split_workspace_bytes
    # exchange slots [n][2][C][h*w] floats, flags [n][2] rounded up to 16 bytes, four control words
    assert bytes_(1, 32, 21, 21) == 2 * 32 * 441 * 4 + 16 + 16
    assert bytes_(3, 32, 21, 21) == 3 * 2 * 32 * 441 * 4 + 32 + 16
    assert bytes_(128, 32, 21, 21) == 128 * 2 * 32 * 441 * 4 + 1024 + 16
    # the geometry is looked at before the workspace
    assert call(hip_lib, name, bytes=0) == INVALID and b"no kernel" in hip_lib.ppo_last_error()
    assert call(hip_lib, name, workspace=OFF) == INVALID and b"no kernel" in hip_lib.ppo_last_error()


def test_sign_tables(hip_lib):
    fwd, bwd = "ppo_impala_stack_tail_forward_signs_bf16x3", "ppo_impala_stack_tail_backward_signs_bf16x3"
    for name in (fwd, bwd):
        assert call(hip_lib, name, n=0, signs=None) == INVALID  # the sign table is looked at even before the batch size
        assert b"%s: null sign table" % name.encode() == hip_lib.ppo_last_error()
    assert call(hip_lib, bwd, signs=table(4, at=2, value=None)) == INVALID
    assert b"null sign map of layer 2" in hip_lib.ppo_last_error()


# ---- the weight-gradient entry points: (..., n, cin, cout, h, w, ...).  tests/test_conv_dispatch_cpu.py has their batch
# size and null-pointer checks; here: the problem tables of the two batched forms and the geometry of all six
def wgrad_call(lib, name, geometry, in_mode=IN_RELU, count=2, ins=None, relu=(ctypes.c_int * 2)(1, 0), dys=None, workspaces=None):
    pooled = "_pooled_" in name
    probe = lib.ppo_conv3x3_backward_weight_pooled_supported(*geometry) if pooled else \
        lib.ppo_conv3x3_backward_weight_supported(in_mode, *geometry)
    assert not probe, "a geometry with a kernel goes to the probes only"
    big, fn = 1 << 40, getattr(lib, name)
    if name == "ppo_conv3x3_backward_weight_f32":
        return fn(P, in_mode, P, P, P, P, big, 1, *geometry, 0, None)
    if name == "ppo_conv3x3_backward_weight_slabs_f32":
        return fn(P, in_mode, P, P, big, 1, *geometry, P, None)
    if name == "ppo_conv3x3_backward_weight_slabs_pooled_f32":
        return fn(P, in_mode, P, P, P, big, 1, *geometry, P, None)
    if name == "ppo_conv3x3_backward_weight_slabs_pooled_indexed_f32":
        return fn(P, None, in_mode, P, P, P, big, 1, *geometry, P, None)
    tables = [t if t is not None else table(count) for t in (ins, dys, workspaces)]
    mode_or_relu = in_mode if name.endswith("_batch_f32") else relu  # the ReLU flags are real: the host code reads them
    return fn(tables[0], mode_or_relu, tables[1], tables[2], big, count, 1, *geometry, P, None)


BATCHED = ["ppo_conv3x3_backward_weight_slabs_batch_f32", "ppo_conv3x3_backward_weight_slabs_batch_mixed_f32"]


@pytest.mark.parametrize("name", BATCHED)
def test_wgrad_problem_tables(hip_lib, name):
    geometry = NO_WGRAD_KERNEL[0]
    for arg, k in itertools.product(("ins", "dys", "workspaces"), (0, 1)):
        assert wgrad_call(hip_lib, name, geometry, **{arg: table(2, at=k, value=None)}) == INVALID, (arg, k)
        assert b"%s: null pointer in problem %d" % (name.encode(), k) == hip_lib.ppo_last_error()
    # a problem beyond `count` is not looked at
    assert wgrad_call(hip_lib, name, geometry, count=1, ins=table(2, at=1, value=None)) == INVALID
    assert b"unsupported geometry" in hip_lib.ppo_last_error()
    if name.endswith("_mixed_f32"):
        assert wgrad_call(hip_lib, name, geometry, relu=None) == INVALID
        assert b"%s: null pointer" % name.encode() == hip_lib.ppo_last_error()
    else:
        assert wgrad_call(hip_lib, name, geometry, in_mode=3) == INVALID
        assert b"%s: unknown in_mode 3" % name.encode() == hip_lib.ppo_last_error()


@pytest.mark.parametrize("name", ["ppo_conv3x3_backward_weight_f32", "ppo_conv3x3_backward_weight_slabs_f32"] + BATCHED)
def test_wgrad_geometry_comes_last(hip_lib, name):
    for geometry in NO_WGRAD_KERNEL:
        assert wgrad_call(hip_lib, name, geometry) == INVALID, geometry
        assert b"conv3x3_wgrad: unsupported geometry cin=%d cout=%d h=%d w=%d in_mode=1" % geometry == hip_lib.ppo_last_error()


@pytest.mark.parametrize("name", ["ppo_conv3x3_backward_weight_slabs_pooled_f32",
                                  "ppo_conv3x3_backward_weight_slabs_pooled_indexed_f32"])
def test_pooled_wgrad_geometry_comes_last(hip_lib, name):
    for geometry, in_mode in itertools.product(NO_WGRAD_KERNEL, (IN_NONE, IN_U8)):
        assert wgrad_call(hip_lib, name, geometry, in_mode=in_mode) == INVALID, geometry
        assert b"conv3x3_wgrad: no pooled-gradient kernel for cin=%d cout=%d h=%d w=%d in_mode=%d" % (*geometry, in_mode) \
            == hip_lib.ppo_last_error()
    assert wgrad_call(hip_lib, name, NO_WGRAD_KERNEL[0], in_mode=IN_RELU) == INVALID
    assert b"%s: in_mode 1 has no pooled-gradient kernel" % name.encode() == hip_lib.ppo_last_error()
