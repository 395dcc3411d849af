"""The 3x3 convolution dispatchers without a GPU: which geometries the probes report, that a probe leaves nothing
behind for the next call of its thread, and what the entry points reject before any HIP call.

Every call here returns from the host-side checks or from a dispatcher's case list; the pointers are made-up addresses
that nothing dereferences.
"""
import itertools

import pytest

INVALID, OK = -1, 0
IN_NONE, IN_RELU, IN_U8 = 0, 1, 2
P = 0x1000  # a non-null pointer that is never followed
NO_KERNEL = dict(cin=7, cout=16, h=30, w=30)

CINS, COUTS, SIDES = (3, 4, 5, 16, 32), (16, 32), (8, 11, 16, 21, 32, 42, 64, 84)

# (in_mode, cin, cout, side), from the case lists of dispatch_conv, dispatch_conv_pool and dispatch_wgrad
FIRST = {(3, 16, 64), (4, 16, 64), (4, 16, 84), (5, 16, 84)}  # the observation convolution: float or uint8 input
UP = {(16, 32, 42), (16, 32, 32)}
BLOCK16 = {(16, 16, 42), (16, 16, 32)}
BLOCK32 = {(32, 32, 21), (32, 32, 16), (32, 32, 11), (32, 32, 8)}


def modes(geos, *in_modes):
    return {(m, *g) for m in in_modes for g in geos}


SUPPORTED = {
    "ppo_conv3x3_forward_supported": modes(FIRST, IN_NONE, IN_U8) | modes(UP, IN_NONE) | modes(BLOCK16 | BLOCK32, IN_NONE, IN_RELU),
    # no in_mode: the gradient of every convolution but the first
    "ppo_conv3x3_backward_data_supported": modes(UP | BLOCK16 | BLOCK32, None),
    "ppo_conv3x3_pool_forward_supported": modes(FIRST, IN_NONE, IN_U8) | modes(UP | {(32, 32, 21), (32, 32, 16)}, IN_NONE),
    "ppo_conv3x3_backward_weight_supported": modes(FIRST, IN_NONE, IN_U8) | modes(UP | {(32, 32, 21), (32, 32, 16)}, IN_NONE)
                                             | modes(BLOCK16 | BLOCK32, IN_RELU),
}


@pytest.mark.parametrize("probe", sorted(SUPPORTED))
def test_supported_geometries(hip_lib, probe):
    fn = getattr(hip_lib, probe)
    in_modes = (None,) if probe == "ppo_conv3x3_backward_data_supported" else (IN_NONE, IN_RELU, IN_U8, 3)
    got = set()
    for m, cin, cout, s in itertools.product(in_modes, CINS, COUTS, SIDES):
        if fn(cin, cout, s, s) if m is None else fn(m, cin, cout, s, s):
            got.add((m, cin, cout, s))
    assert got == SUPPORTED[probe]


def forward(lib, name, *, in_=P, in_mode=IN_NONE, n=1, cin, cout, h, w):
    return getattr(lib, name)(in_, in_mode, P, P, None, P, n, cin, cout, h, w, None)


def backward_data(lib, name, *, in_=P, n=1, cin, cout, h, w):
    return getattr(lib, name)(in_, P, None, None, P, n, cin, cout, h, w, None)


def pool_forward(lib, name, *, in_=P, in_mode=IN_NONE, n=1, cin, cout, h, w):
    return getattr(lib, name)(in_, in_mode, P, P, P, P, n, cin, cout, h, w, None)


def pool_forward_indexed(lib, name, *, in_=P, index=None, in_mode=IN_U8, n=1, cin, cout, h, w):
    return getattr(lib, name)(in_, index, in_mode, P, P, P, P, n, cin, cout, h, w, None)


def backward_weight(lib, name, *, in_=P, in_mode=IN_NONE, n=1, cin, cout, h, w):
    return getattr(lib, name)(in_, in_mode, P, P, P, P, 1 << 20, n, cin, cout, h, w, 0, None)


def weight_slabs(lib, name, *, in_=P, in_mode=IN_NONE, n=1, cin, cout, h, w):
    return getattr(lib, name)(in_, in_mode, P, P, 1 << 20, n, cin, cout, h, w, P, None)


def weight_slabs_batch(lib, name, *, in_=P, n=1, count=1, cin, cout, h, w):
    # (ins, in_mode or the relu flags, dys, workspaces, ...): the tables are read only after n, count and they are checked
    mode_or_relu = IN_RELU if name.endswith("_batch_f32") else P
    return getattr(lib, name)(in_, mode_or_relu, P, P, 1 << 20, count, n, cin, cout, h, w, P, None)


def weight_slabs_pooled(lib, name, *, in_=P, in_mode=IN_NONE, n=1, cin, cout, h, w):
    return getattr(lib, name)(in_, in_mode, P, P, P, 1 << 20, n, cin, cout, h, w, P, None)


def weight_slabs_pooled_indexed(lib, name, *, in_=P, index=None, in_mode=IN_U8, n=1, cin, cout, h, w):
    return getattr(lib, name)(in_, index, in_mode, P, P, P, 1 << 20, n, cin, cout, h, w, P, None)


FORWARD_ENTRIES = [
    (forward, "ppo_conv3x3_forward_f32"),
    (forward, "ppo_conv3x3_forward_packed_f32"),
    (backward_data, "ppo_conv3x3_backward_data_f32"),
    (backward_data, "ppo_conv3x3_backward_data_packed_f32"),
    (pool_forward, "ppo_conv3x3_pool_forward_f32"),
    (pool_forward, "ppo_conv3x3_pool_forward_packed_f32"),
    (pool_forward_indexed, "ppo_conv3x3_pool_forward_packed_indexed_f32"),
]
WGRAD_ENTRIES = [
    (backward_weight, "ppo_conv3x3_backward_weight_f32"),
    (weight_slabs, "ppo_conv3x3_backward_weight_slabs_f32"),
    (weight_slabs_batch, "ppo_conv3x3_backward_weight_slabs_batch_f32"),
    (weight_slabs_batch, "ppo_conv3x3_backward_weight_slabs_batch_mixed_f32"),
    (weight_slabs_pooled, "ppo_conv3x3_backward_weight_slabs_pooled_f32"),
    (weight_slabs_pooled_indexed, "ppo_conv3x3_backward_weight_slabs_pooled_indexed_f32"),
]

# probe, a geometry it reports, the launch that shares its case list, what that launch says to a geometry without a kernel
PROBE_THEN_LAUNCH = [
    ("ppo_conv3x3_forward_supported", (IN_NONE, 16, 16, 42, 42), forward, "ppo_conv3x3_forward_f32", b"unsupported geometry"),
    ("ppo_conv3x3_forward_supported", (IN_NONE, 16, 16, 42, 42), forward, "ppo_conv3x3_forward_packed_f32", b"unsupported geometry"),
    ("ppo_conv3x3_backward_data_supported", (16, 16, 42, 42), backward_data, "ppo_conv3x3_backward_data_f32", b"unsupported geometry"),
    ("ppo_conv3x3_pool_forward_supported", (IN_NONE, 4, 16, 84, 84), pool_forward, "ppo_conv3x3_pool_forward_f32", b"unsupported geometry"),
    ("ppo_conv3x3_backward_weight_supported", (IN_NONE, 4, 16, 84, 84), backward_weight, "ppo_conv3x3_backward_weight_f32",
     b"unsupported geometry"),
    ("ppo_conv3x3_backward_weight_supported", (IN_NONE, 4, 16, 84, 84), weight_slabs, "ppo_conv3x3_backward_weight_slabs_f32",
     b"unsupported geometry"),
    ("ppo_conv3x3_backward_weight_pooled_supported", (4, 16, 84, 84), weight_slabs_pooled,
     "ppo_conv3x3_backward_weight_slabs_pooled_f32", b"no pooled-gradient kernel"),
]


@pytest.mark.parametrize("probe,geometry,call,entry,message", PROBE_THEN_LAUNCH, ids=[p[3] for p in PROBE_THEN_LAUNCH])
def test_probe_leaves_no_state(hip_lib, probe, geometry, call, entry, message):
    assert getattr(hip_lib, probe)(*geometry) == 1
    assert call(hip_lib, entry, **NO_KERNEL) == INVALID  # a launch, not another probe: it reports why
    assert message in hip_lib.ppo_last_error()


def test_pooled_wgrad_geometry(hip_lib):
    for call, entry in WGRAD_ENTRIES[4:]:
        for in_mode in (IN_NONE, IN_U8):
            assert call(hip_lib, entry, in_mode=in_mode, **NO_KERNEL) == INVALID
            assert b"no pooled-gradient kernel" in hip_lib.ppo_last_error()


def test_index_needs_uint8(hip_lib):
    geo = dict(cin=4, cout=16, h=84, w=84)
    for call, entry in ((pool_forward_indexed, "ppo_conv3x3_pool_forward_packed_indexed_f32"),
                        (weight_slabs_pooled_indexed, "ppo_conv3x3_backward_weight_slabs_pooled_indexed_f32")):
        assert call(hip_lib, entry, index=P, in_mode=IN_NONE, **geo) == INVALID
        assert b"the index applies to uint8 observations" in hip_lib.ppo_last_error()


@pytest.mark.parametrize("call,entry", FORWARD_ENTRIES, ids=[e[1] for e in FORWARD_ENTRIES])
def test_forward_n_and_null(hip_lib, call, entry):
    geo = dict(cin=4, cout=16, h=84, w=84)
    assert call(hip_lib, entry, n=-1, **geo) == INVALID
    assert call(hip_lib, entry, n=0, **geo) == OK
    assert call(hip_lib, entry, n=0, **NO_KERNEL) == OK  # an empty batch is done before the geometry is looked at
    assert call(hip_lib, entry, in_=None, n=1, **geo) == INVALID
    assert b"null pointer" in hip_lib.ppo_last_error()


@pytest.mark.parametrize("call,entry", WGRAD_ENTRIES, ids=[e[1] for e in WGRAD_ENTRIES])
def test_wgrad_n_and_null(hip_lib, call, entry):
    geo = dict(cin=4, cout=16, h=84, w=84)
    assert call(hip_lib, entry, n=0, **geo) == INVALID
    assert call(hip_lib, entry, n=-1, **geo) == INVALID
    assert call(hip_lib, entry, in_=None, n=1, **geo) == INVALID
    assert b"null pointer" in hip_lib.ppo_last_error()


@pytest.mark.parametrize("count", [0, 6])
def test_batch_count(hip_lib, count):
    for entry in ("ppo_conv3x3_backward_weight_slabs_batch_f32", "ppo_conv3x3_backward_weight_slabs_batch_mixed_f32"):
        assert weight_slabs_batch(hip_lib, entry, count=count, cin=32, cout=32, h=21, w=21) == INVALID
        assert b"count in 1..5" in hip_lib.ppo_last_error()
