"""CPU: the input conditions of tests/test_mlp_fused_gpu.py, checked on the float64 reference alone
(tests/mlp_float64_torch.py) - what has to hold of the seeded cases for the GPU comparison to mean something: no ratio
on a clip threshold, a gradient in every parameter the loss reaches, bars that plain float32 arithmetic meets at these
shapes, and shapes the kernel's own LDS rule admits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mlp_float64_torch as M  # noqa: E402

CASE_NAMES = list(M.CASES)
# bytes of LDS of a training tile (csrc/mlp_fused.hip, mlp_lds_bytes), worked out by hand from the strides
LDS_BYTES = {(1, 16, 1): 20224, (13, 64, 7): 28416, (24, 512, 20): 143104, (530, 272, 260): 151296,
             (377, 256, 163): 120576, M.REFUSED_SHAPE: 208640}


def rel(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def test_the_cases_cover_every_loss_kind_past_128_rows_and_with_a_ragged_tile():
    for kind in (M.VALUE, M.DISTIL, M.GAUSSIAN, M.PPO):
        of_kind = [c for c in M.CASES.values() if c["kind"] == kind]
        assert any(c["B"] > 128 for c in of_kind), kind
        assert any(c["B"] % 16 for c in of_kind), kind


@pytest.mark.parametrize("name", CASE_NAMES)
def test_no_ratio_sits_on_a_clip_threshold(name):
    """PPO and gaussian cases: every | |rho - 1| - eps | > 1e-5 in float64, for all rows with none left out (a condition
    on the seed), no advantage is zero, and ratios fall on both sides of the clip range and inside it."""
    case = M.make_case(name)
    if case["kind"] not in (M.GAUSSIAN, M.PPO):
        assert case["ref"]["rho"] is None
        return
    rho, eps = case["ref"]["rho"], case["c"]["eps"]
    margin = float(((rho - 1.0).abs() - eps).abs().min())
    adv = case["rows"][2] if case["kind"] == M.GAUSSIAN else case["rows"][3]
    print(f"{name}: smallest | |rho - 1| - eps | = {margin:.3e} over {rho.numel()} ratios, "
          f"{int((rho > 1 + eps).sum())} above, {int((rho < 1 - eps).sum())} below the clip range")
    assert margin > 1e-5
    assert float(adv.abs().min()) > 0.0
    assert bool((rho > 1 + eps).any()) and bool((rho < 1 - eps).any()) and bool(((rho - 1).abs() < eps).any())
    # clipped entries (no gradient through the ratio) and unclipped ones both occur
    dpol = case["ref"]["dheads"][:, :case["c"]["nA"]]
    if case["kind"] == M.GAUSSIAN:
        assert bool((dpol == 0).any()) and bool((dpol != 0).any())
    else:  # (the entropy bonus reaches every logit: the ratio's share is what the clip removes)
        clipped = case["ref"]["stats"][:, 3]
        assert float(clipped.min()) == 0.0 and float(clipped.max()) == 1.0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_reached_parameter_has_a_gradient(name):
    case = M.make_case(name)
    ref, used = case["ref"], case["used"]
    for gname, g in zip(("dw1", "db1", "dw2", "db2", "dwh", "dbh"), ref["grads"]):
        if g is None:
            assert gname == "dbh" and not case["head_bias"]
            continue
        assert float(g.abs().max()) > 0.0, gname
    dwh = ref["grads"][4]
    assert bool((dwh[used].abs().amax(1) > 0).all()), "a head row the loss reads has no gradient"
    if bool((~used).any()):
        assert float(dwh[~used].abs().max()) == 0.0
    if case["kind"] in (M.VALUE, M.DISTIL):  # (a clipped ratio of the policy kinds rightly passes no gradient)
        assert float(ref["dheads"][:, used].abs().min()) > 0.0  # every sample reaches every column the loss reads
    live = [c for c in M.LIVE_STATS[case["kind"]] if not (case["kind"] == M.VALUE and case["c"]["K"] == 0 and c == 1)]
    for col in range(case["n_stats"]):
        nz = float(ref["stats"][:, col].abs().max()) > 0.0
        assert nz == (col in live), (col, nz)
    if case["kind"] == M.GAUSSIAN:
        assert float(ref["dlog_std"].abs().min()) > 0.0
    else:
        assert ref["dlog_std"] is None


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_bars_are_attainable_in_float32(name):
    """The same reference evaluated in float32 on the CPU meets, against float64, the bars the GPU test holds the kernels
    to: 1e-4 forward, 2e-5 gradients, 1e-5 statistics (for relu with float64's gate: the kinks are shared there too)."""
    case = M.make_case(name)
    ref = case["ref"]
    gate = ref["h_pre"] > 0 if case["act"] == "relu" else None
    f32 = M.mlp_step_reference(case["params"], case["x"], case["act"], case["kind"], case["c"], case["rows"],
                               case["log_std"], dt=torch.float32, relu_gate=gate)
    assert f32["heads"].dtype == torch.float32
    for k in ("heads", "h_pre", "hact"):
        e = rel(f32[k], ref[k])
        print(f"MLP_F32_ERR {name} {k} {e:.3e} bar 1e-4")
        assert e <= 1e-4, k
    for gname, g, want in zip(("dw1", "db1", "dw2", "db2", "dwh", "dbh"), f32["grads"], ref["grads"]):
        if want is None:
            continue
        e = rel(g, want)
        print(f"MLP_F32_ERR {name} {gname} {e:.3e} bar 2e-5")
        assert e <= 2e-5, gname
    if ref["dlog_std"] is not None:
        e = rel(f32["dlog_std"], ref["dlog_std"])
        print(f"MLP_F32_ERR {name} dlog_std {e:.3e} bar 2e-5")
        assert e <= 2e-5
    for col in range(case["n_stats"]):
        if float(ref["stats"][:, col].abs().max()) == 0.0:
            assert float(f32["stats"][:, col].abs().max()) == 0.0
            continue
        e = rel(f32["stats"][:, col], ref["stats"][:, col])
        print(f"MLP_F32_ERR {name} stats[{col}] {e:.3e} bar 1e-5")
        assert e <= 1e-5, col


def test_the_cases_agree_with_the_kernels_own_lds_rule():
    """lds_stride / mlp_lds_bytes restated in Python: the hand-worked byte counts, every case admitted, the refused shape
    refused - and the library's ppo_mlp_supported (a host function: no GPU needed) where the library is built."""
    assert [M.lds_stride(n) for n in (1, 16, 17, 32, 64, 260, 272, 512, 530)] == [36, 36, 36, 36, 68, 292, 292, 516, 548]
    shapes = sorted({(c["F"], c["H"], c["NH"]) for c in M.CASES.values()}) + [M.REFUSED_SHAPE]
    assert set(shapes) == set(LDS_BYTES)
    for s in shapes:
        assert M.mlp_lds_bytes(*s) == LDS_BYTES[s], s
        assert M.mlp_supported(*s) == (s != M.REFUSED_SHAPE), s
    assert not M.mlp_supported(4, 24, 2)  # H not a multiple of 16
    try:
        from ppo_amd import _lib
        lib = _lib.load()
    except Exception as e:  # not built on this host: the constants above are the check
        print(f"library not loaded ({type(e).__name__}): Python formula checked against the table only")
        return
    for s in shapes + [(4, 24, 2), (377, 256, 1), (1, 16, 163)]:
        assert bool(lib.ppo_mlp_supported(*s)) == bool(M.mlp_supported(*s)), s
    # the boundary of the 160 KiB rule, found by the Python formula: the library flips at the same F
    H, NH = 512, 20
    fs = np.array([f for f in range(16, 2048, 16)])
    ok = np.array([M.mlp_supported(int(f), H, NH) for f in fs])
    assert ok[0] and not ok[-1]
    edge = int(fs[ok][-1])
    assert lib.ppo_mlp_supported(edge, H, NH) == 1 and lib.ppo_mlp_supported(edge + 1, H, NH) == 0
