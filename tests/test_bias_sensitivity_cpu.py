"""CPU: what makes tests/test_trained_parameters_gpu.py able to fail.  Those tests hold the HIP networks, with every bias
non-zero (oracle/trained_params.perturbed_state_dict), to 1e-4 of the head row's largest entry against float64.  Here the
float64 oracles themselves are evaluated on the perturbed parameters and on every single-tensor bias fault
(oracle/trained_params.single_faults: a bias not added, read one channel off, or exchanged with its same-shaped
neighbour): each fault must move the fused head row [raw_policy | value | advantage (| tvf)] by at least 100 such bars,
so a kernel or a pointer table that commits one of them cannot pass the GPU tests.

Smallest distance over all faults at these seeds (bars of 1e-4 of the right row's largest entry), printed per network as
BIAS_SENSITIVITY lines:
    IMPALA (4,84,84) / 6 actions   405 bars   encoder.stacks.0.blocks.0.conv0.bias zeroed
    IMPALA (3,64,64) / 15 actions  211 bars   encoder.stacks.2.blocks.0.conv0.bias zeroed
    Nature (4,84,84)               527 bars   encoder.conv3.bias zeroed
    MLP (11,) tanh, TVF heads      618 bars   encoder.fc1.bias rotated by one channel
    MLP (11,) relu, TVF heads      603 bars   encoder.fc1.bias zeroed
(Perturbation seed 21.  A seed is only as good as its smallest draw: value_head.bias is one number, and a seed that draws
it near zero leaves "value_head.bias zeroed" closer than 100 bars - take another seed then, never another factor.)
"""
import pytest

torch = pytest.importorskip("torch")

from oracle import model_torch as R  # noqa: E402
from oracle import trained_params as T  # noqa: E402
from ppo_amd import models  # noqa: E402

BAR = 1e-4      # of the head row's largest entry: the forward bar of the GPU tests
MIN_BARS = 100  # every fault must be at least this many bars away


def impala_case(dims, n_actions):
    torch.manual_seed(11)
    init = models.init_parameters(models.ImpalaSpec(dims, hidden_units=256), n_actions, 1, 0.1, True)
    x = torch.randint(0, 256, (4, *dims), generator=torch.Generator().manual_seed(5)).double() / 255.0
    return init, x, lambda sd: T.head_row(R.forward(sd, x))


def nature_case():
    torch.manual_seed(11)
    init = models.init_parameters(models.NatureSpec((4, 84, 84), hidden_units=512), 6, 1, 0.1, True)
    x = torch.randint(0, 256, (4, 4, 84, 84), generator=torch.Generator().manual_seed(5)).double() / 255.0
    return init, x, lambda sd: T.nature_forward(sd, x)


def mlp_case(activation):
    torch.manual_seed(11)
    init = models.init_parameters(models.MLPSpec((11,), hidden_units=64), 3, 1, 0.1, True, n_tvf=4)
    x = torch.randn(8, 11, generator=torch.Generator().manual_seed(5)).double()
    return init, x, lambda sd: T.head_row(R.mlp_forward(sd, x, activation))


CASES = {"impala84": lambda: impala_case((4, 84, 84), 6), "impala64": lambda: impala_case((3, 64, 64), 15),
         "nature": nature_case, "mlp_tanh": lambda: mlp_case("tanh"), "mlp_relu": lambda: mlp_case("relu")}


@pytest.mark.parametrize("case", list(CASES))
def test_every_single_bias_fault_moves_the_head_row_by_100_bars(case):
    init, _x, row_of = CASES[case]()
    sd = T.perturbed_state_dict(init, seed=21)
    for name in T.bias_names(sd):
        assert float(sd[name].abs().max()) > 0 and float(init[name].abs().max()) == 0, name  # perturbed, from zero
        assert bool((sd[name] != 0).all()), name
    assert float(sd["log_std"].abs().min()) > 0
    for name, t in init.items():
        if not name.endswith(".bias") and name != "log_std":
            assert torch.equal(sd[name], t), name  # weights as they were
    sd64 = T.as_double(sd)
    with torch.no_grad():
        right = row_of(sd64)
        scale = float(right.abs().max())
        worst, n = (float("inf"), None), 0
        for label, faulty in T.single_faults(sd64):
            d = float((row_of(faulty) - right).abs().max()) / (BAR * scale)
            n += 1
            worst = min(worst, (d, label))
            assert d >= MIN_BARS, (label, d)
    labels = [label for label, _ in T.single_faults(sd64)]
    assert len(set(labels)) == n
    n_bias = len(T.bias_names(sd))
    n_wide = sum(sd[k].numel() > 1 for k in T.bias_names(sd))
    n_swaps = {"impala84": 6, "impala64": 6, "nature": 1, "mlp_tanh": 1, "mlp_relu": 1}[case]
    assert n == n_bias + n_wide + n_swaps
    print(f"BIAS_SENSITIVITY {case} faults={n} smallest distance={worst[0]:.0f} bars ({worst[1]}) bar={MIN_BARS}")


def test_perturbed_state_dict_is_a_seeded_copy():
    init, _x, _row = CASES["mlp_tanh"]()
    a, b, c = (T.perturbed_state_dict(init, seed=s) for s in (1, 1, 2))
    assert all(torch.equal(a[k], b[k]) for k in a) and list(a) == list(init)
    assert not torch.equal(a["encoder.fc1.bias"], c["encoder.fc1.bias"])
    assert float(init["encoder.fc1.bias"].abs().max()) == 0  # the argument is left alone
    wide = T.perturbed_state_dict(init, seed=1, sigma=1.0)
    assert torch.allclose(wide["encoder.fc1.bias"], a["encoder.fc1.bias"] * 10, rtol=1e-6)
    assert torch.equal(wide["log_std"], a["log_std"])  # N(0, 0.3) whatever sigma is
