"""CPU: the global KL penalty (--gkl_*) and SIDE (--side_*) of the policy phase without a GPU - the flags parse only on a
line that enables them, with the reference's defaults (rl/config.py:378-394, 479-492); the new entry points are declared
alike in the header and the ctypes table and refuse bad arguments before any launch; and the float64 restatement of both
losses (tests/policy_reg_float64_torch.py) reproduces the reference's recorded loss and global_kl
(tests/golden/policy_reg_golden.npz) and has the closed-form gradients include/ppo_amd.h states."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
from conftest import GOLDEN, ROOT

import policy_reg_float64_torch as P
from oracle import model_torch as R
from ppo_amd import _lib
from ppo_amd.config import Config

INVALID = -1  # PPO_E_INVALID
BUF = (ctypes.c_float * 64)()  # stands in for every non-null pointer: nothing is read before the arguments are refused
PTR = ctypes.addressof(BUF)
LINE = ["--model_architecture=dual", "--env_type=synthetic"]


# ---------------------------------------------------------------------------------------------- flags
def test_flags_exist_only_on_a_line_that_enables_them():
    c = Config().setup(LINE + ["--gkl_penalty=0.3", "--gkl_samples=16", "--side_noise_std=1.0", "--side_period=3"])
    assert c._ignored == ["--gkl_penalty=0.3", "--gkl_samples=16", "--side_noise_std=1.0", "--side_period=3"]
    assert (c.gkl.enabled, c.gkl.penalty, c.gkl.samples, c.side.enabled, c.side.noise_std) == (False, 0.01, 1024, False, 0.1)
    c = Config().setup(LINE + ["--gkl_enabled=False", "--side_enabled=False"])
    assert c._ignored == ["--gkl_enabled=False", "--side_enabled=False"] and not c.gkl.enabled and not c.side.enabled
    for on in (["--gkl_enabled=True"], ["--gkl_enabled"], ["--gkl_enabled", "true"]):
        c = Config().setup(LINE + on + ["--gkl_penalty=0.3", "--gkl_samples=16", "--side_period=3"])
        assert c.gkl.enabled and (c.gkl.penalty, c.gkl.samples) == (0.3, 16)
        assert c._ignored == ["--side_period=3"] and not c.side.enabled
    c = Config().setup(LINE + ["--side_enabled=True", "--side_noise_std=1.5", "--side_period=3", "--gkl_samples=4"])
    assert c.side.enabled and (c.side.noise_std, c.side.period) == (1.5, 3)
    assert c._ignored == ["--gkl_samples=4"] and not c.gkl.enabled
    flat = Config().setup(LINE + ["--gkl_enabled=True"]).flatten()
    assert flat["gkl_samples"] == 1024 and "side_period" not in flat
    assert "gkl_samples" not in Config().setup(LINE).flatten()


def test_defaults_are_the_reference_s():
    c = Config().setup(LINE + ["--gkl_enabled=True", "--side_enabled=True"])
    assert c._ignored == []
    assert (c.gkl.enabled, c.gkl.threshold, c.gkl.penalty, c.gkl.source, c.gkl.samples) == (True, -1, 0.01, "rollout", 1024)
    assert (c.side.enabled, c.side.noise_std, c.side.period) == (True, 0.1, 10)


def test_an_unrelated_line_parses_as_before():
    c = Config().setup(LINE + ["--distil_beta=0.5", "--some_unknown_flag=3"])
    assert c._ignored == ["--some_unknown_flag=3"]
    assert not c.gkl.enabled and not c.side.enabled


def test_verify_refuses_bad_values():
    with pytest.raises(ValueError, match="rollout source"):
        Config().setup(LINE + ["--gkl_enabled=True", "--gkl_source=replay"])
    with pytest.raises(ValueError, match="gkl_samples"):
        Config().setup(LINE + ["--gkl_enabled=True", "--gkl_samples=0"])
    with pytest.raises(ValueError, match="side_period"):
        Config().setup(LINE + ["--side_enabled=True", "--side_period=0"])


# ---------------------------------------------------------------------------------------------- ABI
C_TYPES = {"const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "const int32_t *": ctypes.c_void_p,
           "void *": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float}


def header_prototype(name):
    """(result type, [argument ctypes]) of `name` as include/ppo_amd.h declares it."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppo_amd.h")).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        ctype = a[:a.rindex("*") + 1] if "*" in a else a.rsplit(" ", 1)[0]
        args.append(C_TYPES[ctype])
    return m.group(1), args


@pytest.mark.parametrize("name", ["ppo_ppo_loss_side_f32", "ppo_policy_kl_loss_f32"])
def test_header_and_ctypes_agree(hip_lib, name):
    res, args = header_prototype(name)
    assert res == "int" and _lib.SIGNATURES[name] == (ctypes.c_int, args)
    assert hasattr(hip_lib, name)


def test_side_entry_is_the_ppo_entry_plus_two_pointers():
    assert _lib.SIGNATURES["ppo_ppo_loss_side_f32"][1] == \
        _lib.SIGNATURES["ppo_ppo_loss_f32"][1][:-1] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def test_mlp_loss_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "ppo_amd.h")).read()
    body = re.search(r"typedef struct ppo_mlp_loss \{(.*?)\} ppo_mlp_loss;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
    assert names == [n for n, _t in _lib.MlpLoss._fields_]
    assert names[-2:] == ["side_target_logp", "side_penalty"]
    assert re.search(r"PPO_MLP_LOSS_POLICY_KL = 5\b", text) and _lib.MLP_LOSS_POLICY_KL == 5


KL_BAD = {
    "no actions": dict(nA=0),
    "too many actions": dict(nA=33, ldo=40),
    "row shorter than the policy": dict(ldo=3),
    "negative batch": dict(B=-1),
    "null heads": dict(heads=None),
    "null old policy": dict(old=None),
    "null dheads": dict(dheads=None),
}


@pytest.mark.parametrize("name", list(KL_BAD))
def test_kl_entry_refuses(hip_lib, name):
    a = dict(heads=PTR, B=8, ldo=8, nA=4, old=PTR, dheads=PTR)
    a.update(KL_BAD[name])
    rc = hip_lib.ppo_policy_kl_loss_f32(a["heads"], a["B"], a["ldo"], a["nA"], a["old"], 1.0, a["dheads"], None, None)
    assert rc == INVALID and hip_lib.ppo_last_error().startswith(b"ppo_policy_kl_loss_f32:")


def test_kl_entry_takes_an_empty_batch(hip_lib):
    assert hip_lib.ppo_policy_kl_loss_f32(None, 0, 8, 4, None, 1.0, None, None, None) == 0


@pytest.mark.parametrize("bad", ["no actions", "too many actions", "row shorter than policy + value", "null heads", "null returns"])
def test_side_entry_refuses(hip_lib, bad):
    a = dict(heads=PTR, B=8, ldo=8, nA=4, vh=1, returns=PTR)
    a.update({"no actions": dict(nA=0), "too many actions": dict(nA=33, ldo=40), "row shorter than policy + value": dict(ldo=4),
              "null heads": dict(heads=None), "null returns": dict(returns=None)}[bad])
    rc = hip_lib.ppo_ppo_loss_side_f32(a["heads"], a["B"], a["ldo"], a["nA"], a["vh"], PTR, PTR, None, PTR, a["returns"], 0.2, 0.01,
                                       0.5, 1.0, PTR, None, None, PTR, None, None)
    assert rc == INVALID and hip_lib.ppo_last_error().startswith(b"ppo_ppo_loss_side_f32:")


@pytest.mark.parametrize("bad,words", [(dict(n_actions=0), b"bad policy-kl arguments"), (dict(n_actions=33), b"bad policy-kl"),
                                       (dict(old_log_policy=None), b"bad policy-kl"), (dict(n_stats=2), b"one statistics column")])
def test_mlp_kl_kind_refuses(hip_lib, bad, words):
    net = _lib.MlpNet(w1=PTR, b1=PTR, w2=PTR, b2=PTR, wh=PTR, bh=PTR, F=4, H=16, NH=40, act=1)
    grads = _lib.MlpGrads(dw1=PTR, db1=PTR, dw2=PTR, db2=PTR, dwh=PTR, dbh=PTR, dlog_std=None, n_log_std=0)
    f = dict(n_actions=4, old_log_policy=PTR, n_stats=1)
    f.update(bad)
    loss = _lib.MlpLoss(kind=_lib.MLP_LOSS_POLICY_KL, grad_scale=1.0, stats=PTR, n_actions=f["n_actions"],
                        old_log_policy=f["old_log_policy"])
    n_partials = ctypes.c_int(0)
    rc = hip_lib.ppo_mlp_train_f32(PTR, ctypes.addressof(net), ctypes.addressof(grads), None, 0, 8, ctypes.addressof(loss),
                                   PTR, None, PTR, f["n_stats"], 0, PTR, ctypes.addressof(n_partials), None)
    msg = hip_lib.ppo_last_error()
    assert rc == INVALID and msg.startswith(b"ppo_mlp_train_f32:") and words in msg, msg


# ---------------------------------------------------------------------------------------------- the float64 restatement
GOLD = np.load(os.path.join(GOLDEN, "policy_reg_golden.npz"))
META = json.load(open(os.path.join(GOLDEN, "policy_reg_golden.json")))
COMBOS = ["gkl", "side", "both"]


def golden_heads(x, dt=torch.float64):
    """[policy | value] head rows of the golden's initial net on observations x, in dt."""
    sd = {k[len("init_"):]: torch.from_numpy(GOLD[k]).to(dt) for k in GOLD.files if k.startswith("init_")}
    out = R.mlp_forward(sd, torch.from_numpy(x).to(dt), activation="relu")
    return torch.cat([out["raw_policy"], out["value"]], 1)


def golden_case(tag):
    m = META[tag]
    data = {k: torch.from_numpy(GOLD[k]) for k in ("actions", "log_pac", "advantages", "returns", "global_log_policy",
                                                   "side_target_logp")}
    c = dict(nA=META["n_actions"], vh=1, eps=m["ppo_epsilon"], ent_coef=m["entropy_bonus"], vf_coef=m["ppo_vf_coef"],
             loss_scale=1.0, side=m["side_enabled"], gkl_penalty=m["gkl_penalty"] if m["gkl_enabled"] else None)
    return data, c


@pytest.mark.parametrize("tag", COMBOS)
def test_restatement_reproduces_the_golden(tag):
    """The reference ran in float32: its loss (a mean of 32 terms of order one) carries a few roundings of 6e-8, its
    global_kl (a mean of 96 terms below 0.1) the same relative to its size - 2e-6 of max(1, |value|), the bar
    tests/test_distil_golden_gpu.py puts on a loss."""
    data, c = golden_case(tag)
    loss, gkl, _gz, _ggz = P.policy_loss_ref(golden_heads(GOLD["prev_state"]), golden_heads(GOLD["global_states"]), data, c)
    want_loss, want_gkl = GOLD[f"{tag}_result"]
    assert abs(loss - want_loss) <= 2e-6 * max(1.0, abs(want_loss)), (loss, want_loss)
    if c["gkl_penalty"] is None:
        assert gkl is None and np.isnan(want_gkl)
    else:
        assert want_gkl > 1e-3, "old = new would pin nothing"
        assert abs(gkl - want_gkl) <= 2e-6 * max(1.0, abs(want_gkl)), (gkl, want_gkl)
        # the divisor is S * nA: the sum of the rows' KL over S alone is nA times as large
        lp = torch.log_softmax(golden_heads(GOLD["global_states"])[:, :c["nA"]], dim=1)
        rows = (lp.exp() * (lp - data["global_log_policy"].double())).sum(1)
        assert abs(float(rows.sum()) / (META["global_states"] * c["nA"]) - gkl) <= 1e-12


def random_rows(B, nA, ldo, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, ldo, generator=g)
    new_lp = torch.log_softmax(z[:, :nA], dim=1)
    actions = torch.randint(0, nA, (B,), generator=g).int()
    old_lp = P.tilted_log_policy(z[:, :nA], g)
    old_log_pac = new_lp[torch.arange(B), actions.long()] + 0.3 * torch.randn(B, generator=g)
    adv, ret = torch.randn(B, generator=g), torch.randn(B, 2, generator=g)
    target = torch.log_softmax(torch.randn(nA, generator=g), dim=0)
    return z, actions, old_log_pac, old_lp, adv, ret, target


@pytest.mark.parametrize("B,nA", [(1, 2), (65, 7), (130, 32)])
def test_kl_autograd_equals_the_closed_form(B, nA):
    z, _a, _olp, old, _adv, _ret, _t = random_rows(B, nA, 2 * nA + 3, 5 + nA)
    g_auto, kl_auto = P.policy_kl_ref(z, old, nA, 0.37)
    g_closed, kl_closed = P.policy_kl_closed_form(z, old, nA, 0.37)
    assert float(kl_auto.min()) > 0
    assert float((g_auto - g_closed).abs().max()) <= 1e-14 * max(1.0, float(g_closed.abs().max()))
    assert float((kl_auto - kl_closed).abs().max()) <= 1e-14
    assert float(g_auto[:, nA:].abs().max()) == 0.0


@pytest.mark.parametrize("ent_coef", [0.01, 0.0])
@pytest.mark.parametrize("B,nA", [(1, 2), (65, 7), (130, 32)])
def test_side_autograd_equals_the_closed_form(B, nA, ent_coef):
    z, actions, old_log_pac, old_lp, adv, ret, target = random_rows(B, nA, 2 * nA + 3, 11 + nA)
    c = dict(nA=nA, vh=2, eps=0.2, ent_coef=ent_coef, vf_coef=0.5, grad_scale=0.37)
    g_auto, stats, pen = P.ppo_side_ref(z, actions, old_log_pac, old_lp, adv, ret, target, c)
    g_closed = P.ppo_side_closed_form(z, actions, old_log_pac, adv, ret, target, c)
    assert float((g_auto - g_closed).abs().max()) <= 1e-13 * max(1.0, float(g_closed.abs().max()))
    # kl_penalty = -2 H - sum p t, and the gain column holds the SIDE gain
    lp = torch.log_softmax(z[:, :nA].double(), dim=1)
    assert float((pen - (-2 * stats[:, 1] - (lp.exp() * target.double()).sum(1))).abs().max()) <= 1e-13
    assert float((stats[:, 6] - (stats[:, 0] - ent_coef * pen - stats[:, 2])).abs().max()) <= 1e-13
    assert float(g_auto[:, nA + 2:].abs().max()) == 0.0
