"""CPU: the arguments of the distillation modes are refused before any launch (ppo_distil_loss_modes_f32 and the
distil loss of ppo_mlp_train_f32), the --distil_* flags parse with the reference's defaults and wording
(rl/config.py:329-347), and the head subset of --distil_max_heads is the reference's (rl/utils.py:82-104)."""
import ctypes
import os
import re

import pytest
from conftest import ROOT

from ppo_amd import _lib
from ppo_amd.config import Config
from ppo_amd.value_quality import even_sample_down

INVALID = -1  # PPO_E_INVALID
BUF = (ctypes.c_float * 64)()  # stands in for every non-null pointer: nothing is read before the arguments are refused
PTR = ctypes.addressof(BUF)

# (policy_loss, value_loss, delta, pred_actions, n_pred, vector_targets, n_active) -> the message's words
BAD = {
    "policy mode": (dict(policy_loss=3), b"unknown policy_loss 3"),
    "negative policy mode": (dict(policy_loss=-1), b"unknown policy_loss -1"),
    "value mode": (dict(value_loss=4), b"unknown value_loss 4"),
    "delta": (dict(delta=-0.5), b"delta must be >= 0"),
    "actions, two predictions": (dict(pred_actions=PTR, n_pred=2), b"pred_actions needs n_pred == 1"),
    "actions, vector targets": (dict(pred_actions=PTR, vector_targets=1), b"pred_actions needs n_pred == 1"),
    "n_active": (dict(n_active=6, n_pred=5), b"n_active 6 exceeds n_pred 5"),
}


def arguments(**kw):
    a = dict(policy_loss=0, value_loss=0, delta=0.0, l1_scale=0.0, pred_actions=None, n_pred=1, vector_targets=0, n_active=0)
    a.update(kw)
    return a


@pytest.mark.parametrize("name", list(BAD))
def test_modes_entry_refuses(hip_lib, name):
    kw, words = BAD[name]
    a = arguments(**kw)
    nA, ldo = 4, 32
    rc = hip_lib.ppo_distil_loss_modes_f32(PTR, 8, ldo, nA, nA + 1, a["n_pred"], 1, a["vector_targets"], PTR, None, PTR,
                                           None, 1.0, 1.0, PTR, None, None, a["policy_loss"], a["value_loss"], a["delta"],
                                           a["l1_scale"], a["pred_actions"], a["n_active"], None)
    msg = hip_lib.ppo_last_error()
    assert rc == INVALID and msg.startswith(b"ppo_distil_loss_modes_f32:") and words in msg, msg


def test_modes_entry_refuses_action_columns_beyond_the_row(hip_lib):
    rc = hip_lib.ppo_distil_loss_modes_f32(PTR, 8, 8, 4, 5, 1, 1, 0, PTR, None, PTR, None, 1.0, 1.0, PTR, None, None, 0, 0,
                                           0.0, 0.0, PTR, 0, None)
    assert rc == INVALID and b"ppo_distil_loss_modes_f32: pred_actions columns" in hip_lib.ppo_last_error()


@pytest.mark.parametrize("name", list(BAD))
def test_mlp_entry_refuses(hip_lib, name):
    kw, words = BAD[name]
    a = arguments(**kw)
    nA, NH = 4, 32
    net = _lib.MlpNet(w1=PTR, b1=PTR, w2=PTR, b2=PTR, wh=PTR, bh=PTR, F=4, H=16, NH=NH, act=1)
    grads = _lib.MlpGrads(dw1=PTR, db1=PTR, dw2=PTR, db2=PTR, dwh=PTR, dbh=PTR, dlog_std=None, n_log_std=0)
    loss = _lib.MlpLoss(kind=_lib.MLP_LOSS_DISTIL, grad_scale=1.0, n_actions=nA, pred_col=nA + 1, n_pred=a["n_pred"],
                        pred_stride=1, vector_targets=a["vector_targets"], targets=PTR, old_policy=PTR, beta=1.0,
                        distil_policy_loss=a["policy_loss"], distil_value_loss=a["value_loss"], distil_delta=a["delta"],
                        distil_l1_scale=a["l1_scale"], pred_actions=a["pred_actions"], n_active=a["n_active"])
    n_partials = ctypes.c_int(0)
    rc = hip_lib.ppo_mlp_train_f32(PTR, ctypes.addressof(net), ctypes.addressof(grads), None, 0, 8, ctypes.addressof(loss),
                                   PTR, None, None, 0, 0, PTR, ctypes.addressof(n_partials), None)
    msg = hip_lib.ppo_last_error()
    assert rc == INVALID and msg.startswith(b"ppo_mlp_train_f32:") and words in msg, msg


def test_mode_constants():
    assert _lib.DISTIL_POLICY_LOSSES == {"kl_policy": 0, "mse_policy": 1, "mse_logit": 2}
    assert _lib.DISTIL_VALUE_LOSSES == {"mse": 0, "l1": 1, "clipped_mse": 2, "huber": 3}
    header = open(os.path.join(ROOT, "include", "ppo_amd.h")).read()
    named = dict(re.findall(r"(PPO_DISTIL_(?:POLICY|VALUE)_[A-Z_0-9]+) = (\d+)", header))
    assert named == {"PPO_DISTIL_POLICY_KL": "0", "PPO_DISTIL_POLICY_MSE_POLICY": "1", "PPO_DISTIL_POLICY_MSE_LOGIT": "2",
                     "PPO_DISTIL_VALUE_MSE": "0", "PPO_DISTIL_VALUE_L1": "1", "PPO_DISTIL_VALUE_CLIPPED_MSE": "2",
                     "PPO_DISTIL_VALUE_HUBER": "3"}


LINE = ["--model_architecture=dual", "--env_type=synthetic"]


def test_new_flags_and_defaults():
    c = Config().setup(LINE)
    assert (c.distil.adv_lambda, c.distil.delta, c.distil.l1_scale) == (0.6, 0.1, 1 / 30)
    assert (c.distil.loss, c.distil.value_loss, c.distil.target, c.distil.max_heads) == ("kl_policy", "mse", "value", -1)
    assert not [u for u in c._ignored if u.startswith("--distil")]
    c = Config().setup(LINE + ["--distil_adv_lambda=0.9", "--distil_delta=0", "--distil_l1_scale=0.5",
                               "--distil_loss=mse_logit", "--distil_value_loss=huber", "--distil_target=advantage",
                               "--distil_max_heads=3"])
    assert (c.distil.adv_lambda, c.distil.delta, c.distil.l1_scale) == (0.9, 0.0, 0.5)
    assert (c.distil.loss, c.distil.value_loss, c.distil.target, c.distil.max_heads) == ("mse_logit", "huber", "advantage", 3)
    assert c._ignored == []
    for name in ("mse_logit", "mse_policy", "kl_policy"):
        assert Config().setup(LINE + [f"--distil_loss={name}"]).distil.loss == name
    for name in ("mse", "clipped_mse", "l1", "huber"):
        assert Config().setup(LINE + [f"--distil_value_loss={name}"]).distil.value_loss == name
    for name in ("return", "value", "advantage"):
        assert Config().setup(LINE + [f"--distil_target={name}"]).distil.target == name


def test_invalid_names_are_refused_at_start_up():
    with pytest.raises(ValueError, match="Invalid distil_loss kl"):
        Config().setup(LINE + ["--distil_loss=kl"])
    with pytest.raises(ValueError, match="Invalid distil target returns"):
        Config().setup(LINE + ["--distil_target=returns"])
    with pytest.raises(ValueError, match="distil loss"):
        Config().setup(LINE + ["--distil_value_loss=l2"])
    with pytest.raises(ValueError, match="distil_delta"):
        Config().setup(LINE + ["--distil_delta=-1"])


def test_a_line_without_the_flags_parses_as_before():
    c = Config().setup(LINE + ["--distil_beta=0.5", "--distil_order=before_policy"])
    assert (c.distil.beta, c.distil.order, c.distil.period, c.distil.batch_size) == (0.5, "before_policy", 1, -1)
    assert (c.distil.force_ext, c.distil.delay, c.distil.use_policy_opt) == (False, 0, False)
    assert c._ignored == []


@pytest.mark.parametrize("max_heads,want", [(-1, [0, 1, 2, 3, 4]), (0, []), (1, [4]), (3, [0, 2, 4]), (5, [0, 1, 2, 3, 4]),
                                            (9, [0, 1, 2, 3, 4])])
def test_head_subsets_are_the_reference_s(max_heads, want):
    assert [int(k) for k in even_sample_down(range(5), max_heads)] == want
