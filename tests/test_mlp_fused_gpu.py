"""GPU: the fused MLP launches (csrc/mlp_fused.hip) called directly - ppo_mlp_supported, ppo_mlp_forward_f32,
ppo_mlp_train_workspace_floats, ppo_mlp_train_f32 through _lib.MlpNet / MlpGrads / MlpLoss, filled as
models._mlp_train fills them but over plain tensors - against the float64 step of tests/mlp_float64_torch.py, at the
smallest shapes that reach each path of the tiling (tests/test_mlp_float64_cpu.py checks what these seeded cases have to
satisfy for the comparison to mean something):

  tiny-1, tiny-17    F 1, H 16, NH 1, no head bias: 15 waves without a tile, the clamp address F - 1 = 0, a one-row tile,
                     the scalar row store of a single column, dbh = NULL
  ragged-F-*         F 13: fc1's 16-byte weight loads run past the rows' ends and, behind the last row, past the tensor;
                     scalar stores of heads and dheads (NH 7); 33, 37 and 145 rows (the last: ten row blocks of the
                     weight-gradient loop, so its second round of loads, with a ragged last block)
  wide-hidden        H 512: two tiles per wave in fc1, fc2 and both backward layers; 1152 weight-gradient tiles, more
                     than the 255 workgroups x 4 waves take in one round; 16-byte stores throughout
  wide-heads         F 530, H 272, NH 260: 17 tiles in every layer (wave 0 alone takes two), a second staging pass of
                     the observations (row stride above 512 floats), scalar store of the gathered rows, 1156
                     weight-gradient tiles, 19 row blocks, 244 head columns no loss reads
  humanoid           the product's own shape and minibatch

Every parameter tensor is a slice of one float32 arena of NaN with at least 64 NaN behind it: a read outside a tensor
poisons the result.  Every output buffer starts as NaN and carries 64 guard NaN behind it: nothing unwritten passes,
nothing written outside goes unseen."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import mlp_float64_torch as M  # noqa: E402
from ppo_amd import _lib  # noqa: E402

DEV = "cuda"
GUARD = 64
NAN = float("nan")
CASE_NAMES = list(M.CASES)  # smallest first
GRAD_NAMES = ("dw1", "db1", "dw2", "db2", "dwh", "dbh")
PREFILL = 7.0  # stat_sums before an accumulating call


def _p(t):
    return None if t is None else t.data_ptr()


def report(case, what, err, bar):
    print(f"MLP_FUSED_ERR {case} {what} {err:.3e} bar {bar:.0e}")


def close(case, what, got, want, bar):
    """|got - want| <= bar x the largest |want| (no NaN passes)."""
    got, want = got.double().cpu(), want.double()
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got.reshape(want.shape) - want).abs().max()) / scale
    report(case, what, err, bar)
    assert err <= bar, f"{case} {what}: {err:.3e} of the largest entry (bar {bar:.0e})"


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Out:
    """An output buffer of n floats, pre-filled, with GUARD NaN behind it."""

    def __init__(self, *shape, fill=NAN):
        self.n = 1
        for s in shape:
            self.n *= s
        self.buf = torch.full((self.n + GUARD,), NAN, device=DEV)
        self.buf[:self.n] = fill
        self.t = self.buf[:self.n].view(*shape)

    def cpu(self):
        """The contents, after checking that the guard behind them is untouched."""
        assert bool(torch.isnan(self.buf[self.n:]).all()), "written behind an output buffer"
        return self.t.cpu().clone()


class Net:
    """The parameters of a case as slices of one NaN arena (16-byte aligned slots, >= GUARD NaN behind each)."""

    def __init__(self, case):
        sizes = [0 if p is None else p.numel() for p in case["params"]]
        offs, o = [], GUARD
        for n in sizes:
            offs.append(o)
            o += (n + 3) // 4 * 4 + GUARD
        host = torch.full((o,), NAN)
        for p, off in zip(case["params"], offs):
            if p is not None:
                host[off:off + p.numel()] = p.reshape(-1)
        self.host = host
        self.arena = host.to(DEV)
        views = [None if p is None else self.arena[off:off + p.numel()] for p, off in zip(case["params"], offs)]
        self.net = _lib.MlpNet(w1=_p(views[0]), b1=_p(views[1]), w2=_p(views[2]), b2=_p(views[3]), wh=_p(views[4]),
                               bh=_p(views[5]), F=case["F"], H=case["H"], NH=case["NH"], act=1 if case["act"] == "tanh" else 2)
        self.log_std = None if case["log_std"] is None else case["log_std"].to(DEV)

    def check_untouched(self):
        assert same_bits(self.arena.cpu(), self.host), "the parameter arena (tensors or NaN guards) was written to"


_nets, _cache = {}, {}


def net_of(name):
    if name not in _nets:
        _nets[name] = Net(M.make_case(name))
    return _nets[name]


def forward(name, x, index=None, feats=True):
    """ppo_mlp_forward_f32 on the rows of x (through `index` when given) -> heads, h_pre, hact on the CPU."""
    case, net = M.make_case(name), net_of(name)
    B, H, NH = case["B"], case["H"], case["NH"]
    heads, h_pre, hact = Out(B, NH), Out(B, H), Out(B, H)
    xd = x.to(DEV).contiguous()
    idx = None if index is None else index.int().to(DEV)
    rc = _lib.load().ppo_mlp_forward_f32(_p(xd), ctypes.addressof(net.net), _p(idx), B, _p(heads.t),
                                         _p(h_pre.t) if feats else None, _p(hact.t) if feats else None,
                                         _lib.current_stream())
    _lib.check(rc, "ppo_mlp_forward_f32")
    torch.cuda.synchronize()
    net.check_untouched()
    if not feats:
        assert bool(torch.isnan(h_pre.cpu()).all()) and bool(torch.isnan(hact.cpu()).all())
    return heads.cpu(), h_pre.cpu(), hact.cpu()


def fill_loss(case, rows_d, stats, log_std, dls_rows):
    """_lib.MlpLoss for the case's loss kind over the device arrays rows_d (the argument order of the loss references)."""
    c, kind = case["c"], case["kind"]
    L = _lib.MlpLoss()
    L.kind, L.grad_scale, L.stats = kind, c["grad_scale"], _p(stats)
    if kind == M.VALUE:
        L.n_value_heads, L.returns, L.vf_coef, L.value_col = c["vh"], _p(rows_d[0]), c["vf_coef"], c["value_col"]
        L.tvf_col, L.n_tvf, L.tvf_stride, L.tvf_coef, L.tvf_keep_prob = c["tvf_col"], c["K"], c["stride"], c["tvf_coef"], 1.0
        if c["K"]:
            L.tvf_returns, L.tvf_weights = _p(rows_d[1]), _p(c["w_dev"])
    elif kind == M.DISTIL:
        L.n_actions, L.pred_col, L.n_pred, L.pred_stride = c["nA"], c["pred_col"], c["n_pred"], c["stride"]
        L.vector_targets, L.targets, L.old_policy, L.beta = c["vector"], _p(rows_d[0]), _p(rows_d[1]), c["beta"]
    elif kind == M.GAUSSIAN:
        L.n_actions, L.n_value_heads, L.eps_clip, L.vf_coef = c["nA"], c["vh"], c["eps"], c["vf_coef"]
        L.actions_f, L.old_log_pac, L.advantages, L.returns = (_p(t) for t in rows_d)
        L.log_std, L.dlog_std_rows = _p(log_std), _p(dls_rows)
    else:
        L.n_actions, L.n_value_heads, L.eps_clip, L.vf_coef, L.ent_coef = c["nA"], c["vh"], c["eps"], c["vf_coef"], c["ent_coef"]
        L.actions_i, L.old_log_pac, L.old_log_policy, L.advantages, L.returns = (_p(t) for t in rows_d)
    return L


def train(name, x, x_rows, index, rows, accumulate=False):
    """ppo_mlp_train_f32: x [x_rows or B, F] and the per-sample arrays `rows`, read through `index` where given ->
    dict of CPU tensors: the six gradients, dlog_std, heads, stats, stat_sums, dlog_std_rows, partials, workspace."""
    case, net = M.make_case(name), net_of(name)
    lib = _lib.load()
    B, F_, H, NH, kind, c = case["B"], case["F"], case["H"], case["NH"], case["kind"], dict(case["c"])
    n_stats = case["n_stats"]
    n_ls = c["nA"] if kind == M.GAUSSIAN else 3
    g = {"dw1": Out(H, F_), "db1": Out(H), "dw2": Out(H, H), "db2": Out(H), "dwh": Out(NH, H),
         "dbh": Out(NH) if case["head_bias"] else None, "dlog_std": Out(n_ls)}
    G = _lib.MlpGrads(**{k: (None if v is None else _p(v.t)) for k, v in g.items()}, n_log_std=n_ls)
    n_ws = int(lib.ppo_mlp_train_workspace_floats(B, F_, H, NH))
    assert n_ws == B * (4 * H + NH + F_)
    ws, heads, stats, sums = Out(n_ws), Out(B, NH), Out(B, n_stats), Out(n_stats, fill=PREFILL)
    dls_rows = Out(B, n_ls)
    partials, n_part = Out(256), ctypes.c_int(-1)
    xd = x.to(DEV).contiguous()
    rows_d = [t.to(DEV).contiguous() for t in rows]
    idx = None if index is None else index.int().to(DEV)
    c["w_dev"] = c["w"].to(DEV) if c.get("w") is not None else None
    L = fill_loss(dict(case, c=c), rows_d, stats.t, net.log_std, dls_rows.t)
    rc = lib.ppo_mlp_train_f32(_p(xd), ctypes.addressof(net.net), ctypes.addressof(G), _p(idx), x_rows, B, ctypes.addressof(L),
                               _p(ws.t), _p(heads.t), _p(sums.t), n_stats, 1 if accumulate else 0, _p(partials.t),
                               ctypes.byref(n_part), _lib.current_stream())
    _lib.check(rc, "ppo_mlp_train_f32")
    torch.cuda.synchronize()
    net.check_untouched()
    out = {k: (None if v is None else v.cpu()) for k, v in g.items()}
    out.update(heads=heads.cpu(), stats=stats.cpu(), stat_sums=sums.cpu(), dlog_std_rows=dls_rows.cpu(),
               partials=partials.cpu(), n_partials=n_part.value, ws=ws.cpu())
    return out


def indexed_step(name):
    """The training call the float64 comparison is made on, once per case: x and the per-sample arrays are sources of
    3 B rows, read through the index (every row moves)."""
    if name not in _cache:
        case = M.make_case(name)
        _cache[name] = train(name, case["x_big"], case["x_big"].shape[0], case["idx"], case["big"])
    return _cache[name]


def kernel_forward(name):
    key = ("fwd", name)
    if key not in _cache:
        _cache[key] = forward(name, M.make_case(name)["x"])
    return _cache[key]


def float64_step(name):
    """The float64 step the training call is compared with: for relu with the gate of the kernel's own forward."""
    key = ("ref", name)
    if key not in _cache:
        case = M.make_case(name)
        if case["act"] == "relu":
            gate = kernel_forward(name)[1] > 0
            _cache[key] = M.mlp_step_reference(case["params"], case["x"], "relu", case["kind"], case["c"], case["rows"],
                                               case["log_std"], relu_gate=gate)
        else:
            _cache[key] = case["ref"]
    return _cache[key]


# ====================================================================== 1, 2. forward
@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_against_float64(name):
    """heads, h_pre and hact within 1e-4 of the largest float64 entry (the bar of test_mlp_heads_match_float64); the same
    head bits without the feature outputs and with the rows read through an index out of 3 B rows; for relu the kernel's
    gate h_pre > 0 differs from float64's only where |h_pre| <= 1e-5 of the largest."""
    case = M.make_case(name)
    assert _lib.load().ppo_mlp_supported(case["F"], case["H"], case["NH"]) == 1
    assert M.mlp_supported(case["F"], case["H"], case["NH"])
    ref = case["ref"]
    heads, h_pre, hact = kernel_forward(name)
    for what, got in (("heads", heads), ("h_pre", h_pre), ("hact", hact)):
        close(name, f"forward {what}", got, ref[what], 1e-4)
    heads_only, _, _ = forward(name, case["x"], feats=False)
    assert same_bits(heads_only, heads)
    if case["B"] > 1:
        assert bool((case["idx"] != torch.arange(case["B"])).all())
    h_i, p_i, a_i = forward(name, case["x_big"], index=case["idx"])
    assert same_bits(h_i, heads) and same_bits(p_i, h_pre) and same_bits(a_i, hact)
    if case["act"] == "relu":
        p64 = ref["h_pre"]
        differs = (h_pre > 0) != (p64 > 0)
        worst = float(p64[differs].abs().max()) if bool(differs.any()) else 0.0
        report(name, f"relu gate: {int(differs.sum())} of {differs.numel()} differ, largest |h_pre| among them / max",
               worst / float(p64.abs().max()), 1e-5)
        assert worst <= 1e-5 * float(p64.abs().max())
        assert torch.equal(hact, torch.clamp(h_pre, min=0.0))
        assert 0.2 < float((h_pre > 0).float().mean()) < 0.8  # both sides of the kink occur
    else:
        assert float(hact.abs().max()) < 1.0


# ====================================================================== 3, 4, 5. training
@pytest.mark.parametrize("name", CASE_NAMES)
def test_training_against_float64(name):
    """Gradients within 2e-5 of each one's largest float64 entry (check_grads' bar), statistics columns within 1e-5
    (within()'s rule), the training call's heads the forward call's bits; nothing left unwritten, nothing for the head
    columns no loss reads, dlog_std zero unless gaussian; the partial sums of g^2 against the float64 sum over what the
    kernel itself wrote."""
    case, ref = M.make_case(name), float64_step(name)
    B, H, kind, used = case["B"], case["H"], case["kind"], case["used"]
    got = indexed_step(name)
    heads, _h_pre, hact = kernel_forward(name)
    assert same_bits(got["heads"], heads), "the training call's heads differ from the forward call's"
    assert same_bits(got["ws"][B * H:2 * B * H].view(B, H), hact)  # what the weight-gradient launch read as hact
    assert not bool(torch.isnan(got["ws"]).any())
    for gname, want in zip(GRAD_NAMES, ref["grads"]):
        if want is None:
            assert got[gname] is None
            continue
        assert not bool(torch.isnan(got[gname]).any()), f"{gname}: entries left unwritten"
        close(name, gname, got[gname], want, 2e-5)
    if bool((~used).any()):
        assert float(got["dwh"][~used].abs().max()) == 0.0 and float(got["dbh"][~used].abs().max()) == 0.0
    if kind == M.GAUSSIAN:
        close(name, "dlog_std", got["dlog_std"], ref["dlog_std"], 2e-5)
        close(name, "dlog_std_rows", got["dlog_std_rows"], ref["dlog_std_rows"], 1e-5)
        assert bool((got["dlog_std"] != 0).all())
    else:
        assert float(got["dlog_std"].abs().max()) == 0.0  # written: it was NaN
    live = [c for c in M.LIVE_STATS[kind] if not (kind == M.VALUE and case["c"]["K"] == 0 and c == 1)]
    for col in range(case["n_stats"]):
        if col in live:
            close(name, f"stats[{col}]", got["stats"][:, col], ref["stats"][:, col], 1e-5)
        else:
            assert float(got["stats"][:, col].abs().max()) == 0.0
    # stat_sums, overwritten (it held PREFILL) and accumulated: against the float64 column sums of the kernel's own rows.
    # Bar: each thread adds at most ceil(B / 8) <= 38 rows in order, 7 more adds fold the eighths, one more the
    # pre-fill: under 50 roundings of 6e-8 each on partial sums bounded by the column's sum of magnitudes -> 3e-6; 1e-5.
    own = got["stats"].double()
    l1 = own.abs().sum(0)
    acc = train(name, case["x_big"], case["x_big"].shape[0], case["idx"], case["big"], accumulate=True)
    for col in range(case["n_stats"]):
        scale = max(float(l1[col]), 1e-30)
        e_set = abs(float(got["stat_sums"][col]) - float(own[:, col].sum())) / scale
        e_acc = abs(float(acc["stat_sums"][col]) - (PREFILL + float(own[:, col].sum()))) / (scale + PREFILL)
        report(name, f"stat_sums[{col}] overwritten", e_set, 1e-5)
        report(name, f"stat_sums[{col}] accumulated", e_acc, 1e-5)
        assert e_set <= 1e-5 and e_acc <= 1e-5, col
    # ... and against float64's own column sums: the rows are each within 1e-5 of the column's largest entry (above), the
    # summation within 1e-5 of the sum of magnitudes <= B x the largest entry: 2e-5 x B x the largest entry
    for col in range(case["n_stats"]):
        scale = B * max(float(ref["stats"][:, col].abs().max()), 1e-30)
        e = abs(float(got["stat_sums"][col]) - float(ref["stat_sums"][col])) / scale
        report(name, f"stat_sums[{col}] vs float64, of B x the largest entry", e, 2e-5)
        assert e <= 2e-5, col
    assert same_bits(acc["stats"], got["stats"])
    # sum of squares: 1e-5 relative (a per-lane running sum of a few dozen terms, a 6-step wave tree and 3 adds: about 30
    # float32 roundings of positive terms, near 2e-6)
    n = got["n_partials"]
    assert 1 <= n <= 256
    assert bool(torch.isnan(got["partials"][n:]).all()) and not bool(torch.isnan(got["partials"][:n]).any())
    want_sq = sum(float((got[k].double() ** 2).sum()) for k in GRAD_NAMES + ("dlog_std",) if got[k] is not None)
    got_sq = float(got["partials"][:n].double().sum())
    report(name, "sum of squares", abs(got_sq - want_sq) / want_sq, 1e-5)
    assert want_sq > 0 and abs(got_sq - want_sq) <= 1e-5 * want_sq


# ====================================================================== 6. index forms
@pytest.mark.parametrize("name", CASE_NAMES)
def test_index_forms_give_the_same_bits(name):
    """x and the per-sample arrays read out of 3 B rows through the index = the gathered minibatch with the index on the
    per-sample arrays alone = everything gathered and no index; and the same call twice."""
    case = M.make_case(name)
    a = indexed_step(name)
    forms = {"gathered x, indexed arrays": train(name, case["x"], 0, case["idx"], case["big"]),
             "everything gathered": train(name, case["x"], 0, None, case["rows"]),
             "the same call again": train(name, case["x_big"], case["x_big"].shape[0], case["idx"], case["big"])}
    for form, b in forms.items():
        assert b["n_partials"] == a["n_partials"]
        for k in GRAD_NAMES + ("dlog_std", "heads", "stats", "stat_sums", "dlog_std_rows", "partials"):
            if a[k] is None:
                assert b[k] is None
                continue
            assert same_bits(a[k], b[k]), f"{name}, {form}: {k} differs"
    # the gathered rows the rows kernel left for the weight-gradient launch are the minibatch's
    B, F_, H, NH = case["B"], case["F"], case["H"], case["NH"]
    assert same_bits(a["ws"][B * (4 * H + NH):].view(B, F_), case["x"])


# ====================================================================== 7. refusals
def _plain_net(F_, H, NH):
    t = [torch.zeros(n, device=DEV) for n in (H * F_, H, H * H, H, NH * H, NH)]
    return t, _lib.MlpNet(w1=_p(t[0]), b1=_p(t[1]), w2=_p(t[2]), b2=_p(t[3]), wh=_p(t[4]), bh=_p(t[5]), F=F_, H=H, NH=NH,
                          act=1)


def _value_call(F_, H, NH, B, rows=None):
    """Both entry points on a valid value-loss call of the shape, every output NaN before -> (rc forward, message,
    rc train, message, n_partials, outputs)."""
    lib = _lib.load()
    rows = B if rows is None else rows
    keep, net = _plain_net(F_, H, NH)
    x = torch.zeros(max(rows, 1), F_, device=DEV)
    outs = {"heads": Out(max(rows, 1), NH), "dw1": Out(H, F_), "db1": Out(H), "dw2": Out(H, H), "db2": Out(H),
            "dwh": Out(NH, H), "dbh": Out(NH), "dlog_std": Out(3), "stats": Out(max(rows, 1), 4), "sums": Out(4),
            "ws": Out(max(rows, 1) * (4 * H + NH + F_)), "partials": Out(256)}
    G = _lib.MlpGrads(**{k: _p(outs[k].t) for k in GRAD_NAMES + ("dlog_std",)}, n_log_std=3)
    ret = torch.zeros(max(rows, 1), 1, device=DEV)
    L = _lib.MlpLoss()
    L.kind, L.grad_scale, L.stats, L.n_value_heads, L.returns = M.VALUE, 1.0, _p(outs["stats"].t), 1, _p(ret)
    L.vf_coef, L.tvf_keep_prob = 0.5, 1.0
    n_part = ctypes.c_int(-1)
    rc_f = lib.ppo_mlp_forward_f32(_p(x), ctypes.addressof(net), None, B, _p(outs["heads"].t), None, None,
                                   _lib.current_stream())
    msg_f = (lib.ppo_last_error() or b"").decode()
    rc_t = lib.ppo_mlp_train_f32(_p(x), ctypes.addressof(net), ctypes.addressof(G), None, 0, B, ctypes.addressof(L),
                                 _p(outs["ws"].t), _p(outs["heads"].t), _p(outs["sums"].t), 4, 0, _p(outs["partials"].t),
                                 ctypes.byref(n_part), _lib.current_stream())
    msg_t = (lib.ppo_last_error() or b"").decode()
    torch.cuda.synchronize()
    del keep
    return rc_f, msg_f, rc_t, msg_t, n_part.value, {k: v.cpu() for k, v in outs.items()}


def test_refusals_return_without_launching():
    """H not a multiple of 16: PPO_E_INVALID; a shape beyond the LDS limit: ppo_mlp_supported == 0 and both entry points
    fail with the LDS message; no rows: PPO_OK and *n_partials == 0.  Every output buffer keeps its NaN."""
    lib = _lib.load()
    rc_f, msg_f, rc_t, msg_t, n_part, outs = _value_call(4, 24, 2, 5)
    assert rc_f == -1 and rc_t == -1 and "multiple of 16" in msg_f and "multiple of 16" in msg_t and n_part == -1
    assert all(bool(torch.isnan(v).all()) for v in outs.values())
    assert lib.ppo_mlp_supported(4, 24, 2) == 0

    F_, H, NH = M.REFUSED_SHAPE
    assert lib.ppo_mlp_supported(F_, H, NH) == 0 and not M.mlp_supported(F_, H, NH)
    assert all(lib.ppo_mlp_supported(*s) == 1 for s in ((F_, 272, NH), (24, H, 20)))  # each extent alone is admitted
    rc_f, msg_f, rc_t, msg_t, n_part, outs = _value_call(F_, H, NH, 5)
    assert rc_f == -1 and rc_t == -1 and "bytes of LDS" in msg_f and "bytes of LDS" in msg_t
    assert str(M.mlp_lds_bytes(F_, H, NH)) in msg_t and str(M.mlp_lds_bytes(F_, H, NH)) in msg_f
    assert M.mlp_lds_bytes(F_, H, NH, train=False) <= 160 * 1024  # (the inference tile alone would fit: one rule for both)
    assert all(bool(torch.isnan(v).all()) for v in outs.values())

    rc_f, _, rc_t, _, n_part, outs = _value_call(13, 64, 7, 0, rows=0)
    assert rc_f == 0 and rc_t == 0 and n_part == 0
    assert all(bool(torch.isnan(v).all()) for v in outs.values())
