"""GPU: ppo_policy_act_f32, ppo_gaussian_act_f32 and ppo_ppo_loss_f32 called directly on tiny tensors, against float64
(tests/policy_optim_float64.py has the references, the data sets and how every bar is derived;
tests/test_policy_optim_float64_cpu.py checks, without a GPU, that the bars reject wrong variants).  Every output sits in a
sentinel-filled buffer whose guards must survive, every launch runs twice and must give the same bits.  The
internal-generator tests pin which counter feeds which (row, action): offset + b nA + a.

Prints POLOPT64_ERR <case> kernel max, float32 max, ratio, bar; profiles/policy_optim_float64.md records them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import policy_optim_float64 as R  # noqa: E402
from ppo_amd import _lib  # noqa: E402


def _p(t):
    return None if t is None else t.data_ptr()


def _env():
    return _lib.load(), torch.device("cuda"), _lib.current_stream()


def _rows(ref, B):
    return {k: (v[:B] if torch.is_tensor(v) else v) for k, v in ref.items()}


def run_act(lib, st, dev, heads, nA, vh, T, u, seed, offset, greedy):
    """ppo_policy_act_f32 twice into guarded outputs -> {name: cpu tensor}."""
    B, ldo = heads.shape
    runs = []
    for _ in range(2):
        o = {"log_policy": R.guarded((B, nA), dev), "actions": R.guarded((B,), dev, dtype=torch.int32, sentinel=-7),
             "log_pac": R.guarded((B,), dev), "raw_policy": R.guarded((B, nA), dev)}
        if vh:
            o["values"] = R.guarded((B, vh), dev)
        _lib.check(lib.ppo_policy_act_f32(_p(heads), B, ldo, nA, T, _p(u), seed, offset, greedy, _p(o["log_policy"][1]),
                                          _p(o["actions"][1]), _p(o["log_pac"][1]), _p(o["raw_policy"][1]),
                                          _p(o["values"][1]) if vh else None, vh, st), "policy_act")
        torch.cuda.synchronize()
        for name, (buf, out) in o.items():
            assert R.guards_intact(buf, out, -7 if name == "actions" else R.SENTINEL), f"{name}: wrote outside its output"
        runs.append({k: v[1].cpu() for k, v in o.items()})
    for k in runs[0]:
        assert R.same_bits(runs[0][k], runs[1][k]), f"{k}: two launches on the same inputs differ"
    return runs[0]


def check_act(got, z, heads, ref, bar, nA, vh, what):
    """log_policy per element, log_pac, the copies and the actions of the clear rows; -> the log-probability error."""
    B = z.shape[0]
    e = R.lp_err(got["log_policy"], ref)
    assert e <= bar, f"{what}: log_policy {e:.3e} over the bar {bar:.3e}"
    act = got["actions"].long()
    assert int(act.min()) >= 0 and int(act.max()) < nA
    assert R.same_bits(got["log_pac"], got["log_policy"].gather(1, act[:, None])[:, 0]), f"{what}: log_pac is not log_policy[action]"
    e_pac = R.rel_err(got["log_pac"].double().numpy(), ref["lp"].gather(1, act[:, None])[:, 0].numpy(), ref["scale"].numpy())
    assert e_pac <= bar, f"{what}: log_pac {e_pac:.3e} over the bar {bar:.3e}"
    assert R.same_bits(got["raw_policy"], z), f"{what}: raw_policy is not the logits"
    if vh:
        assert R.same_bits(got["values"], heads[:, nA:nA + vh].contiguous()), f"{what}: values are not the value columns"
    if "action" in ref:
        clear = R.clear_rows(ref, bar)
        assert int((~clear).sum()) <= int(R.EXCLUDED_CAP * B), f"{what}: {int((~clear).sum())} of {B} rows left out"
        assert torch.equal(act[clear], ref["action"][clear]), f"{what}: an action is not the float64 argmax"
    return max(e, e_pac)


@pytest.mark.parametrize("data", R.ACT_DATA)
@pytest.mark.parametrize("nA", R.ACT_NA)
def test_policy_act_supplied_uniforms_and_greedy(nA, data):
    lib, dev, st = _env()
    z_all, u_all = R.act_logits(nA, data), R.act_uniforms(nA, data)
    for T in R.ACT_T:
        ref_all = R.policy_act_ref(z_all, T, u_all)
        f32 = R.lp_err(R.policy_act_f32(z_all, T)["lp"], ref_all)
        bar, worst = R.bar_from(f32), 0.0
        for B in R.ACT_B:
            z, ref = z_all[:B].contiguous(), _rows(ref_all, B)
            u = u_all[:B].contiguous().to(dev)
            for vh in R.ACT_VH:
                heads = R.act_heads(z, vh)
                hd = heads.to(dev)
                what = f"nA={nA} {data} T={T} B={B} vh={vh}"
                got = run_act(lib, st, dev, hd, nA, vh, T, u, 0, 0, 0)
                worst = max(worst, check_act(got, z, heads, ref, bar, nA, vh, what))
                greedy = run_act(lib, st, dev, hd, nA, vh, T, None, 0, 0, 1)
                assert torch.equal(greedy["actions"].long(), ref["greedy"]), f"{what}: greedy is not the first argmax"
                assert R.same_bits(greedy["log_policy"], got["log_policy"])
                assert R.same_bits(greedy["log_pac"], greedy["log_policy"].gather(1, ref["greedy"][:, None])[:, 0])
        R.report(f"policy_act nA={nA} {data} T={T} log_policy+log_pac", worst, f32)
    if data == "equal_row":
        assert int(ref_all["greedy"][0]) == 0 and float(ref_all["lp"][0].max() - ref_all["lp"][0].min()) == 0.0


@pytest.mark.parametrize("nA,seed,offset", R.GEN_CASES)
def test_policy_act_internal_generator_counter_layout(nA, seed, offset):
    """uniform = NULL: the actions are the float64 argmax of scores built from uniform01_ref(seed, offset + b nA + a)."""
    lib, dev, st = _env()
    assert seed > 2 ** 32 and offset > 0
    z = R.act_logits(nA, "plain")
    B = z.shape[0]
    ref = R.policy_act_ref(z, 1.0, R.gen_uniforms(seed, offset, B, nA))
    f32 = R.lp_err(R.policy_act_f32(z, 1.0)["lp"], ref)
    for vh in R.ACT_VH:
        heads = R.act_heads(z, vh)
        got = run_act(lib, st, dev, heads.to(dev), nA, vh, 1.0, None, seed, offset, 0)
        e = check_act(got, z, heads, ref, R.bar_from(f32), nA, vh, f"generator nA={nA} vh={vh}")
        R.report(f"policy_act generator nA={nA} vh={vh}", e, f32)
    # another layout gives other actions: the comparison above is not vacuous
    other = R.policy_act_ref(z, 1.0, R.gen_uniforms(seed, offset + 1, B, nA))
    assert not torch.equal(other["action"], ref["action"])


def test_dense_heads_act_forward_draws_the_same_counters():
    """The wave-per-sample caller (gemm.hip's finalize launch): ppo_dense_heads_act_forward_f32 at the shapes of
    test_dense_heads_with_action_sampling_is_bitwise_the_separate_launches, bsz = 37, against float64 on the head rows it
    wrote."""
    lib, dev, st = _env()
    bsz, nA, K, H, vh = 37, 6, 3872, 256, 2
    NH = nA + vh + 3
    seed, offset = 0x1234567890ABCDEF, 987654321 * nA
    g = torch.Generator().manual_seed(bsz * 31 + nA)
    x = torch.randn(bsz, K, generator=g).to(dev)
    W = (torch.randn(H, K, generator=g) * 0.02).to(dev)
    b = torch.randn(H, generator=g).to(dev)
    Wh = (torch.randn(NH, H, generator=g) * 0.1).to(dev)
    bh = torch.randn(NH, generator=g).to(dev)
    ws_bytes = lib.ppo_gemm_workspace_bytes(bsz, H, K)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes // 4, device=dev)
    runs = []
    for _ in range(2):
        h, o = torch.empty(bsz, H, device=dev), torch.empty(bsz, NH, device=dev)
        out = {"log_policy": R.guarded((bsz, nA), dev), "actions": R.guarded((bsz,), dev, dtype=torch.int32, sentinel=-7),
               "log_pac": R.guarded((bsz,), dev), "raw_policy": R.guarded((bsz, nA), dev), "values": R.guarded((bsz, vh), dev)}
        _lib.check(lib.ppo_dense_heads_act_forward_f32(_p(x), 1, _p(W), _p(b), _p(Wh), _p(bh), 1, _p(h), _p(o), bsz, K, H, NH,
                                                       _p(ws), ws_bytes, nA, 1.0, seed, offset, _p(out["log_policy"][1]),
                                                       _p(out["actions"][1]), _p(out["log_pac"][1]), _p(out["raw_policy"][1]),
                                                       _p(out["values"][1]), vh, st), "dense_heads_act")
        torch.cuda.synchronize()
        for name, (buf, v) in out.items():
            assert R.guards_intact(buf, v, -7 if name == "actions" else R.SENTINEL), name
        runs.append(({k: v[1].cpu() for k, v in out.items()}, o.cpu()))
    for k in runs[0][0]:
        assert R.same_bits(runs[0][0][k], runs[1][0][k]), k
    got, heads = runs[0]
    z = heads[:, :nA].contiguous()
    ref = R.policy_act_ref(z, 1.0, R.gen_uniforms(seed, offset, bsz, nA))
    f32 = R.lp_err(R.policy_act_f32(z, 1.0)["lp"], ref)
    e = check_act(got, z, heads, ref, R.bar_from(f32), nA, vh, "dense_heads_act")
    R.report("dense_heads_act bsz=37 nA=6", e, f32)
    assert len(set(got["actions"].tolist())) > 1


@pytest.mark.parametrize("a_star", [0, 5])
@pytest.mark.parametrize("counter", R.BAD_COUNTERS[:2])
def test_policy_act_the_draw_that_rounded_to_one(counter, a_star):
    """Seed 123: `counter` draws k = 2^24 - 1.  Before the clamp in uniform01 that gave u == 1.0f, a Gumbel score of +inf,
    and action a* - probability e^-40 / 5 - was taken, with its true log-probability in log_pac."""
    lib, dev, st = _env()
    z, u, offset = R.bad_draw_case(counter, a_star)
    ref = R.policy_act_ref(z, 1.0, u)
    heads = R.act_heads(z, 0)
    got = run_act(lib, st, dev, heads.to(dev), z.shape[1], 0, 1.0, None, R.BAD_SEED, offset, 0)
    action, log_pac = int(got["actions"][0]), float(got["log_pac"][0])
    print(f"POLOPT64_U1 counter={counter} a*={a_star} action={action} log_pac={log_pac:.6f} "
          f"float64 action={int(ref['action'][0])} log_pac={float(ref['lp'][0, int(ref['action'][0])]):.6f}")
    assert action != a_star, f"action {action} = a*, log_pac {log_pac}"
    assert action == int(ref["action"][0])
    assert np.isfinite(log_pac)
    f32 = R.lp_err(R.policy_act_f32(z, 1.0)["lp"], ref)
    check_act(got, z, heads, ref, R.bar_from(f32), z.shape[1], 0, f"counter={counter} a*={a_star}")


# --------------------------------------------------------------------------------------------- gaussian action step
def run_gauss(lib, st, dev, heads, nA, vh, log_std, normal, seed, offset, deterministic):
    B, ldo = heads.shape
    runs = []
    for _ in range(2):
        o = {k: R.guarded(s, dev) for k, s in (("actions", (B, nA)), ("log_pac", (B, nA)), ("raw_policy", (B, nA)), ("values", (B, vh)))}
        _lib.check(lib.ppo_gaussian_act_f32(_p(heads), B, ldo, nA, _p(log_std), _p(normal), seed, offset, deterministic,
                                            _p(o["actions"][1]), _p(o["log_pac"][1]), _p(o["raw_policy"][1]), _p(o["values"][1]),
                                            vh, st), "gaussian_act")
        torch.cuda.synchronize()
        for name, (buf, out) in o.items():
            assert R.guards_intact(buf, out), f"{name}: wrote outside its output"
        runs.append({k: v[1].cpu() for k, v in o.items()})
    for k in runs[0]:
        assert R.same_bits(runs[0][k], runs[1][k]), f"{k}: two launches on the same inputs differ"
    return runs[0]


@pytest.mark.parametrize("B,nA", [(1, 1), (85, 3), (51, 5), (257, 1)])
def test_gaussian_act_against_float64(B, nA):
    """B nA in {1, 255, 257}: the internal generator (Box-Muller on counters 2 (offset + i), 2 (offset + i) + 1), supplied
    normals and deterministic = 1."""
    lib, dev, st = _env()
    vh, seed, offset = 2, 0xABCDEF0123456789, 1234567891
    g = torch.Generator().manual_seed(B * 13 + nA)
    heads = torch.full((B, nA + vh + 3), R.ACT_SENTINEL)
    heads[:, :nA + vh] = torch.randn(B, nA + vh, generator=g) * 2.0
    log_std = (torch.randn(nA, generator=g) * 0.5 - 0.5)
    mu = heads[:, :nA].contiguous()
    hd, lsd = heads.to(dev), log_std.to(dev)

    def judge(tag, got, ref, f32):
        for name, key in (("actions", "action"), ("log_pac", "log_pac")):
            e32 = R.rel_err(f32[key], ref[key], ref[key + "_scale"])
            e = R.rel_err(got[name].double().numpy(), ref[key], ref[key + "_scale"])
            bar = R.report(f"gaussian_act B={B} nA={nA} {tag} {name}", e, e32)
            assert e <= bar, f"{tag} {name}: {e:.3e} over the bar {bar:.3e}"
        assert R.same_bits(got["raw_policy"], mu) and R.same_bits(got["values"], heads[:, nA:nA + vh].contiguous())

    normal, u1, u2 = R.gaussian_normals_ref(seed, offset, B * nA)
    judge("generator", run_gauss(lib, st, dev, hd, nA, vh, lsd, None, seed, offset, 0),
          R.gaussian_act_ref(mu, log_std, normal.reshape(B, nA)), R.gaussian_act_f32(mu, log_std, u1=u1, u2=u2))
    given = torch.randn(B, nA, generator=g)
    judge("normals", run_gauss(lib, st, dev, hd, nA, vh, lsd, given.to(dev), 0, 0, 0),
          R.gaussian_act_ref(mu, log_std, given.double().numpy()), R.gaussian_act_f32(mu, log_std, normal=given))
    det = run_gauss(lib, st, dev, hd, nA, vh, lsd, given.to(dev), seed, offset, 1)
    assert R.same_bits(det["actions"], mu) and R.same_bits(det["raw_policy"], mu)
    # -(0 * 0) / (2 var) - log_std - log sqrt(2 pi): two float32 subtractions from -0
    want = (np.float32(-0.0) - log_std.numpy()) - np.float32(R.LOG_SQRT_2PI)
    assert R.same_bits(det["log_pac"], torch.from_numpy(np.broadcast_to(want, (B, nA)).copy()))
    assert R.same_bits(det["values"], heads[:, nA:nA + vh].contiguous())


# --------------------------------------------------------------------------------------------- discrete PPO loss
def run_loss(lib, st, dev, inp, B, with_old, indexed, seed):
    """ppo_ppo_loss_f32 twice -> (dheads, stats) on the CPU.  indexed: the per-sample arrays sit in a larger batch, sample b
    in row index[b]."""
    nA, vh = inp["nA"], inp["vh"]
    heads = inp["heads"][:B].contiguous().to(dev)
    ldo = heads.shape[1]
    arrays = {k: inp[k][:B] for k in ("actions", "old_log_pac", "old_log_policy", "adv", "ret")}
    index = None
    if indexed:
        g = torch.Generator().manual_seed(seed)
        Btot = B + 7
        perm = torch.randperm(Btot, generator=g)[:B]
        big = {}
        for k, t in arrays.items():
            full = torch.full((Btot,) + tuple(t.shape[1:]), 5, dtype=t.dtype)  # rows no sample maps to: action 5 is out of
            full[perm] = t                                                  # range for small nA, never read
            big[k] = full
        arrays, index = big, perm.int().to(dev)
    a = {k: t.contiguous().to(dev) for k, t in arrays.items()}
    c = R.LOSS_COEF
    runs = []
    for _ in range(2):
        dbuf, dh = R.guarded((B, ldo), dev)
        sbuf, stats = R.guarded((B, 8), dev)
        _lib.check(lib.ppo_ppo_loss_f32(_p(heads), B, ldo, nA, vh, _p(a["actions"]), _p(a["old_log_pac"]),
                                        _p(a["old_log_policy"]) if with_old else None, _p(a["adv"]), _p(a["ret"]) if vh else None,
                                        c["eps_clip"], c["ent_coef"], c["vf_coef"], c["grad_scale"], _p(dh), _p(stats), _p(index),
                                        st), "ppo_loss")
        torch.cuda.synchronize()
        assert R.guards_intact(dbuf, dh) and R.guards_intact(sbuf, stats), "wrote outside its output"
        runs.append((dh.cpu(), stats.cpu()))
    assert R.same_bits(runs[0][0], runs[1][0]) and R.same_bits(runs[0][1], runs[1][1]), "two launches differ"
    return runs[0]


@pytest.mark.parametrize("vh", R.LOSS_VH)
@pytest.mark.parametrize("nA", R.LOSS_NA)
def test_ppo_loss_against_float64(nA, vh):
    lib, dev, st = _env()
    inp = R.loss_inputs(nA, vh)
    Bmax = max(R.LOSS_B)
    for with_old in (False, True):
        ref_all = R.ppo_loss_ref(inp, Bmax, with_old, **R.LOSS_COEF)
        f32 = R.ppo_loss_f32(inp, Bmax, with_old, **R.LOSS_COEF)
        d32, s32 = R.loss_errs(f32["dheads"], f32["stats"], ref_all)
        decided_all = R.clip_decided(ref_all, R.bar_from(s32["ratio"]))
        worst_d, worst_s = 0.0, {k: 0.0 for k in s32}
        for B in R.LOSS_B:
            ref = _rows(ref_all, B)
            for indexed in (False, True):
                what = f"nA={nA} vh={vh} old={int(with_old)} B={B} indexed={int(indexed)}"
                dh, stats = run_loss(lib, st, dev, inp, B, with_old, indexed, seed=B + nA)
                assert bool((dh[:, nA + vh:] == 0).all()), f"{what}: a spare column's gradient is not 0"
                d, s = R.loss_errs(dh, stats, ref)
                worst_d = max(worst_d, d)
                assert d <= R.bar_from(d32), f"{what}: dheads {d:.3e} over the bar {R.bar_from(d32):.3e}"
                for k, v in s.items():
                    worst_s[k] = max(worst_s[k], v)
                    assert v <= R.bar_from(s32[k]), f"{what}: {k} {v:.3e} over the bar {R.bar_from(s32[k]):.3e}"
                decided = decided_all[:B]
                assert bool(decided[:R.N_PLANTED].all())
                assert int((~decided).sum()) <= int(R.EXCLUDED_CAP * max(B - R.N_PLANTED, 0))
                assert torch.equal(stats[:, 3][decided].double(), ref["stats"][:, 3][decided]), f"{what}: clipped column"
                assert bool(((stats[:, 3] == 0) | (stats[:, 3] == 1)).all())
                if not with_old:
                    assert bool((stats[:, 5] == 0).all())
        R.report(f"ppo_loss nA={nA} vh={vh} old={int(with_old)} dheads", worst_d, d32)
        for k in s32:
            R.report(f"ppo_loss nA={nA} vh={vh} old={int(with_old)} {k}", worst_s[k], s32[k])
