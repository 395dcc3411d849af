"""GPU: the batch-norm kernels (csrc/batchnorm.hip) through the C ABI against float64 numpy on identical inputs.

Reference: nn.BatchNorm2d with torch's defaults as rl/impala.py:63-76 builds it - batch statistics and the running
update in train mode, the per-channel affine map of the running statistics in eval mode, and that map's gradients.

Bounds (u = 2^-24, the float32 unit roundoff; derived, not measured):
  z        s and t are float64 values rounded once (u each, relative) and z = fma(s, x, t) rounds once more, on a value of
           magnitude <= |s x| + |t|: |z - (s x + t)| <= u|s x| + u|t| + u(|s x| + |t|) = 2u(|s x| + |t|).  Bar: 4u(...).
  moments  sums run in float64 (2^-53 per addition, ~m * 2^-53 of the sum of magnitudes at worst): the batch mean, the
           variance (E[x^2] - mean^2 in float64; for 1000 + N(0, 1) the cancellation costs a factor 1e6 of 1e-16) and
           the running updates are float64 values rounded once to float32.  Bar: 2^-22 relative.
  dx       fma(s, dz, r): u|s dz| from s, u(|s dz| + |r|) from the one rounding.  Bar: 4u|s dz| + u|r|.
  dgamma,  float64 sums of exact float64 terms, rounded once: u * |sum| <= u * sum|term|.  Bar: 4u * sum|term|; with the
  dbeta    accumulate flag the stored value is (prior + sum) rounded once, so the prior joins the sum of magnitudes.
Every output sits between canary elements, and one case per operation runs on bases that are not 16-byte aligned."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import _lib  # noqa: E402

U = 2.0 ** -24
EPS, MOM = 1e-5, 0.1
E_INVALID, E_ALIGN = -1, -3
PAD = 64
SHAPES = [
    (1, 1, 1, 2),       # m = 2: the unbiased factor is 2
    (1, 3, 5, 7),       # odd planes, misaligned plane bases
    (3, 5, 21, 21),
    (7, 16, 11, 11),
    (2, 33, 1, 1),
    (32, 32, 21, 21),   # many slices per channel
]
KINDS = ["normal", "offset"]  # offset: 1000 + N(0, 1), which float32 sums do not survive
# (shape, kind, element offset of every map in its allocation): offset 1 takes the all-scalar path
CASES = [(s, k, 0) for s in SHAPES for k in KINDS] + [((1, 3, 5, 7), "normal", 1), ((3, 5, 21, 21), "offset", 1)]
IDS = [f"{'x'.join(map(str, s))}-{k}-{o}" for s, k, o in CASES]


def ptr(t):
    return None if t is None else t.data_ptr()


def launch(name, *a):
    return getattr(_lib.load(), name)(*a, _lib.current_stream())


def call(name, *a):
    rc = launch(name, *a)
    assert rc == 0, _lib.load().ppo_last_error()


class Framed:
    """A float32 device tensor between PAD canary elements, `offset` elements into a 16-byte aligned allocation."""

    def __init__(self, value=None, shape=None, offset=0):
        shape = tuple(value.shape) if value is not None else tuple(shape)
        n = int(np.prod(shape))
        self.flat = torch.full((offset + n + 2 * PAD,), -12345.0, dtype=torch.float32, device="cuda")
        self.lo, self.hi = offset + PAD, offset + PAD + n
        self.t = self.flat[self.lo:self.hi].view(shape)
        self.t.copy_(torch.from_numpy(value)) if value is not None else self.t.fill_(float("nan"))

    def get(self):
        assert bool((self.flat[:self.lo] == -12345.0).all()) and bool((self.flat[self.hi:] == -12345.0).all()), "canary"
        return self.t.cpu().numpy().astype(np.float64)


def draw(shape, kind, seed):
    """Inputs of one case (float32 numpy): maps, non-trivial gamma / beta / running statistics, a prior gradient."""
    n, c, h, w = shape
    r = np.random.default_rng(seed)
    x = r.standard_normal(shape) * 1.5 + 0.25
    if kind == "offset":
        x = 1000.0 + r.standard_normal(shape)
    d = dict(x=x, dz=r.standard_normal(shape), res=r.standard_normal(shape), gamma=r.uniform(0.5, 1.5, c) * r.choice([-1, 1], c),
             beta=r.normal(0, 0.3, c), rm=r.normal(0, 1, c) + (1000.0 if kind == "offset" else 0.0), rv=r.uniform(0.3, 3.0, c),
             prior_g=r.standard_normal(c) * 10, prior_b=r.standard_normal(c) * 10)
    return {k: v.astype(np.float32) for k, v in d.items()}


def workspace(c, extra=0):
    nbytes = int(_lib.load().ppo_batchnorm_workspace_bytes(c))
    assert nbytes == c * 64 * 2 * 8
    return torch.empty(nbytes // 8 + extra, dtype=torch.float64, device="cuda"), nbytes


def dev(a):
    """A device copy; the caller keeps it in a name for as long as a launch reads it."""
    return torch.from_numpy(a).cuda()


def rel(got, ref):
    return np.max(np.abs(got - ref) / np.abs(ref))


def run_batch(d, shape, offset=0):
    n, c, h, w = shape
    x, z = Framed(d["x"], offset=offset), Framed(shape=shape, offset=offset)
    rm, rv, bm, bv = Framed(d["rm"]), Framed(d["rv"]), Framed(shape=(c,)), Framed(shape=(c,))
    nbt = torch.full((1,), 41, dtype=torch.int64, device="cuda")
    ws, nbytes = workspace(c)
    gamma, beta = dev(d["gamma"]), dev(d["beta"])
    call("ppo_batchnorm_batch_forward_f32", ptr(x.t), ptr(gamma), ptr(beta), ptr(rm.t), ptr(rv.t), ptr(nbt),
         ptr(z.t), ptr(bm.t), ptr(bv.t), ptr(ws), nbytes, n, c, h, w, EPS, MOM)
    torch.cuda.synchronize()
    return z, rm, rv, bm, bv, nbt


@pytest.mark.parametrize("shape,kind,offset", CASES, ids=IDS)
def test_batch_forward(shape, kind, offset):
    n, c, h, w = shape
    d = draw(shape, kind, 1)
    z, rm, rv, bm, bv, nbt = run_batch(d, shape, offset)
    x = d["x"].astype(np.float64)
    m = n * h * w
    mean, var = x.mean(axis=(0, 2, 3)), x.var(axis=(0, 2, 3))
    s = d["gamma"].astype(np.float64) / np.sqrt(var + EPS)
    t = d["beta"].astype(np.float64) - mean * s
    bc = (None, slice(None), None, None)
    err = np.abs(z.get() - (s[bc] * x + t[bc]))
    bar = 4 * U * (np.abs(s[bc] * x) + np.abs(t[bc]))
    print(f"z: worst error / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all()
    new_rm = (1 - MOM) * d["rm"].astype(np.float64) + MOM * mean
    new_rv = (1 - MOM) * d["rv"].astype(np.float64) + MOM * var * (m / (m - 1))
    for name, got, ref in (("mean", bm, mean), ("var", bv, var), ("running_mean", rm, new_rm), ("running_var", rv, new_rv)):
        e = rel(got.get(), ref)
        print(f"{name}: relative error {e:.3e}")
        assert e <= 2.0 ** -22, name
    assert int(nbt.item()) == 42


@pytest.mark.parametrize("shape,kind,offset", CASES, ids=IDS)
def test_running_forward(shape, kind, offset):
    n, c, h, w = shape
    d = draw(shape, kind, 2)
    x, z = Framed(d["x"], offset=offset), Framed(shape=shape, offset=offset)
    gamma, beta, rm, rv = (dev(d[k]) for k in ("gamma", "beta", "rm", "rv"))
    call("ppo_batchnorm_running_forward_f32", ptr(x.t), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(z.t), n, c, h, w, EPS)
    torch.cuda.synchronize()
    x64 = d["x"].astype(np.float64)
    s = d["gamma"].astype(np.float64) / np.sqrt(d["rv"].astype(np.float64) + EPS)
    t = d["beta"].astype(np.float64) - d["rm"].astype(np.float64) * s
    bc = (None, slice(None), None, None)
    err = np.abs(z.get() - (s[bc] * x64 + t[bc]))
    bar = 4 * U * (np.abs(s[bc] * x64) + np.abs(t[bc]))
    print(f"z: worst error / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all()


def run_backward(d, shape, offset=0, residual=True, accumulate=0):
    n, c, h, w = shape
    dz, x = Framed(d["dz"], offset=offset), Framed(d["x"], offset=offset)
    res = Framed(d["res"], offset=offset) if residual else None
    dx = Framed(shape=shape, offset=offset)
    dg, db = Framed(d["prior_g"]), Framed(d["prior_b"])
    ws, nbytes = workspace(c)
    gamma, rm, rv = (dev(d[k]) for k in ("gamma", "rm", "rv"))
    call("ppo_batchnorm_running_backward_f32", ptr(dz.t), ptr(x.t), ptr(res.t) if residual else None, ptr(gamma), ptr(rm),
         ptr(rv), ptr(dx.t), ptr(dg.t), ptr(db.t), ptr(ws), nbytes, n, c, h, w, EPS, accumulate)
    torch.cuda.synchronize()
    return dx, dg, db


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("shape,kind,offset", CASES, ids=IDS)
def test_running_backward(shape, kind, offset, residual):
    d = draw(shape, kind, 3)
    dx, dg, db = run_backward(d, shape, offset, residual)
    dz, x = d["dz"].astype(np.float64), d["x"].astype(np.float64)
    r = d["res"].astype(np.float64) if residual else np.zeros(shape)
    inv = 1.0 / np.sqrt(d["rv"].astype(np.float64) + EPS)
    bc = (None, slice(None), None, None)
    sdz = (d["gamma"].astype(np.float64) * inv)[bc] * dz
    err = np.abs(dx.get() - (sdz + r))
    bar = 4 * U * np.abs(sdz) + U * np.abs(r)
    print(f"dx: worst error / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}")
    assert (err <= bar).all()
    terms = dz * (x - d["rm"].astype(np.float64)[bc]) * inv[bc]
    for name, got, tm in (("dgamma", dg, terms), ("dbeta", db, dz)):
        e = np.abs(got.get() - tm.sum(axis=(0, 2, 3)))
        b = 4 * U * np.abs(tm).sum(axis=(0, 2, 3))
        print(f"{name}: worst error / bar {np.max(e / b):.3f}")
        assert (e <= b).all(), name


def test_accumulate_flag_adds():
    shape = (7, 16, 11, 11)
    d = draw(shape, "normal", 4)
    _dx, dg, db = run_backward(d, shape, accumulate=1)
    dz, x = d["dz"].astype(np.float64), d["x"].astype(np.float64)
    bc = (None, slice(None), None, None)
    terms = dz * (x - d["rm"].astype(np.float64)[bc]) / np.sqrt(d["rv"].astype(np.float64) + EPS)[bc]
    for got, tm, prior in ((dg, terms, d["prior_g"]), (db, dz, d["prior_b"])):
        ref = prior.astype(np.float64) + tm.sum(axis=(0, 2, 3))
        bar = 4 * U * (np.abs(tm).sum(axis=(0, 2, 3)) + np.abs(prior))
        assert (np.abs(got.get() - ref) <= bar).all()
        assert (np.abs(got.get() - tm.sum(axis=(0, 2, 3))) > bar).any()  # (the priors are ~10: overwriting would show)


def test_two_runs_are_bit_identical():
    shape = (32, 32, 21, 21)
    d = draw(shape, "offset", 5)
    a, b = run_batch(d, shape), run_batch(d, shape)
    for p, q in zip(a[:5], b[:5]):
        assert torch.equal(p.t, q.t)
    a, b = run_backward(d, shape), run_backward(d, shape)
    for p, q in zip(a, b):
        assert torch.equal(p.t, q.t)


def test_bad_arguments():
    lib = _lib.load()
    shape = (2, 3, 4, 4)
    n, c, h, w = shape
    x = torch.zeros(shape, device="cuda")
    z = torch.full(shape, 7.0, device="cuda")
    v = torch.ones(c, device="cuda")
    ws, nbytes = workspace(c, extra=1)
    fwd = ("ppo_batchnorm_batch_forward_f32", ptr(x), ptr(v), ptr(v), None, None, None, ptr(z), None, None)
    assert launch(*fwd, ptr(ws), nbytes, n, 0, h, w, EPS, MOM) == E_INVALID and b"bad shape" in lib.ppo_last_error()
    assert launch(*fwd, ptr(ws), nbytes, 1, c, 1, 1, EPS, MOM) == E_INVALID and b"n*h*w >= 2" in lib.ppo_last_error()
    assert launch(*fwd, ptr(ws), nbytes - 1, n, c, h, w, EPS, MOM) == E_INVALID and b"workspace" in lib.ppo_last_error()
    assert launch(*fwd, ptr(ws) + 4, nbytes, n, c, h, w, EPS, MOM) == E_ALIGN
    assert launch(*fwd, None, nbytes, n, c, h, w, EPS, MOM) == E_INVALID and b"null" in lib.ppo_last_error()
    assert launch(*fwd, ptr(ws), nbytes, n, c, h, w, -1.0, MOM) == E_INVALID
    assert launch(*fwd, ptr(ws), nbytes, n, c, h, w, EPS, 1.5) == E_INVALID
    assert launch("ppo_batchnorm_running_forward_f32", ptr(x), ptr(v), ptr(v), ptr(v), None, ptr(z), n, c, h, w, EPS) == E_INVALID
    assert launch("ppo_batchnorm_running_forward_f32", ptr(x), ptr(v), ptr(v), ptr(v), ptr(v), ptr(z), n, c, h, 0, EPS) == E_INVALID
    bwd = ("ppo_batchnorm_running_backward_f32", ptr(x), ptr(x), None, ptr(v), ptr(v), ptr(v), ptr(z))
    assert launch(*bwd, None, ptr(v), ptr(ws), nbytes, n, c, h, w, EPS, 0) == E_INVALID
    assert launch(*bwd, ptr(v), ptr(v), ptr(ws), 8, n, c, h, w, EPS, 0) == E_INVALID
    assert launch(*bwd, ptr(v), ptr(v), ptr(ws) + 4, nbytes, n, c, h, w, EPS, 0) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((z == 7.0).all())  # nothing is written on error
    # an empty batch is no error for the forms that need no statistics
    assert launch("ppo_batchnorm_running_forward_f32", ptr(x), ptr(v), ptr(v), ptr(v), ptr(v), ptr(z), 0, c, h, w, EPS) == 0
    assert lib.ppo_batchnorm_workspace_bytes(0) == 0
