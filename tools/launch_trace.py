#!/usr/bin/env python
"""Normalised launch traces of the networks' host code: what a refactor of ppo_amd/models.py has to leave unchanged.

    python tools/launch_trace.py record --root DIR --out FILE.json   (GPU)
    python tools/launch_trace.py compare A.json B.json               (CPU)

`record` puts DIR first on sys.path, so one copy of this tool traces a checkout of another commit and this tree with the
same built library (PPO_AMD_LIB).  It replaces `_call` on the net instances and on the Runner, turns the recorded
inference launch lists off (`use_plans = False`: every launch goes through `_call`) and stores every call as
[entry point, arguments]: an argument typed c_void_p in _lib.SIGNATURES as the ordinal of its address's first appearance
within the case (None stays None), ctypes arrays as their contents, the job tables and structs of TABLES field by field
(their own host addresses, and that of the slab-count word, are temporaries and not recorded), everything else as its value.  `compare` prints the first differing call per case, or `equal: N cases`, and exits non-zero
on any difference.  Batch 8 (the Runner cases: two groups of 16 envs, or what the env stack offers), seeded inputs, a
fresh net per case.
"""
import argparse
import contextlib
import ctypes
import inspect
import json
import os
import sys

# entry point -> {argument index: (struct in _lib, index of the argument that holds the element count or None for one)}
TABLES = {
    "ppo_conv3x3_wgrad_reduce_f32": {0: ("WgradJob", 1)},
    "ppo_conv3x3_pack_weights_f32": {0: ("PackJob", 1)},
    "ppo_impala_stack_tail_pack_bf16x3_jobs": {0: ("SplitPackJob", 1)},
    "ppo_conv3x3_pack_bf16x3_jobs": {0: ("ConvPackJob", 1)},
    "ppo_mlp_forward_f32": {1: ("MlpNet", None)},
    "ppo_mlp_train_f32": {1: ("MlpNet", None), 2: ("MlpGrads", None), 6: ("MlpLoss", None)},
}
# These entry points end with the address of a host int that receives the slab count.  It is a temporary of the caller, whose
# address the host heap hands out again as it pleases: recorded as such, as are the tables above, not as an ordinal.
HOST_COUNT_PREFIX = "ppo_conv3x3_backward_weight_slabs"
B, ROWS = 8, 12  # minibatch rows; rows of the array an obs_indexed minibatch is read out of


class Trace:
    """The calls of one case."""

    def __init__(self, _lib):
        self._lib, self.calls, self.ordinals = _lib, [], {}

    def pointer(self, addr):
        return None if addr is None else self.ordinals.setdefault(int(addr), len(self.ordinals))

    def array(self, arr):
        return [self.pointer(v) for v in arr] if arr._type_ is ctypes.c_void_p else list(arr)

    def struct(self, s):
        out = {}
        for name, ftype in s._fields_:
            v = getattr(s, name)
            out[name] = self.pointer(v) if ftype is ctypes.c_void_p else self.array(v) if isinstance(v, ctypes.Array) else v
        return out

    def record(self, fn_name, args):
        argtypes = self._lib.SIGNATURES[fn_name][1]
        assert len(args) == len(argtypes) - 1, (fn_name, len(args), len(argtypes))  # the stream follows
        tables, out = TABLES.get(fn_name, {}), []
        for k, (a, t) in enumerate(zip(args, argtypes)):
            if k in tables and a is not None:
                struct, count = tables[k]
                T = getattr(self._lib, struct)
                n = 1 if count is None else int(args[count])
                out.append({struct: [self.struct(s) for s in (T * n).from_address(a)]})
            elif k == len(args) - 1 and fn_name.startswith(HOST_COUNT_PREFIX):
                out.append("host int")
            elif isinstance(a, ctypes.Array):
                out.append(self.array(a))
            elif t is ctypes.c_void_p:
                out.append(self.pointer(a))
            else:
                out.append(a)
        self.calls.append([fn_name, out])

    def hook(self, *objs):
        for obj in objs:
            def traced(fn_name, *a, _orig=obj._call):
                self.record(fn_name, a)
                return _orig(fn_name, *a)
            obj._call = traced
            if hasattr(obj, "use_plans"):
                obj.use_plans = False

    def note(self, text):
        self.calls.append(["note", [text]])


def record(root, out_path):
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch
    from ppo_amd import _lib, envs, logger, models, rollout
    from ppo_amd.config import args

    @contextlib.contextmanager
    def switches(**values):
        """Module-level launch switches of ppo_amd.models, for the life of one case (the net is built inside it)."""
        old = {k: getattr(models, k) for k in values}
        for k, v in values.items():
            setattr(models, k, v)
        try:
            yield
        finally:
            for k, v in old.items():
                setattr(models, k, v)

    def seeded(seed=0):
        torch.manual_seed(seed)
        np.random.seed(seed)
        return torch.Generator(device="cpu").manual_seed(seed)

    def observations(g, rows, dims, uint8=True):
        if uint8:
            return torch.randint(0, 256, (rows, *dims), generator=g, dtype=torch.uint8).cuda()
        return torch.randn((rows, *dims), generator=g).cuda()

    def infer(t, net, dims, allow_chain_split=False, uint8=True):
        x = observations(seeded(1), B, dims, uint8)
        t.hook(net)
        if "chain_split" in inspect.signature(net.encode).parameters:
            net.heads(net.encode(x, train=False, chain_split=allow_chain_split), "i")
            return
        net.allow_chain_split = allow_chain_split  # a checkout from before encode() took it as an argument
        try:
            net.heads(net.encode(x, train=False), "i")
        finally:
            net.allow_chain_split = False

    def train(t, net, dims, phases):
        """The minibatch calls `phases` on net, each followed by adam_step."""
        g = seeded(2)
        nA, vh = net.n_actions, net.vh
        obs_all = observations(g, ROWS, dims)
        index = torch.randperm(ROWS, generator=g)[:B].to(torch.int32).cuda()
        rows = index.long()
        log_policy = torch.log_softmax(torch.randn(ROWS, nA, generator=g), dim=1).cuda()
        actions = torch.randint(0, nA, (ROWS,), generator=g, dtype=torch.int32).cuda()
        log_pac = log_policy.gather(1, actions.long()[:, None])[:, 0].contiguous()
        adv, returns = torch.randn(ROWS, generator=g).cuda(), torch.randn(ROWS, vh, generator=g).cuda()
        targets = torch.randn(ROWS, generator=g).cuda()
        obs = obs_all[rows].contiguous()
        mb = [a[rows].contiguous() for a in (actions, log_pac, log_policy, adv, returns)]
        t.hook(net)
        for phase in phases:
            if phase == "ppo":
                net.ppo_minibatch(obs, *mb)
            elif phase == "ppo_indexed":
                if not net.takes_obs_index(obs_all):
                    t.note("takes_obs_index is False: no obs_indexed minibatch")
                    continue
                net.ppo_minibatch(obs_all, actions, log_pac, log_policy, adv, returns, index=index, obs_indexed=True)
            elif phase == "value":
                net.value_minibatch(obs, returns=mb[4])
            elif phase == "value_tvf":
                net.value_minibatch(obs, returns=mb[4], tvf_returns=torch.randn(B, net.K, generator=g).cuda(),
                                    tvf_weights=torch.ones(net.K).cuda())
            elif phase == "distil":
                net.distil_minibatch(obs, targets[rows].contiguous(), mb[2])
            net.adam_step()

    def impala(dims, n_actions, **kw):
        return models.DualHeadNet("impala", dims, n_actions, hidden_units=256, head_scale=0.1, head_bias=True, **kw)

    def runner_case(t, flags, encoder, seed, **model_kw):
        """Two env steps of Runner.generate_rollout, the Runner's own calls included."""
        args.setup([*flags, "--n_steps=2", "--device=cuda", "--disable_logging=True", "--model_architecture=single",
                    f"--model_encoder={encoder}", f"--seed={seed}", "--policy_opt_mini_batch_size=32"])
        seeded(seed)
        shape, n_actions = envs.get_env_spec()
        model = models.TVFModel(encoder, input_dims=shape, actions=n_actions, device="cuda", architecture="single",
                                head_scale=0.1, head_bias=True, **model_kw)
        r = rollout.Runner(model, logger.Logger(quiet=True))
        r.vec_env = envs.create_envs_classic()
        try:
            t.hook(model.policy_net, r)
            r.reset()
            r.generate_rollout()
            torch.cuda.synchronize()
        finally:
            if hasattr(r.vec_env, "close"):
                r.vec_env.close()

    cases = {}

    def case(name, fn, **sw):
        t = Trace(_lib)
        with switches(**sw):
            fn(t)
        torch.cuda.synchronize()
        cases[name] = t.calls
        print(f"{name}: {len(t.calls)} calls", flush=True)

    d84, d64 = (4, 84, 84), (3, 64, 64)
    all_phases = ("ppo", "ppo_indexed", "value", "distil")
    case("impala84/infer", lambda t: infer(t, impala(d84, 6), d84))
    case("impala84/infer_chain_split", lambda t: infer(t, impala(d84, 6), d84, allow_chain_split=True))
    case("impala84/train", lambda t: train(t, impala(d84, 6), d84, all_phases))
    for sw in ({"WGRAD_BATCH_LAUNCH": 0}, {"WGRAD_POOLED_DY": 0}, {"WGRAD_RIDE": 0}, {"FUSE_STACK16_MIN_BATCH": 1},
               {"FUSE_CHAIN_BWD_MIN_BATCH": 1}, {"FUSE_STACK_FULL_BWD": 1}, {"FUSE_STACK_TAIL": 0},
               {"FUSE_STACK_TAIL": 0, "WGRAD_BATCH_LAUNCH": 0}, {"FUSE_STACK_CHAIN": 0}, {"PACKED_WEIGHTS": 0},
               {"ADAM_SCATTER": 1}):
        case("impala84/train/" + ",".join(f"{k}={v}" for k, v in sw.items()),
             lambda t: train(t, impala(d84, 6), d84, all_phases), **sw)
    case("impala84/train/medium", lambda t: train(t, impala(d84, 6, precision="medium"), d84, all_phases))
    for precision in ("high", "medium"):
        case(f"impala64/{precision}/infer", lambda t: infer(t, impala(d64, 15, precision=precision), d64))
        case(f"impala64/{precision}/ppo", lambda t: train(t, impala(d64, 15, precision=precision), d64, ("ppo",)))
    for dims, kw in (((4, 96, 96), {}), ((12, 84, 84), {}), ((3, 20, 28), {"channels": (8, 24), "n_block": 1})):
        name = "impala_any/" + "x".join(map(str, dims))
        case(name + "/infer", lambda t: infer(t, impala(dims, 6, **kw), dims))
        case(name + "/ppo", lambda t: train(t, impala(dims, 6, **kw), dims, ("ppo",)))
    tvf = dict(tvf_fixed_head_horizons=[1, 10, 100, 1000], activation_fn="tanh")
    case("impala84/tvf_tanh/infer", lambda t: infer(t, impala(d84, 6, **tvf), d84))
    case("impala84/tvf_tanh/value", lambda t: train(t, impala(d84, 6, **tvf), d84, ("value_tvf",)))

    def nature(activation_fn):
        return models.DualHeadNet("nature", d84, 6, hidden_units=512, head_scale=0.1, head_bias=True,
                                  activation_fn=activation_fn)
    case("nature84/relu/infer", lambda t: infer(t, nature("relu"), d84))
    case("nature84/relu/ppo", lambda t: train(t, nature("relu"), d84, ("ppo",)))
    case("nature84/tanh/infer", lambda t: infer(t, nature("tanh"), d84))

    def mlp_gaussian(t):
        g = seeded(3)
        net = models.DualHeadNet("mlp", (11,), 3, hidden_units=64, activation_fn="tanh", head_scale=0.1, head_bias=True)
        x, actions, log_pac = (torch.randn(B, n, generator=g).cuda() for n in (11, 3, 3))
        adv, returns = torch.randn(B, generator=g).cuda(), torch.randn(B, 1, generator=g).cuda()
        t.hook(net)
        net.gaussian_minibatch(x, actions, log_pac, adv, returns)
        net.adam_step()
    for fuse in (1, 0):
        case(f"mlp11/FUSE_MLP={fuse}/gaussian", mlp_gaussian, FUSE_MLP=fuse)

    synthetic = ["--agents=32", "--env_type=synthetic", "--env_embed_time=False"]
    case("runner/impala_synthetic", lambda t: runner_case(t, synthetic, "impala", 3, hidden_units=256))
    case("runner/nature_synthetic", lambda t: runner_case(t, synthetic, "nature", 4, hidden_units=512,
                                                          encoder_args={"base_channels": 32}))
    case("runner/mlp_cartpole", lambda t: runner_case(
        t, ["--agents=16", "--env_type=classic", "--env_name=CartPole", "--workers=4", "--model_hidden_units=64", "--gamma=0.99"],
        "mlp", 2, hidden_units=64))

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"root": os.path.abspath(root), "library": _lib.LIB_PATH, "cases": cases}, f,
                  default=lambda scalar: scalar.item())  # numpy / torch scalars among the arguments
    print(f"recorded {len(cases)} cases, {sum(len(c) for c in cases.values())} calls -> {out_path}")


def compare(path_a, path_b) -> int:
    with open(path_a) as f:
        a = json.load(f)["cases"]
    with open(path_b) as f:
        b = json.load(f)["cases"]
    different = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in {path_a if name in a else path_b}")
            different += 1
            continue
        ca, cb = a[name], b[name]
        k = next((k for k, (x, y) in enumerate(zip(ca, cb)) if x != y), None)
        if k is None and len(ca) == len(cb):
            continue
        different += 1
        k = min(len(ca), len(cb)) if k is None else k
        print(f"{name}: call {k} differs ({len(ca)} / {len(cb)} calls)")
        for path, calls in ((path_a, ca), (path_b, cb)):
            print(f"  {path}: {json.dumps(calls[k]) if k < len(calls) else 'no such call'}")
    if different:
        print(f"different: {different} of {len(set(a) | set(b))} cases")
        return 1
    print(f"equal: {len(a)} cases")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    rec = sub.add_parser("record", help="trace every case on the GPU")
    rec.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                     help="the tree whose ppo_amd package is traced")
    rec.add_argument("--out", required=True)
    cmp_ = sub.add_parser("compare", help="compare two recordings (no GPU)")
    cmp_.add_argument("a")
    cmp_.add_argument("b")
    a = ap.parse_args()
    if a.command == "record":
        record(a.root, a.out)
        return 0
    return compare(a.a, a.b)


if __name__ == "__main__":
    sys.exit(main())
