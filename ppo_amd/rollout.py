"""Rollout runner — host mirror of the reference's rl/rollout.py `Runner`: `generate_rollout` (:702-969),
`calculate_returns` (:1182-1285), `train` (:2220-2255) with its policy / value / distil phases
(`train_policy` :1853-1953, `train_value` :1956-2004, `train_distil` :2140-2164), the minibatch functions
(:1331-1449, :1513-1567, :1610-1771), `train_batch` (:2257-2407) and `optimizer_step` (:1287-1321), for
`--model_architecture=single` (PPO) and `dual` (DNA / TVF), discrete and gaussian action distributions.

What changed relative to the reference, and why (MI355X-first):
  * every rollout buffer lives in HBM (`all_obs` [N+1, A, ...], `value`, `log_policy`, `actions`, rewards,
    terminals, TVF values ...); the reference keeps them in host NumPy arrays and re-uploads minibatches
    (rl/rollout.py:189-250, 2349-2372);
  * one device->host copy per env step (the sampled actions) instead of five (:641, 809-813); action
    sampling (Gumbel-max / gaussian) runs on the GPU next to the policy head; with array-stepping envs the
    step is software-pipelined over two env groups;
  * GAE + lambda-returns are one fused HIP scan, TVF returns one HIP kernel; advantage normalisation, the
    minibatch gather, every loss, backward and Adam are HIP kernels (ppo_amd/csrc); minibatches are read
    through an index vector instead of being gathered (only the observations are gathered);
  * statistics are reduced on the device and fetched once per iteration;
  * Random Network Distillation (`--rnd_enabled`, rl/rollout.py:764-766, 1140-1180, 1804-1841): the prediction error
    of a group's observations is written into `int_rewards` right behind that group's policy step, with no host read
    (the reference reads it back every env step); the forward EMS filter and its running variance stay on the host
    in float64 (N tiny updates, bit-exact with the reference); clipping, scaling, GAE and the advantage sum are
    device launches; the predictor trains through the same minibatch loop as the other phases;
  * state hashing (`--hash_enabled`, rl/rollout.py:652-699, 755-762, 895-924): a group's observations are hashed where
    they lie, one launch behind its policy step that writes int32 hashes and nothing else (the reference hashes on the
    host with a Python loop over envs every step); the two float64 count tables are brought up to date once per rollout,
    step by step in the reference's order and bit-identical to its loop - the env groups run a step apart, so they
    cannot be updated during the rollout - and the count-based bonus is added to `int_rewards` before its clip;
  * experience replay (`--replay_mode`, `--replay_size`, rl/replay.py, rl/rollout.py:956-969, 2016-2138): the buffer lies
    in HBM next to the rollout; an add is one scatter launch from `all_obs`, the distil batch one gather launch (buffer,
    or buffer + rollout with `--replay_mixing`) whose targets and old policy are regenerated on the device; which rows
    go where is the reference's index arithmetic on its np.random draws (ppo_amd/replay.py `plan_add`);
  * data parallelism: env columns are sharded over ranks (one process per GPU); the only exchanges are one
    RCCL all-reduce of the flat gradient per optimiser step and one of the three advantage moments per
    batch, so an N-GPU run equals a 1-GPU run with N*A envs up to minibatch composition.  With intrinsic rewards on,
    the three places that need the whole batch join them: the hash tables count every rank's hashes (one column gather
    per rollout), the intrinsic-return filter runs on every rank over every rank's rewards (one or two gathers), and
    `--ir_center` all-reduces its three moments; the RND predictor's gradient is reduced like the other nets'.
"""
import copy
import math
import time

import numpy as np
import torch

from . import _lib, parallel, sns, value_quality
from .config import args
from .models import AdamState, check_optimizer_layout, sgd_state_dict
from .returns import calculate_bootstrapped_returns
from .running_stats import RunningMeanStd


# the synthetic env uploads a group's observations in this many pieces, each as soon as it has been generated (1: one
# copy after the whole group has been stepped).  Measured: 0.491 / 0.474 / 0.487 / 0.524 ms per env step for 1 / 2 / 4 / 8
UPLOAD_CHUNKS = 2


def _p(t):
    return None if t is None else t.data_ptr()


def intrinsic_return_scale(ems_norm, rms, int_rewards, terminals, gamma_int, propagation):
    """The host half of calculate_intrinsic_returns (rl/rollout.py:1148-1164), expression for expression so that the
    float64 results carry the reference's bits: the forward exponential-moving-sum filter over the rollout's (clipped)
    intrinsic rewards [N, A], `rms` (a RunningMeanStd, updated in place) taking in the filter's output after every step.
    Returns (ems_norm [A] float64, intrinsic_reward_norm_scale)."""
    for t in range(int_rewards.shape[0]):
        step_terminals = (not propagation) * terminals[t, :]
        ems_norm = (1 - step_terminals) * gamma_int * ems_norm + int_rewards[t, :]
        rms.update(ems_norm.reshape(-1))
    return ems_norm, (1e-5 + rms.var ** 0.5)


class Optimizer:
    """What the reference's `self.policy_optimizer` etc. stand for here: a net's flat parameter buffer, one
    set of Adam moments over it and the flag group with its hyper-parameters (rl/rollout.py:126-141).  `kind`: 'adam' or
    'sgd', the flag group's --*_opt_optimizer unless given (the distil phase on the policy optimiser takes that
    optimiser's kind along with its state).  An SGD optimiser has no state: `state` stays None and the net's own moments
    are never allocated by it."""

    def __init__(self, net, cfg, state=None, kind=None):
        self.net, self.cfg, self.state = net, cfg, state
        self.kind = kind if kind is not None else cfg.optimizer
        if self.kind not in ("adam", "sgd"):
            raise ValueError(f"Invalid Optimizer {self.kind}")  # make_optimizer's message (rl/rollout.py:139-141)

    def zero_grad(self, set_to_none=True):
        self.net.grad.zero_()

    def state_dict(self):
        """`torch.optim.Adam.state_dict()` (or `torch.optim.SGD.state_dict()`) layout, as the reference checkpoints it
        (rl/rollout.py:412-421)."""
        if self.kind == "sgd":
            return sgd_state_dict(self.net.parameter_count(), self.cfg.lr)
        if self.state is None:
            return self.net.optimizer_state_dict(self.cfg)
        return self.net.adam_state_dict(self.state.exp_avg, self.state.exp_avg_sq, self.state.step, self.cfg)

    def load_state_dict(self, sd):
        """A dict of the other kind is refused (torch would load it and carry on with the wrong hyper-parameters)."""
        check_optimizer_layout(sd, self.kind)
        if self.kind == "sgd":
            return  # no state; lr comes from the flags, as for Adam
        if self.state is None:
            self.net.load_optimizer_state_dict(sd)
        else:
            self.state.exp_avg, self.state.exp_avg_sq, self.state.step = self.net.read_adam_state_dict(sd)


class Runner:
    def __init__(self, model, log, name="agent", action_dist="discrete"):
        if action_dist not in ("discrete", "gaussian"):
            raise ValueError(f"Invalid distribution {action_dist}")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.name = name
        self.model = model
        self.policy_net, self.value_net = model.policy_net, model.value_net
        self.net = self.policy_net
        self.dual = model.architecture == "dual"
        self.log = log
        self.action_dist = action_dist
        self.device = self.net.device
        self.step = 0
        self.batch_counter = 0
        self.vec_env = None
        self.force_generic_rollout = False  # tests: the one-group gym-API loop, to compare the pipelined rollout against
        self.N, self.A = args.n_steps, args.agents
        self.state_shape = tuple(model.input_dims)
        self.n_actions = model.actions
        self.VH = self.net.vh
        self.rnd = model.rnd if getattr(model, "use_rnd", False) else None
        if bool(args.rnd.enabled) != (self.rnd is not None):
            raise ValueError("--rnd_enabled and TVFModel(use_rnd=...) must agree")
        # intrinsic rewards in use (rl/config.py:881-883): RND's prediction error, the hash bonus, or their sum
        self.intrinsic = bool(args.use_intrinsic_rewards)
        if self.VH != (2 if self.intrinsic else 1):
            raise NotImplementedError("value heads: ('ext',), or ('ext', 'int') with intrinsic rewards (RND, the hash bonus)")
        self.world, self.rank = parallel.world_size(), parallel.rank()
        if args.replay.enabled and self.world > 1:
            raise NotImplementedError("experience replay under data parallelism is not built (every rank would keep a buffer "
                                      "of its own env columns and draw its own distil batch)")
        if args.sns.enabled and self.world > 1:
            raise NotImplementedError("noise-scale estimation under data parallelism is not built (a rank's gradients are not the batch's)")
        # batch_norm=True in --model_encoder_args: the rollout's forwards normalise with their own batch's statistics
        # (rl/rollout.py:712), so the env groups cannot run a step apart - see _rollout_pipelined
        self.batch_norm = bool(getattr(model, "batch_norm", False))
        if self.batch_norm and self.world > 1:
            raise NotImplementedError("batch norm under data parallelism is not built (every rank would keep running "
                                      "statistics of its own env columns)")
        # ---- the policy phase's regularisers: global KL (rl/rollout.py:1723-1738) and SIDE (:1662-1679)
        if args.gkl.enabled or args.side.enabled:
            if action_dist != "discrete":
                raise ValueError("--gkl_enabled / --side_enabled: discrete policies only (the reference's global KL reads "
                                 "log_policy, which a gaussian policy lacks; its SIDE refuses mujoco)")
            if args.side.enabled and args.env.type == "mujoco":
                raise ValueError("--side_enabled: not supported for mujoco (rl/rollout.py:1907)")
        if args.gkl.enabled:
            if self.world > 1:
                raise NotImplementedError("the global KL penalty under data parallelism is not built (every rank would draw "
                                          "its global states from its own env columns: the estimate, and the gradient of "
                                          "its penalty, need one sample and one sum across the ranks)")
            if args.gkl.samples > args.n_steps * args.agents:
                raise ValueError(f"--gkl_samples={args.gkl.samples} exceeds the rollout, n_steps x agents = "
                                 f"{args.n_steps * args.agents} (the states are drawn without replacement)")
            if args.gkl.samples % min(args.max_micro_batch_size, args.gkl.samples):
                raise ValueError(f"--gkl_samples={args.gkl.samples} is not a multiple of --max_micro_batch_size="
                                 f"{args.max_micro_batch_size}, the chunk of the global pass")
        self.side_target_policy_logp = None  # [n_actions] device; not saved in checkpoints, as in the reference
        self._mb_pos = None  # (minibatch, micro-batch) of the step function _run_epochs is calling
        self._policy_extra = None  # the policy phase's global-KL / SIDE statistics rows (train_policy, fetch_stats)
        self._gkl_rows = None  # the rollout rows of the global states of the last policy phase ([S] int32, device)
        # simple noise scale (rl/rollout.py:177): smoothed estimates per label, filled by ppo_amd/sns.py when --sns_enabled
        self.noise_stats = {}
        self._tvf_subset_weight_cache = {}
        N, A, nA, VH, dev = self.N, self.A, self.n_actions, self.VH, self.device
        gaussian = action_dist == "gaussian"
        obs_dtype = torch.uint8 if model.policy_net.encoder_kind in ("impala", "nature", "rtg") and args.env.type != "mujoco" else torch.float32
        # ---- rollout buffers, all resident in HBM (time-major, env index contiguous)
        self.all_obs = torch.zeros((N + 1, A, *self.state_shape), dtype=obs_dtype, device=dev)
        self.value = torch.zeros((N + 1, A, VH), dtype=torch.float32, device=dev)
        self.returns = torch.zeros((N, A, VH), dtype=torch.float32, device=dev)
        if gaussian:
            self.actions = torch.zeros((N, A, nA), dtype=torch.float32, device=dev)
            self.log_pac = torch.zeros((N, A, nA), dtype=torch.float32, device=dev)
        else:
            self.actions = torch.zeros((N, A), dtype=torch.int32, device=dev)
            self.log_pac = torch.zeros((N, A), dtype=torch.float32, device=dev)
        self.ext_rewards = torch.zeros((N, A), dtype=torch.float32, device=dev)
        self.log_policy = torch.zeros((N, A, nA), dtype=torch.float32, device=dev)
        self.raw_policy = torch.zeros((N, A, nA), dtype=torch.float32, device=dev)
        self.terminals = torch.zeros((N, A), dtype=torch.bool, device=dev)
        self.advantage = torch.zeros((N, A), dtype=torch.float32, device=dev)
        self.raw_advantage = self.advantage
        self.norm_advantage = torch.zeros((N, A), dtype=torch.float32, device=dev)
        # ---- host staging (pinned): one step of actions down, a whole rollout of rewards/dones up
        self._actions_host = torch.zeros((A, nA) if gaussian else (A,),
                                         dtype=torch.float32 if gaussian else torch.int32).pin_memory()
        self._rewards_host = torch.zeros((N, A), dtype=torch.float32).pin_memory()
        self._dones_host = torch.zeros((N, A), dtype=torch.uint8).pin_memory()
        self.obs = None  # current observation (host), set by reset()
        self.all_time = np.zeros((N + 1, A), np.int32)  # env time of every recorded state (rl/rollout.py:808 all_time)
        self._finished_lengths = [[] for _ in range(N)]  # lengths of the episodes that ended at each env step
        self.time = np.zeros(A, np.int32)
        self.episode_score = np.zeros(A, np.float32)
        self.episode_len = np.zeros(A, np.int32)
        self.ep_count = 0
        # ---- TVF (rl/rollout.py:311-313)
        self.tvf = None
        if model.tvf_fixed_head_horizons is not None:
            from .tvf import TVFRunnerModule
            self.tvf = TVFRunnerModule(self)
            self._tvf_weights_dev = torch.as_tensor(np.asarray(self.tvf_weights, np.float32), device=dev)
            # value-phase weights: duplicate-head weights times the optional h_weighting (rl/tvf.py:51-62)
            self._tvf_value_weights_dev = torch.as_tensor(self.tvf.value_loss_weights(), device=dev)
            self._ext_estimate = torch.zeros((N + 1, A), dtype=torch.float32, device=dev)
        # ---- intrinsic rewards (rl/rollout.py:243-246, 279-280)
        if self.intrinsic:
            self.int_rewards = torch.zeros((N, A), dtype=torch.float32, device=dev)
            self.int_advantage = torch.zeros((N, A), dtype=torch.float32, device=dev)
            self._head_value = torch.zeros((N + 1, A), dtype=torch.float32, device=dev)  # one head's column, unit stride
            self._head_returns = torch.zeros((N, A), dtype=torch.float32, device=dev)
            self._int_rewards_host = torch.zeros((N, A), dtype=torch.float32).pin_memory()
            self._adv_moments = torch.zeros((2, 3), dtype=torch.float64, device=dev)
            self._rnd_stats = torch.zeros(_lib.PPO_RND_STATS, dtype=torch.float32, device=dev)
            self.intrinsic_reward_norm_scale = 1
            self.intrinsic_returns_rms = RunningMeanStd(shape=())
            # one entry per env of the whole run: the filter below runs on every rank over all ranks' rewards
            self.ems_norm = np.zeros([A * self.world])
        # ---- state hashing (rl/rollout.py:253-274): the hashes of a rollout and the two count tables, all in HBM
        self.hash = None
        if args.hash.enabled:
            from .hashing import LinearStateHasher, StateHashTracker
            if obs_dtype != torch.uint8 or len(self.state_shape) != 3:
                raise ValueError("hashing currently requires 8-bit [C, H, W] observations")  # :662
            normed = args.hash.input in ("normed", "normed_offset")
            if normed and model.obs_norm is None:
                raise ValueError(f"--hash_input={args.hash.input} needs --observation_normalization")
            # the first plane of a frame stack for atari, every element otherwise (:264-268)
            hash_state_shape = (1, *self.state_shape[1:]) if args.env.type == "atari" else self.state_shape
            hasher = LinearStateHasher(hash_state_shape, args.hash.bits, device=dev, bias=args.hash.bias)
            self.hash = StateHashTracker(hasher, N, A, decay=args.hash.decay, bonus=args.hash.bonus,
                                         bonus_method=args.hash.bonus_method, quantize=int(args.hash.quantize),
                                         mode=args.hash.input)
            self._hash_norm = model.obs_norm if normed else None
        # ---- experience replay (rl/rollout.py:295-309): the buffer and a rollout's aux records, in HBM
        self.replay_buffer = None
        if args.replay.enabled:
            from .replay import ExperienceReplayBuffer
            self.replay_buffer = ExperienceReplayBuffer(max_size=args.replay.size, obs_shape=self.state_shape,
                                                        obs_dtype=obs_dtype, mode=args.replay.mode,
                                                        thinning=args.replay.thinning, device=dev)
            self._replay_aux = torch.zeros((N * A, ExperienceReplayBuffer.N_AUX), dtype=torch.float32, device=dev)
        # ---- optimisers (rl/rollout.py:126-141)
        self.policy_optimizer = Optimizer(self.policy_net, args.policy_opt)
        self.value_optimizer = Optimizer(self.value_net, args.value_opt) if self.dual else self.policy_optimizer
        # as the reference (rl/rollout.py:145-148): present whenever the distil phase has its own optimiser configured,
        # whatever the architecture (only `dual` ever steps it; its moment buffers are allocated on first use)
        own_distil = args.distil_opt.epochs > 0 and not args.distil.use_policy_opt
        distil_state = AdamState() if args.distil_opt.optimizer == "adam" else None  # an SGD optimiser has no state object
        self.distil_optimizer = Optimizer(self.policy_net, args.distil_opt, distil_state) if own_distil else None
        self.rnd_optimizer = Optimizer(self.rnd, args.rnd_opt) if self.rnd is not None else None  # :154-157
        # ---- device scratch
        self._moments = torch.zeros(3, dtype=torch.float64, device=dev)
        self._moments_ws = torch.zeros(self.lib.ppo_moments_workspace_bytes() // 8, dtype=torch.float64, device=dev)
        self._mean_std = torch.zeros(2, dtype=torch.float32, device=dev)
        self._grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._sample_calls = 0
        # base seed of the counter-based device generators (action sampling, horizon dropout): --seed when given,
        # otherwise one draw from the run's host RNG (the reference's unseeded default gives a different stream per
        # run, rl/config.py:749); saved in checkpoints so that a resumed run continues the same streams
        self._device_seed = int(args.seed) if args.seed >= 0 else int(np.random.randint(1, 2**31 - 1))
        self._step_events = []
        self._phase_stats = {}
        self.timers = {}
        self._reducers = {}
        if self.world > 1:
            # one base seed for all ranks (the rank is mixed in where draws are made): an unseeded run would otherwise
            # checkpoint rank 0's draw and hand it to every rank on resume, i.e. switch the other ranks' streams
            seed_t = torch.tensor([self._device_seed], dtype=torch.int64, device=dev)
            parallel.broadcast_(seed_t)
            self._device_seed = int(seed_t.item())
            self.sync_replicas()
            for net in {id(n): n for n in (self.policy_net, self.value_net)}.values():
                red = parallel.GradReducer(net.grad, net.early_grad_offset)
                self._reducers[id(net)] = red
                net.grad_ready_hook = red.early
            if self.rnd is not None:
                # the predictor's gradient (split 0: no early bucket, the whole buffer is reduced in finish()), under the
                # key optimizer_step looks its optimiser's net up by
                self._reducers[id(self.rnd)] = parallel.GradReducer(self.rnd.grad, 0)
                self._check_rnd_steps_agree()

    def _rnd_steps(self):
        """(rows, per-rank minibatch, optimiser steps) of one RND phase on this rank (train_rnd)."""
        rows = round(self.N * self.A * args.rnd.experience_proportion)
        mb = parallel.local_minibatch(args.rnd_opt.mini_batch_size)
        return rows, mb, args.rnd_opt.epochs * (rows // max(mb, 1))

    def _check_rnd_steps_agree(self):
        """Every optimiser step of the predictor is a collective, so every rank must take the same number of them: said
        here, once, when the ranks are known to be in step - a rank that took fewer would leave the others waiting in
        an all-reduce."""
        mine = self._rnd_steps()
        got = [None] * self.world
        torch.distributed.all_gather_object(got, mine)
        if len(set(got)) != 1:
            raise ValueError(f"the ranks would take different numbers of RND optimiser steps (rows, minibatch, steps per "
                             f"rank: {got}); --agents, --n_steps and the --rnd_* flags must agree on every rank")

    def sync_replicas(self):
        """Data-parallel ranks must hold the same model: the only per-step exchange is the gradient all-reduce, so
        replicas that start apart stay apart, silently.  Parameters, Adam moments and the observation normaliser
        are broadcast from rank 0 (each rank initialised from its own process RNG when --seed is unset, and a
        restored checkpoint is read by every rank on its own), then a digest is compared across ranks."""
        nets = list({id(n): n for n in (self.policy_net, self.value_net)}.values())
        tensors = []
        for net in nets:
            tensors.append(net.flat)
            for t in (net.exp_avg, net.exp_avg_sq):
                if t is not None:
                    tensors.append(t)
        distil_state = self.distil_optimizer.state if self.distil_optimizer is not None else None  # None: SGD, nothing to send
        if distil_state is not None and distil_state.exp_avg is not None:
            tensors += [distil_state.exp_avg, distil_state.exp_avg_sq]
        rnd = self.rnd
        if rnd is not None:
            # the target is never trained, so replicas that drew their own would disagree for good; the predictor as the
            # other nets.  Whether the moments exist is rank 0's to say: a rank without them allocates them to receive
            has = torch.tensor([float(rnd.exp_avg is not None)], dtype=torch.float64, device=self.device)
            parallel.broadcast_(has)
            if has.item() and rnd.exp_avg is None:
                rnd.exp_avg, rnd.exp_avg_sq = torch.zeros_like(rnd.prediction_net.flat), torch.zeros_like(rnd.prediction_net.flat)
            elif not has.item():
                rnd.exp_avg = rnd.exp_avg_sq = None
            tensors += [rnd.target_net.flat, rnd.prediction_net.flat]
            if rnd.exp_avg is not None:
                tensors += [rnd.exp_avg, rnd.exp_avg_sq]
        norm = self.model.obs_norm
        if norm is not None:
            tensors += [norm.mean, norm.var, norm.mu, norm.std]
        for t in tensors:
            parallel.broadcast_(t)
        for net in nets:
            net.mark_weights_changed()
        counters = torch.tensor([float(n._adam_step) for n in nets] + [float(rnd.adam_steps) if rnd is not None else 0.0]
                                + [float(norm.count) if norm is not None else 0.0], dtype=torch.float64, device=self.device)
        parallel.broadcast_(counters)
        for n, c in zip(nets, counters[:len(nets)].tolist()):
            n._adam_step = int(c)
        if rnd is not None:
            rnd.adam_steps = int(counters[-2])
        if norm is not None:
            norm.count = float(counters[-1])
        return parallel.assert_identical_across_ranks(tensors, "model replicas")

    # ------------------------------------------------------------------ helpers
    def _call(self, fn_name, *a):
        rc = getattr(self.lib, fn_name)(*a, _lib.current_stream())
        if rc != 0:
            _lib.check(rc, fn_name)

    @property
    def ext_value(self):
        return self.value[:, :, 0]

    @property
    def ext_returns(self):
        return self.returns[:, :, 0]

    @property
    def int_value(self):
        return self.value[:, :, self.value_heads.index("int")]

    @property
    def int_returns(self):
        return self.returns[:, :, self.value_heads.index("int")]

    @property
    def rnd_lr(self):
        return self._lr(args.rnd_opt)

    @property
    def prev_obs(self):
        return self.all_obs[:-1]

    def anneal(self, x, mode: str = "linear"):
        """rl/rollout.py:331-355: scale x by the remaining (linear) or elapsed (linear_inc / quad_inc) fraction
        of training, measured in env steps over `anneal_target_epoch or epochs` million."""
        assert mode in ["off", "linear", "cos", "cos_linear", "linear_inc", "quad_inc"], f"invalid mode {mode}"
        frac = self.step / ((args.anneal_target_epoch or args.epochs) * 1e6)
        factor = 1.0
        if mode in ("linear", "cos_linear"):
            factor *= float(np.clip(1 - frac, 0, 1))
        if mode == "linear_inc":
            factor *= float(np.clip(frac, 0, 1))
        if mode == "quad_inc":
            factor *= float(np.clip(frac ** 2, 0, 1))
        if mode in ("cos", "cos_linear"):
            factor *= (1 + math.cos(math.pi * 2 * self.step / 20e6)) / 2  # the reference's fixed 20M-step period (:345)
        return x * factor

    def _lr(self, cfg):
        """Learning rate of one optimiser group, annealed linearly to 0 when its lr_anneal flag is set
        (rl/rollout.py:357-392)."""
        return self.anneal(cfg.lr, mode="linear" if cfg.lr_anneal else "off")

    @property
    def policy_lr(self):
        return self._lr(args.policy_opt)

    @property
    def value_lr(self):
        return self._lr(args.value_opt)

    @property
    def distil_lr(self):
        return self._lr(args.distil_opt)

    @property
    def ppo_epsilon(self):
        return self.anneal(args.ppo_epsilon, mode="linear" if args.ppo_epsilon_anneal else "off")

    @property
    def current_entropy_bonus(self):
        """rl/rollout.py:1568-1587: optional rescaling by the size of the action set, optional annealing."""
        if args.entropy_scaling == "off":
            bonus = args.entropy_bonus
        elif args.entropy_scaling == "average":
            assert args.entropy_scaling_base_actions > 0
            bonus = args.entropy_bonus * (args.entropy_scaling_base_actions / self.model.actions)
        elif args.entropy_scaling == "uniform":
            assert args.entropy_scaling_base_actions > 0
            bonus = args.entropy_bonus * (math.log(args.entropy_scaling_base_actions) / math.log(self.model.actions))
        else:
            raise ValueError(f"Invalid entropy_scaling method {args.entropy_scaling}.")
        return self.anneal(bonus) if args.entropy_anneal else bonus

    @property
    def current_advantage_epsilon(self):
        """rl/rollout.py:1589-1594."""
        if args.advantage_epsilon_anneal_factor > 0:
            return args.advantage_epsilon * max((1 / args.advantage_epsilon_anneal_factor) ** (self.step / 10e6), 1e-8)
        return args.advantage_epsilon

    @property
    def value_heads(self):
        return ["ext", "int"] if self.intrinsic else ["ext"]

    @property
    def tvf_horizons(self):
        return self.model.tvf_fixed_head_horizons

    @property
    def tvf_weights(self):
        """Loss weight per TVF head: duplicates removed when spacing the heads (rl/rollout.py:1323-1328)."""
        return np.asarray(self.model.tvf_fixed_head_weights, dtype=np.float32).copy()

    @property
    def K(self):
        return len(self.tvf_horizons)

    def get_current_actions_std(self):
        return 0.0 if self.action_dist == "discrete" else torch.exp(self.policy_net.params["log_std"])

    def reset(self):
        """rl/rollout.py:520-556: reset envs and per-env bookkeeping."""
        assert self.vec_env is not None, "Please assign vec_env first."
        self.obs = self.vec_env.reset()
        if self.tvf is not None:
            self.tvf.episode_length_buffer.clear()
            self.tvf.episode_length_buffer.append(1000)  # rl/rollout.py:553-555
        if self.hash is not None:
            self.hash.reset()  # rl/rollout.py:541-543
        self.time[:] = 0
        self.episode_score[:] = 0
        self.episode_len[:] = 0
        self.step = 0

    # ------------------------------------------------------------------ rollout
    def _forward_heads(self, obs, tag, tail=None, split_nets=()):
        """The head rows of the policy and the value net for `obs`, and whether the policy net's forward took `tail`
        (models.DualHeadNet.encode).  `split_nets`: see _rollout_pipelined."""
        pol, val = self.policy_net, self.value_net
        acts = pol.encode(obs, train=False, tag=tag, tail=tail, chain_split=any(n is pol for n in split_nets))
        hp = pol.heads(acts, tag)
        hv = hp
        if self.dual:
            hv = val.heads(val.encode(obs, train=False, tag=tag, chain_split=any(n is val for n in split_nets)), tag)
        return hp, hv, acts["tail_taken"]

    def _policy_step(self, t, lo=0, hi=None, tag="i", split_nets=()):
        """Forward + action sampling for envs [lo, hi) at env step t; writes those columns of row t of the
        rollout buffers.  The sampling counter is keyed by (rollout, t, env, action), so splitting the envs
        into groups does not change which action any env takes.  Dual architecture: the policy comes from
        policy_net, value (and TVF) estimates from value_net (rl/models.py:809-821)."""
        pol, val = self.policy_net, self.value_net
        hi = self.A if hi is None else hi
        B = hi - lo
        A, nA = self.A, self.n_actions
        final = t >= self.N
        seed = self._device_seed * 1000003 + self.rank
        counter = ((self._sample_calls + t) * A + lo) * nA
        first = t * A + lo  # first (t, env) element of this group's rows: pointer arithmetic, no tensor slicing

        def row(buf):
            if final:
                return None
            return buf.data_ptr() + first * buf.stride(1) * buf.element_size()

        values = None if self.dual else self.value.data_ptr() + first * self.value.stride(1) * 4
        discrete = self.action_dist == "discrete"
        tail = None
        if discrete:
            # the sampling rides on the policy net's dense + heads launch (one launch less per group and env step; same
            # bits) where that net has one (models.DualHeadNet.encode); otherwise it is launched below
            tail = (nA, 1.0, seed & (2**64 - 1), counter, row(self.log_policy), row(self.actions),
                    row(self.log_pac), row(self.raw_policy), values, self.VH)
        hp, hv, sampled = self._forward_heads(self.all_obs[t, lo:hi], tag, tail, split_nets)

        if sampled:
            pass
        elif discrete:
            self._call("ppo_policy_act_f32", _p(hp), B, pol.nh, nA, 1.0, None, seed & (2**64 - 1), counter, 0,
                       row(self.log_policy), row(self.actions), row(self.log_pac), row(self.raw_policy), values, self.VH)
        else:
            self._call("ppo_gaussian_act_f32", _p(hp), B, pol.nh, nA, _p(pol.params["log_std"]), None,
                       seed & (2**64 - 1), counter, 0, row(self.actions), row(self.log_pac), row(self.raw_policy),
                       values, self.VH)
        if self.dual:
            self.value[t, lo:hi].copy_(hv[:, val.col_value:val.col_value + self.VH])
        if self.tvf is not None:
            rec = self.tvf.tvf_untrimmed_value  # == tvf_value unless --tvf_trimming
            rec[t, lo:hi].copy_(hv[:, val.col_tvf:].view(B, val.K, self.VH))
            rec[t, lo:hi, 0].zero_()  # the first value head (h = 0) is zero by definition (rl/rollout.py:791)
        if self.rnd is not None and not final:
            # rl/rollout.py:764-766 without the host read: one channel-normalise launch, the two networks, and the error
            # straight into this group's columns of row t (the final state's error is never used, :871-878)
            self.rnd.prediction_error(self.all_obs[t, lo:hi], err=self.int_rewards[t, lo:hi], err_stride=1, tag="r" + tag)
        if self.hash is not None and self._hash_norm is None and t >= 1:
            # rl/rollout.py:756-757 without the host: row t holds what the envs returned at step t - 1 (the final state
            # included); one launch on this group's stream writes its hashes, the tables follow after the rollout
            self.hash.hash_step(self.all_obs[t, lo:hi], t - 1, lo, hi)

    def _policy_step_chunks(self, t, tag="i"):
        """A batch-norm model's policy step at env step t: ONE step over all A envs on the current stream, in chunks of
        --max_micro_batch_size in row order as detached_batch_forward cuts them (rl/rollout.py:558-598) - each chunk is
        its own batch-norm batch and its own update of the running statistics, in both nets of a dual model."""
        micro = max(int(args.max_micro_batch_size), 1)
        for lo in range(0, self.A, micro):
            self._policy_step(t, lo, min(self.A, lo + micro), tag=tag)

    def _hash_normed_row(self, t):
        """The normed hash inputs read the normaliser's constants as they stand after step t - 1's statistics update and
        before step t's (rl/rollout.py:735-741, 757): called between the upload of row t and norm.update(all_obs[t])."""
        if self.hash is not None and self._hash_norm is not None and t >= 1:
            self.hash.hash_step(self.all_obs[t], t - 1, 0, self.A, norm=self._hash_norm)

    def _finish_hashing(self):
        """End of a rollout (rl/rollout.py:895-924): bring the tables up to date from obs_hashes, step by step in the
        reference's order - the env groups run a step apart, so it cannot happen during the rollout - then pay the bonus
        from the final recent counts, before the clip of the intrinsic rewards (calculate_intrinsic_returns).

        Data parallel: the tables count the hashes of every rank's envs (one gather, [N, world * A] int32), so they are
        replicated - the tables a one-rank run over the same envs holds - and the bonus, the `binary` threshold and the
        log lines read them as they are; the bonus goes to the rank's own columns."""
        self.hash.update_counts(parallel.gather_columns(self.hash.obs_hashes) if self.world > 1 else None)
        if self.hash.bonus != 0:
            self.hash.add_bonus(self.int_rewards)
        if not args.disable_logging:
            self.hash.launch_stats()  # read in calculate_returns with the other statistics

    def _log_finished(self, finished, ep_len, ep_score, t=None):
        if finished.any():
            self.ep_count += int(finished.sum())
            if t is not None:
                self._finished_lengths[t].extend(int(x) for x in np.asarray(ep_len)[finished])
            for s, l in zip(ep_score[finished][:8], ep_len[finished][:8]):
                if getattr(self, "_pending_episodes", None) is not None:
                    self._pending_episodes.append((s, l))  # logged once the rollout stands (generate_rollout)
                    continue
                self.log.watch_full("ep_score", s, history_length=100)
                self.log.watch_full("ep_length", l, history_length=100)

    def generate_rollout(self):
        """Fill the rollout buffers with N steps from A envs (rl/rollout.py:702-969).

        With a `SplitVecEnv` of array-stepping parts the step is software-pipelined: the GPU runs the policy
        for one group of envs while the host steps the other group, so neither waits for the whole of the
        other (the reference overlaps nothing: rl/rollout.py:792-816 is forward -> sync -> step)."""
        assert self.vec_env is not None, "Please attach vector environment first."
        N, A = self.N, self.A
        self.model.train()  # rl/rollout.py:712 (read by batch-norm nets only); eval() again at the end, :927
        try:
            self._generate_rollout(N, A)
        finally:
            self.model.eval()

    def _generate_rollout(self, N, A):
        self._finished_lengths = [[] for _ in range(N)]
        if self.intrinsic and self.rnd is None:
            self.int_rewards.zero_()  # rl/rollout.py:714 (with RND every element is written during the rollout)
        env = self.vec_env
        parts = [env] if self.force_generic_rollout else getattr(env, "parts", [env])
        if not self.force_generic_rollout and all(hasattr(p, "step_arrays") for p in parts):
            # array-stepping groups: the synthetic env, and gym-API envs behind the process pool and its vector
            # wrappers (ppo_amd/hybrid_vec_env.py `PoolGroup`, ppo_amd/wrappers.py `parts`)
            nets = list({id(n): n for n in (self.policy_net, self.value_net)}.values())
            armed = [n for n in nets if n.chain_split_armed()]
            # the two-workgroups-per-image launch (models.CHAIN_SPLIT) can, in principle, time out waiting for a partner
            # workgroup; its results are then void.  An env that can be put back exactly is, and the rollout is redone
            snap = self._rollout_snapshot(env) if armed and getattr(env, "exact_snapshot", False) else None
            self._pending_episodes = []
            self._rollout_pipelined(parts, armed)
            if armed and any(n.chain_split_error() for n in armed):
                self._chain_split_failed(armed, env, snap, parts)
            for s_, l_ in self._pending_episodes:
                self.log.watch_full("ep_score", s_, history_length=100)
                self.log.watch_full("ep_length", l_, history_length=100)
            self._pending_episodes = None
            if hasattr(env, "finish_rollout"):
                # what the vector wrappers do to the rewards needs every env's reward of a step at once (the running
                # return statistics): applied here, step by step in the reference's order, once the rollout is in
                env.finish_rollout(self._rewards_host.numpy(), self._dones_host.numpy())
        else:
            self._rollout_generic(env)
        if self.hash is not None:
            self._finish_hashing()
        self.ext_rewards.copy_(self._rewards_host, non_blocking=True)
        self.terminals.view(torch.uint8).copy_(self._dones_host, non_blocking=True)
        if self.tvf is not None:
            self.tvf.apply_trimming(self.all_time, self._finished_lengths)  # no-op unless --tvf_trimming
        self._sample_calls += N + 1
        self.step += N * A * self.world

    def _rollout_snapshot(self, env):
        """Everything a pipelined rollout changes on the host, for an env whose save_state is complete."""
        from . import checkpoint
        from .wrappers import VecWrapper
        layers, inner = [], env
        while isinstance(inner, VecWrapper):
            layers.append((inner, inner.snapshot_state()))
            inner = inner.__dict__.get("env")
        snap = {"env": copy.deepcopy(checkpoint.save_env_state(inner)), "inner": inner, "layers": layers,
                "time": self.time.copy(),
                "episode_score": self.episode_score.copy(), "episode_len": self.episode_len.copy(),
                "ep_count": self.ep_count, "np_random": np.random.get_state()}
        if self.tvf is not None:
            snap["episode_length_buffer"] = list(self.tvf.episode_length_buffer)
        return snap

    def _chain_split_failed(self, nets, env, snap, parts):
        """A workgroup of the two-workgroups-per-image launch gave up waiting for its partner's half of a map: the head
        outputs of this rollout (and the actions drawn from them) cannot be trusted.  The one-workgroup launch takes
        over for the rest of the run, and the rollout is generated again: from the saved start state where the env
        can be put back exactly (same bytes as a run with PPO_AMD_CHAIN_SPLIT=0: the sampling counter has not
        moved), otherwise from where the envs are now (their N steps are lost, nothing else)."""
        from . import checkpoint
        for n in nets:
            n.chain_split_disable()
        self.log.warn("the split chained launch timed out waiting for a partner workgroup: switched to one workgroup "
                      "per image for the rest of the run and redoing this rollout"
                      + (" from its start state" if snap is not None else " from the envs' current state"))
        if snap is not None:
            for wrapper, state in snap["layers"]:
                wrapper.restore_snapshot(state)
            checkpoint.restore_env_state(snap["inner"], snap["env"])
            self.time = snap["time"].copy()
            self.episode_score[:] = snap["episode_score"]
            self.episode_len[:] = snap["episode_len"]
            self.ep_count = snap["ep_count"]
            np.random.set_state(snap["np_random"])
            if self.tvf is not None:
                self.tvf.episode_length_buffer.clear()
                self.tvf.episode_length_buffer.extend(snap["episode_length_buffer"])
            self._pending_episodes = []
        elif hasattr(env, "finish_rollout"):
            # the lost steps were real env steps: the vector wrappers' statistics take them in as usual
            env.finish_rollout(self._rewards_host.numpy().copy(), self._dones_host.numpy().copy())
        self._finished_lengths = [[] for _ in range(self.N)]
        if self.intrinsic:
            self.int_rewards.zero_()  # rl/rollout.py:714; every element is written again below
        self._rollout_pipelined(parts, [])

    def _rollout_pipelined(self, parts, split_nets=()):
        """`split_nets`: the networks whose forwards may take the two-workgroups-per-image launch during this rollout
        (the caller checks their error word afterwards)."""
        N = self.N
        self.all_time[0] = self.time
        rew_np, done_np = self._rewards_host.numpy(), self._dones_host.numpy()
        act_np = self._actions_host.numpy()
        bounds = np.cumsum([0] + [p.num_envs for p in parts]).tolist()
        assert bounds[-1] == self.A
        P = len(parts)
        if len(self._step_events) < P:
            self._step_events = [torch.cuda.Event() for _ in range(P)]
            self._copy_events = [torch.cuda.Event() for _ in range(P)]
            self._copy_stream = torch.cuda.Stream(device=self.device)
            self._part_streams = [torch.cuda.Stream(device=self.device) for _ in range(P)]
        events, copy_events, copy_stream = self._step_events, self._copy_events, self._copy_stream
        main = torch.cuda.current_stream()
        # each env group has its own compute stream (and scratch-buffer set), so the policy steps of the two
        # groups overlap on the GPU: at half the batch most kernels expose fewer workgroups than there are CUs
        streams = self._part_streams if P > 1 else [main]
        # the optimiser steps leave the packed convolution operands stale and the next forward repacks them on its own
        # stream; on a group's stream that would race the other group's forward, which reads them: repack here, on main
        for net in {id(n): n for n in (self.policy_net, self.value_net)}.values():
            net._refresh_packed()
        copy_stream.wait_stream(main)  # earlier readers of all_obs (the previous train phase) are done
        for s_ in streams:
            if s_ is not main:
                s_.wait_stream(main)
        norm = self.model.obs_norm
        # the groups run a step apart, each sending its own next observations up as it is stepped - unless a step needs
        # every env's observations at once (observation normalisation, batch norm: the lock-step loop below)
        own_upload = norm is None and not self.batch_norm

        # a group may be stepped (and uploaded) in several pieces: a leaf's H2D runs while the next leaf is stepped
        leaves = []
        for i in range(P):
            lo, row = bounds[i], []
            for leaf in getattr(parts[i], "leaves", [parts[i]]):
                row.append((leaf, lo, lo + leaf.num_envs))
                lo += leaf.num_envs
            leaves.append(row)

        def upload(i, t, only=None):
            # H2D of group i's observations (pinned -> HBM) into row t on the copy stream, so it runs on a DMA engine
            # under the other group's policy step.  (set_stream rather than the `with torch.cuda.stream` context: this
            # runs 2 x 257 times per rollout and the host is on the critical path; the caller restores the stream)
            torch.cuda.set_stream(copy_stream)
            for leaf, lo, hi in (leaves[i] if only is None else [only]):
                self.all_obs[t, lo:hi].copy_(leaf.obs_t, non_blocking=True)

        def enqueue(i, t):
            # policy + sampling for group i at step t behind its upload (issued when its envs were stepped), actions D2H;
            # all async
            lo, hi = bounds[i], bounds[i + 1]
            torch.cuda.set_stream(streams[i])
            streams[i].wait_event(copy_events[i])
            self._policy_step(t, lo, hi, tag=tags[i], split_nets=split_nets)
            if t < N:
                host_rows[i].copy_(self.actions[t, lo:hi], non_blocking=True)
                events[i].record()

        def step_envs(i, t):
            # the one host wait of group i's step: its actions have landed; then step it on host cores, leaf by leaf,
            # each leaf's next observations going up as soon as they exist
            events[i].synchronize()
            for leaf, lo, hi in leaves[i]:
                if own_upload and UPLOAD_CHUNKS > 1 and hasattr(leaf, "step_upload"):
                    # stepping and upload in one call: each quarter of the group goes up while the rest is stepped
                    torch.cuda.set_stream(copy_stream)
                    leaf.step_upload(act_np[lo:hi], rew_np[t, lo:hi], done_np[t, lo:hi], self.all_obs[t + 1, lo:hi],
                                     copy_stream, UPLOAD_CHUNKS)
                    continue
                leaf.step_arrays(act_np[lo:hi], rew_np[t, lo:hi], done_np[t, lo:hi])
                if own_upload:
                    upload(i, t + 1, only=(leaf, lo, hi))
            if own_upload:
                copy_events[i].record()  # (current stream = the copy stream: upload() left it so)
            lo, hi = bounds[i], bounds[i + 1]
            time_now, ep_len, ep_score = parts[i].last_episode_stats
            done = done_np[t, lo:hi].astype(bool)
            self.all_time[t + 1, lo:hi] = parts[i].landed_time(done)
            self._log_finished(done, ep_len, ep_score, t)

        tags = [f"i{i}" if P > 1 else "i" for i in range(P)]
        host_rows = [self._actions_host[bounds[i]:bounds[i + 1]] for i in range(P)]
        if norm is not None or self.batch_norm:
            # Observation normalisation: the running statistics take in EVERY env's observation of step t before any
            # group's forward of step t (rl/rollout.py:735-741), so the groups cannot run a step apart.  Per step: both
            # uploads, one statistics update on the first group's stream, then the groups' policy steps on their own
            # streams; the host steps group i while the GPU still runs the later groups' policy steps.  (The generic
            # path synchronised the whole device once per env step and overlapped nothing.)
            # A batch-norm model has the same shape for another reason: a forward normalises with the statistics of its
            # own batch, which is all A envs (in chunks, _policy_step_chunks), and every forward updates the running
            # statistics, so the policy step is one, on the first group's stream, before any env is stepped.
            if not hasattr(self, "_norm_event"):
                self._norm_event = torch.cuda.Event()
            try:
                for t in range(N + 1):
                    for i in range(P):
                        upload(i, t)
                    copy_events[0].record()
                    torch.cuda.set_stream(streams[0])
                    streams[0].wait_event(copy_events[0])
                    self._hash_normed_row(t)
                    if norm is not None and t < N:
                        norm.update(self.all_obs[t])
                    if self.batch_norm:
                        self._policy_step_chunks(t, tag=tags[0])
                    self._norm_event.record()
                    for i in range(P):
                        if self.batch_norm:
                            if t < N:  # (stream 0, behind the policy step)
                                host_rows[i].copy_(self.actions[t, bounds[i]:bounds[i + 1]], non_blocking=True)
                                events[i].record()
                            continue
                        torch.cuda.set_stream(streams[i])
                        streams[i].wait_event(self._norm_event)
                        self._policy_step(t, bounds[i], bounds[i + 1], tag=tags[i], split_nets=split_nets)
                        if t < N:
                            host_rows[i].copy_(self.actions[t, bounds[i]:bounds[i + 1]], non_blocking=True)
                            events[i].record()
                    if t < N:
                        for i in range(P):
                            step_envs(i, t)
                        # the next step's upload overwrites nothing the GPU still reads, but its statistics update
                        # must follow this step's forwards (they read mu / std): order stream 0 behind the others
                        for s_ in streams[1:]:
                            streams[0].wait_stream(s_)
            finally:
                torch.cuda.set_stream(main)
            for s_ in streams:
                if s_ is not main:
                    main.wait_stream(s_)
            main.wait_stream(copy_stream)
            self.time = self.all_time[N].copy()
            self.obs = parts[0].obs if P == 1 else np.concatenate([p.obs for p in parts])
            return
        try:
            for i in range(P):  # the observations the envs hold now are row 0; later rows go up from step_envs
                upload(i, 0)
                copy_events[i].record()
            for t in range(N + 1):
                for i in range(P):
                    enqueue(i, t)  # needs obs(i, t): group i was stepped for t-1 below
                    j, tj = (i + 1) % P, (t if i + 1 == P else t - 1)
                    if 0 <= tj < N:
                        step_envs(j, tj)  # overlaps the GPU work just queued for group i
        finally:
            torch.cuda.set_stream(main)
        for s_ in streams:
            if s_ is not main:
                main.wait_stream(s_)
        main.wait_stream(copy_stream)  # as in the normalised path above: the next phase starts behind every upload
        self.time = self.all_time[N].copy()
        self.obs = parts[0].obs if P == 1 else np.concatenate([p.obs for p in parts])

    def _rollout_generic(self, env):
        """gym-API vector env (`step(actions) -> obs, rew, done, infos`), one group.  Also the path taken with
        observation normalisation: the running statistics are updated from ALL envs' observations of step t
        before that step's forward, as the reference does (rl/rollout.py:735-741), which the group-pipelined
        rollout cannot express."""
        N = self.N
        norm = self.model.obs_norm
        rew_np, done_np = self._rewards_host.numpy(), self._dones_host.numpy()
        act_np = self._actions_host.numpy()
        stream = torch.cuda.current_stream()
        for t in range(N + 1):
            self.all_time[t] = self.time
            # zero-copy view: with the process pool self.obs IS the shared pinned block, so this is one async H2D
            src = self.obs if self.obs.flags.c_contiguous else np.ascontiguousarray(self.obs)
            self.all_obs[t].copy_(torch.from_numpy(src), non_blocking=True)
            self._hash_normed_row(t)
            if norm is not None and t < N:
                norm.update(self.all_obs[t])
            if self.batch_norm:
                self._policy_step_chunks(t)
            else:
                self._policy_step(t)
            if t == N:
                break  # final state: only its value estimate is needed (rl/rollout.py:871-878)
            self._actions_host.copy_(self.actions[t], non_blocking=True)
            stream.synchronize()  # the one device->host sync of the step: the envs need the actions
            self.obs, rew, dones, infos = env.step(act_np.copy())
            rew_np[t] = rew
            done_np[t] = dones
            self.time = np.asarray([i.get("time", 0) for i in infos], np.int32)  # rl/rollout.py:753
            self._log_finished(np.asarray(dones, bool), np.asarray([i.get("ep_length", 0) for i in infos]),
                               np.asarray([i.get("ep_score", 0.0) for i in infos]), t)

    @torch.no_grad()
    def detached_batch_forward(self, obs, aux_features=None, max_batch_size=None, **kwargs):
        """Forward a large batch in chunks, results concatenated (rl/rollout.py:557-598)."""
        max_batch_size = max_batch_size or args.max_micro_batch_size
        obs = self.model.prep_for_model(obs)
        chunks = []
        for i in range(0, obs.shape[0], max_batch_size):
            out = self.model.forward(obs[i:i + max_batch_size], **kwargs)
            chunks.append({k: v.clone() for k, v in out.items()})
        return {k: torch.cat([c[k] for c in chunks], dim=0) for k in chunks[0]}

    # ------------------------------------------------------------------ returns
    def calculate_returns(self):
        """Advantages (lambda_policy) and value targets (lambda_value) in one fused scan
        (rl/rollout.py:1182-1285 -> rl/returns.py:7-67), then the TVF return targets (rl/tvf.py:210-271)."""
        N, A = self.N, self.A
        self.model.eval()  # rl/rollout.py:1192
        if self.replay_buffer is not None:
            # first, so that the draws of the add come before those of the TVF return sampler below and of the log lines
            # at the end, as in the reference (whose add closes generate_rollout, rl/rollout.py:956-969)
            self._add_rollout_to_replay()
        if self.tvf is not None:
            self._ext_estimate.copy_(self.tvf.get_tvf_ext_value_estimate(new_gamma=args.gamma))
            value = self._ext_estimate
        elif self.VH > 1:
            # the scan wants unit-stride rows: the ext head's column of the [N + 1, A, VH] buffer is copied out, and its
            # returns are copied back into column 0 (same arithmetic as with one head)
            self._head_value.copy_(self.ext_value)
            value = self._head_value
        else:
            value = self.value.view(N + 1, A)
        ret_out = self.returns if self.VH == 1 else self._head_returns
        self._call("ppo_gae_scan_f32", _p(self.ext_rewards), _p(value), _p(value[N]), _p(self.terminals),
                   _lib.PPO_TERM_U8, _p(self.advantage), _p(ret_out), N, A, A, float(args.gamma),
                   float(args.lambda_policy), float(args.lambda_value), _lib.PPO_SCAN_AUTO)
        if self.VH > 1:
            self.ext_returns.copy_(ret_out)
            value = self.ext_value  # (what the log lines below read; _head_value is reused for the int head)
        if self.intrinsic:
            self._add_intrinsic_advantage()
        if self.tvf is not None:
            self.tvf.tvf_returns[..., 0].copy_(self.tvf.calculate_tvf_returns(value_head="ext"))
        if not args.disable_logging:
            self.log_returns(value)

    def _rollout_aux(self, out, time_and_step):
        """The rollout's aux records [N * A, 16] float32 into `out` (device): reward and action (generate_aux_buffer,
        rl/rollout.py:2006-2014), with `time_and_step` also the env time and the global step of every row (:957-968; the
        rollout's steps start where `self.step` stood before it).  vtarg stays 0: the aux phase is not built."""
        R = type(self.replay_buffer)
        n = self.N * self.A
        out.zero_()
        out[:, R.AUX_REWARD].copy_(self.ext_rewards.view(n))
        actions = self.actions[:, :, 0] if self.actions.dim() == 3 else self.actions  # continuous: the first one (rl/replay.py:184-186)
        out[:, R.AUX_ACTION].copy_(actions.reshape(n))
        if time_and_step:
            out[:, R.AUX_TIME].copy_(torch.from_numpy(self.all_time[:self.N].reshape(n)).to(self.device, non_blocking=True))
            start = self.step - n * self.world
            out[:, R.AUX_STEP].copy_(torch.arange(start, start + n, dtype=torch.int64, device=self.device))
        return out

    def _add_rollout_to_replay(self):
        """rl/rollout.py:956-969: the rollout's observations and aux records go into the buffer, read where they lie -
        one scatter launch (ExperienceReplayBuffer.add_experience)."""
        n = self.N * self.A
        self.replay_buffer.add_experience(self.all_obs[:self.N].view(n, *self.state_shape),
                                          self._rollout_aux(self._replay_aux, time_and_step=True))

    def log_hashing(self, states, recent):
        """rl/rollout.py:1243-1250: the visited (hashed) states so far, how many this rollout added, and the bins whose
        recent count is at least 1.  The two counts were reduced on the device at the end of the rollout and came to the
        host in log_returns' one copy."""
        states, recent = int(states), int(recent)
        old = self.log["hash_states"] if "hash_states" in self.log else 0  # the value logged after the previous rollout
        self.log.watch("hash_states", states, display_width=8, display_name="h_states")
        self.log.watch("*hash_delta", int(states - old), display_name="h_delta")
        self.log.watch("*hash_recent", recent, display_name="h_batch")

    def calculate_intrinsic_returns(self):
        """rl/rollout.py:1140-1180 (and the clip of :929): normalises `int_rewards` in place and fills `int_advantage`
        and `int_returns`; returns `int_advantage` (device).

        One device->host copy of the N x A rewards; the forward EMS filter and the running variance of its output are
        N float64 updates on the host, exactly the reference's expressions (a device kernel would save nothing and lose
        bit-exactness); the scale goes back as a scalar argument.  NumPy >= 2: `int_rewards / scale` with the float64
        NumPy scalar `scale` is a float64 division (and the mean of --ir_center a float64 mean), which the fixture
        records and ppo_scale_shift_clip_f32 follows."""
        N, A = self.N, self.A
        n = N * A
        if args.ir.normalize and self.world > 1:
            # the filter runs on every rank over every rank's rewards [N, world * A] (and terminals), so ems_norm, the
            # running variance and the scale are the one-rank run's and the same everywhere.  `.cpu()` is a copy on the
            # current stream, which the gather has made wait for its collective: the host reads the finished array
            rewards = np.clip(parallel.gather_columns(self.int_rewards).cpu().numpy(), -5, 5)  # :929
            terminals = np.zeros(rewards.shape, bool) if args.ir.propagation \
                else parallel.gather_columns(self.terminals).cpu().numpy()
            self.ems_norm, self.intrinsic_reward_norm_scale = intrinsic_return_scale(
                self.ems_norm, self.intrinsic_returns_rms, rewards, terminals, args.gamma_int, args.ir.propagation)
        elif args.ir.normalize:
            self._int_rewards_host.copy_(self.int_rewards)
            rewards = np.clip(self._int_rewards_host.numpy(), -5, 5)  # :929
            terminals = self.terminals.cpu().numpy() if not args.ir.propagation else np.zeros((N, A), bool)
            self.ems_norm, self.intrinsic_reward_norm_scale = intrinsic_return_scale(
                self.ems_norm, self.intrinsic_returns_rms, rewards, terminals, args.gamma_int, args.ir.propagation)
        self._call("ppo_scale_shift_clip_f32", _p(self.int_rewards), n, 5.0,
                   float(self.intrinsic_reward_norm_scale) if args.ir.normalize else 1.0, None, _p(self.int_rewards))
        if args.ir.center:
            # the mean of the scaled rewards, summed in float64 in a fixed order, then one more pass that subtracts it
            # (the mean of the whole batch: the moments are summed over ranks first, as in _normalize_advantages)
            self._call("ppo_moments_f64", _p(self.int_rewards), n, _p(self._moments), _p(self._moments_ws))
            parallel.allreduce_sum_(self._moments)
            self._call("ppo_scale_shift_clip_f32", _p(self.int_rewards), n, 0.0, 1.0, _p(self._moments), _p(self.int_rewards))
        self._head_value.copy_(self.int_value)
        value = self._head_value
        # both lambdas are lambda_policy, so the "returns" output is advantage + V (:1179)
        self._call("ppo_gae_scan_f32", _p(self.int_rewards), _p(value), _p(value[N]),
                   None if args.ir.propagation else _p(self.terminals),
                   _lib.PPO_TERM_NONE if args.ir.propagation else _lib.PPO_TERM_U8, _p(self.int_advantage),
                   _p(self._head_returns), N, A, A, float(args.gamma_int), float(args.lambda_policy),
                   float(args.lambda_policy), _lib.PPO_SCAN_AUTO)
        self.int_returns.copy_(self._head_returns)
        return self.int_advantage

    def _add_intrinsic_advantage(self):
        """advantage += ir_scale * int_advantage, and the three log lines (rl/rollout.py:1226-1231)."""
        n = self.N * self.A
        logging = not args.disable_logging
        if logging:
            self._call("ppo_moments_f64", _p(self.advantage), n, _p(self._adv_moments[0]), _p(self._moments_ws))
        int_advantage = self.calculate_intrinsic_returns()
        self._call("ppo_axpy_f32", _p(self.advantage), _p(int_advantage), float(args.ir.scale), n)
        if logging:
            self._call("ppo_moments_f64", _p(int_advantage), n, _p(self._adv_moments[1]), _p(self._moments_ws))
            parallel.allreduce_sum_(self._adv_moments)  # the log lines speak of the whole batch
            (_e1, e2, _n), (i1, i2, cnt) = self._adv_moments.cpu().tolist()
            scale = float(args.ir.scale)
            mean = scale * i1 / cnt
            self.log.watch("*adv_int_mean", mean, display_width=0)  # watch_mean_std("*adv_int", ...)
            self.log.watch("*adv_int_std", math.sqrt(max(scale * scale * i2 / cnt - mean * mean, 0.0)), display_width=0)
            self.log.watch_mean("adv_ratio", math.sqrt(e2 / (scale * scale * i2)) if i2 > 0 and scale else float("inf"),
                                display_width=0)
            self.log.watch_mean("*ir_scale", float(self.intrinsic_reward_norm_scale))

    @property
    def reward_scale(self):
        """What the env stack multiplied the rewards by (rl/rollout.py:1793-1802)."""
        if args.env.reward_normalization == "off":
            return 1.0
        if args.env.reward_normalization != "rms":
            raise ValueError(f"Invalid reward normalization {args.env.reward_normalization}")
        from . import wrappers
        norm = wrappers.get_wrapper(self.vec_env, wrappers.VecNormalizeRewardWrapper)
        return 1.0 if norm is None else float(1.0 / norm.std)

    def log_returns(self, value_estimate):
        """The diagnostics the reference writes at the end of calculate_returns (rl/rollout.py:1199, 1252-1285):
        moments of the value estimates / advantages / returns every batch; feature statistics and explained
        variance every 4th batch unless --disable_ev."""
        N = self.N
        head0 = self.value_heads[0]
        named = [("*ext_value_estimates", value_estimate, {}), ("adv_ext", self.advantage, {"display_width": 0})]
        for i, head in enumerate(self.value_heads):
            named.append((f"*return_{head}", self.returns[..., i], {"display_width": 0}))
            named.append((f"value_{head}", self.value[..., i], {"display_name": "v_" + head}))
        # (the two hashing counts, int64 on the device, ride along in the same device->host copy)
        counts = self.hash.device_stats if self.hash is not None else None
        extra = value_quality.log_batch_moments(self.log, named, extra=counts)
        if self.hash is not None:
            self.log_hashing(*extra)
        self.log.watch_mean("reward_scale", self.reward_scale, display_width=0, history_length=1)
        self.log.watch_mean("entropy_bonus", self.current_entropy_bonus, display_width=0, history_length=1)
        self.log.watch("*gamma", args.gamma)
        if self.tvf is not None:
            self.log.watch("*tvf_gamma", args.tvf.gamma)
            self.log.watch_stats("*tvf_return_ext", self.tvf.tvf_returns[:, :, -1].cpu().numpy())
        if self.replay_buffer is not None and self.batch_counter % 4 == 0:
            self.replay_buffer.log_stats(self.log)  # rl/rollout.py:1272-1276
        if args.disable_ev or self.batch_counter % 4 != 3:
            return
        value_quality.log_feature_statistics(
            self.log, self.detached_batch_forward(self.all_obs[0], output="full", include_features=True))
        ext_value = self.value[..., self.value_heads.index("ext")] if "ext" in self.value_heads else self.value[..., 0]
        targets = calculate_bootstrapped_returns(self.ext_rewards, self.terminals, ext_value[N], float(args.gamma))
        if self.tvf is not None:
            self.tvf.log_tvf_curve_quality(ext_value[:N], targets)
        else:
            value_quality.log_dna_value_quality(self.log, ext_value[:N], targets)

    # ------------------------------------------------------------------ training
    def _normalize_advantages(self):
        """(a - mean) / (std + eps) over the whole (global) batch (rl/rollout.py:1887-1900)."""
        n = self.N * self.A
        self._call("ppo_moments_f64", _p(self.advantage), n, _p(self._moments), _p(self._moments_ws))
        parallel.allreduce_sum_(self._moments)
        self._call("ppo_normalize_f32", _p(self.advantage), n, _p(self._moments), float(self.current_advantage_epsilon),
                   _p(self.norm_advantage), _p(self._mean_std))
        if args.advantage_clipping is not None:
            self.norm_advantage.clamp_(-args.advantage_clipping, args.advantage_clipping)

    def optimizer_step(self, optimizer=None, label="policy", norm_out=None):
        """All-reduce (DP) + global-norm clip + Adam or SGD in the flat buffer (rl/rollout.py:1287-1321)."""
        opt = optimizer or self.policy_optimizer
        net, cfg = opt.net, opt.cfg
        red = self._reducers.get(id(net))
        if red is not None:
            red.finish()  # late bucket + join of the early one that left during the backward pass
        max_grad_norm = args.max_grad_norm if args.grad_clip_mode == "global_norm" else 0.0
        norm = self._grad_norm if norm_out is None else norm_out
        if opt.kind == "sgd":
            net.sgd_step(lr=self._lr(cfg), max_grad_norm=max_grad_norm, grad_div=float(self.world), grad_norm_out=norm)
        else:
            net.adam_step(lr=self._lr(cfg), beta1=cfg.adam_beta1, beta2=cfg.adam_beta2, eps=cfg.adam_epsilon,
                          max_grad_norm=max_grad_norm, grad_div=float(self.world), grad_norm_out=norm, state=opt.state)
        return norm

    def _micro_batches(self, mb, force_micro_batch_size=None):
        """(micro-batch size, count) of a per-rank minibatch of mb samples (rl/rollout.py:2310-2316): the reference
        splits a minibatch into passes of at most --max_micro_batch_size samples whose gradients accumulate."""
        micro = force_micro_batch_size if force_micro_batch_size is not None else min(args.max_micro_batch_size, mb)
        if micro <= 0 or mb % micro:
            raise ValueError(f"minibatch {mb} is not a multiple of the micro-batch size {micro}")
        return micro, mb // micro

    class _Accumulator:
        """Gradient accumulation over the micro-batches of one minibatch.  Every backward pass of the HIP path
        OVERWRITES net.grad, so passes 2.. are added into a second flat buffer (ppo_accumulate_f32) and the sum is
        copied back before the optimiser step; with one micro-batch nothing happens.  The data-parallel early-bucket
        hook is parked meanwhile: only the accumulated gradient may leave."""

        def __init__(self, runner, net, count):
            self.r, self.net, self.count, self.k = runner, net, count, 0
            self.hook = net.grad_ready_hook
            if count > 1:
                net.grad_ready_hook = None
                self.acc = net._buf("grad_accum", tuple(net.grad.shape))

        def after_backward(self):
            if self.count > 1:
                if self.k == 0:
                    self.acc.copy_(self.net.grad)
                else:
                    self.r._call("ppo_accumulate_f32", _p(self.acc), _p(self.net.grad), self.net.grad.numel())
            self.k += 1

        def finish(self):
            if self.count > 1:
                self.net.grad.copy_(self.acc)
                self.net._presummed = 0  # the last pass's sums of g^2 are not the accumulated gradient's
            self.restore_hook()

        def restore_hook(self):
            """Also the exit path of a failed step: the parked hook must come back whatever happened."""
            self.net.grad_ready_hook = self.hook

    def _noise_pass(self, net, step_fn, obs_all):
        """step(index) for a noise-scale estimate (ppo_amd/sns.py): one forward + backward pass of a phase's minibatch
        step `step_fn` with loss_scale 1 on the rows `index` of the batch `obs_all` [B, *state_shape], through the input
        form the phase's epochs use (_run_epochs): the fused MLP index read, the in-conv index read, or a gather launch.
        The per-sample statistics are dropped."""
        B = int(obs_all.shape[0])
        obs_rows = obs_all.view(B, -1)
        row_bytes = obs_rows.shape[1] * obs_rows.element_size()
        fused = bool(getattr(net, "mlp_fused", False)) and net.obs_norm is None and self.all_obs.dtype == torch.float32
        in_conv = not fused and hasattr(net, "takes_obs_index") and net.takes_obs_index(self.all_obs)

        def one_pass(idx):
            if fused:
                step_fn(obs_rows, idx, 1.0, stat_sums=None, stat_accumulate=False, obs_indexed=True)
            elif in_conv:
                step_fn(obs_all, idx, 1.0, obs_indexed=True)
            else:
                rows = int(idx.shape[0])
                mb_obs = net._buf("mb_obs", (rows, *self.state_shape), self.all_obs.dtype)
                self._call("ppo_gather_rows", _p(obs_rows), row_bytes, B, _p(idx), rows, _p(mb_obs))
                step_fn(mb_obs, idx, 1.0)
        return one_pass

    class _GlobalKLPass:
        """The global KL pass of a policy minibatch (rl/rollout.py:1723-1738): KL(new || old) over the S global states
        `rows` (rows of the rollout, [S] int32 device) against `old` [S, nA], in chunks of at most --max_micro_batch_size
        states, through the input form the phase uses.  With a penalty every chunk is a forward + backward pass whose
        gradient joins the minibatch's accumulator (n_passes of them); with --gkl_penalty=0 it is a forward alone.  The
        reference repeats the pass in every micro-batch at scale 1 / micro_batches; here it runs once at scale 1."""

        def __init__(self, runner, net, rows, old, stat_rows):
            self.r, self.net, self.rows, self.old, self.stat_rows = runner, net, rows, old, stat_rows
            self.S = int(rows.shape[0])
            self.chunk = min(args.max_micro_batch_size, self.S)
            self.penalty = float(args.gkl.penalty)
            self.n_passes = self.S // self.chunk if self.penalty != 0 else 0

        def run(self, k, after_backward, form, obs_all, obs_rows, row_bytes, B):
            net, r, nA = self.net, self.r, self.r.n_actions
            scale = self.penalty / (self.S * nA)  # F.kl_div's "batchmean" over the arrays flattened to [S * nA]
            for c, lo in enumerate(range(0, self.S, self.chunk)):
                idx, old = self.rows[lo:lo + self.chunk], self.old[lo:lo + self.chunk]
                out = self.stat_rows[k]
                if self.penalty == 0:
                    if form == "gather":
                        x = net._buf("gkl_obs", (self.chunk, *r.state_shape), r.all_obs.dtype)
                        r._call("ppo_gather_rows", _p(obs_rows), row_bytes, B, _p(idx), self.chunk, _p(x))
                        kl = net.policy_kl_rows(x, old)
                    else:
                        kl = net.policy_kl_rows(obs_rows if form == "fused" else obs_all, old, index=idx, obs_indexed=True)
                    r._call("ppo_colsum_f32", _p(kl), self.chunk, 1, 1, _p(out), 1 if c else 0)
                    continue
                if form == "fused":
                    net.policy_kl_minibatch(obs_rows, old, scale, index=idx, obs_indexed=True, stat_sums=out,
                                            stat_accumulate=bool(c))
                    after_backward()
                    continue
                if form == "in_conv":
                    kl = net.policy_kl_minibatch(obs_all, old, scale, index=idx, obs_indexed=True)
                else:
                    x = net._buf("gkl_obs", (self.chunk, *r.state_shape), r.all_obs.dtype)
                    r._call("ppo_gather_rows", _p(obs_rows), row_bytes, B, _p(idx), self.chunk, _p(x))
                    kl = net.policy_kl_minibatch(x, old, scale)
                after_backward()
                r._call("ppo_colsum_f32", _p(kl), self.chunk, 1, 1, _p(out), 1 if c else 0)

    def _run_epochs(self, label, optimizer, epochs, mini_batch_size, step_fn, n_stats, rows=None, obs=None,
                    extra_pass=None, stat_rows=None):
        """Permutation minibatching over the rollout (rl/rollout.py:2257-2407): per epoch one host shuffle
        (np.random, as the reference :2319-2320); per minibatch — in micro-batches of at most --max_micro_batch_size
        samples, gradients accumulated, each pass scaled by 1 / micro_batches (:2331-2374) — gather the observations,
        run step_fn(mb_obs, index, loss_scale) -> per-sample stats [n, n_stats], then step the optimiser; the stats
        are column-summed into one device row per minibatch.  `rows`: train on the first `rows` samples of the
        time-major batch only (the RND phase, rl/rollout.py:1830).  `obs`: a contiguous device tensor [S, *state_shape]
        of the rollout's dtype to train over instead of the rollout's observations (the distil batch drawn from the replay
        buffer); the per-sample data step_fn reads through the index then has S rows too.  `extra_pass`: passes that follow
        a minibatch's micro-batches (_GlobalKLPass): extra_pass.n_passes of them write net.grad and join the accumulator,
        so the optimiser sees the sum of all passes and the data-parallel early-bucket hook stays parked until it is
        complete.  `stat_rows`: the [epochs * minibatches, n_stats] device rows to use instead of the label's own."""
        if obs is None:
            B = self.N * self.A if rows is None else int(rows)
            obs_all = self.all_obs[:self.N].view(self.N * self.A, *self.state_shape)[:B]
        else:
            if rows is not None or obs.dtype != self.all_obs.dtype or tuple(obs.shape[1:]) != self.state_shape \
                    or not obs.is_contiguous():
                raise ValueError(f"obs must be a contiguous {self.all_obs.dtype} [S, {self.state_shape}] tensor (and rows unset)")
            B = int(obs.shape[0])
            obs_all = obs
        net = optimizer.net
        mb = parallel.local_minibatch(mini_batch_size)  # the flag is the GLOBAL minibatch
        if B % mb:
            raise ValueError(f"batch {B} is not a multiple of the per-rank minibatch {mb}")
        n_mb = B // mb
        micro, n_micro = self._micro_batches(mb)
        obs_rows = obs_all.view(B, -1)
        row_bytes = obs_rows.shape[1] * obs_rows.element_size()
        # MLP nets on the fused path read their rows of the whole batch through the permutation and column-sum the
        # statistics in their weight-gradient launch: no gather launch, no column-sum launch
        fused = bool(getattr(net, "mlp_fused", False)) and net.obs_norm is None and self.all_obs.dtype == torch.float32
        # ... and the IMPALA nets read uint8 image rows through the permutation in their first convolution
        in_conv = not fused and hasattr(net, "takes_obs_index") and net.takes_obs_index(self.all_obs)
        mb_obs = None if (fused or in_conv) else net._buf("mb_obs", (micro, *self.state_shape), self.all_obs.dtype)
        if stat_rows is None:
            stat_rows = net._buf(f"stat_rows_{label}", (epochs * n_mb, n_stats))
        elif tuple(stat_rows.shape) != (epochs * n_mb, n_stats) or not stat_rows.is_contiguous():
            raise ValueError(f"stat_rows must be a contiguous [{epochs * n_mb}, {n_stats}] tensor")
        form = "fused" if fused else ("in_conv" if in_conv else "gather")
        n_extra = extra_pass.n_passes if extra_pass is not None else 0
        norm_rows = net._buf(f"norm_rows_{label}", (epochs * n_mb,))
        if args.sns.enabled and epochs > 0 and sns.wants_noise_estimate(self, label):
            # noise of the first update only, before epoch 0's shuffle (rl/rollout.py:2290-2294)
            start_time = time.time()
            sns.estimate_noise_scale(self, B, self._noise_pass(net, step_fn, obs_all), net, label)
            self.log.watch_mean(f"sns_time_{label}", (time.time() - start_time) / args.sns.period, display_width=8,
                                display_name=f"t_s{label[:3]}")
        k = 0
        for _epoch in range(epochs):
            ordering = np.arange(B, dtype=np.int32)
            np.random.shuffle(ordering)
            order_dev = torch.from_numpy(ordering).to(self.device, non_blocking=True)
            for j in range(n_mb):
                acc = self._Accumulator(self, net, n_micro + n_extra)
                try:
                    for u in range(n_micro):
                        idx = order_dev[j * mb + u * micro:j * mb + (u + 1) * micro]
                        self._mb_pos = (k, u)  # for step functions that keep statistics rows of their own (SIDE)
                        if fused:
                            step_fn(obs_rows, idx, 1.0 / n_micro, stat_sums=stat_rows[k], stat_accumulate=bool(u),
                                    obs_indexed=True)
                            acc.after_backward()
                            continue
                        if in_conv:
                            stats = step_fn(obs_all, idx, 1.0 / n_micro, obs_indexed=True)
                        else:
                            self._call("ppo_gather_rows", _p(obs_rows), row_bytes, B, _p(idx), micro, _p(mb_obs))
                            stats = step_fn(mb_obs, idx, 1.0 / n_micro)
                        acc.after_backward()
                        self._call("ppo_colsum_f32", _p(stats), micro, n_stats, n_stats, _p(stat_rows[k]), 1 if u else 0)
                    if extra_pass is not None:
                        extra_pass.run(k, acc.after_backward, form, obs_all, obs_rows, row_bytes, B)
                    acc.finish()
                finally:
                    acc.restore_hook()
                    self._mb_pos = None
                self.optimizer_step(optimizer, label, norm_out=norm_rows[k:k + 1])  # the norm lands in its row: no copy launch
                k += 1
        self._phase_stats[label] = (stat_rows, norm_rows, mb)

    def train_policy(self):
        """PPO epochs over the rollout (rl/rollout.py:1853-1953); the single architecture trains the value
        head in the same pass (:1744-1746)."""
        if args.policy_opt.epochs == 0:
            return
        B = self.N * self.A
        net = self.policy_net
        self._normalize_advantages()
        returns = None if self.dual else self.returns
        net.zero_untouched_grads()
        epochs = args.policy_opt.epochs
        extra_pass = stat_rows = side_t = side_stat = None
        self._policy_extra = None
        if args.gkl.enabled or args.side.enabled:
            # one buffer for the phase's statistics - the eight PPO columns, then the global KL sums, then the SIDE penalty
            # sums, a row per minibatch each - so that fetch_stats reads them in one device->host copy
            n = epochs * (B // parallel.local_minibatch(args.policy_opt.mini_batch_size))
            flat = net._buf("stat_rows_policy_reg", (n * 10,))
            flat.zero_()
            stat_rows, gkl_stat, side_stat = flat[:8 * n].view(n, 8), flat[8 * n:9 * n].view(n, 1), flat[9 * n:].view(n, 1)
            self._policy_extra = {"flat": flat, "n": n, "gkl": bool(args.gkl.enabled), "side": bool(args.side.enabled),
                                  "S": int(args.gkl.samples)}
        if args.side.enabled:
            # the target policy of state-independent exploration (rl/rollout.py:1903-1918): redrawn every --side_period
            # rollouts, the reference's draw on the model's device (under data parallelism rank 0's, for all)
            if self.side_target_policy_logp is None or self.batch_counter % args.side.period == 0:
                bias = torch.normal(0, args.side.noise_std, size=[self.n_actions], dtype=torch.float32, device=self.device)
                if self.world > 1:
                    parallel.broadcast_(bias)
                self.side_target_policy_logp = torch.log_softmax(bias, dim=0).contiguous()
                if not args.disable_logging:
                    t = self.side_target_policy_logp.double()
                    self.log.watch_mean("side_target_entropy", float(-(t.exp() * t).sum()), display_name="ste")
            side_t = self.side_target_policy_logp
        if args.gkl.enabled:
            # the global states (rl/rollout.py:1922-1934): a draw without replacement from the rollout, at the reference's
            # place in the np.random stream (before epoch 0's shuffle), and the policy on them before the first update
            S = int(args.gkl.samples)
            rows_host = np.random.choice(B, S, replace=False)
            self._gkl_rows = torch.from_numpy(rows_host.astype(np.int32)).to(self.device)
            old = net._buf("gkl_old_log_policy", (S, self.n_actions))
            obs_rows = self.all_obs[:self.N].view(B, -1)
            chunk = min(args.max_micro_batch_size, S)
            x = net._buf("gkl_obs", (chunk, *self.state_shape), self.all_obs.dtype)
            for lo in range(0, S, chunk):
                self._call("ppo_gather_rows", _p(obs_rows), obs_rows.shape[1] * obs_rows.element_size(), B,
                           _p(self._gkl_rows[lo:lo + chunk]), chunk, _p(x))
                old[lo:lo + chunk].copy_(net.forward(x, exclude_value=True)["log_policy"])
            extra_pass = self._GlobalKLPass(self, net, self._gkl_rows, old, gkl_stat)
        if self.action_dist == "discrete":
            def step(mb_obs, idx, loss_scale, **kw):
                pen = None
                if side_t is not None and self._mb_pos is not None:
                    pen = net._buf("side_penalty", (int(idx.shape[0]), 1))
                stats = net.ppo_minibatch(mb_obs, self.actions, self.log_pac, self.log_policy, self.norm_advantage,
                                          returns, eps_clip=self.ppo_epsilon, ent_coef=self.current_entropy_bonus,
                                          vf_coef=args.ppo_vf_coef, loss_scale=loss_scale, index=idx,
                                          side_target_logp=side_t, side_penalty=pen, **kw)
                if pen is not None:
                    k, u = self._mb_pos
                    self._call("ppo_colsum_f32", _p(pen), pen.shape[0], 1, 1, _p(side_stat[k]), 1 if u else 0)
                return stats
        else:
            actions, log_pac = self.actions.view(B, self.n_actions), self.log_pac.view(B, self.n_actions)

            def step(mb_obs, idx, loss_scale, **kw):
                return net.gaussian_minibatch(mb_obs, actions, log_pac, self.norm_advantage, returns,
                                              eps_clip=self.ppo_epsilon, vf_coef=args.ppo_vf_coef, loss_scale=loss_scale,
                                              index=idx, **kw)
        self._run_epochs("policy", self.policy_optimizer, epochs, args.policy_opt.mini_batch_size, step, 8,
                         extra_pass=extra_pass, stat_rows=stat_rows)

    def train_value(self):
        """Value phase of the dual architecture (rl/rollout.py:1956-2004): value_net regresses the value
        targets, and the TVF heads their truncated-return targets."""
        if args.value_opt.epochs == 0:
            return
        B = self.N * self.A
        net = self.value_net
        use_ext = self.tvf is None or args.tvf.include_ext
        returns = self.returns.view(B, self.VH) if use_ext else None
        tvf_returns = self.tvf.tvf_returns[:, :, :, -1].reshape(B, self.K) if self.tvf is not None else None
        weights = self._tvf_value_weights_dev if self.tvf is not None else None
        net.zero_untouched_grads()

        keep = 1.0 - args.tvf.horizon_dropout if self.tvf is not None else 1.0
        seed = self._device_seed * 1000003 + 7919 * (self.rank + 1)

        def step(mb_obs, idx, loss_scale, **kw):
            off = self.tvf.next_dropout_offset(idx.shape[0] * self.K) if keep < 1.0 else 0
            return net.value_minibatch(mb_obs, returns=returns, tvf_returns=tvf_returns, tvf_weights=weights,
                                       vf_coef=args.ppo_vf_coef, tvf_coef=args.tvf.coef, loss_scale=loss_scale, index=idx,
                                       tvf_keep_prob=keep, dropout_seed=seed, dropout_offset=off, **kw)

        if args.sns.enabled and self.tvf is not None and sns.wants_noise_estimate(self, "value_heads") \
                and args.sns.max_heads > 0:
            # per-horizon noise estimates (rl/rollout.py:1981-1990): the TVF loss alone on heads 0..head
            def make_step(head):
                subset = self._tvf_subset_weights(self._required_tvf_heads(-head))

                def head_step(mb_obs, idx, loss_scale, **kw):
                    off = self.tvf.next_dropout_offset(idx.shape[0] * self.K) if keep < 1.0 else 0
                    return net.value_minibatch(mb_obs, returns=None, tvf_returns=tvf_returns, tvf_weights=subset,
                                               vf_coef=args.ppo_vf_coef, tvf_coef=args.tvf.coef, loss_scale=loss_scale,
                                               index=idx, tvf_keep_prob=keep, dropout_seed=seed, dropout_offset=off, **kw)
                return self._noise_pass(net, head_step, self.all_obs[:self.N].view(B, *self.state_shape))
            sns.log_accumulated_gradient_norms(self, make_step, net)
            if args.sns.fake_noise:
                sns.log_fake_accumulated_gradient_norms(self, net.n_parameters())
        self._run_epochs("value", self.value_optimizer, args.value_opt.epochs, args.value_opt.mini_batch_size, step, 4)

    def wants_distil_update(self, location=None):
        """rl/rollout.py:2211-2218."""
        return (self.dual and args.distil_opt.epochs > 0 and self.step >= args.distil.delay * 1e6
                and self.batch_counter % args.distil.period == args.distil.period - 1
                and (location is None or location == args.distil.order))

    def _distil_old_policy_key(self):
        """Which recorded policy the distil constraint compares against (rl/rollout.py:1397-1412): the raw policy - the
        means of a gaussian policy, the logits under --distil_loss=mse_logit - or the log-policy."""
        return "raw_policy" if self.action_dist == "gaussian" or args.distil.loss == "mse_logit" else "log_policy"

    def _distil_head_weights(self, use_tvf):
        """-> (weights, head_subset) of the distil loss: the duplicate-head weights of all TVF heads, or with
        0 < --distil_max_heads < K those of even_sample_down's heads and 0 on the others (rl/rollout.py:1336-1362), a
        device vector cached per subset.  Unlike tvf.subset_head_weights these carry no scale: the kernel takes the
        sqrt(|S|) mean from its n_active."""
        if not use_tvf:
            return None, None
        if not 0 < args.distil.max_heads < self.K:
            return self._tvf_weights_dev, None
        from .value_quality import even_sample_down
        subset = [int(k) for k in even_sample_down(range(self.K), int(args.distil.max_heads))]
        key = ("distil", tuple(subset))
        dev = self._tvf_subset_weight_cache.get(key)
        if dev is None:
            w = np.zeros(self.K, np.float32)
            w[subset] = self.tvf_weights[subset]
            dev = self._tvf_subset_weight_cache[key] = torch.as_tensor(w, device=self.device)
        return dev, subset

    def _distil_step(self, prev_state, targets, old_policy, use_tvf, pred_actions=None, **kw):
        """One distil minibatch under the --distil_* flags: what train_distil, train_distil_minibatch and the noise-scale
        passes all run."""
        weights, subset = self._distil_head_weights(use_tvf)
        return self.policy_net.distil_minibatch(
            prev_state, targets, old_policy, beta=args.distil.beta, use_tvf=use_tvf, weights=weights,
            gaussian=self.action_dist == "gaussian", policy_loss=args.distil.loss, value_loss=args.distil.value_loss,
            delta=args.distil.delta, l1_scale=args.distil.l1_scale, pred_actions=pred_actions, head_subset=subset, **kw)

    def get_distil_batch(self, samples_wanted=None):
        """Targets and the policy to stay close to, from the rollout (rl/rollout.py:2050-2112, the
        replay-free path): value_net's estimates recorded during the rollout, and either the rollout's
        policy (`before_policy`) or the just-updated policy re-evaluated over the batch (`after_policy`)."""
        N, A = self.N, self.A
        B = N * A
        if self.replay_buffer is not None:
            wanted = samples_wanted if samples_wanted is not None else (args.distil.batch_size if args.distil.batch_size > 0 else B)
            return self._get_replay_distil_batch(int(wanted))
        if samples_wanted not in (None, B) or (0 < args.distil.batch_size != B):
            raise NotImplementedError("without a replay buffer (--replay_mode, --replay_size) distillation trains on the "
                                      "rollout: distil_batch_size = rollout")
        use_tvf = self.tvf is not None and not args.distil.force_ext
        batch = {"use_tvf": use_tvf}
        if use_tvf:
            assert args.distil.target == "value", "Only value targets supported for TVF distil"
            batch["distil_targets"] = self.tvf.tvf_untrimmed_value[:N, :, :, 0].reshape(B, self.K)
        elif args.distil.target == "value":
            batch["distil_targets"] = self.ext_value[:N].reshape(B)  # (a view with one head, a copy of column 0 with two)
        else:
            # "return" / "advantage" (:2077-2094): GAE(--distil_adv_lambda) of the rollout's rewards under value_net's
            # recorded estimates, one scan; the "return" target is its ret output, f32(adv) + V.  Either is predicted by
            # the advantage head's entry for the action taken (:1364-1368), so the batch carries the actions.
            if self.action_dist != "discrete":
                raise ValueError(f"--distil_target={args.distil.target} needs discrete actions: the advantage head is "
                                 "indexed by the action taken")
            net = self.policy_net
            if self.VH > 1:  # the scan wants unit-stride rows
                value = net._buf("distil_gae_value", (N + 1, A))
                value.copy_(self.ext_value)
            else:
                value = self.value.view(N + 1, A)
            targets = net._buf("distil_gae_targets", (N, A))
            as_return = args.distil.target == "return"
            self._call("ppo_gae_scan_f32", _p(self.ext_rewards), _p(value), _p(value[N]), _p(self.terminals),
                       _lib.PPO_TERM_U8, None if as_return else _p(targets), _p(targets) if as_return else None, N, A, A,
                       float(args.tvf.gamma), float(args.distil.adv_lambda), float(args.distil.adv_lambda),
                       _lib.PPO_SCAN_AUTO)
            batch["distil_targets"] = targets.view(B)
            batch["distil_actions"] = self.actions.view(B)
        key = self._distil_old_policy_key()
        if args.distil.order == "before_policy":
            old = getattr(self, key).view(B, self.n_actions)
        else:
            net = self.policy_net
            old = net._buf("distil_old_policy", (B, self.n_actions))
            obs = self.all_obs[:N].view(B, *self.state_shape)
            chunk = max(args.max_micro_batch_size, 1)
            for i in range(0, B, chunk):
                out = net.forward(obs[i:i + chunk], exclude_value=True)
                old[i:i + chunk].copy_(out[key])
        batch["old_policy"] = old
        return batch

    def get_replay_sample(self, samples_wanted: int, with_aux=False):
        """rl/rollout.py:2016-2048 on the device: `samples_wanted` rows of the replay buffer - of buffer + current rollout
        with --replay_mixing, of the rollout alone while the buffer is empty - drawn as the reference draws them
        (np.random.choice without replacement, only when fewer rows are wanted than there are), gathered by ONE launch
        into a [S, *state_shape] device buffer.  Returns (obs, aux or None)."""
        buf, net = self.replay_buffer, self.policy_net
        n = self.N * self.A
        n_a = buf.current_size
        mix = bool(args.replay.mixing) or n_a == 0
        total = n_a + (n if mix else 0)
        if samples_wanted < total:
            sample = np.random.choice(total, samples_wanted, replace=False)
        else:
            sample = np.arange(total)
        S = len(sample)
        sample_dev = torch.from_numpy(sample.astype(np.int32)).to(self.device, non_blocking=True)
        obs = net._buf("replay_sample_obs", (S, *self.state_shape), self.all_obs.dtype)
        aux = net._buf("replay_sample_aux", (S, buf.N_AUX)) if with_aux else None
        extra = self.all_obs[:self.N].view(n, *self.state_shape) if mix else None
        extra_aux = self._rollout_aux(net._buf("replay_mix_aux", (n, buf.N_AUX)), time_and_step=False) if mix and with_aux else None
        buf.gather(sample_dev, obs, out_aux=aux, extra=extra, extra_aux=extra_aux)
        return obs, aux

    def _get_replay_distil_batch(self, samples_wanted: int):
        """The reference's slow path (rl/rollout.py:2114-2138): a sample of the replay buffer, its targets regenerated
        from value_net and the policy to stay close to from policy_net as they stand now, in chunks of
        --max_micro_batch_size.  Everything stays on the device."""
        assert args.distil.target == "value", "Replay distil required value targets."
        use_tvf = self.tvf is not None and not args.distil.force_ext
        obs, _aux = self.get_replay_sample(samples_wanted)
        S = int(obs.shape[0])
        pol, val = self.policy_net, self.value_net
        key = self._distil_old_policy_key()
        old = pol._buf("replay_distil_old_policy", (S, self.n_actions))
        targets = pol._buf("replay_distil_targets", (S, self.K) if use_tvf else (S,))
        chunk = max(args.max_micro_batch_size, 1)
        for i in range(0, S, chunk):
            out = val.forward(obs[i:i + chunk], exclude_policy=True)
            targets[i:i + chunk].copy_(out["tvf_value"][:, :, 0] if use_tvf else out["value"][:, 0])
            old[i:i + chunk].copy_(pol.forward(obs[i:i + chunk], exclude_value=True)[key])
        return {"use_tvf": use_tvf, "prev_state": obs, "distil_targets": targets, "old_policy": old}

    def train_distil(self):
        """Distillation phase (rl/rollout.py:2140-2164): policy_net's value (or TVF) heads learn value_net's
        estimates under a KL constraint that keeps the policy where it is."""
        if args.distil_opt.epochs == 0:
            return
        batch = self.get_distil_batch()
        net = self.policy_net
        net.zero_untouched_grads()

        def step(mb_obs, idx, loss_scale, **kw):
            return self._distil_step(mb_obs, batch["distil_targets"], batch["old_policy"], batch["use_tvf"],
                                     pred_actions=batch.get("distil_actions"), loss_scale=loss_scale, index=idx, **kw)
        opt = self.policy_optimizer if args.distil.use_policy_opt else self.distil_optimizer
        # (with a replay buffer the batch is the sample drawn from it, otherwise the rollout where it lies)
        self._run_epochs("distil", Optimizer(net, args.distil_opt, opt.state, kind=opt.kind), args.distil_opt.epochs,
                         args.distil_opt.mini_batch_size, step, 4, obs=batch.get("prev_state"))

    def train_rnd(self):
        """The predictor's phase (rl/rollout.py:1824-1841): --rnd_opt_epochs epochs of minibatches over the first
        round(B * --rnd_experience_proportion) samples of the time-major batch, read through the minibatch index.

        Data parallel: B is the rank's share of the batch and the flag the GLOBAL minibatch, so the ranks take the steps
        of a one-rank run together, each a collective (optimizer_step); that they all take the same number was checked
        when the reducer was set up (_check_rnd_steps_agree), and that the rows divide into whole minibatches is
        checked before the first of them (_run_epochs).  Feature statistics and loss_rnd are the rank's own, as the other
        phases' statistics are."""
        if args.rnd_opt.epochs == 0:
            return
        rows, mb, _steps = self._rnd_steps()
        if mb < 2:
            raise ValueError("--rnd_opt_mini_batch_size must be at least 2 (the feature variance over one row is NaN)")
        self._rnd_stats.zero_()

        def step(obs, idx, loss_scale, **kw):
            return self.rnd.train_minibatch(obs, idx, loss_scale, stats=self._rnd_stats).view(-1, 1)
        self._run_epochs("rnd", self.rnd_optimizer, args.rnd_opt.epochs, args.rnd_opt.mini_batch_size, step, 1, rows=rows)

    def train(self):
        """rl/rollout.py:2220-2255: [distil] -> policy -> (dual) value -> [distil] -> [rnd]."""
        self._phase_stats = {}
        self.model.eval()  # rl/rollout.py:2228
        if self.wants_distil_update("before_policy"):
            self.train_distil()
        self.train_policy()
        if self.dual:
            self.train_value()
            if self.wants_distil_update("after_policy"):
                self.train_distil()
        if self.rnd is not None:
            self.train_rnd()  # :2252-2253
        self.batch_counter += 1

    # ---- the reference's dict-based minibatch API (rl/rollout.py:1331, 1513, 1610, 2257), for callers that
    # drive the phases themselves; `data` holds minibatch-sized device tensors
    def train_policy_minibatch(self, data, loss_scale=1.0):
        """rl/rollout.py:1610-1771.  With --side_enabled the target is self.side_target_policy_logp; with --gkl_enabled
        `data` also holds "*global_states" [S, *state_shape] and "*global_log_policy" [S, n_actions], and the result
        "global_kl" (a host tensor, as the reference's)."""
        net = self.policy_net
        returns = data.get("returns") if not self.dual else None
        side_pen = None
        if self.action_dist == "discrete":
            side_t = None
            if args.side.enabled:
                side_t = self.side_target_policy_logp
                if side_t is None:
                    raise ValueError("--side_enabled: no target policy yet (train_policy draws side_target_policy_logp)")
                side_pen = net._buf("side_penalty", (int(data["prev_state"].shape[0]), 1))
            stats = net.ppo_minibatch(data["prev_state"], data["actions"].to(torch.int32), data["log_pac"],
                                      data.get("log_policy"), data["advantages"], returns, eps_clip=self.ppo_epsilon,
                                      ent_coef=self.current_entropy_bonus, vf_coef=args.ppo_vf_coef,
                                      loss_scale=loss_scale, side_target_logp=side_t, side_penalty=side_pen)
        else:
            stats = net.gaussian_minibatch(data["prev_state"], data["actions"], data["log_pac"], data["advantages"],
                                           returns, eps_clip=self.ppo_epsilon, vf_coef=args.ppo_vf_coef,
                                           loss_scale=loss_scale)
        s = stats.double().mean(0).cpu().numpy()
        result = {"loss": float(-s[6] * loss_scale), "kl_approx": float(s[4]), "kl_true": float(s[5]), "clip_frac": float(s[3])}
        if side_pen is not None and not args.disable_logging:
            t = self.side_target_policy_logp.double()
            self.log.watch_mean("side_kl_penalty", float(side_pen.double().mean()), display_name="skl")
            self.log.watch_mean("side_target_entropy", float(-(t.exp() * t).sum()), display_name="ste")
        if args.gkl.enabled:
            states = self.model.prep_for_model(data["*global_states"])
            old = data["*global_log_policy"].to(self.device, torch.float32).contiguous()
            S = int(states.shape[0])
            div = S * self.n_actions  # F.kl_div's "batchmean" over the arrays flattened to [S * n_actions] (:1728-1731)
            if args.gkl.penalty != 0:
                # the second forward + backward of the minibatch: its gradient is added to the PPO pass's
                ppo_grad = net._buf("grad_ppo_pass", tuple(net.grad.shape))
                ppo_grad.copy_(net.grad)
                kl = net.policy_kl_minibatch(states, old, args.gkl.penalty / div, loss_scale=loss_scale)
                self._call("ppo_accumulate_f32", _p(net.grad), _p(ppo_grad), net.grad.numel())
                net._presummed = 0  # the sums of g^2 the KL pass left are not the summed gradient's
            else:
                kl = net.policy_kl_rows(states, old)
            global_kl = kl.double().sum().cpu() / div
            if args.gkl.penalty != 0:
                gkl_loss = float(global_kl) * args.gkl.penalty
                result["loss"] += gkl_loss * loss_scale  # -gain, and gkl_loss comes off every sample's gain (:1735)
                if not args.disable_logging:
                    self.log.watch_mean("*loss_gkl", gkl_loss, history_length=64 * args.policy_opt.epochs,
                                        display_name="ls_gkl", display_width=8)
            result["global_kl"] = global_kl.to(torch.float32)
        return result

    @staticmethod
    def _required_tvf_heads(single_value_head):
        """rl/rollout.py:1518-1524: None -> all heads, h >= 0 -> [h], h < 0 -> heads 0..-h."""
        if single_value_head is None:
            return None
        return [int(single_value_head)] if single_value_head >= 0 else list(range(-int(single_value_head) + 1))

    def _tvf_subset_weights(self, heads):
        """The device weight vector that trains the TVF heads `heads` alone (tvf.subset_head_weights), cached per set."""
        from .tvf import subset_head_weights
        key = tuple(heads)
        dev = self._tvf_subset_weight_cache.get(key)
        if dev is None:
            dev = torch.as_tensor(subset_head_weights(self.tvf_weights, heads), device=self.device)
            self._tvf_subset_weight_cache[key] = dev
        return dev

    def train_value_minibatch(self, data, loss_scale=1.0, single_value_head=None):
        """rl/rollout.py:1513-1567.  single_value_head: train the TVF head h alone (h >= 0) or heads 0..-h (h < 0)."""
        heads = self._required_tvf_heads(single_value_head)
        weights = None
        if "tvf_returns" in data:
            weights = self._tvf_value_weights_dev if heads is None else self._tvf_subset_weights(heads)
        stats = self.value_net.value_minibatch(data["prev_state"], returns=data.get("returns"),
                                               tvf_returns=data.get("tvf_returns"), tvf_weights=weights,
                                               vf_coef=args.ppo_vf_coef, tvf_coef=args.tvf.coef, loss_scale=loss_scale)
        total = stats[:, 2].double() * loss_scale
        return {"loss": float(total.mean()), "loss_std": float(total.std())}

    def train_rnd_minibatch(self, data, loss_scale: float = 1.0, **kwargs):
        """rl/rollout.py:1804-1821: the predictor's gradients for one minibatch of observations."""
        x = self.model.prep_for_model(data["prev_state"])
        stats = torch.zeros(_lib.PPO_RND_STATS, dtype=torch.float32, device=self.device)
        err = self.rnd.train_minibatch(x, None, loss_scale, stats=stats)
        loss = float(err.double().mean()) * loss_scale
        _sum, feat_mean, feat_var, feat_max, _n = stats.cpu().tolist()
        if not args.disable_logging:
            self.log.watch_mean("loss_rnd", loss / loss_scale)
            self.log.watch_mean("*feat_mean", feat_mean)
            self.log.watch_mean("*feat_var", feat_var)
            self.log.watch_mean("*feat_max", feat_max, display_precision=1)
        return {"loss": loss}

    def train_distil_minibatch(self, data, loss_scale=1.0, **kwargs):
        """rl/rollout.py:1331-1449.  `data`: prev_state, distil_targets, old_log_policy or (gaussian policies,
        --distil_loss=mse_logit) old_raw_policy, and with a --distil_target other than value distil_actions."""
        use_tvf = self.tvf is not None and not args.distil.force_ext
        actions = None
        if not use_tvf and args.distil.target != "value":
            actions = data["distil_actions"].to(torch.int32).contiguous()
        stats = self._distil_step(data["prev_state"], data["distil_targets"], data["old_" + self._distil_old_policy_key()],
                                  use_tvf, pred_actions=actions, loss_scale=loss_scale)
        total = stats[:, 2].double() * loss_scale
        return {"loss": float(total.mean()), "loss_std": float(total.std())}

    def train_batch(self, batch_data, mini_batch_func, mini_batch_size, optimizer, label, epoch=None, hooks=None,
                    thinning=1.0, force_micro_batch_size=None, delta_threshold=None):
        """One epoch of permutation minibatches through `mini_batch_func(data, loss_scale=...)`, the reference's
        dict-based API (rl/rollout.py:2257-2407): minibatches are split into micro-batches of `force_micro_batch_size`
        (default min(--max_micro_batch_size, minibatch)) samples whose gradients accumulate under
        loss_scale = 1 / micro_batches; `thinning` keeps that fraction of every micro-batch; `hooks`
        ("after_micro_batch"(context), "after_mini_batch"(context) -> truthy stops before the optimiser step) are
        called as the reference calls them; entries whose name starts with '*' are passed through whole.  Returns
        {'mini_batches', 'outputs'[, 'did_break']}."""
        if delta_threshold is not None and delta_threshold > 0:
            raise Exception("Not supported")
        assert "prev_state" in batch_data, "Batches must contain 'prev_state' field of dims (B, *state_shape)"
        B = len(batch_data["prev_state"])
        for k_, v in batch_data.items():
            if not k_.startswith("*"):
                assert len(v) == B, f"Batch input must all match in entry count. Expecting {B} but found {len(v)} on {k_}"
        mb = parallel.local_minibatch(mini_batch_size)
        assert B % mb == 0
        n_mb = B // mb
        micro, n_micro = self._micro_batches(mb, force_micro_batch_size)
        ordering = np.arange(B)
        np.random.shuffle(ordering)
        data = {k_: (v.to(self.device) if isinstance(v, torch.Tensor) else torch.as_tensor(v).to(self.device))
                for k_, v in batch_data.items()}
        net = optimizer.net
        outputs, context, counter = [], {}, 0
        for j in range(n_mb):
            optimizer.zero_grad()
            acc = self._Accumulator(self, net, n_micro)
            try:
                for u in range(n_micro):
                    sample = ordering[counter * micro:(counter + 1) * micro]
                    counter += 1
                    if thinning < 1.0:
                        sample = sample[:int(micro * thinning)]
                    idx = torch.from_numpy(sample).to(self.device)
                    micro_context = {"epoch": epoch, "mini_batch": j, "micro_batch": u, "is_first": j == 0,
                                     "is_last": j == n_mb - 1}
                    micro_data = {"context": micro_context}
                    for k_, v in data.items():
                        micro_data[k_] = v if k_.startswith("*") else v[idx].contiguous()
                    outputs.append(mini_batch_func(micro_data, loss_scale=1 / n_micro))
                    acc.after_backward()
                    if hooks is not None and "after_micro_batch" in hooks:
                        hooks["after_micro_batch"](micro_context)
                acc.finish()
            finally:
                acc.restore_hook()
            context = {"mini_batches": j + 1, "outputs": outputs}
            if hooks is not None and "after_mini_batch" in hooks:
                stop = bool(hooks["after_mini_batch"](context))
                if self.world > 1:
                    # a stop decided from rank-local data (a KL threshold, say) must be everyone's: otherwise one rank
                    # leaves while the others issue the late-bucket all-reduce and the collective sequences diverge
                    flag = torch.tensor([1.0 if stop else 0.0], device=self.device)
                    torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
                    stop = bool(flag.item() > 0)
                if stop:
                    red = self._reducers.get(id(net))
                    if red is not None:
                        red.abandon()  # the early bucket already left during the backward pass: join it before leaving
                    context["did_break"] = True
                    break
            self.optimizer_step(optimizer, label)
        return context

    def fetch_stats(self):
        """ONE device->host copy per phase and iteration with everything the reference logs per minibatch
        (rl/rollout.py:1685-1691, 1759-1769, 1317, 1427-1446, 1563)."""
        out = {}
        if "policy" in self._phase_stats:
            stat_rows, norm_rows, mb = self._phase_stats["policy"]
            extra = self._policy_extra
            if extra is None:
                s = stat_rows.cpu().numpy().astype(np.float64) / mb
            else:  # the PPO columns, the global KL sums and the SIDE penalty sums in the one copy (train_policy)
                n = extra["n"]
                flat = extra["flat"].cpu().numpy().astype(np.float64)
                s = flat[:8 * n].reshape(n, 8) / mb
            out.update({"loss_pg": s[:, 0].mean(), "entropy": s[:, 1].mean(), "loss_v_ext": s[:, 2].mean(),
                        "clip_frac": s[:, 3].mean(), "kl_approx": s[:, 4].mean(), "kl_true": s[:, 5].mean(),
                        "loss_policy": s[:, 6].mean(), "grad_policy": float(norm_rows.mean().item()),
                        "adv_mean": float(self._mean_std[0].item()), "adv_std": float(self._mean_std[1].item())})
            if extra is not None and extra["gkl"]:
                # global_kl per minibatch: the sum of the rows' KL over S * n_actions (F.kl_div's "batchmean" on the
                # flattened arrays, rl/rollout.py:1728-1731); with a penalty, gkl_loss comes off every sample's gain (:1735)
                global_kl = flat[8 * n:9 * n] / (extra["S"] * self.n_actions)
                out["global_kl"] = global_kl.mean()
                if args.gkl.penalty != 0:
                    out["*loss_gkl"] = (args.gkl.penalty * global_kl).mean()
                    out["loss_policy"] -= out["*loss_gkl"]
            if extra is not None and extra["side"]:
                out["side_kl_penalty"] = (flat[9 * n:] / mb).mean()
        if "value" in self._phase_stats:
            stat_rows, norm_rows, mb = self._phase_stats["value"]
            s = stat_rows.cpu().numpy().astype(np.float64) / mb
            out.update({"loss_v_ext": s[:, 0].mean(), "loss_tvf": s[:, 1].mean(), "loss_value": s[:, 2].mean(),
                        "grad_value": float(norm_rows.mean().item())})
        if "distil" in self._phase_stats:
            stat_rows, norm_rows, mb = self._phase_stats["distil"]
            s = stat_rows.cpu().numpy().astype(np.float64) / mb
            out.update({"loss_distil_value": s[:, 0].mean(), "loss_distil_policy": s[:, 1].mean(),
                        "loss_distil": s[:, 2].mean(), "distil_mse": s[:, 3].mean(),
                        "grad_distil": float(norm_rows.mean().item())})
        if "rnd" in self._phase_stats:  # rl/rollout.py:1814-1818; one row of sums for the whole phase (csrc/rnd.hip)
            stat_rows, norm_rows, mb = self._phase_stats["rnd"]
            _sum, feat_mean, feat_var, feat_max, calls = self._rnd_stats.cpu().numpy().astype(np.float64)
            out.update({"loss_rnd": (stat_rows.cpu().numpy().astype(np.float64) / mb).mean(),
                        "*feat_mean": feat_mean / calls, "*feat_var": feat_var / calls, "*feat_max": feat_max,
                        "grad_rnd": float(norm_rows.mean().item())})
        if not args.disable_logging:
            named = {"*loss_gkl": dict(history_length=64 * args.policy_opt.epochs, display_name="ls_gkl", display_width=8),
                     "side_kl_penalty": dict(display_name="skl")}  # rl/rollout.py:1736, 1678
            for k_, v in out.items():
                self.log.watch_mean(k_, v, **named.get(k_, {}))
        return out

    # ------------------------------------------------------------------ checkpoints (rl/rollout.py:394-517)
    def get_checkpoints(self, path):
        """[(epoch_M, filename)] newest first (rl/rollout.py:460-470)."""
        from .ppo import get_checkpoints
        return get_checkpoints(path)

    def save_checkpoint(self, filename, step, disable_log=False, disable_replay=False, disable_env_state=False,
                        disable_optimizer=False):
        """Model under the reference's state_dict names, optimiser states, counters, env / wrapper state;
        gzip container when --checkpoint_compression (file name + '.gz').  Returns the path written.

        Data parallel: replicas hold the same model, so rank 0 writes it; what differs per rank — its env columns'
        state, its reward normaliser, its host RNG (minibatch permutations) — is gathered to rank 0 and stored as one
        entry per rank.  Every rank must call this (it is a collective when world > 1)."""
        from . import checkpoint
        local = {"np_random": np.random.get_state(), "ep_count": self.ep_count, "time": self.time.copy(),
                 "episode_score": self.episode_score.copy(), "episode_len": self.episode_len.copy()}
        if self.tvf is not None:
            local["episode_length_buffer"] = [int(x) for x in self.tvf.episode_length_buffer]  # rl/rollout.py:399
            local["tvf_dropout_calls"] = int(self.tvf._dropout_calls)  # a resumed run must not replay dropout masks
        if not disable_env_state and self.vec_env is not None:
            local["env_state"] = checkpoint.save_env_state(self.vec_env)
        per_rank = [local]
        if self.world > 1:
            per_rank = [None] * self.world if self.rank == 0 else None
            torch.distributed.gather_object(checkpoint.to_plain(local), per_rank, dst=0)
        if self.rank != 0:
            return None
        # the reference's top-level keys (rl/rollout.py:396-407; tests/golden/checkpoint_golden.json is their tree) ...
        data = {"step": step, "ep_count": self.ep_count, "batch_counter": self.batch_counter,
                "episode_length_buffer": [int(x) for x in self.tvf.episode_length_buffer] if self.tvf is not None else [1000],
                "model_state_dict": dict(self.model.state_dict()), "reward_scale": float(self.reward_scale) if self.vec_env is not None else 1.0,
                "episode_score": self.episode_score.copy(),
                # ... and this package's own: the data-parallel layout and the device generators' position
                "world": self.world, "sample_calls": self._sample_calls, "device_seed": self._device_seed,
                "rank_state": per_rank}
        if not disable_optimizer:  # torch.optim.Adam.state_dict() layout each; the reference writes the value
            data["policy_optimizer_state_dict"] = self.policy_optimizer.state_dict()  # optimiser's even when it is
            data["value_optimizer_state_dict"] = self.value_optimizer.state_dict()    # the policy optimiser (single)
            if self.distil_optimizer is not None:
                data["distil_optimizer_state_dict"] = self.distil_optimizer.state_dict()
            if self.rnd_optimizer is not None:
                data["rnd_optimizer_state_dict"] = self.rnd_optimizer.state_dict()  # rl/rollout.py:416-417
        if self.model.obs_norm is not None:
            data["obs_rms"] = self.model.obs_norm.state_dict()  # rl/rollout.py:438-439
        if self.intrinsic:
            # rl/rollout.py:434-436; the reference pickles the RunningMeanStd object, here its three float64 moments
            data["ems_norm"] = self.ems_norm.copy()
            rms = self.intrinsic_returns_rms
            data["intrinsic_returns_rms"] = {"mean": np.float64(rms.mean), "var": np.float64(rms.var),
                                             "count": float(rms.count)}
        if args.sns.enabled:
            data["noise_stats"] = sns.noise_stats_to_plain(self.noise_stats)  # rl/rollout.py:428-429, as plain data
        if self.hash is not None:
            data.update(self.hash.state_dict())  # rl/rollout.py:409-411: hash_global_counts, hash_recent_counts
        if self.replay_buffer is not None and not disable_replay:
            data["replay_buffer"] = self.replay_buffer.save_state(force_copy=False)  # rl/rollout.py:431-432
        return checkpoint.save(data, filename, bool(args.checkpoint_compression))

    def load_checkpoint(self, checkpoint_path):
        """Restores model, optimisers, counters and this rank's env / RNG state; returns the env step
        (rl/rollout.py:472-517).  Every rank reads the file itself."""
        from . import checkpoint
        cp = checkpoint.load(checkpoint_path)
        self.model.load_state_dict(cp["model_state_dict"])
        for key, opt in (("policy_optimizer_state_dict", self.policy_optimizer),
                         ("value_optimizer_state_dict", self.value_optimizer if self.dual else None),
                         ("distil_optimizer_state_dict", self.distil_optimizer),
                         ("rnd_optimizer_state_dict", self.rnd_optimizer)):
            if opt is not None and key in cp:
                opt.load_state_dict(cp[key])
        if self.model.obs_norm is not None:
            self.model.obs_norm.load_state_dict(cp["obs_rms"])  # rl/rollout.py:511-513
        if self.intrinsic:  # rl/rollout.py:507-509
            self.ems_norm = np.asarray(cp["ems_norm"], np.float64).copy()
            if self.ems_norm.shape != (self.A * self.world,):  # global state: one entry per env of the whole run
                raise ValueError(f"ems_norm: {self.ems_norm.size} envs in the checkpoint, "
                                 f"{self.A * self.world} in this run ({self.world} rank(s) of {self.A})")
            rms = cp["intrinsic_returns_rms"]
            self.intrinsic_returns_rms.restore_state((np.float64(rms["mean"]), np.float64(rms["var"]), rms["count"]))
        if args.sns.enabled:  # rl/rollout.py:495
            self.noise_stats = sns.noise_stats_from_plain(cp.get("noise_stats"), self)
        if self.hash is not None:  # rl/rollout.py:500-502
            self.hash.load_state_dict(cp)
        if self.replay_buffer is not None:  # rl/rollout.py:504-505
            if "replay_buffer" in cp:
                self.replay_buffer.load_state(cp["replay_buffer"])
            else:
                self.log.warn("the checkpoint holds no replay buffer (written with disable_replay): the buffer starts empty")
        self.step = cp["step"]
        self.ep_count = cp.get("ep_count", 0)
        self.batch_counter = cp.get("batch_counter", 0)
        self._sample_calls = cp.get("sample_calls", 0)
        self._device_seed = int(cp.get("device_seed", self._device_seed))
        ranks = cp.get("rank_state") or []
        if len(ranks) == self.world:
            mine = ranks[self.rank]
            if mine.get("np_random") is not None:
                np.random.set_state(mine["np_random"])
            self.ep_count = mine.get("ep_count", self.ep_count)
            if mine.get("time") is not None:
                self.time = np.asarray(mine["time"], np.int32).copy()
            for key in ("episode_score", "episode_len"):
                if mine.get(key) is not None:
                    getattr(self, key)[:] = mine[key]
            if self.tvf is not None and mine.get("episode_length_buffer") is not None:
                self.tvf.episode_length_buffer.clear()
                self.tvf.episode_length_buffer.extend(mine["episode_length_buffer"])
            if self.tvf is not None:
                self.tvf._dropout_calls = int(mine.get("tvf_dropout_calls", self.tvf._dropout_calls))
            if mine.get("env_state") and self.vec_env is not None:
                checkpoint.restore_env_state(self.vec_env, mine["env_state"])
                if hasattr(self.vec_env, "parts"):
                    self.obs = np.concatenate([p.obs for p in self.vec_env.parts])
                elif hasattr(self.vec_env, "obs"):
                    self.obs = self.vec_env.obs
        elif ranks:
            self.log.warn(f"checkpoint was written by {len(ranks)} rank(s), this run has {self.world}: model and "
                          "optimiser restored, env / RNG state not")
        return self.step
