"""Run configuration — host mirror of the reference's rl/config.py for the flags the PPO hot path reads.

Same flag names, defaults and access pattern as the reference (`rl.config.args`, a global
singleton read at call time; grouped flags appear as `--<prefix>_<name>` and are read as
`args.<prefix>.<name>`, rl/config.py:38-185).  Defaults cite rl/config.py line numbers.
Flags of out-of-scope subsystems are accepted and ignored with a
note, so existing launch lines keep working.  The `hash` group is registered only on a launch line that enables hashing
(`--hash_enabled[=True]`), the `replay` group only on one that names a `--replay_mode` other than `off`, the `sns` group
only on one that enables noise-scale estimation (`--sns_enabled[=True]`), the `gkl` and `side` groups only on one that
enables them (`--gkl_enabled[=True]`, `--side_enabled[=True]`): every other line parses exactly as it did before state
hashing, the replay buffer, the simple noise scale, the global KL penalty and state-independent exploration were built.
"""
import argparse
import os
import sys


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


class _Group:
    """A prefixed flag group: fields declared as (name, type, default, help)."""
    FIELDS = ()

    def __init__(self, prefix):
        self._prefix = prefix
        for name, _t, default, _h in self.FIELDS:
            setattr(self, name, default)

    def add(self, parser):
        for name, t, default, h in self.FIELDS:
            kw = dict(type=str2bool, nargs="?", const=True) if t is bool else dict(type=t)
            parser.add_argument(f"--{self._prefix}_{name}", default=default, help=h, **kw)

    def update(self, ns):
        for name, *_ in self.FIELDS:
            setattr(self, name, getattr(ns, f"{self._prefix}_{name}"))

    def flatten(self):
        return {f"{self._prefix}_{name}": getattr(self, name) for name, *_ in self.FIELDS}


class OptimizerConfig(_Group):  # rl/config.py:249-311
    EPOCH_DEFAULTS = {"policy_opt": 2, "value_opt": 1, "distil_opt": 2, "rnd_opt": 1}  # :261-267

    def __init__(self, prefix):
        super().__init__(prefix)
        self.epochs = self.EPOCH_DEFAULTS.get(prefix, 0)

    def add(self, parser):
        super().add(parser)
        parser.set_defaults(**{f"{self._prefix}_epochs": self.EPOCH_DEFAULTS.get(self._prefix, 0)})

    FIELDS = (
        ("optimizer", str, "adam", "[adam|sgd]"),
        ("epochs", int, 2, "training epochs per batch (default: policy 2, value 1, distil 2)"),
        ("mini_batch_size", int, 256, "examples per optimisation step (global, across ranks)"),
        ("lr", float, 2.5e-4, "learning rate"),
        ("lr_anneal", bool, False, "anneal learning rate linearly to 0"),
        ("adam_epsilon", float, 1e-5, "Adam epsilon"),
        ("adam_beta1", float, 0.9, "Adam beta1"),
        ("adam_beta2", float, 0.999, "Adam beta2"),
    )


class ModelConfig(_Group):  # rl/config.py:458-476
    FIELDS = (
        ("architecture", str, "dual", "[dual|single]  (north-star PPO = single)"),
        ("encoder", str, "nature", "[nature|impala|rtg|mlp]"),
        ("encoder_args", str, None, "dict of encoder arguments (impala: channels, n_block, down_sample [pool|stride|none], "
                                    "batch_norm [True: bn0 / bn1 in every residual block, batch statistics during the "
                                    "rollout, running statistics everywhere else; one GPU]; "
                                    "nature: base_channels; rtg: accepted and ignored)"),
        ("hidden_units", int, 256, "encoder output features"),
        ("head_scale", float, 0.1, "orthogonal-init gain of the heads"),
        ("head_bias", bool, True, "bias on the output heads"),
    )


class EnvConfig(_Group):  # rl/config.py:495-603
    FIELDS = (
        ("name", str, "Pong", "environment name"),
        ("type", str, "atari", "[atari|procgen|mujoco|classic|synthetic]"),
        ("embed_time", bool, True, "append a time channel"),
        ("embed_action", bool, True, "embed last action"),
        ("reward_normalization", str, "rms", "[off|rms]"),
        ("reward_normalization_clipping", float, 10.0, "clip rewards after normalisation, negative to disable (:509)"),
        ("max_repeated_actions", int, 100, "penalise repeating one action more than this many times (:513)"),
        ("repeated_action_penalty", float, 0.0, "the penalty (:514)"),
        ("warmup_period", int, 250, "random warm-up steps to desynchronise envs"),
        ("timeout", str, "auto", "episode step limit in agent steps: auto (atari 27000, procgen 1000, mujoco 1001, else off) or a number, 0 = off (:503)"),
        ("repeat_action_probability", float, 0.0, "ALE sticky actions (:504)"),
        ("noop_duration", int, 30, "maximum number of no-ops after a reset, 0 = none (:505)"),
        ("per_step_termination_probability", float, 0.0, "probability that a step ends the episode (:506)"),
        ("reward_clipping", str, "off", "[off|<R>|sqrt] (:507)"),
        ("deferred_rewards", int, 0, "pay all rewards at this step (-1: at the end), 0 = off (:510)"),
        ("full_action_space", bool, False, "ALE full action set (:517)"),
        ("resolution", str, "nature", "[full|nature|half|muzero] (:520)"),
        ("color_mode", str, "default", "[default|bw|rgb|yuv|hsv]; default = bw for atari, yuv for procgen (:521)"),
        ("frame_stack", int, -1, "frames stacked, -1 = 4 for atari else 1 (:522)"),
        ("frame_skip", int, -1, "simulator frames per agent step, -1 = 4 for atari else 1 (:523)"),
        ("embed_state", bool, False, "draw a compressed state history onto the frame (:526)"),
        ("atari_terminal_on_loss_of_life", bool, False, "(:529)"),
        ("atari_rom_check", bool, True, "(:530; the ROM table is not part of this build: accepted and ignored)"),
        ("procgen_difficulty", str, "hard", "[hard|easy] (:533)"),
        ("zero_obs", bool, False, "blank observations (the reference's --debug_zero_obs)"),
        ("synthetic_done_prob", float, 0.01, "synthetic env: per-step termination probability"),
        ("synthetic_threads", int, 16, "synthetic env: host threads generating observations (a GPU's share of the host cores)"),
        ("synthetic_actions", int, 0, "synthetic env: size of the action set (0 = 6, the Pong-shaped default)"),
        ("synthetic_shape", str, None, "synthetic env: observation shape 'C,H,W' (default 4,84,84; procgen-shaped: 3,64,64)"),
        ("pipeline_parts", int, 2, "split the envs into this many groups so host stepping overlaps the GPU policy step"),
        ("pipeline_leaves", int, 1, "step and upload each group in this many pieces, a piece's upload running while the next is stepped (measured: 0.494 / 0.558 / 0.792 ms per env step for 1 / 2 / 4 - a thread-pool dispatch per piece costs more than the overlap returns)"),
    )


class DistilConfig(_Group):  # rl/config.py:329-354
    LOSSES = ("mse_logit", "mse_policy", "kl_policy")
    VALUE_LOSSES = ("mse", "clipped_mse", "l1", "huber")
    TARGETS = ("return", "value", "advantage")
    FIELDS = (
        ("order", str, "after_policy", "[after_policy|before_policy]"),
        ("beta", float, 1.0, "weight of the policy constraint"),
        ("target", str, "value", "[return|value|advantage]  (return / advantage: GAE over the rollout against the "
                                 "advantage head's entry for the action taken; discrete actions, no TVF, no replay)"),
        ("batch_size", int, -1, "distil batch size, negative = the rollout"),
        ("adv_lambda", float, 0.6, "GAE lambda of the return / advantage distil targets"),
        ("period", int, 1, "distil every this many batches"),
        ("loss", str, "kl_policy", "[mse_logit|mse_policy|kl_policy]  (discrete policies; gaussian ones ignore it)"),
        ("max_heads", int, -1, "max TVF heads to distil, -1 = all"),
        ("force_ext", bool, False, "distil the ext value head even when TVF is on"),
        ("value_loss", str, "mse", "[mse|clipped_mse|l1|huber]"),
        ("delta", float, 0.1, "delta of the huber value loss (0 = abs)"),
        ("l1_scale", float, 1 / 30, "scale of the l1 value loss"),
        ("delay", float, 0, "millions of steps before distillation starts"),
        ("use_policy_opt", bool, False, "share the policy optimiser's moments"),
    )


class TVFConfig(_Group):  # rl/config.py:209-246
    FIELDS = (
        ("enabled", bool, False, "truncated value functions"),
        ("value_heads", int, 128, "number of horizon heads"),
        ("max_horizon", int, 30000, "longest horizon"),
        ("gamma", float, None, "TVF discount (None = gamma)"),
        ("coef", float, 1.0, "TVF loss coefficient"),
        ("head_spacing", str, "geometric", "[geometric|linear]"),
        ("return_mode", str, "advanced", "[standard|advanced|full|...]"),
        ("return_distribution", str, "exponential", "[fixed|exponential|uniform|hyperbolic|quadratic]"),
        ("return_samples", int, 8, "n-step samples per horizon"),
        ("return_use_log_interpolation", bool, False, "interpolate in log-horizon space"),
        ("include_ext", bool, False, "also train the ext value head in the value phase"),
        ("trimming", str, "off", "[off|timelimit|est_term] reduce horizons past the episode end to the time left (:217)"),
        ("trimming_mode", str, "average", "[interpolate|average|substitute|random] (:218)"),
        ("trim_advantages", str, "trimmed", "[trimmed|untrimmed|average] value estimate used for advantages (:219)"),
        ("trim_clip", float, -1.0, "if >= 0 clips how much trimming can change a value estimate (:220)"),
        ("eta_minh", int, 128, "estimated-termination trimming: minimum horizon (:221)"),
        ("eta_buffer", int, 32, "estimated-termination trimming: steps added to the percentile (:222)"),
        ("eta_percentile", float, 90.0, "estimated-termination trimming: percentile of episode lengths (:223)"),
        ("head_weighting", str, "off", "[off|h_weighted]"),
        ("horizon_dropout", float, 0.0, "fraction of horizons excluded per sample in the TVF loss (:224)"),
        ("feature_window", int, -1, "limits each head to a window of this many features (:233)"),
        ("feature_sparsity", float, 0.0, "zeros out this proportion of features for each head (:234)"),
    )


class RNDConfig(_Group):  # rl/config.py:397-410
    FIELDS = (
        ("enabled", bool, False, "Random Network Distillation: intrinsic rewards from a predictor's error"),
        ("experience_proportion", float, 0.25, "fraction of the rollout the predictor trains on"),
    )


class HashConfig(_Group):  # rl/config.py:412-429
    FIELDS = (
        ("enabled", bool, False, "state hashing: counts of visited (hashed) states"),
        ("bits", int, 16, "bits of the hash; the two count tables hold 2^bits float64 each"),
        ("bonus", float, 0.0, "intrinsic reward bonus for novel hashed states"),
        ("method", str, "linear", "[linear]  (conv is not built)"),
        ("input", str, "raw", "[raw|raw_centered|normed|normed_offset]"),
        ("bonus_method", str, "hyperbolic", "[hyperbolic|quadratic|binary]"),
        ("rescale", int, 1, "downscale factor of the hashed frame (only 1 is built)"),
        ("quantize", float, 1, "quantisation step of the hashed bytes (integers only)"),
        ("bias", float, 0.0, "range of the hasher's uniform bias"),
        ("decay", float, 0.99, "per-step decay of the recent counts"),
    )


def _flag_enabled_on(argv, flag):
    """Whether a launch line holds the boolean `flag` with a true value: `flag`, `flag=<true>` or `flag <true>`."""
    for i, a in enumerate(argv):
        value = None
        if a == flag:
            nxt = argv[i + 1] if i + 1 < len(argv) else None
            value = "true" if nxt is None or nxt.startswith("--") else nxt
        elif a.startswith(flag + "="):
            value = a.split("=", 1)[1]
        if value is not None:
            try:
                if str2bool(value):
                    return True
            except argparse.ArgumentTypeError:
                return True  # the parser reports the bad value
    return False


def hashing_enabled_on(argv):
    """Whether a launch line enables state hashing somewhere: a `--hash_enabled`, `--hash_enabled=<true>` or
    `--hash_enabled <true>` on it.  (A later `--hash_enabled=False` on such a line is then the parser's to resolve: the
    last one wins, and verify() refuses a bonus that is left without hashing.)"""
    return _flag_enabled_on(argv, "--hash_enabled")


class SimpleNoiseScaleConfig(_Group):  # rl/config.py:188-206
    LABELS = ("policy", "distil", "value", "value_heads")
    FIELDS = (
        ("enabled", bool, False, "simple noise scale estimates (critical batch size) of the update phases"),
        # the reference's default is this list, which its own ast.literal_eval cannot take; a string is parsed
        ("labels", str, ["policy", "distil", "value", "value_heads"], "value|value_heads|distil|policy"),
        ("period", int, 3, "generate estimates every n updates"),
        ("max_heads", int, 7, "limit to this number of heads when doing per head noise estimate"),
        ("b_big", int, 2048, "rows of the large batch"),
        ("b_small", int, 128, "rows of the small batch"),
        ("fake_noise", bool, False, "also log estimates of synthetic gradients whose noise follows the horizon"),
        ("smoothing_mode", str, "ema", "[ema|avg]"),
        # the reference types these int and so cannot parse its own defaults (0.2e6) from a command line
        ("smoothing_horizon_avg", float, 1e6, "how big to make the averaging window (env steps)"),
        ("smoothing_horizon_s", float, 0.2e6, "how much to smooth s"),
        ("smoothing_horizon_g2", float, 1.0e6, "how much to smooth g2"),
        ("smoothing_horizon_policy", float, 5e6, "how much to smooth g2 for policy (normally much higher)"),
    )

    def __init__(self, prefix):
        super().__init__(prefix)
        self.labels = list(self.labels)  # a list of this instance's own, not the one FIELDS holds

    def update(self, ns):
        super().update(ns)
        if not isinstance(self.labels, str):
            self.labels = list(self.labels)

    def label_list(self):
        """The labels as a list: the default list as it is, a string through ast.literal_eval (rl/sns.py:294)."""
        import ast
        labels = self.labels
        if isinstance(labels, str):
            try:
                labels = ast.literal_eval(labels)
            except (ValueError, SyntaxError):
                raise ValueError(f"--sns_labels={self.labels}: a Python list of labels, such as \"['policy', 'value']\", "
                                 "or one quoted label") from None
        if isinstance(labels, str):
            labels = [labels]
        if not isinstance(labels, (list, tuple)):
            raise ValueError(f"--sns_labels={self.labels}: a list of labels")
        return [str(x).lower() for x in labels]


def sns_enabled_on(argv):
    """Whether a launch line enables noise-scale estimation (`--sns_enabled[=True]`): only then are the `sns` flags
    registered."""
    return _flag_enabled_on(argv, "--sns_enabled")


class ReplayConfig(_Group):  # rl/config.py:357-375
    MODES = ("off", "overwrite", "sequential", "uniform")
    FIELDS = (
        ("mode", str, "off", "[overwrite|sequential|uniform|off]"),
        ("size", int, 0, "size of the replay buffer (rows, resident in HBM), 0 = off"),
        ("mixing", bool, False, "distil on a sample of buffer + current rollout"),
        ("thinning", float, 1.0, "adds this fraction of the experience to the replay buffer"),
    )

    @property
    def enabled(self):
        return self.size > 0 and self.mode != "off"


def replay_mode_on(argv):
    """Whether a launch line names a replay mode other than `off` (`--replay_mode=<m>` or `--replay_mode <m>`): only then
    are the `replay` flags registered.  On any other line they are unknown flags as before - and in the reference, too,
    such a line (`--replay_size=5` alone, say) enables nothing."""
    for i, a in enumerate(argv):
        value = None
        if a == "--replay_mode":
            value = argv[i + 1] if i + 1 < len(argv) else ""
        elif a.startswith("--replay_mode="):
            value = a.split("=", 1)[1]
        if value is not None and value != "off":
            return True
    return False


class GlobalKLConfig(_Group):  # rl/config.py:378-394
    FIELDS = (
        ("enabled", bool, False, "estimate KL(new || old) over a fixed random sample of the rollout's states"),
        ("threshold", float, -1, "read nowhere (as in the reference)"),
        ("penalty", float, 0.01, "penalty on the global KL in the policy loss, 0 = the statistic only"),
        ("source", str, "rollout", "[rollout]"),
        ("samples", int, 1024, "number of states in the global sample"),
    )


class SIDEConfig(_Group):  # rl/config.py:479-492
    FIELDS = (
        ("enabled", bool, False, "state-independent exploration: a KL penalty towards a random target policy"),
        ("noise_std", float, 0.1, "standard deviation of the target policy's logits"),
        ("period", int, 10, "redraw the target every n rollouts"),
    )


def gkl_enabled_on(argv):
    """Whether a launch line enables the global KL penalty (`--gkl_enabled[=True]`): only then are the `gkl` flags
    registered."""
    return _flag_enabled_on(argv, "--gkl_enabled")


def side_enabled_on(argv):
    """Whether a launch line enables state-independent exploration (`--side_enabled[=True]`): only then are the `side`
    flags registered."""
    return _flag_enabled_on(argv, "--side_enabled")


class IRConfig(_Group):  # rl/config.py:445-455
    FIELDS = (
        ("propagation", bool, True, "intrinsic returns propagate through the end of an episode"),
        ("scale", float, 0.3, "intrinsic advantage scale"),
        ("center", bool, False, "per-batch centring of intrinsic rewards"),
        ("normalize", bool, True, "normalise intrinsic rewards to unit-variance returns"),
    )


class Config:
    def __init__(self):
        self.policy_opt = OptimizerConfig("policy_opt")
        self.value_opt = OptimizerConfig("value_opt")
        self.distil_opt = OptimizerConfig("distil_opt")
        self.distil = DistilConfig("distil")
        self.model = ModelConfig("model")
        self.env = EnvConfig("env")
        self.tvf = TVFConfig("tvf")
        self.rnd_opt = OptimizerConfig("rnd_opt")
        self.rnd = RNDConfig("rnd")
        self.ir = IRConfig("ir")
        self.hash = HashConfig("hash")  # not in _groups: registered per launch line (setup)
        self.replay = ReplayConfig("replay")  # likewise
        self.sns = SimpleNoiseScaleConfig("sns")  # likewise
        self.gkl = GlobalKLConfig("gkl")  # likewise
        self.side = SIDEConfig("side")  # likewise
        # (a flag belongs to the group with the longest matching prefix: rnd_opt_lr is rnd_opt's, rnd_enabled is rnd's)
        self._groups = (self.policy_opt, self.value_opt, self.distil_opt, self.distil, self.model, self.env, self.tvf,
                        self.rnd_opt, self.rnd, self.ir)
        # top-level defaults (rl/config.py line numbers)
        self.agents = 256              # :791
        self.n_steps = 256             # :790
        self.gamma = 0.999             # :769
        self.gamma_int = 0.99          # :770
        self.lambda_policy = 0.95      # :772
        self.lambda_value = 0.95       # :773
        self.ppo_epsilon = 0.2         # :789
        self.entropy_bonus = 0.01      # :785
        self.ppo_vf_coef = 0.5         # :784
        self.max_grad_norm = 20.0      # :775
        self.grad_clip_mode = "global_norm"  # :776
        self.advantage_epsilon = 1e-8  # :792
        self.advantage_clipping = None
        self.ppo_epsilon_anneal = False
        self.entropy_scaling = "off"           # [off|average|uniform]
        self.entropy_scaling_base_actions = 18
        self.entropy_anneal = False
        self.advantage_epsilon_anneal_factor = 0.0
        self.anneal_target_epoch = None
        self.max_micro_batch_size = 512  # :760
        self.device = "cpu"            # :731 (the reference default; this build requires a GPU)
        self.upload_batch = False      # :732
        self.observation_normalization = False  # :756
        self.observation_normalization_epsilon = 0.003  # :757
        self.freeze_observation_normalization = False  # :758
        self.observation_scaling = "scaled"     # :755
        self.seed = -1                 # :749
        self.epochs = 50.0             # millions of env steps
        self.limit_epochs = None
        self.benchmark_mode = False
        self.disable_logging = False   # :733
        self.disable_ev = False
        self.output_folder = "./"
        self.experiment_name = "Run"
        self.run_name = "run"
        self.restore = "auto"          # :720
        self.initial_model = None      # :728
        self.checkpoint_every = int(10e6)  # :752
        self.save_checkpoints = True   # :736
        self.save_initial_checkpoint = False  # :737
        self.save_early_checkpoint = False    # :738
        self.debug_print_freq = 60     # DebugConfig.print_freq
        self.checkpoint_compression = True  # :726
        self.workers = -1              # :722
        self.threads = 2               # :723
        self.precision = "medium"      # :764
        self.sync_envs = False
        self.override_reward_normalization_gamma = None  # :780
        self.log_folder = None
        self._ignored = []

    # ---- properties the reference derives (rl/config.py:885-901)
    RESOLUTIONS = {"full": (210, 160), "procgen": (64, 64), "nature": (84, 84), "muzero": (96, 96), "half": (105, 80)}

    @property
    def use_intrinsic_rewards(self):  # rl/config.py:881-883 (a bonus without --hash_enabled cannot be set: verify())
        return bool(self.rnd.enabled) or bool(self.hash.enabled and self.hash.bonus != 0)

    @property
    def batch_size(self):
        return self.n_steps * self.agents

    @property
    def reward_normalization_gamma(self):  # rl/config.py:875-880
        if self.override_reward_normalization_gamma is not None:
            return self.override_reward_normalization_gamma
        return self.tvf.gamma if self.tvf.enabled else self.gamma

    @property
    def tvf_return_n_step(self):
        return round(1 / (1 - self.lambda_value)) if self.lambda_value < 1 else self.n_steps

    def build_parser(self):
        p = argparse.ArgumentParser(description="MI355X-native PPO trainer (drop-in for dremovd/PPO train.py)")
        a = p.add_argument
        a("--agents", type=int, default=self.agents)
        a("--n_steps", type=int, default=self.n_steps)
        a("--gamma", type=float, default=self.gamma)
        a("--gamma_int", type=float, default=self.gamma_int, help="discount rate for intrinsic rewards")
        a("--lambda_policy", type=float, default=self.lambda_policy)
        a("--lambda_value", type=float, default=self.lambda_value)
        a("--ppo_epsilon", type=float, default=self.ppo_epsilon)
        a("--entropy_bonus", type=float, default=self.entropy_bonus)
        a("--ppo_vf_coef", type=float, default=self.ppo_vf_coef)
        a("--max_grad_norm", type=float, default=self.max_grad_norm)
        a("--grad_clip_mode", type=str, default=self.grad_clip_mode, help="[off|global_norm]")
        a("--advantage_epsilon", type=float, default=self.advantage_epsilon)
        a("--advantage_clipping", type=float, default=None)
        a("--ppo_epsilon_anneal", type=str2bool, nargs="?", const=True, default=False)
        a("--entropy_scaling", type=str, default="off", help="[off|average|uniform]")
        a("--entropy_scaling_base_actions", type=int, default=18)
        a("--entropy_anneal", type=str2bool, nargs="?", const=True, default=False)
        a("--advantage_epsilon_anneal_factor", type=float, default=0.0)
        a("--anneal_target_epoch", type=float, default=None)
        a("--max_micro_batch_size", type=int, default=self.max_micro_batch_size)
        a("--device", type=str, default=self.device)
        a("--upload_batch", type=str2bool, nargs="?", const=True, default=self.upload_batch)
        a("--observation_normalization", type=str2bool, nargs="?", const=True, default=False)
        a("--observation_normalization_epsilon", type=float, default=0.003)
        a("--freeze_observation_normalization", type=str2bool, nargs="?", const=True, default=False)
        a("--observation_scaling", type=str, default="scaled",
          help="[scaled|centered|unit] (rl/models.py:846-855) what a uint8 observation becomes: x/255, x/255 - 0.5 or "
               "(x/255 - 0.5) * 6, applied in the load of the kernels that read it; float32 observations are used as they are")
        a("--seed", type=int, default=self.seed)
        a("--epochs", type=float, default=self.epochs, help="millions of env steps to train for")
        a("--limit_epochs", type=float, default=None)
        a("--benchmark_mode", type=str2bool, nargs="?", const=True, default=False)
        a("--disable_logging", type=str2bool, nargs="?", const=True, default=False)
        a("--disable_ev", type=str2bool, nargs="?", const=True, default=False)
        a("--output_folder", type=str, default=self.output_folder)
        a("--experiment_name", type=str, default=self.experiment_name)
        a("--run_name", type=str, default=self.run_name)
        a("--restore", type=str, default=self.restore, help="[never|auto|always]")
        a("--initial_model", type=str, default=None, help="checkpoint (in log_folder) to start from at step 0")
        a("--log_folder", type=str, default=None)
        a("--checkpoint_every", type=int, default=self.checkpoint_every)
        a("--save_checkpoints", type=str2bool, nargs="?", const=True, default=True)
        a("--save_initial_checkpoint", type=str2bool, nargs="?", const=True, default=False)
        a("--save_early_checkpoint", type=str2bool, nargs="?", const=True, default=False)
        a("--debug_print_freq", type=int, default=self.debug_print_freq)
        a("--checkpoint_compression", type=str2bool, nargs="?", const=True, default=True)
        a("--workers", type=int, default=self.workers)
        a("--threads", type=int, default=self.threads)
        a("--precision", type=str, default=self.precision,
          help="[low|medium|high] (train.py:166-178): high = exact float32 everywhere; low / medium also allow the "
               "split-bf16 launches (3 bf16 MFMAs per product, ~16-bit products) where they exist - the IMPALA encoder's "
               "16- and 32-channel convolutions and the nature encoder's convolution passes listed in models.NATURE_SPLIT; "
               "rtg, mlp, batch-norm nets and the RND networks stay exact float32")
        # accepted as before; the value follows --rnd_enabled, as the reference's property of that name (rl/config.py:881)
        a("--use_intrinsic_rewards", type=str2bool, nargs="?", const=True, default=False)
        a("--sync_envs", type=str2bool, nargs="?", const=True, default=False)
        a("--override_reward_normalization_gamma", type=float, default=None)
        for g in self._groups:
            g.add(p)
        return p

    def setup(self, argv=None):
        """Parse argv (default sys.argv[1:]) like rl.config.args.setup() (rl/config.py:709-801)."""
        argv = list(sys.argv[1:] if argv is None else argv)
        parser = self.build_parser()
        # the hash flags exist only on a line that enables hashing; on any other line they are unknown flags as before
        # (ignored with a note, in command-line order) and args.hash holds the defaults
        self.hash = HashConfig("hash")
        self.replay = ReplayConfig("replay")  # the same for the replay flags and a --replay_mode other than off
        self.sns = SimpleNoiseScaleConfig("sns")  # and for the sns flags and --sns_enabled
        self.gkl = GlobalKLConfig("gkl")  # and for the gkl flags and --gkl_enabled
        self.side = SIDEConfig("side")  # and for the side flags and --side_enabled
        optional = ((self.hash,) if hashing_enabled_on(argv) else ()) + ((self.replay,) if replay_mode_on(argv) else ()) \
            + ((self.sns,) if sns_enabled_on(argv) else ()) + ((self.gkl,) if gkl_enabled_on(argv) else ()) \
            + ((self.side,) if side_enabled_on(argv) else ())
        groups = self._groups + optional
        for g in optional:
            g.add(parser)
        ns, unknown = parser.parse_known_args(argv)
        for k, v in vars(ns).items():
            if any(k.startswith(g._prefix + "_") for g in groups) or k == "use_intrinsic_rewards":
                continue
            setattr(self, k, v)
        for g in groups:
            g.update(ns)
        self._ignored = [u for u in unknown if u.startswith("--")]
        self.verify()
        return self

    def verify(self):
        if self.model.architecture not in ("single", "dual"):
            raise ValueError(f"Invalid architecture {self.model.architecture}, use [dual|single]")
        if self.grad_clip_mode not in ("off", "global_norm"):
            raise ValueError("Invalid clip_mode.")
        if self.tvf.gamma is None:
            self.tvf.gamma = self.gamma
        # make_optimizer's refusal (rl/rollout.py:126-141), at set-up rather than at the first step, and OptimizerConfig.auto
        # (rl/config.py:308-311).  The rollout is what one phase sees over all ranks - the quantity the global minibatch
        # divides: --agents is per rank, so n_steps x agents x world size
        rollout = self.batch_size * int(os.environ.get("WORLD_SIZE", "1"))
        for opt in (self.policy_opt, self.value_opt, self.distil_opt, self.rnd_opt):
            if opt.optimizer not in ("adam", "sgd"):
                raise ValueError(f"Invalid Optimizer {opt.optimizer}")
            if opt.adam_beta1 < 0:
                if opt.epochs == 0 or opt.mini_batch_size <= 0:
                    raise ValueError(f"--{opt._prefix}_adam_beta1={opt.adam_beta1} (auto) needs --{opt._prefix}_epochs > 0 "
                                     f"and a positive minibatch: beta1 = 1 - 1 / ((rollout / mini_batch_size) * epochs)")
                opt.adam_beta1 = 1 - (1 / ((rollout / opt.mini_batch_size) * opt.epochs))
                print(f"Set {opt._prefix} beta1 to {opt.adam_beta1}")
        # the reference raises these two in the middle of an update (rl/rollout.py:1414, 2096; :1383 for the value loss)
        if self.distil.loss not in DistilConfig.LOSSES:
            raise ValueError(f"Invalid distil_loss {self.distil.loss}")
        if self.distil.target not in DistilConfig.TARGETS:
            raise ValueError(f"Invalid distil target {self.distil.target}")
        if self.distil.value_loss not in DistilConfig.VALUE_LOSSES:
            raise ValueError(f"Invalid loss distil loss {self.distil.value_loss}")
        if self.observation_scaling not in ("scaled", "centered", "unit"):  # the model's own refusal (rl/models.py:855)
            raise ValueError(f"Invalid observation_scaling mode {self.observation_scaling}")
        if self.distil.delta < 0:
            raise ValueError(f"--distil_delta={self.distil.delta} must be >= 0")
        if self.rnd.enabled:
            assert self.observation_normalization, "RND requires observation normalization"  # rl/config.py:408-410
        if self.hash.bonus != 0:
            assert self.hash.enabled, "use_hashing must be enabled."  # rl/config.py:871-872
        if self.hash.enabled:
            if self.hash.method == "conv":
                raise NotImplementedError("--hash_method=conv is not built: its 1x1 squeeze layer is drawn from the global "
                                          "RNG, not the seeded generator, so its tables do not survive a restart")
            if self.hash.method != "linear":
                raise ValueError(f"Invalid hashing method '{self.hash.method}' (linear)")
            if self.hash.rescale != 1:
                raise NotImplementedError("--hash_rescale != 1 is not built (it needs OpenCV's INTER_AREA rounding)")
            if self.hash.quantize != int(self.hash.quantize) or not 0 <= self.hash.quantize <= 255:
                raise NotImplementedError("--hash_quantize must be an integer in [0, 255]: the hashed bytes are uint8")
            if self.hash.input not in ("raw", "raw_centered", "normed", "normed_offset"):
                raise ValueError(f"Invalid hash_input {self.hash.input}")
            if self.hash.bonus_method not in ("hyperbolic", "quadratic", "binary"):
                raise ValueError(f"Invalid hash_bonus_method {self.hash.bonus_method}")
            if not 1 <= self.hash.bits <= 24:
                raise ValueError(f"--hash_bits={self.hash.bits}: 1 to 24 bits (two float64 tables of 2^bits entries)")
        if self.replay.mode not in ReplayConfig.MODES:
            raise ValueError(f"Invalid replay mode '{self.replay.mode}' (overwrite, sequential, uniform, off)")
        if self.replay.mode != "off":
            if self.replay.size <= 0:
                raise ValueError(f"--replay_mode={self.replay.mode} needs a --replay_size > 0")
            if not 0 < self.replay.thinning <= 1:
                raise ValueError(f"--replay_thinning={self.replay.thinning}: a fraction in (0, 1]")
        if self.sns.enabled:
            if self.sns.smoothing_mode not in ("ema", "avg"):
                raise ValueError(f"Invalid smoothing mode {self.sns.smoothing_mode}.")
            bad = [x for x in self.sns.label_list() if x not in SimpleNoiseScaleConfig.LABELS]
            if bad:
                raise ValueError(f"--sns_labels: {bad} not in policy | value | distil | value_heads")
            if self.sns.period < 1 or self.sns.b_small < 1:
                raise ValueError("--sns_period and --sns_b_small must be at least 1")
            # b_small must divide b_big (rl/sns.py:146, 198; asserted there in the middle of an update): the rollout for
            # `policy`, --sns_b_big for every other label
            labels = self.sns.label_list()
            if "policy" in labels and self.batch_size % self.sns.b_small:
                raise ValueError(f"--sns_b_small={self.sns.b_small} must divide the rollout, n_steps x agents = "
                                 f"{self.batch_size}, which is the policy estimate's b_big")
            if set(labels) - {"policy"} and self.sns.b_big % self.sns.b_small:
                raise ValueError(f"--sns_b_small={self.sns.b_small} must divide --sns_b_big={self.sns.b_big}")
        if self.gkl.enabled:
            if self.gkl.source != "rollout":  # asserted in the middle of an update by the reference (rl/rollout.py:1924)
                raise ValueError(f"--gkl_source={self.gkl.source}: only rollout source supported at the moment")
            if self.gkl.samples < 1:
                raise ValueError(f"--gkl_samples={self.gkl.samples} must be at least 1")
        if self.side.enabled and self.side.period < 1:
            raise ValueError(f"--side_period={self.side.period} must be at least 1")
        # EnvConfig.auto (rl/config.py:563-600)
        if self.env.frame_skip in (None, -1):
            self.env.frame_skip = 4 if self.env.type == "atari" else 1
        if self.env.frame_stack in (None, -1):
            self.env.frame_stack = 4 if self.env.type == "atari" else 1
        if self.env.color_mode not in ("default", "bw", "rgb", "yuv", "hsv"):
            raise ValueError(f"Invalid color mode {self.env.color_mode}")
        if self.env.color_mode == "default":
            self.env.color_mode = {"atari": "bw", "procgen": "yuv"}.get(self.env.type, "bw")
        if self.env.timeout == "auto":
            if self.env.type == "atari":
                self.env.timeout = 27000
            elif self.env.type == "procgen":
                self.env.timeout = {"bigfish": 6000, "bossfight": 8000, "plunder": 4000}.get(self.env.name, 1000)
            elif self.env.type == "mujoco":
                self.env.timeout = (50 if self.env.name.lower() == "reacher" else 1000) + 1
            else:
                self.env.timeout = 0  # unlimited
        else:
            self.env.timeout = int(self.env.timeout)
        if self.env.type in ("procgen", "mujoco") and (self.env.frame_stack != 1 or self.env.frame_skip != 1):
            raise ValueError(f"Frame stacking / skipping not supported on {self.env.type} yet")  # (:555-560)
        if self.restore in ("True", "true", True):  # rl/config.py:810-812
            self.restore = "always"
        if self.restore not in ("always", "never", "auto"):
            raise ValueError(f"Expecting {self.restore} to be one of ['always', 'never', 'auto']")

    def flatten(self):
        d = {k: v for k, v in vars(self).items() if not k.startswith("_") and not isinstance(v, _Group)}
        d["use_intrinsic_rewards"] = self.use_intrinsic_rewards
        for g in self._groups + ((self.hash,) if self.hash.enabled else ()) + ((self.replay,) if self.replay.enabled else ()) \
                + ((self.sns,) if self.sns.enabled else ()) + ((self.gkl,) if self.gkl.enabled else ()) \
                + ((self.side,) if self.side.enabled else ()):
            d.update(g.flatten())
        return d


args = Config()
