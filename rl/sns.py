from ppo_amd.sns import *  # noqa: F401,F403
from ppo_amd import sns as _impl
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith('__')})
