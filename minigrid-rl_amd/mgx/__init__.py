"""mgx -- MI355X-native vectorised MiniGrid (PlaygroundEnv) engine.

Host-side mirror of the reference's env/rollout interface (Idokorro/MiniGrid-RL
src/custom_env.py, src/environment.py, src/ppo.py) over libmgx.so (HIP/gfx950).
"""
from ._lib import MgxError, mission_text  # noqa: F401
from .describe import LLMDescriptionWrapper  # noqa: F401
from .engine import MgxEngine, gae, gae_dones, random_actions  # noqa: F401
from .evaluation import (EvalCallback, GraphEvaluator, StopTrainingOnRewardThreshold, evaluate_policy,  # noqa: F401
                         evaluate_test_protocol, summarize_missions)
from .expert import ExpertActor, expert_reference  # noqa: F401
from .imitation import BCTrainer, Demonstrations, bc_loss, collect_demonstrations  # noqa: F401
from .moe import FusedMoEActor, MoEPolicy, route_by_task, route_from_gate  # noqa: F401
from .vec_env import MgxVecEnv  # noqa: F401

__all__ = ["BCTrainer", "Demonstrations", "EvalCallback", "ExpertActor", "FusedMoEActor", "GraphEvaluator", "LLMDescriptionWrapper", "MgxEngine", "MgxError", "MgxVecEnv", "MoEPolicy", "StopTrainingOnRewardThreshold", "bc_loss", "collect_demonstrations", "evaluate_policy", "evaluate_test_protocol", "expert_reference", "gae", "gae_dones", "mission_text", "random_actions", "route_by_task", "route_from_gate", "summarize_missions"]
