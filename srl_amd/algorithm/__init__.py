"""Algorithm plugins of the hot path; importing this package registers them under the reference's names:
trainers ``mappo`` / ``mappo-hip`` / ``mappg``, policies ``actor-critic`` / ``actor-critic-separate`` / ``actor-critic-shared`` (+ the continuous-action names), the
per-game presets of ``game_policies`` (football, atari-vision, overcooked), the multi-agent ``smac_rnn``, IMPALA's ``dmlab``,
trajectory post-processor ``gae``; the Q-learning family: trainer ``q-learning``, policy ``atari-dqn``, trajectory post-processor
``n-step-return``."""
from srl_amd.algorithm import actor_critic, dmlab_policy, gae, game_policies, mappg, mappo, smac_policy  # noqa: F401
from srl_amd.algorithm import dqn_policy, nstep, qlearning  # noqa: F401
