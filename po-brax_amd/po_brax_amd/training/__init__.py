"""Learner-side pieces with a native path (po_brax/training in the reference): the networks and
their actors, the observation normaliser, the critic pass and GAE, and the PPO loss with its head
gradient (``ppo_loss``) under the smallest learner that closes the loop (``PPOLearner``)."""
from . import gae, networks, normalization, ppo  # noqa: F401
from .gae import ValueFunction, compute_gae  # noqa: F401
from .networks import FeedForwardModel, NormalTanhPolicy, make_model, make_models  # noqa: F401
from .normalization import ObservationNormalizer, create_observation_normalizer  # noqa: F401
from .ppo import PPOLearner, ppo_loss  # noqa: F401
