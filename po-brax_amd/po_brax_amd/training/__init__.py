"""Learner-side pieces with a native path (po_brax/training in the reference): the networks and
their actors, the observation normaliser, the critic pass and GAE, and the PPO loss with its head
gradient (``ppo_loss``) under the smallest learner that closes the loop (``PPOLearner``), and its
recurrent counterpart (``RecurrentPPOLearner``: truncated BPTT through the GRU kernels)."""
from . import gae, networks, normalization, optim, ppo  # noqa: F401
from .gae import RecurrentValueFunction, ValueFunction, compute_gae  # noqa: F401
from .networks import (FeedForwardModel, NormalTanhPolicy, RecurrentModel, RecurrentTanhPolicy,  # noqa: F401
                       make_model, make_models, make_recurrent_model)
from .normalization import ObservationNormalizer, create_observation_normalizer  # noqa: F401
from .optim import FusedAdam  # noqa: F401
from .ppo import PPOLearner, RecurrentPPOLearner, ppo_loss  # noqa: F401
