"""Learner-side pieces with a native inference path (po_brax/training in the reference)."""
from . import gae, networks, normalization  # noqa: F401
from .gae import ValueFunction, compute_gae  # noqa: F401
from .networks import FeedForwardModel, NormalTanhPolicy, make_model, make_models  # noqa: F401
from .normalization import ObservationNormalizer, create_observation_normalizer  # noqa: F401
