"""The enums of the agent statistics and of the exploration study — reference: recogym/constants.py (same names, same values)."""
from enum import Enum


class AgentStats(Enum):
    """Agent statistics."""
    # Confidence interval.
    Q0_025 = 0
    Q0_500 = 1
    Q0_975 = 2
    # Number of samples (users) in the training data.
    SAMPLES = 3
    AGENTS = 4
    SUCCESSES = 5  # Clicks.
    FAILURES = 6  # Non-clicks.


class AgentInit(Enum):
    """What build_agents needs to construct an agent."""
    CTOR = 0  # Agent constructor.
    DEF_ARGS = 1  # Default agent arguments.


class TrainingApproach(Enum):
    """Which acts of an evolution step the next agent is trained on (evaluate_agent)."""
    ALL_DATA = 0  # Everything, accumulated.
    SLIDING_WINDOW_ALL_DATA = 1  # Every `sliding_window_samples`-th act.
    ALL_EXPLORATION_DATA = 2  # The explored acts, accumulated.
    SLIDING_WINDOW_EXPLORATION_DATA = 3  # Every `sliding_window_samples`-th act where it explored.
    MOST_VALUABLE = 4  # Not implemented by the reference (its `assert False`).
    LAST_STEP = 5  # Everything of the last step only.


class EvolutionCase(Enum):
    """The keys of evaluate_agent's result."""
    SUCCESS = 0
    FAILURE = 1
    ACTIONS = 2
    SUCCESS_GREEDY = 3
    FAILURE_GREEDY = 4


class RoiMetrics(Enum):
    """Return-of-investment data."""
    ROI_MEAN = 0
    ROI_0_025 = 1
    ROI_0_975 = 2
    ROI_SUCCESS = 3
    ROI_FAILURE = 4
