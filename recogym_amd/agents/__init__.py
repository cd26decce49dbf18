from .abstract import Agent
from .random_agent import RandomAgent, random_args
from .organic_user_count import OrganicUserEventCounterAgent, organic_user_count_args
from .last_view_table import LastViewTableAgent
from .logreg_frozen import LogregFrozenAgent
from .logreg_ips import LogregMulticlassIpsAgent, logreg_multiclass_ips_args
from .logreg_poly import LogregPolyAgent, LogregPolyFrozenAgent, logreg_poly_args
from .bayesian_poly_vb import BayesianAgentVB, BayesianVBFrozenAgent, bayesian_poly_args
from .nn_ips import NnIpsAgent, NnIpsFrozenAgent, nn_ips_args
from .pytorch_mlr import PyTorchMLRAgent, PyTorchMLRFrozenAgent, pytorch_mlr_args
from .feature_feed import train_data_from_log
from .bandit_mf import BanditMFSquareAgent, bandit_mf_square_args
from .organic_count import OrganicCount, organic_count_args
from .bandit_count import BanditCount, bandit_count_args
from .epsilon_greedy import EpsilonGreedy, epsilon_greedy_args
from .organic_mf import OrganicMFSquare, organic_mf_square_args
