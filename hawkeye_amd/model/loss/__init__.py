from .MAMC_loss import MAMCLoss, NPairsLoss  # noqa: F401
from .CIN_loss import CINLoss  # noqa: F401
from .peer_learning_loss import PeerLearningLoss  # noqa: F401
from .APINet_loss import APINetLoss  # noqa: F401
from .NTS_loss import NTSLoss  # noqa: F401
from .CrossX_loss import CrossXLoss  # noqa: F401
from .DCL_loss import DCLLoss  # noqa: F401
from .InterpParts_loss import InterpPartsLoss  # noqa: F401
from .MGE_loss import MGELoss  # noqa: F401
