"""Message-passing network (``src/Models/MessagePassingNetwork``): HIP inference path (model.py), training mode (train.py)."""
from .model import NodeClassificationMPNSimple, get_mpn_model  # noqa: F401
