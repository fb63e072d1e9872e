"""Model classes registered under the reference's META_ARCHITECTURE names ("next" row 4 of SURVEY 8f)."""
from .mcan import MCAN, MLP
from .cross_modality_transformer import CrossModalityTransformer
from .mmf_m4c import MMF_M4C

__all__ = ["MCAN", "MLP", "CrossModalityTransformer", "MMF_M4C"]
