from .image import NeuralImage
from .nerf import NeuralRadianceField
from .neural_sdf import NeuralSDF
from .neural_sdf_tex import NeuralSDFTex
from .spc_field import SPCField

__all__ = ["NeuralImage", "NeuralRadianceField", "NeuralSDF", "NeuralSDFTex", "SPCField"]
