from .nerf import NeuralRadianceField
from .neural_sdf import NeuralSDF
from .neural_sdf_tex import NeuralSDFTex

__all__ = ["NeuralRadianceField", "NeuralSDF", "NeuralSDFTex"]
