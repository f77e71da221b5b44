from .image import NeuralImage
from .nerf import NeuralRadianceField
from .neural_sdf import NeuralSDF
from .neural_sdf_tex import NeuralSDFTex

__all__ = ["NeuralImage", "NeuralRadianceField", "NeuralSDF", "NeuralSDFTex"]
