from .nerf import NeuralRadianceField
from .neural_sdf import NeuralSDF

__all__ = ["NeuralRadianceField", "NeuralSDF"]
