from .blas_grid import BLASGrid
from .hash_grid import HashGrid, geometric_resolutions
from .latent_grid import LatentGrid
from .triplanar_grid import TriplanarFeatureVolume, TriplanarGrid
from .octree_grid import OctreeGrid
from .codebook_grid import CodebookOctreeGrid
