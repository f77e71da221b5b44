"""``AxisAlignedBBoxAS``: the whole cube [-1, 1]^3 as one occupied cell (reference wisp/accelstructs/aabb_as.py, a one-level
dense octree marched at level 0). Here that is a fully occupied ``OctreeAS`` of level 0: ``raytrace`` gives each ray's
entry and exit of the cube, ``raymarch`` samples between them."""
from . import OctreeAS


class AxisAlignedBBoxAS(OctreeAS):
    def __init__(self):
        super().__init__(0)

    def name(self) -> str:
        return "AABB"
