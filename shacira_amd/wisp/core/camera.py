"""``Camera``: the part of ``kaolin.render.camera.Camera`` that the reference's datasets and ray generation read
(wisp/ops/raygen/raygen.py:46-119, wisp/datasets/formats/nerf_standard_dataset.py:391-410), restated here because kaolin is
not a dependency of this package. One object holds V cameras of one image size: a batch of view matrices [V, 4, 4] (world to
camera, the camera looking down its -z axis with +y up) and per-camera focal lengths and principal-point offsets in pixels.
Nothing here is differentiable on purpose: the reference does not optimise poses."""
from enum import IntEnum

import torch


class CameraFOV(IntEnum):
    HORIZONTAL = 0
    VERTICAL = 1


def blender_coords():
    """The basis change B of a z-up (Blender) world into the y-up world of the renderer: a point p becomes B p,
    (x, y, z) -> (x, z, -y)."""
    return torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]], dtype=torch.float64)


def _look_at(eye, at, up):
    backward = eye - at
    backward = backward / backward.norm(dim=-1, keepdim=True)
    right = torch.cross(up, backward, dim=-1)
    right = right / right.norm(dim=-1, keepdim=True)
    true_up = torch.cross(backward, right, dim=-1)
    rot = torch.stack([right, true_up, backward], dim=-2)              # rows: the camera's axes in the world
    view = torch.zeros(eye.shape[:-1] + (4, 4), dtype=eye.dtype, device=eye.device)
    view[..., :3, :3] = rot
    view[..., :3, 3] = -(rot @ eye.unsqueeze(-1)).squeeze(-1)
    view[..., 3, 3] = 1.0
    return view


class _Extrinsics:
    """``camera.extrinsics``: the rigid transform between the world and the cameras."""

    def __init__(self, camera):
        self._camera = camera

    def inv_transform_rays(self, origins, dirs):
        """Camera-space rays [N, 3] into the world, with kaolin's leading camera axis: ([V, N, 3], [V, N, 3])."""
        view = self._camera.view_matrix()
        rot = view[:, :3, :3]                                          # world -> camera; its transpose goes back
        pos = self._camera.cam_pos()
        origins = origins.to(view.dtype).unsqueeze(0) @ rot + pos.unsqueeze(1)
        dirs = dirs.to(view.dtype).unsqueeze(0) @ rot
        return origins, dirs


class Camera:
    def __init__(self, view, focal_x, focal_y, x0, y0, width, height, near, far, fov_distance=None):
        self._view = view                      # [V, 4, 4]
        self._focal_x, self._focal_y = focal_x, focal_y        # [V]
        self._x0, self._y0 = x0, y0            # [V]
        self._fov_distance = fov_distance      # [V] or None (pinhole)
        self.width, self.height = int(width), int(height)
        self.near, self.far = float(near), float(far)

    # ------------------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_args(cls, view_matrix=None, eye=None, at=None, up=None, focal_x=None, focal_y=None, fov=None, width=None,
                  height=None, near=1e-2, far=1e2, x0=0.0, y0=0.0, fov_distance=None, dtype=torch.float64, device=None):
        """By ``view_matrix`` ([4, 4] or [V, 4, 4]) or by ``eye`` / ``at`` / ``up``; by ``focal_x`` (``focal_y`` defaults to it)
        or by ``fov``, the vertical field of view in radians. ``fov_distance`` not None makes an orthographic camera."""
        if width is None or height is None:
            raise ValueError("Camera.from_args needs width and height")
        as_t = lambda v: torch.as_tensor(v, dtype=dtype, device=device)
        if view_matrix is not None:
            if eye is not None or at is not None or up is not None:
                raise ValueError("Camera.from_args takes view_matrix or eye / at / up, not both")
            view = as_t(view_matrix).clone()
            if view.dim() == 2:
                view = view.unsqueeze(0)
        else:
            if eye is None or at is None or up is None:
                raise ValueError("Camera.from_args needs view_matrix or all of eye, at, up")
            eye, at, up = as_t(eye), as_t(at), as_t(up)
            if eye.dim() == 1:
                eye, at, up = eye.unsqueeze(0), at.unsqueeze(0), up.unsqueeze(0)
            view = _look_at(eye, at.expand_as(eye), up.expand_as(eye))
        if view.shape[1:] != (4, 4):
            raise ValueError(f"view matrices must be [V, 4, 4], got {tuple(view.shape)}")
        V = view.shape[0]
        per_cam = lambda v: as_t(v).reshape(-1).expand(V).clone()
        if fov_distance is not None:
            fd = per_cam(fov_distance)
            fx = fy = torch.ones(V, dtype=dtype, device=view.device)
            if focal_x is not None:
                fx = per_cam(focal_x)
                fy = per_cam(focal_y if focal_y is not None else focal_x)
        else:
            fd = None
            if focal_x is not None:
                fx = per_cam(focal_x)
                fy = per_cam(focal_y if focal_y is not None else focal_x)
            elif fov is not None:
                fy = height / (2.0 * torch.tan(per_cam(fov) / 2.0))
                fx = fy.clone()
            else:
                raise ValueError("Camera.from_args needs focal_x or fov (or fov_distance for an orthographic camera)")
        return cls(view, fx, fy, per_cam(x0), per_cam(y0), width, height, near, far, fd)

    @classmethod
    def cat(cls, cameras):
        cameras = list(cameras)
        first = cameras[0]
        for c in cameras[1:]:
            if (c.width, c.height, c.near, c.far, c.lens_type) != (first.width, first.height, first.near, first.far,
                                                                   first.lens_type):
                raise ValueError("Camera.cat: image size, clipping planes and lens must agree")
        j = lambda name: torch.cat([getattr(c, name) for c in cameras])
        fd = None if first._fov_distance is None else j("_fov_distance")
        return cls(j("_view"), j("_focal_x"), j("_focal_y"), j("_x0"), j("_y0"), first.width, first.height, first.near,
                   first.far, fd)

    # -------------------------------------------------------------------------------------------------------- container
    def __len__(self):
        return self._view.shape[0]

    def __getitem__(self, idx):
        if isinstance(idx, int):
            idx = slice(idx, idx + 1) if idx != -1 else slice(idx, None)
        g = lambda t: t[idx]
        fd = None if self._fov_distance is None else g(self._fov_distance)
        return Camera(g(self._view), g(self._focal_x), g(self._focal_y), g(self._x0), g(self._y0), self.width, self.height,
                      self.near, self.far, fd)

    def to(self, *args, **kwargs):
        g = lambda t: t.to(*args, **kwargs)
        fd = None if self._fov_distance is None else g(self._fov_distance)
        return Camera(g(self._view), g(self._focal_x), g(self._focal_y), g(self._x0), g(self._y0), self.width, self.height,
                      self.near, self.far, fd)

    @property
    def device(self):
        return self._view.device

    @property
    def dtype(self):
        return self._view.dtype

    # ------------------------------------------------------------------------------------------------------- intrinsics
    @property
    def lens_type(self):
        return "pinhole" if self._fov_distance is None else "ortho"

    @property
    def focal_x(self):
        return self._focal_x

    @property
    def focal_y(self):
        return self._focal_y

    @property
    def x0(self):
        return self._x0

    @property
    def y0(self):
        return self._y0

    @property
    def fov_distance(self):
        return self._fov_distance

    def tan_half_fov(self, axis=CameraFOV.VERTICAL):
        if axis == CameraFOV.HORIZONTAL:
            return self.width / (2.0 * self._focal_x)
        return self.height / (2.0 * self._focal_y)

    # ------------------------------------------------------------------------------------------------------- extrinsics
    @property
    def extrinsics(self):
        return _Extrinsics(self)

    def view_matrix(self):
        return self._view

    def inv_view_matrix(self):
        inv = torch.zeros_like(self._view)
        rot_t = self._view[:, :3, :3].transpose(1, 2)
        inv[:, :3, :3] = rot_t
        inv[:, :3, 3] = self.cam_pos()
        inv[:, 3, 3] = 1.0
        return inv

    def cam_pos(self):
        """[V, 3]: -R^T t of the view matrix [R | t]."""
        rot_t = self._view[:, :3, :3].transpose(1, 2)
        return -(rot_t @ self._view[:, :3, 3:4]).squeeze(-1)

    @property
    def t(self):
        """[V, 3, 1]: the translation column of the view matrices (kaolin's ``extrinsics.t``)."""
        return self._view[:, :3, 3:4]

    @t.setter
    def t(self, value):
        """In place: the translation column replaced, the rotation kept. With ``value = s * t`` the camera position -R^T t is
        scaled by s about the world's origin."""
        self._view[:, :3, 3] = torch.as_tensor(value, dtype=self.dtype, device=self.device).reshape(-1, 3)

    def translate(self, offset):
        """In place: the cameras moved by ``offset`` [3] (or [V, 3]) in the world, rotation unchanged -- ``cam_pos()`` becomes
        ``cam_pos() + offset`` (kaolin's ``extrinsics.translate``: t becomes t - R offset)."""
        offset = torch.as_tensor(offset, dtype=self.dtype, device=self.device).reshape(-1, 3)
        self._view[:, :3, 3] = self._view[:, :3, 3] - (self._view[:, :3, :3] @ offset.expand(len(self), 3).unsqueeze(-1)).squeeze(-1)
        return self

    def normalize(self, center, scale):
        """In place, the net effect of ``translate(-center)`` followed by ``t = t * scale``: the camera position becomes
        (pos - center) * scale, the rotation is unchanged -- what a data set applies to its ray origins when it moves and
        scales its point cloud into [-1, 1]^3."""
        self.translate(-torch.as_tensor(center, dtype=self.dtype, device=self.device))
        self.t = self.t * float(scale)
        return self

    def change_coordinate_system(self, basis_change):
        """In place: the world's points p become B p (B a 3x3 orthonormal basis change). The view matrix becomes V B4^-1, so
        every camera-space point, and with it the picture, stays what it was."""
        b4 = torch.eye(4, dtype=self.dtype, device=self.device)
        b4[:3, :3] = torch.as_tensor(basis_change, dtype=self.dtype, device=self.device)
        self._view = self._view @ torch.linalg.inv(b4)
        return self
