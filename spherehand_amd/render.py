"""Differentiable renderers and render losses -- the module-level API of the
reference's mesh/render.py (same class names, constructor arguments, forward
signatures and return values), running on the hand-written HIP kernels.

    BallRender               mesh/render.py:10-53
    HandBallPrimitiveRender  mesh/render.py:56-90
    DataToModelLoss          mesh/render.py:93-142
    DepthRasterizationFunction / DepthRasterization / DepthRender  mesh/render.py:282-331
    TriangleDepthRaster      depth_rasterization.forward, differentiable at any width x height
    AntialiasedDepthRaster   the same, clamped and antialiased: gradients at the silhouette too
    MeshAttributeRaster      TriangleDepthRaster + per-pixel maps of per-vertex attributes (part maps, correspondences)
    AntialiasedAttributeRaster  the maps and the clamped depth, both antialiased: outline gradients for the maps too
    MeshNormalRaster         a unit normal map from area-weighted vertex normals, and the depth: gradients reach z
    SilhouetteDistance       the distance of projected points to the observed silhouette: a pull from any distance
    SilhouetteCoverage       its complement: the distance of observed pixels to the rendered silhouette, a pull on the mesh
    DepthNormalMap           a unit normal map from a depth image, differentiable in the depth: observed or rendered
    NormalConsistencyLoss    1 - m . o between two normal maps: the orientation term
    MeshVertices             bone transforms or pose -> the mesh's vertices, differentiable: the mesh terms' way to the pose
    KeypointPoseSolver       the 41 keypoints -> the pose, by Levenberg-Marquardt from a start pose: the way INTO the mesh path
    MeshPoseFitter           the pose fitted to an observed depth image: Gauss-Newton ICP on the mesh, from such a start
    MultiViewMeshPoseFitter  the same on several depth views of every sample: one pose, one rigid transform per view
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .hand_model import radii_of, sparse_skin, unique_skin
from .kinematicsTransformation import keypoint_skinning


class BallRender(nn.Module):
    """forward(xyz_centers[N,>=3], radiuses[N]) -> [N,H,W]: one orthographic
    front-surface depth map per sphere, background 100 (mesh/render.py:26-53).
    One launch of the sphere rasterizer with J = 1; differentiable in both
    arguments."""

    def __init__(self, width, height):
        super().__init__()
        self.width = width
        self.height = height

    def forward(self, xyz_centers, radiuses):
        n = xyz_centers.shape[0]
        spheres = torch.cat([xyz_centers[:, 0:3], radiuses.reshape(n, 1)], dim=1).view(n, 1, 4)
        return ops.SphereDepthRaster.apply(spheres.float(), self.height, self.width)


class HandBallPrimitiveRender(nn.Module):
    """forward(T[B,17,4,4]) -> (part_maps[B,41,H,W], depth_maps[B,H,W])
    (mesh/render.py:81-90).  depth_maps comes from the fused min kernel and
    carries the gradient; the 41x larger part_maps, which only the reference's
    viewer reads (mesh/interactive_viewer.py:61), is rendered by a second launch
    and returned detached unless `differentiable_part_maps` is set."""

    def __init__(self, bones, width, height, differentiable_part_maps=False):
        super().__init__()
        self.width = width
        self.height = height
        self.ball_renderer = BallRender(width, height)
        self.lbs = keypoint_skinning(bones)
        self.num_vertices = self.lbs.num_vertices
        radiuses = [r for bone in bones for _, r in bone.get('keypoint', [])]
        self.register_buffer('radiuses', torch.tensor(radiuses).float().unsqueeze(0))
        self.differentiable_part_maps = differentiable_part_maps

    def spheres(self, transformation_mats):
        T = transformation_mats
        if T.is_cuda and T.dtype == torch.float32 and self.lbs.single_bone:   # one launch per direction (keypoint_skin.hip)
            if T.dim() == 5:
                T = T.squeeze(2)
            lbs = self.lbs
            return ops.KeypointSpheres.apply(T, lbs.kp_bone, lbs.skin_wv, self.radiuses.view(-1), lbs.kp_bone_start,
                                             lbs.kp_bone_points, lbs.right_hand)
        pts = self.lbs(transformation_mats)                                  # [B,41,4]
        B = pts.shape[0]
        return torch.cat([pts[:, :, 0:3], self.radiuses.expand(B, -1).unsqueeze(-1)], dim=2)

    def pose_spheres(self, hand_transformation_mat, parameters):
        """spheres(hand_transformation_mat(parameters)) without the bone transforms visiting HBM: pose [B,26] -> sphere
        records [B,41,4], one launch per direction (ops.PoseSpheres; the same records and pose gradient, bit for bit,
        as the two modules chained).  `hand_transformation_mat`: the kinematicsTransformation.HandTransformationMat
        whose offset matrices the bones carry."""
        fk, lbs = hand_transformation_mat, self.lbs
        if not (parameters.is_cuda and parameters.dtype == torch.float32 and lbs.single_bone and fk.offset.shape[0] == 17):
            return self.spheres(fk(parameters))
        return ops.PoseSpheres.apply(parameters, fk.offset, fk.offset_inv, lbs.kp_bone, lbs.skin_wv, self.radiuses.view(-1),
                                     lbs.kp_bone_start, lbs.kp_bone_points, lbs.right_hand)

    def pose_depth(self, hand_transformation_mat, parameters):
        """pose [B,26] -> depth maps [B,H,W] (the differentiable output of forward(), without the part maps): the fit
        chain's three launches per direction."""
        fk, lbs = hand_transformation_mat, self.lbs
        if not (parameters.is_cuda and parameters.dtype == torch.float32 and lbs.single_bone and fk.offset.shape[0] == 17
                and parameters.shape[0] > 0):
            return ops.SphereDepthRaster.apply(self.pose_spheres(fk, parameters), self.height, self.width)
        return ops.PoseDepthRaster.apply(parameters, fk.offset, fk.offset_inv, lbs.kp_bone, lbs.skin_wv, self.radiuses.view(-1),
                                         lbs.kp_bone_start, lbs.kp_bone_points, lbs.right_hand, self.height, self.width)

    def forward(self, transformation_mats):
        sph = self.spheres(transformation_mats).contiguous()
        B = sph.shape[0]
        depth_maps = ops.SphereDepthRaster.apply(sph, self.height, self.width)
        flat = sph.view(-1, 4)
        if self.differentiable_part_maps:
            balls = self.ball_renderer(flat[:, 0:3], flat[:, 3])
        else:
            with torch.no_grad():
                balls = self.ball_renderer(flat[:, 0:3], flat[:, 3])
        part_maps = balls.view(B, self.num_vertices, self.height, self.width)
        return part_maps, depth_maps


class DataToModelLoss(nn.Module):
    """forward(dms[N,H,W], joints[N,J,3]) -> scalar: mean over all pixels of
    clamp(min_j | ||(xg,yg,depth) - c_j|| - r_j |, 0, 50) on pixels with depth <=
    99 (mesh/render.py:123-142).  `mesh` is the model dict or a list of radii
    (mesh/render.py:107-117)."""

    def __init__(self, width, height, mesh):
        super().__init__()
        self.width = width
        self.height = height
        radiuses = torch.from_numpy(np.asarray(radii_of(mesh), np.float32))
        self.num_joints = len(radiuses)
        self.register_buffer('radiuses', radiuses.view(1, 1, 1, self.num_joints))

    def forward(self, dms, joints):
        num_batch = dms.shape[0]
        joints = joints.reshape(num_batch, self.num_joints, 3)
        return ops.DataToModel.apply(dms.reshape(num_batch, self.height, self.width).float(), joints.float(),
                                     self.radiuses.view(-1))


class DepthRasterizationFunction(torch.autograd.Function):
    """mesh/render.py:282-287: the extension call + clamp(max=100).  Forward only
    (the reference defines no backward; callers detach the result)."""

    @staticmethod
    def forward(ctx, width, height, face_vertices):
        depth_maps = ops.tri_raster_fwd(width, height, face_vertices.contiguous())
        return torch.clamp(depth_maps, max=100.0)


class DepthRasterization(nn.Module):
    """mesh/render.py:289-312.  forward(vertices[B,NV,>=3]) -> [B,height,width]:
    rasterize at 640x640, clamp, bilinear-downsample -- by default as ONE fused kernel that
    only rasterizes the source pixels the resize reads (`fused`).  `np_faces` is NOT
    modified (the reference swaps its columns in place for the right hand, :298-300).

    differentiable=True (square sizes up to 320 only, checked here): where grad is enabled and `vertices` requires grad,
    the depth is differentiable w.r.t. vertices[..., :3] (ops.MeshDepthRaster) -- the same bits as the default path.
    The sphere renderer's contract: the gradient routes to each tap's owner face and holds coverage fixed; there is no
    gradient for edge, silhouette or visibility changes.  The reference defines no backward here (:282-287)."""

    def __init__(self, width, height, np_faces, right_hand=True, differentiable=False):
        super().__init__()
        if differentiable and not (width == height and ops.mesh_owner_supported(width)):
            raise ValueError("differentiable DepthRasterization takes square sizes up to 320, not %r x %r" % (width, height))
        self.differentiable = differentiable
        self.width = width
        self.height = height
        faces = np.array(np_faces, dtype=np.int64, copy=True)
        if right_hand:
            faces[:, [0, 1]] = faces[:, [1, 0]]
        self.register_buffer('faces', torch.from_numpy(faces).view(-1))
        self.register_buffer('faces_i32', torch.from_numpy(faces.astype(np.int32)).contiguous())
        self.num_faces = len(faces)
        self.fused = True     # False: explicit 640x640 raster, then torch clamp + interpolate

    def forward(self, vertices):
        num_batch = vertices.shape[0]
        if self.differentiable and vertices.requires_grad and torch.is_grad_enabled():
            if not (vertices.is_cuda and vertices.dtype == torch.float32 and vertices.shape[-1] in (3, 4)):
                raise RuntimeError("the differentiable mesh path takes CUDA fp32 vertices [B,NV,3 or 4]")
            return ops.MeshDepthRaster.apply(ops.vertices4(vertices)[0], self.faces_i32, self.height, 640, 100.0)
        on_kernel = vertices.is_cuda and vertices.shape[-1] == 4 and vertices.dtype == torch.float32
        if on_kernel and self.fused and self.width == self.height and 2 * self.width <= 641:
            # raster + clamp + resize in one pass over the sampled source pixels only
            return ops.mesh_depth_fwd(vertices.contiguous(), self.faces_i32, self.height, 640, 100.0)
        if on_kernel:
            # face gather fused into the rasterizer (no [B,F,3,3] intermediate)
            raw = ops.tri_raster_indexed_fwd(640, 640, vertices.contiguous(), self.faces_i32)
            rendered_dm = torch.clamp(raw, max=100.0).unsqueeze(1)
        else:
            face_vertices = vertices[:, self.faces, 0:3].view(num_batch, self.num_faces, 3, 3)
            rendered_dm = DepthRasterizationFunction.apply(640, 640, face_vertices).unsqueeze(1)
        return torch.nn.functional.interpolate(rendered_dm, size=(self.height, self.width), mode='bilinear',
                                               align_corners=False).squeeze(1)


class TriangleDepthRaster(nn.Module):
    """depth_rasterization.forward (mesh/cuda_kernel/depth_rasterization_cuda_kernel.cu:18-134) on an indexed mesh, at
    its own resolution and differentiable.  forward(vertices[B,NV,>=3], pixel-space x, y, z) -> the RAW depth
    [B,height,width], background 1000, with no clamp and no resize, bit-identical to the forward-only raster.  Any
    width x height the raster takes.  `np_faces` gets the right hand's winding swap that DepthRasterization applies
    (mesh/render.py:298-300) and is not modified.

    Where grad is enabled and `vertices` requires grad, the depth is differentiable w.r.t. vertices[..., :3]
    (ops.TriRasterIndexed; ops.TriRaster takes face soups [B,F,3,3]).  Each pixel's gradient goes to the face that owns
    its depth and coverage is held fixed: there is no edge, silhouette or visibility gradient.  Clamp the result in torch
    as the reference does (torch.clamp(depth, max=100.0) passes the gradient at equality)."""

    def __init__(self, width, height, np_faces, right_hand=True):
        super().__init__()
        self.width = width
        self.height = height
        faces = np.array(np_faces, dtype=np.int64, copy=True)
        if right_hand:
            faces[:, [0, 1]] = faces[:, [1, 0]]
        self.register_buffer('faces_i32', torch.from_numpy(faces.astype(np.int32)).contiguous())

    def forward(self, vertices):
        if vertices.dim() != 3 or vertices.shape[-1] < 3:
            raise RuntimeError("TriangleDepthRaster takes vertices [B,NV,>=3]")
        v = vertices if vertices.shape[-1] in (3, 4) else vertices[..., :3]
        if v.requires_grad and torch.is_grad_enabled():
            return ops.TriRasterIndexed.apply(v, self.faces_i32, self.width, self.height)
        return ops.tri_raster_indexed_fwd(self.width, self.height, ops.vertices4(v)[0], self.faces_i32)


class AntialiasedDepthRaster(nn.Module):
    """TriangleDepthRaster's depth, clamped and then antialiased across the silhouette (ops.TriAntialias;
    include/spherehand_hip.h states the pass): forward(vertices[B,NV,>=3], pixel-space x, y, z) returns
    clamp(raw, max=clamp_max) [B,height,width] with the pixel pairs that straddle a silhouette edge blended by where the
    edge crosses between their centres.  Differentiable w.r.t. vertices[..., :3]: interior gradients through the faces
    that own the pixels (TriangleDepthRaster's contract), outline gradients in x, y through the pass.
    silhouette(vertices) is the antialiased 0/1 coverage: a mask differentiable in x, y.

    `np_faces` gets the right hand's winding swap (mesh/render.py:298-300) and is not modified.  The edge table
    (ops.tri_edge_table) is built once from the swapped faces; `np_vertices` (rest positions [NV,C]) welds corners with
    bit-identical rows, which a mesh that stores every face's corners separately needs -- without it, every edge of such
    a mesh is a silhouette edge."""

    def __init__(self, width, height, np_faces, right_hand=True, np_vertices=None, clamp_max=100.0):
        super().__init__()
        self.width = width
        self.height = height
        self.clamp_max = clamp_max
        faces = np.array(np_faces, dtype=np.int64, copy=True)
        if right_hand:
            faces[:, [0, 1]] = faces[:, [1, 0]]
        self.register_buffer('faces_i32', torch.from_numpy(faces.astype(np.int32)).contiguous())
        self.register_buffer('edges_i32', torch.from_numpy(ops.tri_edge_table(faces, np_vertices)).contiguous())

    def _raster(self, vertices):
        if vertices.dim() != 3 or vertices.shape[-1] < 3:
            raise RuntimeError("AntialiasedDepthRaster takes vertices [B,NV,>=3]")
        v = vertices if vertices.shape[-1] in (3, 4) else vertices[..., :3]
        depth, owner = ops.TriRasterIndexedOwner.apply(v, self.faces_i32, self.width, self.height)
        return v, depth, owner

    def forward(self, vertices):
        v, depth, owner = self._raster(vertices)
        c = torch.clamp(depth, max=self.clamp_max)
        return ops.TriAntialias.apply(c, depth.detach(), owner, v, self.faces_i32, self.edges_i32)

    def silhouette(self, vertices):
        v, depth, owner = self._raster(vertices)
        cover = (owner >= 0).float()
        return ops.TriAntialias.apply(cover, depth.detach(), owner, v, self.faces_i32, self.edges_i32)


class MeshAttributeRaster(nn.Module):
    """TriangleDepthRaster plus per-pixel maps of per-vertex attributes (ops.TriInterpolate; include/spherehand_hip.h
    states the interpolation): forward(vertices[B,NV,>=3] pixel-space x, y, z, attributes [B,NV,C] or [NV,C]) ->
    (maps [B,C,height,width], depth [B,height,width]).  `depth` is TriangleDepthRaster's raw depth, the same bits and
    differentiable as there.  A map pixel is its owner face's three attribute rows weighted by the clamped, normalised
    barycentric weights the depth used (screen-linear: the camera is orthographic), 0 at background pixels; the maps are
    differentiable w.r.t. the attributes and vertices[..., :2], coverage held fixed.  With
    hand_model.dense_skin_weights as attributes the maps are a soft part segmentation, with the rest positions a dense
    correspondence map.  `np_faces` gets the right hand's winding swap (mesh/render.py:298-300) and is not modified."""

    def __init__(self, width, height, np_faces, right_hand=True):
        super().__init__()
        self.width = width
        self.height = height
        faces = np.array(np_faces, dtype=np.int64, copy=True)
        if right_hand:
            faces[:, [0, 1]] = faces[:, [1, 0]]
        self.register_buffer('faces_i32', torch.from_numpy(faces.astype(np.int32)).contiguous())

    def forward(self, vertices, attributes):
        if vertices.dim() != 3 or vertices.shape[-1] < 3:
            raise RuntimeError("MeshAttributeRaster takes vertices [B,NV,>=3]")
        v = vertices if vertices.shape[-1] in (3, 4) else vertices[..., :3]
        depth, owner = ops.TriRasterIndexedOwner.apply(v, self.faces_i32, self.width, self.height)
        return ops.TriInterpolate.apply(attributes, owner, v, self.faces_i32), depth


class AntialiasedAttributeRaster(nn.Module):
    """MeshAttributeRaster's maps and AntialiasedDepthRaster's depth from one raster, both antialiased across the
    silhouette: forward(vertices[B,NV,>=3] pixel-space x, y, z, attributes [B,NV,C] or [NV,C], 1 <= C <= 64) ->
    (maps [B,C,height,width], depth [B,height,width]).  One owner forward, ops.TriInterpolate, ops.TriAntialiasMaps on
    the maps (every pair decided once for all channels; include/spherehand_hip.h states the pass) and ops.TriAntialias on
    clamp(raw, max=clamp_max).  `depth` has AntialiasedDepthRaster's bits.  The maps are differentiable w.r.t. the
    attributes and vertices[..., :2]: inside the faces as MeshAttributeRaster's, and at the outline through the pass, so
    a part map, a correspondence map or any per-vertex signal can be fitted in x, y by render-and-compare.  With
    attributes ones [NV,1] the map is AntialiasedDepthRaster.silhouette() wherever the interpolated value is exactly 1.

    `np_faces` gets the right hand's winding swap (mesh/render.py:298-300) and is not modified; the edge table and
    `np_vertices` are AntialiasedDepthRaster's."""

    def __init__(self, width, height, np_faces, right_hand=True, np_vertices=None, clamp_max=100.0):
        super().__init__()
        self.width = width
        self.height = height
        self.clamp_max = clamp_max
        faces = np.array(np_faces, dtype=np.int64, copy=True)
        if right_hand:
            faces[:, [0, 1]] = faces[:, [1, 0]]
        self.register_buffer('faces_i32', torch.from_numpy(faces.astype(np.int32)).contiguous())
        self.register_buffer('edges_i32', torch.from_numpy(ops.tri_edge_table(faces, np_vertices)).contiguous())

    def forward(self, vertices, attributes):
        if vertices.dim() != 3 or vertices.shape[-1] < 3:
            raise RuntimeError("AntialiasedAttributeRaster takes vertices [B,NV,>=3]")
        v = vertices if vertices.shape[-1] in (3, 4) else vertices[..., :3]
        depth, owner = ops.TriRasterIndexedOwner.apply(v, self.faces_i32, self.width, self.height)
        raw = depth.detach()
        maps = ops.TriInterpolate.apply(attributes, owner, v, self.faces_i32)
        maps = ops.TriAntialiasMaps.apply(maps, raw, owner, v, self.faces_i32, self.edges_i32)
        c = torch.clamp(depth, max=self.clamp_max)
        return maps, ops.TriAntialias.apply(c, raw, owner, v, self.faces_i32, self.edges_i32)


class MeshNormalRaster(nn.Module):
    """A normal map and the depth from one raster: forward(vertices[B,NV,>=3] pixel-space x, y, z, points=None) ->
    (normal_map [B,3,height,width], depth [B,height,width]).  One owner forward, ops.TriVertexNormals on `points`
    ([B,NV,>=3]; default: the vertices' x, y, z), ops.TriInterpolate of the vertex normals and ops.Unit3Maps on the
    result (include/spherehand_hip.h states all three).  Background pixels are (0, 0, 0); every owned pixel has unit
    length.  `depth` is TriangleDepthRaster's raw depth, the same bits.

    antialias=True adds ops.TriAntialiasMaps after the normalisation and returns AntialiasedDepthRaster's depth
    (clamp(raw, max=clamp_max) through ops.TriAntialias), as AntialiasedAttributeRaster does: a blended outline pixel is
    then SHORTER than 1, and its length carries the coverage.

    The normals are those of the points given.  Pixel-space x, y with a depth-unit z is an anisotropic space: its normals
    are good for consistency losses and for the out-of-plane gradient, not for angles.  For metric normals pass the
    unprojected skinned points (SparseSkinning without a camera) as `points`.

    Orientation: the raster's cull (mesh/cuda_kernel/depth_rasterization_cuda_kernel.cu:33) draws a face when
    (y2 - y0)(x1 - x0) >= (y1 - y0)(x2 - x0), which is a non-negative z of e1 x e2 for the faces as the raster takes
    them: in their own winding drawn faces point away from the camera (smaller depth is nearer).  The module builds its
    normal tables from those faces with corners 1 and 2 exchanged, which negates every face normal exactly, so the normals
    of drawn faces have z <= 0: they point at the camera.  (Only with `points` in a space of the vertices' handedness.)
    ops.tri_vertex_normals itself never flips.

    The map is differentiable w.r.t. `points` in x, y and z (through the normals) and w.r.t. vertices[..., :2] (through
    the interpolation weights, and the outline with antialias=True); coverage and owner are held fixed.  `np_faces` gets
    the right hand's winding swap (mesh/render.py:298-300) and is not modified; `np_vertices` (rest positions [NV,C])
    welds vertices with bit-identical rows for the normals' sums and for the edge table -- a mesh that stores every face's
    corners separately gets faceted normals without it."""

    def __init__(self, width, height, np_faces, right_hand=True, np_vertices=None, antialias=False, clamp_max=100.0):
        super().__init__()
        self.width = width
        self.height = height
        self.antialias = antialias
        self.clamp_max = clamp_max
        faces = np.array(np_faces, dtype=np.int64, copy=True)
        if right_hand:
            faces[:, [0, 1]] = faces[:, [1, 0]]
        self.register_buffer('faces_i32', torch.from_numpy(faces.astype(np.int32)).contiguous())
        turned = np.ascontiguousarray(faces[:, [0, 2, 1]])
        self.register_buffer('normal_faces_i32', torch.from_numpy(turned.astype(np.int32)).contiguous())
        if np_vertices is not None:
            self.num_vertices = len(np_vertices)
        else:
            self.num_vertices = None
        self._np_faces, self._np_weld = turned, (None if np_vertices is None else np.array(np_vertices, copy=True))
        self._tables = {}
        if antialias:
            self.register_buffer('edges_i32', torch.from_numpy(ops.tri_edge_table(faces, np_vertices)).contiguous())

    def _normal_tables(self, NV, device):
        """The tables for NV vertices on `device` (built on first use: without np_vertices the constructor does not know NV)."""
        key = (NV, str(device))
        if key not in self._tables:
            if self.num_vertices is not None and NV != self.num_vertices:
                raise RuntimeError("MeshNormalRaster was built for %d vertices" % self.num_vertices)
            self._tables[key] = ops.tri_vertex_tables(self._np_faces, NV, self._np_weld).to(device)
        return self._tables[key]

    def forward(self, vertices, points=None):
        if vertices.dim() != 3 or vertices.shape[-1] < 3:
            raise RuntimeError("MeshNormalRaster takes vertices [B,NV,>=3]")
        v = vertices if vertices.shape[-1] in (3, 4) else vertices[..., :3]
        if points is None:
            p = v
        else:
            if points.dim() != 3 or points.shape[-1] < 3 or points.shape[:2] != vertices.shape[:2]:
                raise RuntimeError("points must be [B,NV,>=3] with the vertices' B and NV")
            p = points if points.shape[-1] in (3, 4) else points[..., :3]
        depth, owner = ops.TriRasterIndexedOwner.apply(v, self.faces_i32, self.width, self.height)
        tables = self._normal_tables(v.shape[1], v.device)
        normals = ops.TriVertexNormals.apply(p, self.normal_faces_i32, tables)
        maps = ops.TriInterpolate.apply(normals[..., :3], owner, v, self.faces_i32)
        maps = ops.Unit3Maps.apply(maps)
        if not self.antialias:
            return maps, depth
        raw = depth.detach()
        maps = ops.TriAntialiasMaps.apply(maps, raw, owner, v, self.faces_i32, self.edges_i32)
        c = torch.clamp(depth, max=self.clamp_max)
        return maps, ops.TriAntialias.apply(c, raw, owner, v, self.faces_i32, self.edges_i32)


class SilhouetteDistance(nn.Module):
    """The silhouette term of model fitting: the distance from projected model points to the observed foreground
    (ops.distance_transform, ops.DistanceSample; include/spherehand_hip.h states both).  observe(depth[B,H,W]) computes
    and keeps the exact squared distance transform of the pixels with depth < fg_max, once per observation.
    forward(points[B,N,>=2], pixel-space x, y first -- vertices, sphere centres and key points as the rasters take them)
    -> the per-point distances [B,N] in pixels, bilinear between pixel centres and saturated at max_dist; loss(points) is
    their mean.  Differentiable w.r.t. points[..., :2]: a point outside the observed silhouette gets a gradient of about
    unit length, however far the silhouette is: d value / d point points away from the nearest observed pixel, so a
    descent step moves the point towards it; a point inside gets 0.  A
    point outside the image samples the border, with no gradient in the clamped component."""

    def __init__(self, fg_max, max_dist=float('inf')):
        super().__init__()
        self.fg_max = float(fg_max)
        self.max_dist = float(max_dist)
        self.d2 = None

    def observe(self, depth):
        self.d2 = ops.distance_transform(depth.detach().contiguous(), self.fg_max)
        return self.d2

    def forward(self, points):
        if self.d2 is None:
            raise RuntimeError("SilhouetteDistance: observe(depth) first")
        return ops.DistanceSample.apply(points, self.d2, self.max_dist)

    def loss(self, points):
        return self.forward(points).mean()


class SilhouetteCoverage(nn.Module):
    """SilhouetteDistance's complement: the distance from every OBSERVED pixel to the RENDERED silhouette
    (ops.nearest_site_transform, ops.SilhouetteCover; include/spherehand_hip.h states both).  SilhouetteDistance pulls
    model points that lie outside the observation towards it and gives a model that lies inside nothing -- a mesh shrunk
    to a dot inside the observed hand is a minimum of that half.  This half pulls the mesh over observed pixels it does
    not cover.  observe(depth[B,H,W]) keeps the observation (observed: depth < fg_max) and each crop's count of observed
    pixels.  forward(vertices[B,NV,>=3], pixel-space x, y, z) renders the mesh at width x height with the owner raster
    (under no_grad), transforms that depth (rendered: depth < render_fg_max) and returns [B]: the mean distance in pixels
    of each crop's observed pixels to the nearest rendered pixel, saturated at max_dist; loss(vertices) is its mean.
    Coverage is decided at pixel centres: an observed pixel the render covers has distance 0.  Differentiable w.r.t.
    vertices[..., :2] only -- a gradient in x and y: every uncovered observed pixel pulls its nearest rendered pixel's
    owner face towards itself with the weights the depth used there, the nearest pixel and the weights held fixed.
    `np_faces` gets the right hand's winding swap (mesh/render.py:298-300) and is not modified."""

    def __init__(self, width, height, np_faces, fg_max, max_dist=float('inf'), right_hand=True, render_fg_max=1000.0):
        super().__init__()
        self.width = width
        self.height = height
        self.fg_max = float(fg_max)
        self.max_dist = float(max_dist)
        self.render_fg_max = float(render_fg_max)
        faces = np.array(np_faces, dtype=np.int64, copy=True)
        if right_hand:
            faces[:, [0, 1]] = faces[:, [1, 0]]
        self.register_buffer('faces_i32', torch.from_numpy(faces.astype(np.int32)).contiguous())
        self.observed = None
        self.count = None

    def observe(self, depth):
        if depth.dim() != 3 or tuple(depth.shape[1:]) != (self.height, self.width):
            raise RuntimeError("SilhouetteCoverage: observe takes depth [B,%d,%d]" % (self.height, self.width))
        self.observed = depth.detach().contiguous().float()
        self.count = (self.observed < self.fg_max).sum((1, 2)).clamp(min=1).float()
        return self.count

    def forward(self, vertices):
        if self.observed is None:
            raise RuntimeError("SilhouetteCoverage: observe(depth) first")
        if vertices.dim() != 3 or vertices.shape[-1] < 3:
            raise RuntimeError("SilhouetteCoverage takes vertices [B,NV,>=3]")
        v = vertices if vertices.shape[-1] in (3, 4) else vertices[..., :3]
        with torch.no_grad():
            depth, owner = ops.tri_raster_indexed_owner_fwd(self.width, self.height, ops.vertices4(v.detach())[0],
                                                            self.faces_i32)
            d2, nearest = ops.nearest_site_transform(depth, self.render_fg_max)
        dist = ops.SilhouetteCover.apply(v, self.faces_i32, owner, d2, nearest, self.observed, self.fg_max, self.max_dist)
        return dist.sum((1, 2)) / self.count

    def loss(self, vertices):
        return self.forward(vertices).mean()


class MeshDataToModelLoss(nn.Module):
    """DataToModelLoss (mesh/render.py:93-142) for the triangle mesh: the distance from every observed 3-D point to its
    closest point on the mesh surface, at any distance and in x, y and z (ops.MeshDataToModel; include/spherehand_hip.h
    states it).  forward(observed[B,H,W], vertices[B,NV,3 or 4] in model space) -> the mean over ALL B H W pixels of the
    distance saturated at max_dist, a pixel that is no data point counting as 0: the reference's normalisation.
    distances(observed, vertices) -> (dist [B,H,W], face [B,H,W] int32, rows of np_faces, -1 without one).
    pixel_to_model = (ax, bx, ay, by): pixel (row i, column j) is the point (ax j + bx, ay i + by, observed);
    (1, 0, 1, 0) is the raster's pixel space, MeshDataToModelLoss.reference_grid(width, height) the reference's
    millimetre grid.  A pixel is a data point iff observed < fg_max.  The default fg_max is the fp32 successor of 99,
    99.00000762939453 = 99 + 2^-17: for every fp32 value, observed < fg_max iff observed <= 99 iff not observed > 99,
    the reference's background rule (mesh/render.py:138); a NaN is no data point here, where the reference carries it
    into the mean.  `np_faces` is used as given -- the distance does not depend on winding -- and is not modified."""

    REFERENCE_FG_MAX = float(np.nextafter(np.float32(99.0), np.float32(np.inf)))

    def __init__(self, width, height, np_faces, pixel_to_model=(1.0, 0.0, 1.0, 0.0), fg_max=REFERENCE_FG_MAX, max_dist=50.0):
        super().__init__()
        self.width = width
        self.height = height
        self.pixel_to_model = tuple(float(t) for t in pixel_to_model)
        self.fg_max = float(fg_max)
        self.max_dist = float(max_dist)
        faces = np.array(np_faces, dtype=np.int64, copy=True).reshape(-1, 3)
        self.register_buffer('faces_i32', torch.from_numpy(faces.astype(np.int32)).contiguous())

    @staticmethod
    def reference_grid(width, height):
        """(ax, bx, ay, by) of mesh/render.py:99-100: x = (j - width / 2) 300 / width, y = (i - height / 2) 300 / height."""
        return (300.0 / width, -150.0, 300.0 / height, -150.0)

    def distances(self, observed, vertices):
        if observed.dim() != 3 or tuple(observed.shape[1:]) != (self.height, self.width):
            raise RuntimeError("MeshDataToModelLoss takes observed [B,%d,%d]" % (self.height, self.width))
        return ops.MeshDataToModel.apply(observed.detach().float(), vertices.float(), self.faces_i32, self.pixel_to_model,
                                         self.fg_max, self.max_dist)

    def forward(self, observed, vertices):
        return self.distances(observed, vertices)[0].mean()


class DepthNormalMap(nn.Module):
    """The unit normal map of a depth image (ops.DepthNormals; include/spherehand_hip.h, shr_depth_normals_fwd states
    it): forward(depth[B,H,W]) -> [B,3,H,W].  A pixel is foreground iff depth < fg_max; differences do not cross a
    background pixel, the image border or a depth step above max_step (one-sided there), and a pixel without a usable
    neighbour along an axis gets (0, 0, 0), as every background pixel does.  pixel_to_model = (ax, bx, ay, by) has
    MeshDataToModelLoss's meaning; only ax and ay are used, as the model-space widths of a pixel step: (1, 0, 1, 0) gives
    the pixel-space normals MeshNormalRaster produces by default, MeshDataToModelLoss.reference_grid metric ones.
    Orientation as MeshNormalRaster: z <= 0, towards the camera.  Differentiable w.r.t. depth, so it serves an observation
    (detached) and any rendered depth alike: BallRender, TriangleDepthRaster, AntialiasedDepthRaster,
    DepthRender(..., differentiable=True)."""

    def __init__(self, fg_max, pixel_to_model=(1.0, 0.0, 1.0, 0.0), max_step=float('inf')):
        super().__init__()
        self.fg_max = float(fg_max)
        ax, _, ay, _ = (float(t) for t in pixel_to_model)
        self.scale = (ax, ay)
        self.max_step = float(max_step)

    def forward(self, depth):
        if depth.dim() != 3:
            raise RuntimeError("DepthNormalMap takes depth [B,H,W]")
        return ops.DepthNormals.apply(depth.float(), self.fg_max, self.scale, self.max_step)


class NormalConsistencyLoss(nn.Module):
    """The orientation term of model fitting: forward(model_map[B,3,H,W], observed_map[B,3,H,W]) -> [B], per crop the
    mean of 1 - m . o over the pixels where both maps are non-zero (0 for a crop without one); loss(...) is the mean over
    crops.  The maps are MeshNormalRaster's or DepthNormalMap's.  An antialiased outline pixel, shorter than 1, weighs by
    its coverage.  observed_map gets no gradient.  A composition of torch operations: DESIGN.md 4.4k has its cost next to
    the normal kernels'."""

    def forward(self, model_map, observed_map):
        if model_map.dim() != 4 or model_map.shape[1] != 3 or model_map.shape != observed_map.shape:
            raise RuntimeError("NormalConsistencyLoss takes two maps [B,3,H,W] of one shape")
        o = observed_map.detach()
        both = ((model_map.detach() != 0).any(1) & (o != 0).any(1)).to(model_map.dtype)
        term = (1.0 - (model_map * o).sum(1)) * both
        return term.sum((1, 2)) / both.sum((1, 2)).clamp(min=1.0)

    def loss(self, model_map, observed_map):
        return self.forward(model_map, observed_map).mean()


class SparseSkinning(nn.Module):
    """LinearBlendSkinning (+ optional orthographic camera) of the full mesh on the
    HIP kernel: forward(T[B,17,4,4], camera=None, rand_f=None) -> [B,NV,4].
    distinct=True: only the mesh's DISTINCT vertices (hand_model.unique_skin: 1 721 of 10 144 -- the reference stores
    each face's corners separately) -> [B,NU,4]; `vertex_index` [NV] maps a mesh vertex to its row.
    Where grad is enabled and T requires grad the result is differentiable w.r.t. T (ops.SkinVertices: the same bits;
    rand_f gets no gradient); MeshVertices is the module that fixes the camera and goes on to the pose."""

    def __init__(self, mesh, right_hand=True, distinct=False):
        super().__init__()
        if distinct:
            start, bone, wv, index = unique_skin(mesh)
            self.vertex_index = index
        else:
            start, bone, wv = sparse_skin(mesh)
            self.vertex_index = None
        self.register_buffer('skin_vertex_start', torch.from_numpy(start))
        self.register_buffer('skin_bone', torch.from_numpy(bone))
        self.register_buffer('skin_wv', torch.from_numpy(wv))
        self.right_hand = right_hand
        self.num_vertices = len(start) - 1

    def forward(self, transformation_mats, camera=None, rand_f=None):
        T = transformation_mats
        rand_f = None if rand_f is None else rand_f.detach().contiguous().float()
        if T.requires_grad and torch.is_grad_enabled():            # differentiable w.r.t. T: the same vertices, bit for bit
            return ops.SkinVertices.apply(T.contiguous().float(), self.skin_vertex_start, self.skin_bone, self.skin_wv,
                                          self.right_hand, camera, rand_f)
        return ops.lbs_project(T.contiguous().float(), self.skin_vertex_start, self.skin_bone,
                               self.skin_wv, self.right_hand, camera, rand_f)


class MeshVertices(nn.Module):
    """The triangle mesh's vertices from bone transforms or from the pose, differentiable: what carries the gradient of
    the mesh terms (TriangleDepthRaster, AntialiasedDepthRaster, MeshAttributeRaster, MeshNormalRaster,
    SilhouetteDistance, SilhouetteCoverage, MeshDataToModelLoss) from the vertices on to the hand.
    forward(T[B,17,4,4], rand_f=None) -> [B,NV,4] (ops.SkinVertices); pose_vertices(fk, params[B,26], rand_f=None) -> the
    same vertices and the pose gradient of fk followed by forward, bit for bit, in one launch per direction
    (ops.PoseVertices), `fk` being the kinematicsTransformation.HandTransformationMat whose offset matrices the bones carry.
    camera = (cx, cy, fx, fy): pixel-space vertices as the rasters take them, pixel_camera(W, H) for a W x H image;
    camera=None: model-space vertices (millimetres), which pair with MeshDataToModelLoss.reference_grid.
    distinct=True skins the mesh's 1 721 distinct vertices (hand_model.unique_skin), otherwise all 10 144 records.
    `faces`: np.int64 [F,3] indexing this module's rows, winding as the mesh stores it (the term modules swap it for the
    right hand themselves); `rest_vertices`: np.float32 [NV,3], the module's rows at the rest pose in model space, the
    np_vertices= welding argument of the antialias and normal modules.  rand_f (a random draw) gets no gradient."""

    def __init__(self, mesh, camera=(320.0, 320.0, 640 / 300, 640 / 300), right_hand=True, distinct=True):
        super().__init__()
        self.lbs = SparseSkinning(mesh, right_hand=right_hand, distinct=distinct)
        self.camera = None if camera is None else tuple(float(c) for c in camera)
        self.num_vertices = self.lbs.num_vertices
        faces = np.asarray(mesh['faces'], np.int64)
        self.faces = self.lbs.vertex_index[faces] if distinct else faces.copy()
        rest = np.asarray(mesh['vertices'], np.float32)[:, :3]
        if distinct:
            first = np.full(self.num_vertices, -1, np.int64)
            index = self.lbs.vertex_index
            first[index[::-1]] = np.arange(len(index))[::-1]          # the first mesh vertex of each row
            rest = rest[first]
        if right_hand:
            rest = rest * np.array([-1.0, 1.0, 1.0], np.float32)     # (mesh/pointTransformation.py:44-45)
        self.rest_vertices = np.ascontiguousarray(rest, np.float32)

    @staticmethod
    def pixel_camera(width, height):
        """(cx, cy, fx, fy) of the orthographic camera that maps the reference's 300 mm window onto width x height pixels
        (mesh/render.py:325 at 640 x 640, DepthRender's camera)."""
        return (width / 2, height / 2, width / 300, height / 300)

    def forward(self, transformation_mats, rand_f=None):
        return self.lbs(transformation_mats, self.camera, rand_f)

    def pose_vertices(self, hand_transformation_mat, parameters, rand_f=None):
        fk, lbs = hand_transformation_mat, self.lbs
        if not (parameters.is_cuda and parameters.dtype == torch.float32 and fk.offset.shape[0] == 17):
            return self.forward(fk(parameters), rand_f)
        return ops.PoseVertices.apply(parameters.contiguous(), fk.offset, fk.offset_inv, lbs.skin_vertex_start, lbs.skin_bone,
                                      lbs.skin_wv, lbs.right_hand, self.camera,
                                      None if rand_f is None else rand_f.detach().contiguous().float())


class KeypointPoseSolver(nn.Module):
    """The inverse of HandBallPrimitiveRender.pose_spheres: the hand's 41 keypoints (the hourglass's output, a previous
    frame, an annotation; the frame pose_spheres outputs: model millimetres, x negated for the right hand) -> the 26 pose
    parameters MeshVertices.pose_vertices and every mesh term take.  A REFINEMENT from a start pose: `iters`
    Levenberg-Marquardt iterations on sum_j w_j |k_j(p) - K_j|^2 + sum_i stiffness_i (p_i - params0_i)^2 by one HIP launch
    (ops.pose_ik; include/spherehand_hip.h has the iteration), one wave per crop.
        forward(keypoints[B,41,3 or 4], params0[B,26], weights=None) -> params[B,26], differentiable in `keypoints`
            (ops.PoseFromKeypoints: the implicit-function gradient in Gauss-Newton form, exact at zero residual)
        solve(keypoints, params0, weights=None) -> (params, cost0, cost)      no autograd
        jacobian(params[B,26]) -> (keypoints[B,41,4], jac[B,123,26])
        initial_pose(keypoints) -> [B,26]: a start from nothing, see there for what it is not.
    weights: [41] or [B,41], each >= 0; stiffness: [26], each >= 0 (a buffer).  From starts within 0.2 rad / 2 mm of
    the pose, exact keypoints are recovered in 8 iterations."""

    def __init__(self, mesh, right_hand=True, iters=12, lambda0=1e-3, stiffness=None):
        super().__init__()
        from .hand_model import sphere_model
        from .kinematicsTransformation import HandTransformationMat
        bones = mesh['bones'] if isinstance(mesh, dict) else mesh
        self.fk = HandTransformationMat([np.asarray(b['offset_matrix']).astype(np.float32) for b in bones])
        wv, _, bone = sphere_model(bones)
        self.register_buffer('kp_bone', torch.from_numpy(bone.astype(np.int32)))
        self.register_buffer('kp_wv', torch.from_numpy(np.ascontiguousarray(wv, np.float32)))
        self.register_buffer('stiffness', None if stiffness is None else
                             torch.as_tensor(np.asarray(stiffness, np.float32)).reshape(26).clone())
        self.right_hand = bool(right_hand)
        self.iters = int(iters)
        self.lambda0 = float(lambda0)
        self.num_keypoints = len(bone)

    def _args(self, keypoints, params0, weights):
        K = keypoints[..., :3].contiguous().float()
        weights = None if weights is None else weights.detach().contiguous().float()
        return K, params0.detach().contiguous().float(), weights

    def forward(self, keypoints, params0, weights=None):
        K, p0, weights = self._args(keypoints, params0, weights)
        return ops.PoseFromKeypoints.apply(K, p0, self.fk.offset, self.fk.offset_inv, self.kp_bone, self.kp_wv, self.right_hand,
                                           weights, self.stiffness, self.iters, self.lambda0)

    def solve(self, keypoints, params0, weights=None):
        K, p0, weights = self._args(keypoints, params0, weights)
        return ops.pose_ik(K.detach(), p0, self.fk.offset, self.fk.offset_inv, self.kp_bone, self.kp_wv, self.right_hand,
                           weights, self.stiffness, self.iters, self.lambda0)

    def jacobian(self, params):
        return ops.pose_keypoints_jacobian(params.detach().contiguous().float(), self.fk.offset, self.fk.offset_inv,
                                           self.kp_bone, self.kp_wv, self.right_hand)

    @torch.no_grad()
    def initial_pose(self, keypoints):
        """keypoints [B,41,3 or 4] -> a start pose [B,26] (the keypoints' dtype): the palm placed by the rigid alignment
        (Kabsch) of the palm bones' rest keypoints with the given ones, Euler angles read off for Rz Ry Rx (one of the
        equivalent triples; at cos(y) = 0 the one with z = 0), fingers at 0.  Plain torch, fp64 inside, any device; a
        helper, not a hot path.  It makes NO convergence promise: every finger bone carries two keypoints on its axis, so
        a finger has twisted poses with the same keypoints, and from this start 20 unconstrained iterations reached the
        exact keypoints in 74 % of 256 sampled poses (fp64 restatement); the rest sit in local minima.
        The solver is specified from a start near the pose: the previous frame, or a regressed one."""
        K = keypoints[..., :3].double()
        B = K.shape[0]
        sign = K.new_tensor([-1.0 if self.right_hand else 1.0, 1.0, 1.0])
        palm = self.kp_bone.to(K.device) < 2
        y = K[:, palm] * sign                                           # model frame
        q = self.kp_wv.to(K.device).double()[palm, :3].unsqueeze(0)
        qm, ym = q.mean(1, keepdim=True), y.mean(1, keepdim=True)
        H = (y - ym).transpose(1, 2) @ (q - qm)                          # sum (y - ym)(q - qm)^T
        U, _, Vh = torch.linalg.svd(H)
        d = torch.sign(torch.linalg.det(U @ Vh))
        D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=1))
        R = U @ D @ Vh
        t = (ym - qm @ R.transpose(1, 2)).squeeze(1)
        cy = torch.sqrt(R[:, 0, 0] ** 2 + R[:, 1, 0] ** 2)
        flat = cy < 1e-9
        ay = torch.atan2(-R[:, 2, 0], cy)
        az = torch.where(flat, torch.zeros_like(cy), torch.atan2(R[:, 1, 0], R[:, 0, 0]))
        ax = torch.where(flat, torch.atan2(-R[:, 1, 2], R[:, 1, 1]), torch.atan2(R[:, 2, 1], R[:, 2, 2]))
        p = K.new_zeros(B, 26)
        p[:, 0], p[:, 1], p[:, 2], p[:, 3:6] = ax, ay, az, t
        return p.to(keypoints.dtype)


class MeshPoseFitter(nn.Module):
    """The pose fitted to an observed depth image through the triangle mesh: `iters` Gauss-Newton / Levenberg-Marquardt
    iterations on sum dist^2 + sum_i stiffness_i (p_i - prior_i)^2, dist being MeshDataToModelLoss's distance of every
    observed point to its closest point on the mesh, saturated at max_dist (ops.pose_icp; include/spherehand_hip.h,
    shr_pose_icp_normal and shr_pose_lm_step, has the equations and the iteration).  Each iteration is one closest-point
    search, where a first-order step through MeshDataToModelLoss and MeshVertices.pose_vertices needs the same search for
    a far smaller gain.  A REFINEMENT from a start pose: the intended start is KeypointPoseSolver's pose from the
    network's keypoints, or the previous frame's pose.
        solve(observed[B,H,W], params0[B,26], prior=None) -> (params, cost0, cost)
        normal_equations(observed, params) -> (A [B,26,26], g [B,26], cost [B] fp64, count [B] int32)
    There is NO autograd through the solve: the observation is data, and nothing here is differentiable.
    pixel_to_model, fg_max, max_dist: MeshDataToModelLoss's.  stiffness: [26], each >= 0 (a buffer); prior: [B,26], default
    the start pose.  One depth view does not determine an occluded finger: without stiffness the matrix of such a crop
    is singular up to rounding and the damping alone bounds the step (DESIGN.md 4.4n has what was measured)."""

    def __init__(self, mesh, width, height, pixel_to_model=None, right_hand=True, iters=10, lambda0=1e-3, stiffness=None,
                 fg_max=MeshDataToModelLoss.REFERENCE_FG_MAX, max_dist=50.0):
        super().__init__()
        from .kinematicsTransformation import HandTransformationMat
        self.vertices = MeshVertices(mesh, camera=None, right_hand=right_hand, distinct=True)
        self.fk = HandTransformationMat([np.asarray(b['offset_matrix']).astype(np.float32) for b in mesh['bones']])
        self.register_buffer('faces_i32', torch.from_numpy(np.ascontiguousarray(self.vertices.faces, np.int32)))
        self.register_buffer('stiffness', None if stiffness is None else
                             torch.as_tensor(np.asarray(stiffness, np.float32)).reshape(26).clone())
        self.width, self.height = int(width), int(height)
        p2m = MeshDataToModelLoss.reference_grid(width, height) if pixel_to_model is None else pixel_to_model
        self.pixel_to_model = tuple(float(t) for t in p2m)
        self.right_hand = bool(right_hand)
        self.iters = int(iters)
        self.lambda0 = float(lambda0)
        self.fg_max = float(fg_max)
        self.max_dist = float(max_dist)

    def _observed(self, observed):
        if observed.dim() != 3 or tuple(observed.shape[1:]) != (self.height, self.width):
            raise RuntimeError("MeshPoseFitter takes observed [B,%d,%d]" % (self.height, self.width))
        return observed.detach().contiguous().float()

    @torch.no_grad()
    def solve(self, observed, params0, prior=None):
        lbs = self.vertices.lbs
        return ops.pose_icp(self._observed(observed), params0.detach().contiguous().float(), self.faces_i32, self.fk.offset,
                            self.fk.offset_inv, lbs.skin_vertex_start, lbs.skin_bone, lbs.skin_wv, self.right_hand,
                            self.pixel_to_model, self.fg_max, self.max_dist, self.iters, self.lambda0, self.stiffness,
                            None if prior is None else prior.detach().contiguous().float())

    @torch.no_grad()
    def normal_equations(self, observed, params):
        lbs = self.vertices.lbs
        observed, params = self._observed(observed), params.detach().contiguous().float()
        verts = self.vertices.pose_vertices(self.fk, params)
        dist, face = ops.mesh_data_to_model(observed, verts, self.faces_i32, self.pixel_to_model, self.fg_max, self.max_dist)
        return ops.pose_icp_normal(observed, verts, self.faces_i32, dist, face, params, self.fk.offset, self.fk.offset_inv,
                                   lbs.skin_vertex_start, lbs.skin_bone, lbs.skin_wv, self.right_hand, self.pixel_to_model,
                                   self.fg_max, self.max_dist)


class MultiViewMeshPoseFitter(MeshPoseFitter):
    """MeshPoseFitter on several depth views of every sample: ONE pose in the model frame fitted to V observed depth
    images, each iteration one Levenberg-Marquardt step on the sum of all views' point-to-mesh costs (ops.pose_icp_views;
    include/spherehand_hip.h, shr_pose_icp_normal_views).  view [B,V,4,4] is rigid and maps the model frame to view v's
    frame, x_v = R x + t; its rotation is NOT checked to be orthonormal.  All views share width, height, pixel_to_model,
    fg_max and max_dist; a missing camera is an all-background image and adds nothing.
        solve(observed[B,V,H,W], view[B,V,4,4], params0[B,26], prior=None) -> (params, cost0, cost)
        normal_equations(observed, view, params) -> (A [B,26,26], g [B,26], cost [B] fp64, count [B] int32)
        views_from_cameras(camera_poses, inv_camera_poses, ref=0) -> view [B,V,4,4]
    A REFINEMENT from a start pose, as MeshPoseFitter: the intended start is KeypointPoseSolver's pose, or the pose of the
    previous frame.  There is NO autograd through the solve.  What further views buy -- the fingers one view hides, and the
    bone origins a single view cannot move -- is measured in DESIGN.md 4.4o; two views can still end in a wrong basin."""

    def _observed(self, observed):
        if observed.dim() != 4 or tuple(observed.shape[2:]) != (self.height, self.width):
            raise RuntimeError("MultiViewMeshPoseFitter takes observed [B,V,%d,%d]" % (self.height, self.width))
        return observed.detach().contiguous().float()

    @staticmethod
    def views_from_cameras(camera_poses, inv_camera_poses, ref=0):
        """camera_poses, inv_camera_poses [B,V,4,4] as MutualTransformation takes them -> view [B,V,4,4] =
        inv_camera_poses[:, v] @ camera_poses[:, ref], its (ref, v) entry: the pose then lives in camera ref's frame.  Plain
        torch, any device; a helper, not a hot path."""
        if camera_poses.dim() != 4 or camera_poses.shape != inv_camera_poses.shape or tuple(camera_poses.shape[2:]) != (4, 4):
            raise RuntimeError("camera_poses and inv_camera_poses must be [B,V,4,4]")
        return torch.matmul(inv_camera_poses, camera_poses[:, ref].unsqueeze(1)).contiguous()

    @torch.no_grad()
    def solve(self, observed, view, params0, prior=None):
        lbs = self.vertices.lbs
        return ops.pose_icp_views(self._observed(observed), view.detach().contiguous().float(),
                                  params0.detach().contiguous().float(), self.faces_i32, self.fk.offset, self.fk.offset_inv,
                                  lbs.skin_vertex_start, lbs.skin_bone, lbs.skin_wv, self.right_hand, self.pixel_to_model,
                                  self.fg_max, self.max_dist, self.iters, self.lambda0, self.stiffness,
                                  None if prior is None else prior.detach().contiguous().float())

    @torch.no_grad()
    def normal_equations(self, observed, view, params):
        lbs = self.vertices.lbs
        observed, params = self._observed(observed), params.detach().contiguous().float()
        view = view.detach().contiguous().float()
        B, V, H, W = observed.shape
        vverts = ops.view_vertices(self.vertices.pose_vertices(self.fk, params), view)
        dist, face = ops.mesh_data_to_model(observed.view(B * V, H, W), vverts.view(B * V, vverts.shape[2], 4), self.faces_i32,
                                            self.pixel_to_model, self.fg_max, self.max_dist)
        return ops.pose_icp_normal_views(observed, vverts, self.faces_i32, dist.view(B, V, H, W), face.view(B, V, H, W), view,
                                         params, self.fk.offset, self.fk.offset_inv, lbs.skin_vertex_start, lbs.skin_bone,
                                         lbs.skin_wv, self.right_hand, self.pixel_to_model, self.fg_max, self.max_dist)


class SpherePoseFitter(nn.Module):
    """The pose fitted to observed depth through the SPHERE model, the 41 spheres HandBallPrimitiveRender hangs on the
    pose: `iters` Gauss-Newton / Levenberg-Marquardt iterations on sum dist^2 + sum_i stiffness_i (p_i - prior_i)^2, dist
    being DataToModelLoss's distance min_j | |p - c_j| - r_j | of every observed point, saturated at max_dist, summed over
    V views (ops.sphere_icp; include/spherehand_hip.h, shr_sphere_icp_normal and shr_pose_lm_step, has the equations and
    the iteration).  A point meets 41 spheres where the mesh fit's search meets 3 382 faces: search and row are one launch.
        solve(observed, params0, view=None, prior=None) -> (params, cost0, cost)
        normal_equations(observed, params, view=None) -> (A [B,26,26], g [B,26], cost [B] fp64, count [B] int32,
                                                          moments [B,41,12] fp64: per sphere sum u u^T, sum d u, sum d^2, rows)
        uncertainty(observed, params, <normal_equations' further arguments>, residual_var=1.0)
            -> (cov [B,26,26], sphere_cov [B,41,3,3], sigma [B,41] mm, ok [S]); inherited by every fitter below
        views_from_cameras(camera_poses, inv_camera_poses, ref=0) -> view [B,V,4,4]   (MultiViewMeshPoseFitter's)
    observed is [B,V,H,W] with view [B,V,4,4] rigid (x_v = R x + t; its rotation is NOT checked to be orthonormal), or
    [B,H,W] with view=None: one view, the identity.  A REFINEMENT from a start pose: the intended start is
    KeypointPoseSolver's pose from the network's keypoints, or the previous frame's pose; it can end in a wrong basin.
    There is NO autograd through the solve.  stiffness: [26], each >= 0 (a buffer); prior: [B,26], default the start pose.
    The observation must be one the SPHERE model explains: the shipped radii are a fat proxy of the shipped mesh, and on a
    mesh-rendered observation this fit moves the pose away from the mesh's (DESIGN.md 4.4p has the figures).  Handing its
    result to MeshPoseFitter on the same observation is not supported."""

    def __init__(self, mesh, width, height, pixel_to_model=None, right_hand=True, iters=10, lambda0=1e-3, stiffness=None,
                 fg_max=MeshDataToModelLoss.REFERENCE_FG_MAX, max_dist=50.0):
        super().__init__()
        from .hand_model import sphere_model
        from .kinematicsTransformation import HandTransformationMat
        bones = mesh['bones'] if isinstance(mesh, dict) else mesh
        self.fk = HandTransformationMat([np.asarray(b['offset_matrix']).astype(np.float32) for b in bones])
        wv, radii, bone = sphere_model(bones)
        self.register_buffer('kp_bone', torch.from_numpy(bone.astype(np.int32)))
        self.register_buffer('kp_wv', torch.from_numpy(np.ascontiguousarray(wv, np.float32)))
        self.register_buffer('radii', torch.from_numpy(np.ascontiguousarray(radii, np.float32)))
        self.register_buffer('stiffness', None if stiffness is None else
                             torch.as_tensor(np.asarray(stiffness, np.float32)).reshape(26).clone())
        self.width, self.height = int(width), int(height)
        p2m = MeshDataToModelLoss.reference_grid(width, height) if pixel_to_model is None else pixel_to_model
        self.pixel_to_model = tuple(float(t) for t in p2m)
        self.right_hand = bool(right_hand)
        self.iters = int(iters)
        self.lambda0 = float(lambda0)
        self.fg_max = float(fg_max)
        self.max_dist = float(max_dist)
        self.num_spheres = len(bone)

    views_from_cameras = staticmethod(MultiViewMeshPoseFitter.views_from_cameras)

    def _observed(self, observed, view):
        if view is None:
            if observed.dim() != 3:
                raise RuntimeError("SpherePoseFitter takes observed [B,%d,%d] without a view" % (self.height, self.width))
            observed = observed.unsqueeze(1)
            view = torch.eye(4, dtype=torch.float32, device=observed.device).expand(observed.shape[0], 1, 4, 4)
        if observed.dim() != 4 or tuple(observed.shape[2:]) != (self.height, self.width):
            raise RuntimeError("SpherePoseFitter takes observed [B,V,%d,%d] with view [B,V,4,4]" % (self.height, self.width))
        return observed.detach().contiguous().float(), view.detach().contiguous().float()

    @torch.no_grad()
    def solve(self, observed, params0, view=None, prior=None):
        observed, view = self._observed(observed, view)
        return ops.sphere_icp(observed, view, params0.detach().contiguous().float(), self.fk.offset, self.fk.offset_inv,
                              self.kp_bone, self.kp_wv, self.radii, self.right_hand, self.pixel_to_model, self.fg_max,
                              self.max_dist, self.iters, self.lambda0, self.stiffness,
                              None if prior is None else prior.detach().contiguous().float())

    @torch.no_grad()
    def normal_equations(self, observed, params, view=None):
        observed, view = self._observed(observed, view)
        return ops.sphere_icp_normal(observed, view, params.detach().contiguous().float(), self.fk.offset, self.fk.offset_inv,
                                     self.kp_bone, self.kp_wv, self.radii, self.right_hand, self.pixel_to_model, self.fg_max,
                                     self.max_dist)

    @staticmethod
    def _bands(equations):
        """(E, F) of what this class's normal_equations returns: the frame fitters have neither"""
        return None, None

    @torch.no_grad()
    def uncertainty(self, observed, params, *args, residual_var=1.0, **kwargs):
        """How well the images determine the pose `params` [B,26]: the class's own normal_equations(observed, params, ...)
        evaluated there (the further arguments are that method's), and from its A -- and E and F where the class has them --
        the marginal covariance of every frame (ops.pose_lm_covariance; include/spherehand_hip.h,
        shr_pose_lm_seq2_covariance) with the fitter's stiffness as the prior's information and its seq_len (1 for the
        frame fitters) -> (cov [B,26,26] fp64, sphere_cov [B,J,3,3] fp64 in the MODEL frame, mm^2, sigma [B,J] fp64 =
        sqrt(trace sphere_cov), mm, ok [S] bool: False where a sequence's matrix is not positive definite, its frames NaN).
        It is the Gauss-Newton (Laplace) covariance AT THE GIVEN POSE per unit of residual variance, times residual_var,
        which is the caller's to estimate.  It is NOT a bound on the error: saturated rows contribute nothing, so a term cut
        by max_dist, max_resid, kp_max, ts_max or acc_max is silent here as well; it says nothing about another basin (a
        finger the view hides has a large sigma and can still be further off than it); without a stiffness a direction the
        images leave free makes the matrix singular.  NO autograd through it."""
        equations = self.normal_equations(observed, params, *args, **kwargs)
        E, F = self._bands(equations)
        params = params.detach().contiguous().float()
        jac = ops.pose_keypoints_jacobian(params, self.fk.offset, self.fk.offset_inv, self.kp_bone, self.kp_wv, self.right_hand)[1]
        cov, sphere_cov, status = ops.pose_lm_covariance(equations[0], E, F, getattr(self, 'seq_len', 1), self.stiffness, jac)
        cov, sphere_cov = cov * float(residual_var), sphere_cov * float(residual_var)
        sigma = (sphere_cov[..., 0, 0] + sphere_cov[..., 1, 1] + sphere_cov[..., 2, 2]).sqrt()
        return cov, sphere_cov, sigma, status == 0


class SphereRenderPoseFitter(SpherePoseFitter):
    """SpherePoseFitter with the reference's other term (mesh/multiview_utility.py:96-129 fits MSELoss(render, observed)
    beside DataToModelLoss): `iters` Levenberg-Marquardt iterations on
        sum dist^2 + render_weight sum min(|D - O'|, max_resid)^2 + sum_i stiffness_i (p_i - prior_i)^2,
    D the sphere model's rendered depth (shr_sphere_raster_fwd's rule; `background` where no sphere is hit) and O' the
    observation with its background set to `background`, over every pixel of every view (ops.sphere_icp_render;
    include/spherehand_hip.h, shr_sphere_render_normal).  The data-to-model distance alone is blind to a sphere that lies
    over observed background or in front of the observed surface: no observed point is nearest to it, so nothing but the
    stiffness holds it.  Here every model pixel is a row.  The row's derivative holds the owner and the silhouette fixed,
    as ops.SphereDepthRaster's backward does.
        solve(observed, params0, view=None, prior=None) -> (params, cost0, cost)
        normal_equations(observed, params, view=None) -> (A, g, cost, count, moments) of the SUM of the two terms' A, g and
                                                          cost; count and moments are the render term's own
    render_weight = 0 is SpherePoseFitter bit for bit.  The defaults are the best row of DESIGN.md 4.4q's study.  Everything
    else, the limits included, is SpherePoseFitter's: a refinement from a start pose, NO autograd through the solve, the
    rotation NOT checked."""

    # the study's best row
    DEFAULT_RENDER_WEIGHT = 1.0
    DEFAULT_MAX_RESID = 10.0

    def __init__(self, mesh, width, height, pixel_to_model=None, right_hand=True, iters=10, lambda0=1e-3, stiffness=None,
                 fg_max=MeshDataToModelLoss.REFERENCE_FG_MAX, max_dist=50.0, render_weight=None, max_resid=None,
                 background=100.0):
        super().__init__(mesh, width, height, pixel_to_model, right_hand, iters, lambda0, stiffness, fg_max, max_dist)
        self.render_weight = float(self.DEFAULT_RENDER_WEIGHT if render_weight is None else render_weight)
        self.max_resid = float(self.DEFAULT_MAX_RESID if max_resid is None else max_resid)
        self.background = float(background)
        if not (self.render_weight >= 0.0 and self.render_weight < float("inf")) or not self.max_resid >= 0.0 or \
                not abs(self.background) < float("inf"):
            raise ValueError("render_weight must be finite and >= 0, max_resid >= 0 and background finite")

    def _tables(self):
        return self.fk.offset, self.fk.offset_inv, self.kp_bone, self.kp_wv, self.radii

    @torch.no_grad()
    def solve(self, observed, params0, view=None, prior=None):
        observed, view = self._observed(observed, view)
        return ops.sphere_icp_render(observed, view, params0.detach().contiguous().float(), *self._tables(), self.right_hand,
                                     self.pixel_to_model, self.fg_max, self.max_dist, self.iters, self.lambda0, self.stiffness,
                                     None if prior is None else prior.detach().contiguous().float(), self.render_weight,
                                     self.max_resid, self.background)

    @torch.no_grad()
    def normal_equations(self, observed, params, view=None):
        observed, view = self._observed(observed, view)
        params = params.detach().contiguous().float()
        A, g, cost = ops.sphere_icp_normal(observed, view, params, *self._tables(), self.right_hand, self.pixel_to_model,
                                           self.fg_max, self.max_dist)[:3]
        return ops.sphere_render_normal(observed, view, params, *self._tables(), self.right_hand, self.pixel_to_model,
                                        self.fg_max, self.max_resid, self.background, self.render_weight, (A, g, cost))


class SpherePriorPoseFitter(SphereRenderPoseFitter):
    """SphereRenderPoseFitter with the two terms a sphere-model tracker carries beside its image terms: `iters`
    Levenberg-Marquardt iterations on
        SphereRenderPoseFitter's energy + kp_weight sum w min(|k - c|, kp_max)^2 + limit_weight sum_i h_i^2,
    k the keypoints the network predicts per view (they ARE the sphere centres), w their confidence, c the sphere centres
    in the view's frame, and h_i the distance of pose parameter i beyond `limits` (ops.sphere_icp_priors;
    include/spherehand_hip.h, shr_sphere_prior_normal).  One depth view does not determine the pose: a finger the view
    hides is held by the stiffness alone, and nothing else keeps a flex inside the range a hand can take.
        solve(observed, params0, view=None, prior=None, keypoints=None, confidence=None) -> (params, cost0, cost)
        normal_equations(observed, params, view=None, keypoints=None, confidence=None)
            -> (A, g, cost, count [B,2], moments) of the SUM of the four terms' A, g and cost; count (pairs with rows, limit
               rows) and moments are the new terms' own
    keypoints is [B,V,41,3] in each view's frame -- what the network and Hand3DHeatmapRender.inv_camera give per view --
    or [B,41,3] with view=None; confidence [B,V,41] (or [B,41]) >= 0, None: 1.  A NaN keypoint or a confidence of 0 drops
    the pair.  limits = (lower [26], upper [26]), default joint_angle.pose_limits(): the support of the reference's pose
    distribution on the 20 finger parameters, the palm free; limits=False: no limit term.  Without keypoints and with
    limit_weight = 0 it is SphereRenderPoseFitter bit for bit.  The defaults are the best row of DESIGN.md 4.4r's study;
    the same section says what the terms do NOT fix: with the keypoints themselves wrong by more than kp_max the anchor
    is silent, and a limit is no substitute for an observation.  Collision between spheres is NOT a term here.  Everything
    else is SphereRenderPoseFitter's: a refinement from a start pose, NO autograd through the solve, the rotation
    NOT checked."""

    # the study's best `noise`, one-view row at sigma_k = 5 mm
    DEFAULT_KP_WEIGHT = 0.1
    DEFAULT_KP_MAX = float("inf")
    DEFAULT_LIMIT_WEIGHT = 1e4

    def __init__(self, mesh, width, height, pixel_to_model=None, right_hand=True, iters=10, lambda0=1e-3, stiffness=None,
                 fg_max=MeshDataToModelLoss.REFERENCE_FG_MAX, max_dist=50.0, render_weight=None, max_resid=None,
                 background=100.0, kp_weight=None, kp_max=None, limit_weight=None, limits=None):
        super().__init__(mesh, width, height, pixel_to_model, right_hand, iters, lambda0, stiffness, fg_max, max_dist,
                         render_weight, max_resid, background)
        self.kp_weight = float(self.DEFAULT_KP_WEIGHT if kp_weight is None else kp_weight)
        self.kp_max = float(self.DEFAULT_KP_MAX if kp_max is None else kp_max)
        self.limit_weight = float(self.DEFAULT_LIMIT_WEIGHT if limit_weight is None else limit_weight)
        if not (self.kp_weight >= 0.0 and self.kp_weight < float("inf")) or not self.kp_max >= 0.0 or \
                not (self.limit_weight >= 0.0 and self.limit_weight < float("inf")):
            raise ValueError("kp_weight and limit_weight must be finite and >= 0, kp_max >= 0")
        if limits is None:
            from .joint_angle import pose_limits
            limits = pose_limits()
        if limits is False:
            lower = upper = None
        else:
            lower, upper = (torch.as_tensor(np.asarray(t, np.float32)).reshape(26).clone() for t in limits)
        self.register_buffer('lower', lower)
        self.register_buffer('upper', upper)

    def _targets(self, observed, view, keypoints, confidence):
        single = view is None
        observed, view = self._observed(observed, view)
        if keypoints is not None:
            keypoints = keypoints.detach().float()
            keypoints = (keypoints.unsqueeze(1) if single and keypoints.dim() == 3 else keypoints).contiguous()
        if confidence is not None:
            confidence = confidence.detach().float()
            confidence = (confidence.unsqueeze(1) if single and confidence.dim() == 2 else confidence).contiguous()
        limits = None if self.lower is None else (self.lower, self.upper)
        return observed, view, keypoints, confidence, limits

    @torch.no_grad()
    def solve(self, observed, params0, view=None, prior=None, keypoints=None, confidence=None):
        observed, view, keypoints, confidence, limits = self._targets(observed, view, keypoints, confidence)
        return ops.sphere_icp_priors(observed, view, params0.detach().contiguous().float(), *self._tables(), self.right_hand,
                                     self.pixel_to_model, self.fg_max, self.max_dist, self.iters, self.lambda0, self.stiffness,
                                     None if prior is None else prior.detach().contiguous().float(), self.render_weight,
                                     self.max_resid, self.background, keypoints, confidence, self.kp_weight, self.kp_max,
                                     limits, self.limit_weight)

    @torch.no_grad()
    def normal_equations(self, observed, params, view=None, keypoints=None, confidence=None):
        observed, view, keypoints, confidence, limits = self._targets(observed, view, keypoints, confidence)
        params = params.detach().contiguous().float()
        A, g, cost = SphereRenderPoseFitter.normal_equations(self, observed, params, view)[:3]
        return ops.sphere_prior_normal(view, params, *self._tables()[:4], self.right_hand, keypoints, confidence,
                                       self.kp_weight, self.kp_max, limits, self.limit_weight, (A, g, cost))


class PoseVaePrior(nn.Module):
    """The frozen pose VAE as a Gauss-Newton term of the sphere fit (include/spherehand_hip.h, shr_pose_vae_normal):
        weight (sum_i r_i^2 + latent_weight sum_k mu_k^2),  r = c - 100 recon(c / 100) in mm
    over the 41 model-frame sphere centres c, mu the network's latent mean (z = mu: no draw, no logvar term).  The
    reference's PoseVae behind --prior (network/pose_vae.py:11-99) is a first-order training term; here its exact Jacobian
    enters the normal equations.  Holds the packed network (pose_vae.pack_fit_weights) as a buffer; hand it to a fitter as
    `pose_prior=`.  weight None: DEFAULT_WEIGHT, DESIGN.md 4.4zzz's.  What the term does NOT give: the network saw the global
    pose in training, so r is not invariant under a translation of the hand (DESIGN.md 4.4zzz has the figures), and r of a
    plausible pose is not zero (rms 5.8 mm on the sampler's poses): it is a loose prior, no observation."""

    # no row of the study helps the hidden finger, and every weight from 0.1 on costs the well-observed
    # frames, so the default is the reference's ratio of its prior weight (1e-2) to its data weight (mv_projection, 1)
    DEFAULT_WEIGHT = 1e-2

    def __init__(self, weights=None, weight=None, latent_weight=0.0):
        super().__init__()
        from . import pose_vae
        self.weight = float(self.DEFAULT_WEIGHT if weight is None else weight)
        self.latent_weight = float(latent_weight)
        if not (self.weight >= 0.0 and self.weight < float("inf")) or \
                not (self.latent_weight >= 0.0 and self.latent_weight < float("inf")):
            raise ValueError("weight and latent_weight must be finite and >= 0")
        module = pose_vae.PoseVae(41 * 3, 32, model_path=pose_vae.DEFAULT_WEIGHTS if weights is None else weights)
        self.register_buffer('blob', pose_vae.pack_fit_weights(module))

    def term(self):
        """(blob, weight, latent_weight): the loops' pose_prior argument."""
        return self.blob, self.weight, self.latent_weight


class SphereCollisionPoseFitter(SpherePriorPoseFitter):
    """SpherePriorPoseFitter with the term a sphere-model tracker carries against self-penetration: `iters`
    Levenberg-Marquardt iterations on
        SpherePriorPoseFitter's energy + collision_weight sum_k max(m_k - |c_a - c_b|, 0)^2
    over the reference's 690 sphere pairs (mesh/render.py:145-176; every finger sphere against the palm's and against the
    other fingers'), c the sphere centres in the model frame and m_k the pair's minimum distance in mm
    (ops.sphere_icp_priors with `collision`; include/spherehand_hip.h, shr_sphere_collision_normal).  The table is
    hand_model.collision_table(mesh, min_dist, radius_scale): m_k = min_dist, the reference's constant 6 mm, or with
    radius_scale m_k = min(radius_scale (r_a + r_b), the pair's distance at the rest pose) -- the shipped radii are a fat
    proxy, so the plain radius sum is already violated at rest.
        solve(observed, params0, view=None, prior=None, keypoints=None, confidence=None) -> (params, cost0, cost)
        normal_equations(observed, params, view=None, keypoints=None, confidence=None)
            -> (A, g, cost, count [B], penetration [B,690]) of the SUM of the five terms' A, g and cost; count (pairs with
               rows) and penetration (h at an active pair, 0 elsewhere) are the new term's own
    collision_weight = 0 is SpherePriorPoseFitter bit for bit.  The defaults come from DESIGN.md 4.4s's study, which also
    says what the term does NOT fix: it keeps centres apart, not surfaces, it pushes along the line between two centres
    whatever the image says, and poses the sampler itself produces have pairs under 6 mm.  Everything else is
    SpherePriorPoseFitter's: a refinement from a start pose, NO autograd through the solve, the rotation NOT checked."""

    # the study's row
    DEFAULT_COLLISION_WEIGHT = 1.0
    DEFAULT_MIN_DIST = 6.0
    DEFAULT_RADIUS_SCALE = None

    def __init__(self, mesh, width, height, pixel_to_model=None, right_hand=True, iters=10, lambda0=1e-3, stiffness=None,
                 fg_max=MeshDataToModelLoss.REFERENCE_FG_MAX, max_dist=50.0, render_weight=None, max_resid=None,
                 background=100.0, kp_weight=None, kp_max=None, limit_weight=None, limits=None, collision_weight=None,
                 min_dist=None, radius_scale=None, *, pose_prior=None):
        super().__init__(mesh, width, height, pixel_to_model, right_hand, iters, lambda0, stiffness, fg_max, max_dist,
                         render_weight, max_resid, background, kp_weight, kp_max, limit_weight, limits)
        from .hand_model import collision_table
        if pose_prior is not None and not isinstance(pose_prior, PoseVaePrior):
            raise ValueError("pose_prior must be a PoseVaePrior or None")
        self.pose_prior = pose_prior                           # (a submodule: it moves with the fitter)
        self.collision_weight = float(self.DEFAULT_COLLISION_WEIGHT if collision_weight is None else collision_weight)
        if not (self.collision_weight >= 0.0 and self.collision_weight < float("inf")):
            raise ValueError("collision_weight must be finite and >= 0")
        self.min_dist = float(self.DEFAULT_MIN_DIST if min_dist is None else min_dist)
        self.radius_scale = self.DEFAULT_RADIUS_SCALE if radius_scale is None else float(radius_scale)
        a, b, m = collision_table(mesh, self.min_dist, self.radius_scale)
        self.register_buffer('pair_a', torch.from_numpy(a))
        self.register_buffer('pair_b', torch.from_numpy(b))
        self.register_buffer('pair_min', torch.from_numpy(m))

    def _pairs(self):
        return self.pair_a, self.pair_b, self.pair_min

    def _pose_prior(self):
        """The loops' pose_prior: (blob, weight, latent_weight), or None without a weighted prior."""
        return None if self.pose_prior is None or self.pose_prior.weight == 0.0 else self.pose_prior.term()

    @torch.no_grad()
    def solve(self, observed, params0, view=None, prior=None, keypoints=None, confidence=None):
        observed, view, keypoints, confidence, limits = self._targets(observed, view, keypoints, confidence)
        return ops.sphere_icp_priors(observed, view, params0.detach().contiguous().float(), *self._tables(), self.right_hand,
                                     self.pixel_to_model, self.fg_max, self.max_dist, self.iters, self.lambda0, self.stiffness,
                                     None if prior is None else prior.detach().contiguous().float(), self.render_weight,
                                     self.max_resid, self.background, keypoints, confidence, self.kp_weight, self.kp_max,
                                     limits, self.limit_weight, collision=self._pairs(), collision_weight=self.collision_weight,
                                     pose_prior=self._pose_prior())

    @torch.no_grad()
    def normal_equations(self, observed, params, view=None, keypoints=None, confidence=None):
        params = params.detach().contiguous().float()
        A, g, cost = SpherePriorPoseFitter.normal_equations(self, observed, params, view, keypoints, confidence)[:3]
        out = ops.sphere_collision_normal(params, *self._tables()[:4], self.right_hand, self._pairs(), self.collision_weight,
                                          (A, g, cost))
        term = self._pose_prior()
        if term is not None:                                   # added in place: `out` holds the same A, g and cost
            ops.pose_vae_normal(params, *self._tables()[:4], self.right_hand, *term, accumulate_into=(A, g, cost))
        return out


class SphereSequencePoseFitter(SphereCollisionPoseFitter):
    """SphereCollisionPoseFitter over SEQUENCES of seq_len consecutive frames fitted jointly: the batch's B = S seq_len
    frames are S sequences, the frames of one adjacent, and the energy of a sequence is
        the sum over its frames of SphereCollisionPoseFitter's energy
        + temporal_weight sum_t frame_weight[t] sum_j min(|c_j(t + 1) - c_j(t)|, ts_max)^2,
    c the sphere centres in the model frame (ops.sphere_icp_sequence; include/spherehand_hip.h,
    shr_sphere_temporal_normal and shr_pose_lm_seq_step).  The term is the reference's TemporalSmoothnessLoss
    (network/util_modules.py:360-381) as Gauss-Newton rows; it couples frame t and t + 1, so the normal equations of a
    sequence are block-tridiagonal and lambda, the cost and the accept decision belong to the sequence.  Unlike the
    reference, which detaches the previous frame, the term pulls BOTH frames of a pair.
        solve(observed, params0, view=None, prior=None, keypoints=None, confidence=None, frame_weight=None)
            -> (params [B,26], cost0 [S], cost [S])
        normal_equations(observed, params, view=None, keypoints=None, confidence=None, frame_weight=None)
            -> (A, g, E, cost, count [B]) of the SUM of the six terms' A, g and cost; E [B,26,26] (frame t's rows, frame
               t + 1's columns) and count (the spheres with rows of the pair ending at the frame) are the new term's own
    frame_weight [B] >= 0 weighs the pair (t, t + 1) at t (None: 1): 0 cuts a sequence at a scene change.  With
    seq_len = 1 it is SphereCollisionPoseFitter bit for bit.  The defaults come from DESIGN.md 4.4t's study, which also
    says what the term does NOT fix: it penalises motion itself, so it lags a hand that really moves, and one rejected
    frame rejects its whole sequence.  Everything else is SphereCollisionPoseFitter's: a refinement from a start pose,
    NO autograd through the solve, the rotation NOT checked."""

    # the study's row
    DEFAULT_TEMPORAL_WEIGHT = 0.1
    DEFAULT_TS_MAX = float("inf")

    def __init__(self, mesh, width, height, seq_len, pixel_to_model=None, right_hand=True, iters=10, lambda0=1e-3,
                 stiffness=None, fg_max=MeshDataToModelLoss.REFERENCE_FG_MAX, max_dist=50.0, render_weight=None,
                 max_resid=None, background=100.0, kp_weight=None, kp_max=None, limit_weight=None, limits=None,
                 collision_weight=None, min_dist=None, radius_scale=None, temporal_weight=None, ts_max=None, *,
                 pose_prior=None):
        super().__init__(mesh, width, height, pixel_to_model, right_hand, iters, lambda0, stiffness, fg_max, max_dist,
                         render_weight, max_resid, background, kp_weight, kp_max, limit_weight, limits, collision_weight,
                         min_dist, radius_scale, pose_prior=pose_prior)
        self.seq_len = int(seq_len)
        self.temporal_weight = float(self.DEFAULT_TEMPORAL_WEIGHT if temporal_weight is None else temporal_weight)
        self.ts_max = float(self.DEFAULT_TS_MAX if ts_max is None else ts_max)
        if self.seq_len < 1 or not (self.temporal_weight >= 0.0 and self.temporal_weight < float("inf")) or \
                not self.ts_max >= 0.0:
            raise ValueError("seq_len must be >= 1, temporal_weight finite and >= 0, ts_max >= 0")

    @staticmethod
    def _frame_weight(frame_weight):
        return None if frame_weight is None else frame_weight.detach().contiguous().float()

    @torch.no_grad()
    def solve(self, observed, params0, view=None, prior=None, keypoints=None, confidence=None, frame_weight=None):
        observed, view, keypoints, confidence, limits = self._targets(observed, view, keypoints, confidence)
        return ops.sphere_icp_sequence(observed, view, params0.detach().contiguous().float(), *self._tables(), self.seq_len,
                                       self.right_hand, self.pixel_to_model, self.fg_max, self.max_dist, self.iters,
                                       self.lambda0, self.stiffness,
                                       None if prior is None else prior.detach().contiguous().float(), self.render_weight,
                                       self.max_resid, self.background, keypoints, confidence, self.kp_weight, self.kp_max,
                                       limits, self.limit_weight, self._pairs(), self.collision_weight, self.temporal_weight,
                                       self.ts_max, self._frame_weight(frame_weight), pose_prior=self._pose_prior())

    @torch.no_grad()
    def normal_equations(self, observed, params, view=None, keypoints=None, confidence=None, frame_weight=None):
        params = params.detach().contiguous().float()
        A, g, cost = SphereCollisionPoseFitter.normal_equations(self, observed, params, view, keypoints, confidence)[:3]
        return ops.sphere_temporal_normal(params, *self._tables()[:4], self.seq_len, self.right_hand, self.temporal_weight,
                                          self.ts_max, self._frame_weight(frame_weight), (A, g, cost))

    @staticmethod
    def _bands(equations):
        return equations[2], None


class SphereTrajectoryPoseFitter(SphereSequencePoseFitter):
    """SphereSequencePoseFitter with a constant-velocity term: the energy of a sequence gains
        accel_weight sum_k triple_weight[k] sum_j min(|c_j(k - 1) - 2 c_j(k) + c_j(k + 1)|, acc_max)^2
    over its triples of consecutive frames (ops.sphere_icp_trajectory; include/spherehand_hip.h, shr_sphere_accel_normal
    and shr_pose_lm_seq2_step).  The second difference is zero on a hand that moves steadily, where the first difference
    of SphereSequencePoseFitter penalises motion itself; the energy is of the family of network/util_modules.py:349-381, the
    reference has no counterpart of the term.  A row couples three frames, so the normal equations of a sequence are
    block-pentadiagonal.
        solve(observed, params0, view=None, prior=None, keypoints=None, confidence=None, frame_weight=None,
              triple_weight=None) -> (params [B,26], cost0 [S], cost [S])
        normal_equations(observed, params, view=None, keypoints=None, confidence=None, frame_weight=None,
                         triple_weight=None)
            -> (A, g, E, F, cost, count [B]) of the SUM of the seven terms' A, g, cost and E; F [B,26,26] (frame t's rows,
               frame t + 2's columns) and count (the spheres with rows of the triple ending at the frame) are the new
               term's own
    triple_weight [B] >= 0 weighs the triple centred at k (None: 1): 0 at the two frames around a scene change cuts the
    sequence there.  With accel_weight = 0 (or seq_len < 3) it is SphereSequencePoseFitter bit for bit.  The defaults
    (accel_weight 0.1, acc_max 20 mm, temporal_weight 0: the first-difference term is OFF) come from DESIGN.md 4.4u's
    study on three sequences of eight frames: that row is the only one at or below the frame-by-frame fit's keypoint error
    on steady motion (0.40 against 0.44 mm, jitter 0.49 against 0.73 mm) and stays beside it where the motion turns (0.45
    against 0.41 mm), where SphereSequencePoseFitter's default gives 1.64 mm.  What the term does NOT fix: a finger hidden
    for two frames stays 37 mm off (acc_max cuts the term exactly there; acc_max = inf brings it to 26 mm, no better than
    the first difference, and costs 2.2 mm where the motion turns); weights of 1 and above wreck the fit; a real
    acceleration is penalised; one rejected frame rejects its whole sequence.  Everything else is SphereSequencePoseFitter's:
    a refinement from a start pose, one accept decision per sequence, NO autograd through the solve, the rotation
    NOT checked."""

    # the study's row
    DEFAULT_TEMPORAL_WEIGHT = 0.0
    DEFAULT_ACCEL_WEIGHT = 0.1
    DEFAULT_ACC_MAX = 20.0

    def __init__(self, mesh, width, height, seq_len, pixel_to_model=None, right_hand=True, iters=10, lambda0=1e-3,
                 stiffness=None, fg_max=MeshDataToModelLoss.REFERENCE_FG_MAX, max_dist=50.0, render_weight=None,
                 max_resid=None, background=100.0, kp_weight=None, kp_max=None, limit_weight=None, limits=None,
                 collision_weight=None, min_dist=None, radius_scale=None, temporal_weight=None, ts_max=None,
                 accel_weight=None, acc_max=None, *, pose_prior=None):
        super().__init__(mesh, width, height, seq_len, pixel_to_model, right_hand, iters, lambda0, stiffness, fg_max, max_dist,
                         render_weight, max_resid, background, kp_weight, kp_max, limit_weight, limits, collision_weight,
                         min_dist, radius_scale, temporal_weight, ts_max, pose_prior=pose_prior)
        self.accel_weight = float(self.DEFAULT_ACCEL_WEIGHT if accel_weight is None else accel_weight)
        self.acc_max = float(self.DEFAULT_ACC_MAX if acc_max is None else acc_max)
        if not (self.accel_weight >= 0.0 and self.accel_weight < float("inf")) or not self.acc_max >= 0.0:
            raise ValueError("accel_weight must be finite and >= 0, acc_max >= 0")

    @torch.no_grad()
    def solve(self, observed, params0, view=None, prior=None, keypoints=None, confidence=None, frame_weight=None,
              triple_weight=None):
        observed, view, keypoints, confidence, limits = self._targets(observed, view, keypoints, confidence)
        return ops.sphere_icp_trajectory(observed, view, params0.detach().contiguous().float(), *self._tables(), self.seq_len,
                                         self.right_hand, self.pixel_to_model, self.fg_max, self.max_dist, self.iters,
                                         self.lambda0, self.stiffness,
                                         None if prior is None else prior.detach().contiguous().float(), self.render_weight,
                                         self.max_resid, self.background, keypoints, confidence, self.kp_weight, self.kp_max,
                                         limits, self.limit_weight, self._pairs(), self.collision_weight, self.temporal_weight,
                                         self.ts_max, self._frame_weight(frame_weight), self.accel_weight, self.acc_max,
                                         self._frame_weight(triple_weight), pose_prior=self._pose_prior())

    @torch.no_grad()
    def normal_equations(self, observed, params, view=None, keypoints=None, confidence=None, frame_weight=None,
                         triple_weight=None):
        params = params.detach().contiguous().float()
        A, g, E, cost, _ = SphereSequencePoseFitter.normal_equations(self, observed, params, view, keypoints, confidence,
                                                                     frame_weight)
        return ops.sphere_accel_normal(params, *self._tables()[:4], self.seq_len, self.right_hand, self.accel_weight,
                                       self.acc_max, self._frame_weight(triple_weight), (A, g, cost), E)

    @staticmethod
    def _bands(equations):
        return equations[2], equations[3]


class SphereWindowTracker(SphereTrajectoryPoseFitter):
    """SphereTrajectoryPoseFitter over a STREAM of frames: a fixed-lag smoother.  seq_len is the length W of a window that
    slides over S streams one frame at a time; when the oldest frame leaves, everything the fit knew through it -- its own
    image, keypoint, limit and collision terms, its stiffness, the temporal and acceleration rows that reach it and the prior
    it carried itself -- is folded into a Gaussian prior on the next two frames (ops.pose_window_marginalize;
    include/spherehand_hip.h, shr_pose_window_marginalize), the Schur complement of its block, and the window is fitted
    again with that prior as one more term (ops.sphere_icp_window, shr_pose_window_prior_normal).  The window's equations
    stay block-pentadiagonal.  On a quadratic energy marginalise-and-slide IS the full-batch fit of the newest frames
    (DESIGN.md 4.4z); on this one it is that fit's linearisation.
        begin(observed, params0, view=None, keypoints=None, confidence=None) -> (window, params [S W,26], cost0 [S], cost [S])
            the first W frames of S streams in solve's layout (B = S W, a stream's frames adjacent), fitted without a prior:
            SphereTrajectoryPoseFitter.solve bit for bit.  window: a dict of the fitted poses `params`, the poses the fit
            started from `start`, the per-frame `inputs` and the carried `prior` (None), for advance
        advance(window, observed_new, params_new=None, view_new=None, keypoints_new=None, confidence_new=None)
            -> (window, params [S W,26], cost0 [S], cost [S], status [S] int32, left [S,26])
            one new frame per stream ([S,H,W], or [S,V,H,W] with view_new [S,V,4,4]): the oldest frame is marginalised at the
            window's fitted poses, the window shifts by one frame, the new frame starts from params_new [S,26] or, without it,
            from the constant-velocity extrapolation 2 p_{W-1} - p_{W-2}, and the window is fitted with the new prior.
            left: the pose the leaving frame left with, the fixed-lag smoothed estimate; status: the marginalisation's, 1
            where the leaving frame's matrix had a pivot that is not positive and finite.  The new window also holds
            `departing`, the equations (A, g, E, F, cost, trial) that were marginalised, and `record`, the entry's outputs
        track(observed [S,N,...], params0 [S,N,26] or [S,W,26], view=None, keypoints=None, confidence=None)
            -> (smoothed [S,N,26], filtered [S,N,26], status [S,N-W])
            the loop over advance for a recorded stream: smoothed is each frame's pose when it left the window (the last
            window's poses at the end), filtered its pose after the first fit it was part of.  N == W is solve bit for bit
        normal_equations(..., window=None) -> SphereTrajectoryPoseFitter's, with the prior's term added when a window that
            carries one is given: uncertainty(observed, params, ..., window=window) then returns marginals that carry the
            marginalised past.
    The departing system is formed from the existing entries alone, nothing restated: frame 0's own terms by
    SphereCollisionPoseFitter.normal_equations on frame 0, the temporal entry weighted so that only the pair (0, 1) remains,
    the acceleration entry weighted so that only the triple centred at 1 remains, both over sub-sequences of min(W, 3)
    frames, and the carried prior by shr_pose_window_prior_normal.
    What it does NOT do: the prior is linearised ONCE, at the poses the frame left with, and never relinearised -- a later
    fit that moves frames 1 and 2 far from there meets a quadratic that no longer is the energy's; rows that are saturated at
    that moment (max_dist, max_resid, kp_max, ts_max, acc_max) are silent in the prior for good, as in DESIGN.md 4.4y, so a
    finger hidden when its frame leaves is not remembered; a failed pivot drops the whole past of that stream (status); there
    is still ONE accept decision per window; frame_weight, triple_weight and an explicit prior pose are not taken.
    Everything else is SphereTrajectoryPoseFitter's: a refinement from a start pose, NO autograd, the rotation NOT checked."""

    def _fit(self, inputs, params0, prior):
        observed, view, keypoints, confidence, limits = inputs
        return ops.sphere_icp_window(observed, view, params0, *self._tables(), self.seq_len, self.right_hand,
                                     self.pixel_to_model, self.fg_max, self.max_dist, self.iters, self.lambda0, self.stiffness,
                                     None, self.render_weight, self.max_resid, self.background, keypoints, confidence,
                                     self.kp_weight, self.kp_max, limits, self.limit_weight, self._pairs(), self.collision_weight,
                                     self.temporal_weight, self.ts_max, None, self.accel_weight, self.acc_max, None, prior,
                                     self._pose_prior())

    @torch.no_grad()
    def begin(self, observed, params0, view=None, keypoints=None, confidence=None):
        inputs = self._targets(observed, view, keypoints, confidence)
        start = params0.detach().contiguous().float()
        if start.dim() != 2 or start.shape[0] % self.seq_len != 0:
            raise RuntimeError("begin takes params0 [S W,26], the first W = %d frames of every stream" % self.seq_len)
        params, cost0, cost = self._fit(inputs, start, None)
        return dict(params=params, start=start, inputs=inputs, prior=None), params, cost0, cost

    def _departing(self, window):
        """(A, g, E, F, cost, trial) over sub-sequences of n = min(W, 3) frames: every term that involves frame 0"""
        W, n = self.seq_len, min(self.seq_len, 3)
        observed, view, keypoints, confidence, _ = window['inputs']
        S = window['params'].shape[0] // W
        first = lambda t: None if t is None else t.view((S, W) + tuple(t.shape[1:]))[:, 0].contiguous()   # noqa: E731
        trial = window['params'].view(S, W, 26)[:, :n].reshape(S * n, 26).contiguous()
        A0, g0, c0 = SphereCollisionPoseFitter.normal_equations(self, first(observed), first(window['params']), first(view),
                                                                first(keypoints), first(confidence))[:3]
        dev = trial.device
        A = torch.zeros((S * n, 26, 26), dtype=torch.float64, device=dev)
        g = torch.zeros((S * n, 26), dtype=torch.float64, device=dev)
        cost = torch.zeros((S * n,), dtype=torch.float64, device=dev)
        A.view(S, n, 26, 26)[:, 0].copy_(A0)
        g.view(S, n, 26)[:, 0].copy_(g0)
        cost.view(S, n)[:, 0].copy_(c0)
        at = lambda t: torch.zeros((S, n), device=dev).index_fill_(1, torch.tensor([t], device=dev), 1.0).reshape(S * n)   # noqa: E731
        A, g, E, cost, _ = ops.sphere_temporal_normal(trial, *self._tables()[:4], n, self.right_hand, self.temporal_weight,
                                                      self.ts_max, at(0), (A, g, cost))
        F = None
        if n == 3:
            A, g, E, F, cost, _ = ops.sphere_accel_normal(trial, *self._tables()[:4], n, self.right_hand, self.accel_weight,
                                                          self.acc_max, at(1), (A, g, cost), E)
        if window['prior'] is not None:
            A, g, E, cost = ops.pose_window_prior_normal(trial, *window['prior'], n, (A, g, cost), E)
        return A, g, E, F, cost, trial

    @torch.no_grad()
    def advance(self, window, observed_new, params_new=None, view_new=None, keypoints_new=None, confidence_new=None):
        W, n = self.seq_len, min(self.seq_len, 3)
        params = window['params']
        S = params.shape[0] // W
        new = self._targets(observed_new, view_new, keypoints_new, confidence_new)
        if new[0].shape[0] != S or any((a is None) != (b is None) for a, b in zip(new[:4], window['inputs'][:4])):
            raise RuntimeError("advance takes one new frame for each of the %d streams, with the inputs begin was given" % S)
        departing = self._departing(window)
        A, g, E, F, cost, trial = departing
        prior0 = window['start'].view(S, W, 26)[:, :n].reshape(S * n, 26).contiguous()
        record = ops.pose_window_marginalize(A, g, E, F, cost, trial, n, prior0, self.stiffness)
        p = params.view(S, W, 26)
        left = p[:, 0].clone()
        if params_new is None:
            params_new = 2.0 * p[:, W - 1] - p[:, W - 2] if W > 1 else p[:, 0]
        params_new = params_new.detach().float().reshape(S, 1, 26)
        shift = lambda old, t: None if old is None else \
            torch.cat((old.view((S, W) + tuple(old.shape[1:]))[:, 1:], t.unsqueeze(1)), 1).reshape(old.shape).contiguous()   # noqa: E731
        inputs = tuple(shift(a, b) for a, b in zip(window['inputs'][:4], new[:4])) + (new[4],)
        start = torch.cat((p[:, 1:], params_new), 1).reshape(S * W, 26).contiguous()
        prior = record[:4]
        fitted, cost0, cost_w = self._fit(inputs, start, prior)
        window = dict(params=fitted, start=start, inputs=inputs, prior=prior, departing=departing, record=record)
        return window, fitted, cost0, cost_w, record[4], left

    @torch.no_grad()
    def track(self, observed, params0, view=None, keypoints=None, confidence=None):
        W = self.seq_len
        S, N = observed.shape[:2]
        if N < W or params0.dim() != 3 or params0.shape[0] != S or params0.shape[1] not in (N, W):
            raise RuntimeError("track takes observed [S,N,...], N >= W = %d, and params0 [S,N,26] or [S,W,26]" % W)
        head = lambda t: None if t is None else t[:, :W].reshape((S * W,) + tuple(t.shape[2:]))   # noqa: E731
        frame = lambda t, k: None if t is None else t[:, k]   # noqa: E731
        window, params, _, _ = self.begin(head(observed), head(params0), head(view), head(keypoints), head(confidence))
        filtered = torch.empty((S, N, 26), dtype=torch.float32, device=params.device)
        smoothed = torch.empty_like(filtered)
        filtered[:, :W] = params.view(S, W, 26)
        status = torch.zeros((S, N - W), dtype=torch.int32, device=params.device)
        for k in range(W, N):
            window, params, _, _, st, left = self.advance(window, frame(observed, k), frame(params0, k) if params0.shape[1] == N
                                                          else None, frame(view, k), frame(keypoints, k), frame(confidence, k))
            smoothed[:, k - W], filtered[:, k], status[:, k - W] = left, params.view(S, W, 26)[:, W - 1], st
        smoothed[:, N - W:] = params.view(S, W, 26)
        return smoothed, filtered, status

    @torch.no_grad()
    def normal_equations(self, observed, params, view=None, keypoints=None, confidence=None, frame_weight=None,
                         triple_weight=None, window=None):
        A, g, E, F, cost, count = SphereTrajectoryPoseFitter.normal_equations(self, observed, params, view, keypoints, confidence,
                                                                              frame_weight, triple_weight)
        if window is not None and window['prior'] is not None:
            A, g, E, cost = ops.pose_window_prior_normal(params.detach().contiguous().float(), *window['prior'], self.seq_len,
                                                         (A, g, cost), E)
        return A, g, E, F, cost, count


class SphereRadiiCalibrator(SphereCollisionPoseFitter):
    """The sphere RADII calibrated to the hand in the frames: every fitter above takes the 41 radii as a constant of the
    shipped model, and they are a fat proxy.  The batch's B = G group_size frames are G groups, the
    frames of one adjacent -- one person's hand in group_size poses; each frame keeps its own pose, the frames of a group
    SHARE one radius table, and both are fitted jointly: `iters` Levenberg-Marquardt iterations on the group's energy
        the sum over its frames of SphereCollisionPoseFitter's energy (without the render term)
        + sum_j shape_stiffness_j (r_j - radii0_j)^2
    (ops.sphere_icp_calibrate; include/spherehand_hip.h, shr_sphere_icp_radii_normal and shr_pose_lm_shared_step).  A
    shared unknown couples every frame of its group, so the normal equations are an arrowhead -- the pose blocks, one
    41 x 41 radius block and a coupling per frame -- solved by the Schur complement on the radius block, and lambda, the
    cost and the accept decision belong to the group.
        solve(observed, params0, view=None, prior=None, keypoints=None, confidence=None, radii0=None)
            -> (params [B,26], radii [G,41], cost0 [G], cost [G])
        normal_equations(observed, params, view=None, keypoints=None, confidence=None, radii=None)
            -> (A, g, cost, count [B], C [B,26,41], R [G,41,41], gs [G,41]): A, g and cost the SUM of the four terms', count
               the data term's rows; C, R and gs are the data term's own (no other term depends on the radii)
    radii0 [G,41] (or [41] for every group) defaults to the shipped table.  shape_stiffness: [41] or a number, each >= 0,
    None: DEFAULT_SHAPE_STIFFNESS, from DESIGN.md 4.4v's grid; with 0 a sphere that owns no data point in any frame of its
    group leaves the radius block singular, and the step, which has no special case for a bad pivot, stays.  The result is used by handing a group's table to any of the fitters above: fitter.radii.copy_(radii[g]).
    render_weight other than 0 raises ValueError: the render rows' d D / d r columns are out of scope here, and a term
    whose radius gradient is missing gives no descent direction for the cost the accept test sees.  The collision table
    stays the one built at construction, from the shipped radii.  Data points are explained by the sphere SURFACE nearest to
    them, so one view constrains a radius only where that sphere owns points; shape_stiffness holds the others.  Everything
    else is SphereCollisionPoseFitter's: a refinement from a start, NO autograd through the solve, the rotation NOT checked."""

    # the grid's row
    DEFAULT_SHAPE_STIFFNESS = 1.0

    def __init__(self, mesh, width, height, group_size, pixel_to_model=None, right_hand=True, iters=10, lambda0=1e-3,
                 stiffness=None, fg_max=MeshDataToModelLoss.REFERENCE_FG_MAX, max_dist=50.0, render_weight=0.0,
                 max_resid=None, background=100.0, kp_weight=None, kp_max=None, limit_weight=None, limits=None,
                 collision_weight=None, min_dist=None, radius_scale=None, shape_stiffness=None, *, pose_prior=None):
        if pose_prior is not None:
            raise ValueError("SphereRadiiCalibrator takes no pose_prior: its loop does not issue the term")
        if render_weight is None or float(render_weight) != 0.0:
            raise ValueError("SphereRadiiCalibrator has no render term: its radius columns are not formed (render_weight must be 0)")
        super().__init__(mesh, width, height, pixel_to_model, right_hand, iters, lambda0, stiffness, fg_max, max_dist, 0.0,
                         max_resid, background, kp_weight, kp_max, limit_weight, limits, collision_weight, min_dist,
                         radius_scale)
        self.group_size = int(group_size)
        if self.group_size < 1:
            raise ValueError("group_size must be >= 1")
        nu = np.asarray(self.DEFAULT_SHAPE_STIFFNESS if shape_stiffness is None else shape_stiffness, np.float32)
        nu = np.full(self.num_spheres, nu, np.float32) if nu.ndim == 0 else nu.reshape(self.num_spheres)
        if not (nu >= 0).all():
            raise ValueError("shape_stiffness must be >= 0")
        self.register_buffer('shape_stiffness', torch.from_numpy(nu.copy()))

    def _radii(self, radii, B):
        if B % self.group_size != 0:
            raise RuntimeError("the batch's %d frames are not groups of %d" % (B, self.group_size))
        G = B // self.group_size
        if radii is None:
            radii = self.radii
        radii = radii.detach().float().to(self.radii.device)
        return (radii.unsqueeze(0).expand(G, -1) if radii.dim() == 1 else radii).contiguous()

    @torch.no_grad()
    def solve(self, observed, params0, view=None, prior=None, keypoints=None, confidence=None, radii0=None):
        observed, view, keypoints, confidence, limits = self._targets(observed, view, keypoints, confidence)
        return ops.sphere_icp_calibrate(observed, view, params0.detach().contiguous().float(), *self._tables()[:4],
                                        self._radii(radii0, observed.shape[0]), self.group_size, self.right_hand,
                                        self.pixel_to_model, self.fg_max, self.max_dist, self.iters, self.lambda0, self.stiffness,
                                        None if prior is None else prior.detach().contiguous().float(), self.shape_stiffness,
                                        None, keypoints, confidence, self.kp_weight, self.kp_max, limits, self.limit_weight,
                                        self._pairs(), self.collision_weight)

    @torch.no_grad()
    def normal_equations(self, observed, params, view=None, keypoints=None, confidence=None, radii=None):
        observed, view, keypoints, confidence, limits = self._targets(observed, view, keypoints, confidence)
        params = params.detach().contiguous().float()
        A, g, cost, count, C, R, gs = ops.sphere_icp_radii_normal(
            observed, view, params, *self._tables()[:4], self._radii(radii, observed.shape[0]), self.group_size, self.right_hand,
            self.pixel_to_model, self.fg_max, self.max_dist)[:7]
        A, g, cost = ops.sphere_prior_normal(view, params, *self._tables()[:4], self.right_hand, keypoints, confidence,
                                             self.kp_weight, self.kp_max, limits, self.limit_weight, (A, g, cost))[:3]
        A, g, cost = ops.sphere_collision_normal(params, *self._tables()[:4], self.right_hand, self._pairs(),
                                                 self.collision_weight, (A, g, cost))[:3]
        return A, g, cost, count, C, R, gs

    def uncertainty(self, *args, **kwargs):
        """Not available: the radii make the system an arrowhead, and the covariance of that system (the pose blocks'
        marginals with the shared block eliminated) is out of scope."""
        raise NotImplementedError("SphereRadiiCalibrator has no uncertainty: the arrowhead system's covariance is not implemented")


class DepthRender(nn.Module):
    """mesh/render.py:315-331.  forward(T[B,17,4,4], rand_fx[B]=None) -> depth
    [B,S,S] in mm, background 100: skinning + camera (one launch), triangle raster
    with the face gather fused (fill, raster, decode), clamp + bilinear resize.

    differentiable=True (image sizes up to 320 only, checked here): where grad is enabled and T requires grad, the depth
    is differentiable w.r.t. T (ops.MeshDepthRender; rand_fx gets no gradient) and bit-identical to the default path.
    The sphere renderer's contract (ops.SphereDepthRaster): the gradient routes to each tap's owner face and holds
    coverage fixed; there is no gradient for edge, silhouette or visibility changes.  The reference defines no backward
    for the mesh (mesh/render.py:282-287)."""

    def __init__(self, mesh, image_size, differentiable=False):
        super().__init__()
        if differentiable and not ops.mesh_owner_supported(image_size):
            raise ValueError("differentiable DepthRender takes image sizes up to 320, not %r" % (image_size,))
        self.differentiable = differentiable
        # the skinned vertices never leave this module: the distinct ones are enough, the faces index them (identical
        # face corners, hence identical images; 16 -> 4 us of skinning and a sixth of the vertex traffic per call)
        self.lbs = SparseSkinning(mesh, distinct=True)
        self.camera = (320.0, 320.0, 640 / 300, 640 / 300)             # :325
        self.rasterizer = DepthRasterization(image_size, image_size, self.lbs.vertex_index[np.asarray(mesh['faces'], np.int64)])

    def forward(self, transformation_mats, rand_fx=None):
        ras = self.rasterizer
        T = transformation_mats
        if self.differentiable and T.requires_grad and torch.is_grad_enabled():
            if not T.is_cuda:
                raise RuntimeError("the differentiable mesh path needs CUDA bone transformations")
            return ops.MeshDepthRender.apply(T, None if rand_fx is None else rand_fx.detach().contiguous().float(),
                                             self.lbs.skin_vertex_start, self.lbs.skin_bone, self.lbs.skin_wv,
                                             self.lbs.right_hand, self.camera, ras.faces_i32, ras.height)
        if T.is_cuda and ras.fused and ras.width == ras.height and 2 * ras.width <= 641:
            # skinning + camera + raster + clamp + resize: one launch where the lattice kernel applies
            # (shr_mesh_render_fwd), the two launches below through a workspace otherwise -- the same bits
            return ops.mesh_render_fwd(T.contiguous().float(), self.lbs.skin_vertex_start, self.lbs.skin_bone,
                                       self.lbs.skin_wv, self.lbs.right_hand, self.camera,
                                       None if rand_fx is None else rand_fx.contiguous().float(), ras.faces_i32,
                                       ras.height, 640, 100.0)
        skinned_points = self.lbs(transformation_mats, self.camera, rand_fx)
        return self.rasterizer(skinned_points)


class HeatmapRender(nn.Module):
    """forward(uvd_points[B,J,>=3]) -> (uv_hm[B,J,S,S], scaled_d_hm[B,J,S,S]): a
    Gaussian exp(-0.5*sigma*d^2) per joint and the joint's depth painted where the
    Gaussian exceeds 0.05 (mesh/render.py:226-248)."""

    def __init__(self, hm_size, sigma=1.0):
        super().__init__()
        self.sigma = sigma
        self.height = self.width = hm_size
        grid = torch.arange(hm_size, dtype=torch.float32)
        self.register_buffer('u_grid', grid.view(1, 1, 1, hm_size))
        self.register_buffer('v_grid', grid.view(1, 1, hm_size, 1))

    def forward(self, uvd_points):
        assert uvd_points.ndimension() == 3
        u = uvd_points[:, :, 0, None, None]
        v = uvd_points[:, :, 1, None, None]
        uv_hm = torch.exp(-0.5 * self.sigma * ((self.u_grid - u) ** 2 + (self.v_grid - v) ** 2))
        d = uvd_points[:, :, 2, None, None].expand_as(uv_hm)
        return uv_hm, torch.where(uv_hm > 0.05, d, torch.zeros_like(d))


class Hand3DHeatmapRender(nn.Module):
    """forward(T[B,17,4,4], rand_f=None) -> (uv heat-maps, depth heat-maps, xyz of the
    41 key-points back-projected from the heat-map camera) (mesh/render.py:274-279)."""

    def __init__(self, bones, heatmap_size):
        super().__init__()
        from .pointTransformation import InverseOthographicalProjection, OthographicalProjection
        self.width = self.height = heatmap_size
        self.hm_renderer = HeatmapRender(heatmap_size)
        half, f = heatmap_size / 2, heatmap_size / 300
        self.camera = OthographicalProjection(half, half, f, f)
        self.inv_camera = InverseOthographicalProjection(half, half, f, f)
        self.lbs = keypoint_skinning(bones)
        self.num_vertices = self.lbs.num_vertices
        self._skin_bone_i32 = None

    def forward(self, transformation_mats, rand_f=None, uv_scale=1.0, d_scale=1.0):
        """(uv_scale / d_scale: HandSynthesizer's heat-map scalings, applied in the same launch on the GPU path)"""
        T = transformation_mats
        if T.is_cuda and not torch.is_grad_enabled() and T.dtype == torch.float32:
            # forward-only GPU path: skinning + camera (one launch), then Gaussians + depth painting +
            # back-projection (one launch)
            lbs = self.lbs
            if self._skin_bone_i32 is None or self._skin_bone_i32.device != T.device:
                self._skin_bone_i32 = lbs.skin_bone.to(device=T.device, dtype=torch.int32).contiguous()
                self._inv_k = self.inv_camera.inv_k_mat[0].cpu().tolist()
            cam = self.camera
            uvd = ops.lbs_project(T.contiguous(), lbs.skin_vertex_start, self._skin_bone_i32, lbs.skin_wv, lbs.right_hand,
                                  (cam.cx, cam.cy, cam.fx, cam.fy), None if rand_f is None else rand_f.contiguous().float())
            return ops.heatmap_paint(uvd, self.width, self.hm_renderer.sigma, self._inv_k, uv_scale, d_scale)
        uvd_points = self.camera(self.lbs(T), rand_f)
        hms, dms = self.hm_renderer(uvd_points)
        return hms * uv_scale, dms * d_scale, self.inv_camera(uvd_points)


def _collision_pairs():
    """Every finger sphere against the 11 palm spheres, and against every sphere of
    another finger (mesh/render.py:150-162): 330 + 360 pairs."""
    a, b = [], []
    for p in range(11):
        for q in range(11, 41):
            a.append(p); b.append(q)
    for p in range(11, 41):
        for q in range(p + 1, 41):
            if (p - 11) // 6 != (q - 11) // 6:
                a.append(p); b.append(q)
    return a, b


class CollisionLoss(nn.Module):
    """sum of relu(min_dist^2 - |c_a - c_b|^2) over the pair table (mesh/render.py:168-176)."""

    def __init__(self, min_dist=6):
        super().__init__()
        self.min_sq_dist = min_dist ** 2
        a, b = _collision_pairs()
        self.register_buffer('joint_1', torch.tensor(a).long())
        self.register_buffer('joint_2', torch.tensor(b).long())

    def forward(self, joints):
        joints = joints.reshape(joints.shape[0], -1, 3)
        sq = ((joints[:, self.joint_1] - joints[:, self.joint_2]) ** 2).sum(-1)
        return torch.relu(self.min_sq_dist - sq).sum()


# The 35 sphere pairs whose distance is held to [0.80, 1.05] x its rest length
# (data of mesh/bone_length.py:36-55: 20 palm pairs + 3 per finger).
BONE_PAIRS_1 = [3, 2, 3, 8, 2, 2, 9, 8, 4, 8, 7, 4, 6, 7, 0, 5, 7, 7, 6, 6] + \
    [11 + 6 * f + 2 * k for f in range(5) for k in range(3)]
BONE_PAIRS_2 = [2, 9, 8, 2, 4, 10, 10, 4, 10, 7, 4, 6, 10, 6, 5, 1, 0, 5, 5, 1] + \
    [12 + 6 * f + 2 * k for f in range(5) for k in range(3)]
BONE_REST_LENGTH = [
    25.212656021118164, 18.249488830566406, 27.5742244720459, 38.532264709472656, 25.10819435119629,
    31.173757553100586, 18.329626083374023, 19.15080451965332, 16.209327697753906, 21.52261734008789,
    32.740535736083984, 30.58920669555664, 33.205970764160156, 11.672294616699219, 17.084707260131836,
    17.084720611572266, 16.697546005249023, 23.92103385925293, 20.87999725341797, 22.58038330078125,
    27.55999755859375, 15.471183776855469, 13.214692115783691, 21.748210906982422, 13.021653175354004,
    16.643720626831055, 18.83765983581543, 12.724685668945312, 16.238431930541992, 18.04928970336914,
    11.045844078063965, 11.320968627929688, 30.078536987304688, 16.255985260009766, 19.434825897216797]


class BoneLengthLoss(nn.Module):
    """mean relu(min^2 - d^2) + mean relu(d^2 - max^2) over the 35 pairs (mesh/render.py:196-206)."""

    def __init__(self):
        super().__init__()
        rest = torch.tensor(BONE_REST_LENGTH).float()
        self.register_buffer('joint_1', torch.tensor(BONE_PAIRS_1).long())
        self.register_buffer('joint_2', torch.tensor(BONE_PAIRS_2).long())
        self.register_buffer('max_length', ((rest * 1.05) ** 2).unsqueeze(0))
        self.register_buffer('min_length', ((rest * 0.80) ** 2).unsqueeze(0))

    def forward(self, joints):
        joints = joints.reshape(joints.shape[0], -1, 3)
        sq = ((joints[:, self.joint_1] - joints[:, self.joint_2]) ** 2).sum(-1)
        return torch.relu(self.min_length - sq).mean() + torch.relu(sq - self.max_length).mean()
