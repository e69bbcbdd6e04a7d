"""The differentiable DepthRender through the C ABI (no Python op in the loop), HIP events on the launching stream:
  forward          today's DepthRender (shr_mesh_render_fwd)
  forward+owners   shr_lbs_project + shr_mesh_depth_owner_fwd (ops.MeshDepthRender.forward)
  backward         shr_mesh_depth_bwd + shr_lbs_project_bwd (ops.MeshDepthRender.backward)
at 64 crops @256^2 and 256 crops @128^2 (and the two smaller sizes)."""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from spherehand_amd import _lib, hand_model
from spherehand_amd.render import DepthRender
from spherehand_amd.kinematicsTransformation import HandTransformationMat
from spherehand_amd.joint_angle import sample_poses
mesh = hand_model.load_mesh()
lib = _lib.lib()
fk = HandTransformationMat([b["offset_matrix"].astype("float32") for b in mesh["bones"]]).cuda()
stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    for B, S in ((64, 256), (256, 128), (256, 64), (256, 32)):
        dr = DepthRender(mesh, S).cuda()
        T = fk(sample_poses(B, seed=1).cuda()).contiguous()
        l = dr.lbs
        faces = dr.rasterizer.faces_i32
        NV, F = l.num_vertices, faces.shape[0]
        verts = torch.empty(B, NV, 4, device="cuda"); out = torch.empty(B, S, S, device="cuda"); out2 = torch.empty_like(out)
        owner = torch.empty(B, S, S, 4, dtype=torch.int32, device="cuda")
        g = torch.randn(B, S, S, device="cuda")
        gv = torch.empty(B, NV, 4, device="cuda"); gT = torch.empty(B, 17, 4, 4, device="cuda")
        ws = torch.empty(lib.shr_mesh_depth_bwd_workspace_bytes(B, NV), dtype=torch.uint8, device="cuda")
        cx, cy, fx, fy = dr.camera
        p = lambda t: t.data_ptr()
        tabs = (p(l.skin_vertex_start), p(l.skin_bone), p(l.skin_wv))
        fwd = lambda s: lib.shr_mesh_render_fwd(p(T), B, 17, NV, *tabs, 1, cx, cy, fx, fy, None, p(faces), F, 640, S, 100.0,
                                                p(verts), p(out), s)
        def fwd_owner(s):
            lib.shr_lbs_project(p(T), B, 17, NV, *tabs, 1, 1, cx, cy, fx, fy, None, p(verts), s)
            return lib.shr_mesh_depth_owner_fwd(p(verts), p(faces), B, NV, F, 640, S, 100.0, p(out2), p(owner), s)
        def bwd(s):
            lib.shr_mesh_depth_bwd(p(verts), p(faces), p(owner), p(g), B, NV, F, 640, S, p(gv), p(ws), s)
            return lib.shr_lbs_project_bwd(p(gv), B, 17, NV, *tabs, 1, cx, cy, fx, fy, None, p(gT), s)
        raster_bwd = lambda s: lib.shr_mesh_depth_bwd(p(verts), p(faces), p(owner), p(g), B, NV, F, 640, S, p(gv), p(ws), s)
        assert fwd(stream.cuda_stream) == 0 and fwd_owner(stream.cuda_stream) == 0 and bwd(stream.cuda_stream) == 0
        stream.synchronize()
        t1 = bench.mean_launch_us(fwd, stream, 50, 3, 5, warm_ms=20.0)
        t2 = bench.mean_launch_us(fwd_owner, stream, 50, 3, 5, warm_ms=20.0)
        t3 = bench.mean_launch_us(bwd, stream, 50, 3, 5, warm_ms=20.0)
        t4 = bench.mean_launch_us(raster_bwd, stream, 50, 3, 5, warm_ms=20.0)
        print("B=%d S=%d: forward %.1f us | forward+owners %.1f us | backward %.1f us (raster backward alone %.1f) | "
              "same depth bits: %s" % (B, S, t1, t2, t3, t4, torch.equal(out, out2)), flush=True)
