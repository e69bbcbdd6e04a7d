"""What further depth views buy the mesh pose fit, on the CPU in fp64 with the tests' restatement
(tests/pose_icp_views_ref.py): section 4.4n's 20 poses (pose_icp_ref.poses, seeds 21-24, the palm 50 mm deep) self-rendered
at 48 x 40, starts p* + N(0, 0.1) rad / N(0, 2 mm), 10 iterations, lambda0 = 1e-3, stiffness 1 on the 23 angles, for
V = 1 (the model frame), 2 (+ 90 degrees about y through the palm) and 3 (+ 90 degrees about x).  Prints per V the cost
ratio, the mean vertex error, the bone-origin error (the translation column of the 17 bone transforms) and the smallest
eigenvalue of A and of A + diag(mu) at the start, per crop and summarised.  No device is used; about ten minutes."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pose_icp_ref as ref  # noqa: E402
import pose_icp_views_ref as vref  # noqa: E402
from spherehand_amd import hand_model  # noqa: E402

W, H, ITERS, SEEDS, KINDS = 48, 40, 10, (21, 22, 23, 24), ("identity", "y", "x")


def bone_origins(model, p):
    T = model.fk.forward_torch(p.double())
    T = T.squeeze(2) if T.dim() == 5 else T
    return T[..., :3, 3]


def main():
    mesh = hand_model.load_mesh()
    model = ref.hand_model(mesh, True)
    p2m, mu = ref.grid(W, H), torch.as_tensor(ref.STIFFNESS)
    rows = {V: [] for V in (1, 2, 3)}
    start = []
    for seed in SEEDS:
        p, p0 = ref.poses(5, seed)
        p0 = p0.float().double()
        view = vref.views(5, KINDS, spread=False)
        observed = vref.render_views(model, view, p, W, H)
        origin = lambda q: (bone_origins(model, q) - bone_origins(model, p)).norm(dim=-1).mean(1)   # noqa: E731
        start.append(torch.stack([vref.vertex_error(model, p0, p), origin(p0)], 1))
        for V in (1, 2, 3):
            vw, obs = view[:, :V], observed[:, :V]
            dist, face = vref.search_views(model, vw, obs, p0, p2m)
            A = vref.normal_views(model, vw, obs, p0, dist, face, p2m)[0]
            eig_a = torch.linalg.eigvalsh(A)
            eig_m = torch.linalg.eigvalsh(A + torch.diag(mu))[:, 0]
            q, c0, c, lm = vref.solve_views(model, vw, obs, p0, p2m, ITERS, stiffness=mu)
            out = torch.stack([c0 / c, vref.vertex_error(model, q, p), origin(q), eig_a[:, 0], eig_a[:, 0] / eig_a[:, -1], eig_m,
                               c0, c, lm.last_step], 1)
            rows[V].append(out)
            for b in range(5):
                print("seed %d crop %d V=%d: points %s; cost %.4g -> %.4g; vertex error %.3f mm, bone origins %.3f mm; min eig A %.3g "
                      "(%.3g of the largest), A + mu %.3g; last step %.3g"
                      % (seed, b, V, [(obs[b, v] < ref.FG_MAX).sum() for v in range(V)], out[b, 6], out[b, 7], out[b, 1], out[b, 2],
                         out[b, 3], out[b, 4], out[b, 5], out[b, 8]), flush=True)
    start = torch.cat(start)
    print("start: mean vertex error %.2f mm (median %.2f), bone-origin error %.2f mm (median %.2f)"
          % (start[:, 0].mean(), np.median(start[:, 0].numpy()), start[:, 1].mean(), np.median(start[:, 1].numpy())))
    for V in (1, 2, 3):
        r = torch.cat(rows[V])
        print("V=%d: cost0 / cost median %.3g (worst %.3g); mean vertex error %.2f mm (median %.2f); bone-origin error %.2f mm "
              "(median %.2f); min eig A exactly 0 in %d of %d, min eig of A + mu %.3g .. %.3g; vertex error per crop %s"
              % (V, np.median(r[:, 0].numpy()), r[:, 0].min(), r[:, 1].mean(), np.median(r[:, 1].numpy()), r[:, 2].mean(),
                 np.median(r[:, 2].numpy()),
                 int((r[:, 3] == 0).sum()), len(r), r[:, 5].min(), r[:, 5].max(), np.round(r[:, 1].numpy(), 2).tolist()))


if __name__ == "__main__":
    main()
