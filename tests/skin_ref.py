"""Skinning + camera restated with torch operations, as the DENSE sum the reference forms
(mesh/pointTransformation.py:39-46: every bone's matrix times every vertex's weighted position, summed over the bones;
:84-99: the orthographic camera).  Any device, fp32 or fp64, autograd by torch: the independent check of
shr_lbs_vertices_bwd / shr_pose_vertices_* and the reference chain of the pose fit."""
import numpy as np
import torch


def dense_table(start, bone, wv, NB, dtype=torch.float64, device="cpu"):
    """The CSR skin table (hand_model.sparse_skin / unique_skin) as the reference's dense buffer [NB, NV, 4] =
    weight * vertex (0 where a bone does not move a vertex; the sum where a bone lists a vertex twice)."""
    start, bone, wv = (np.asarray(a) for a in (start, bone, wv))
    NV = len(start) - 1
    dense = np.zeros((NB, NV, 4), np.float64)
    vid = np.repeat(np.arange(NV), np.diff(start))
    np.add.at(dense, (bone.astype(np.int64), vid), wv.astype(np.float64))
    return torch.from_numpy(dense).to(dtype).to(device)


def skin(T, dense, right_hand=True, camera=None, rand_f=None):
    """T [B,NB,4,4] (or [B,NB,1,4,4]), dense [NB,NV,4] -> vertices [B,NV,4] in T's dtype.
    camera=None: the skinned points (project = 0); camera=(cx,cy,fx,fy): u = fx x + cx w, v = fy y + cy w, or with
    rand_f [B]: u = x rand_f fx + cx, v = y rand_f fy + cy, w = 1."""
    if T.dim() == 5:
        T = T.squeeze(2)
    dense = dense.to(T.dtype)
    acc = torch.einsum("bkrc,kvc->bvr", T, dense)              # sum over bones k of T[b,k] @ dense[k,v]
    if right_hand:
        acc = acc * torch.tensor([-1.0, 1.0, 1.0, 1.0], dtype=T.dtype, device=T.device)
    if camera is None:
        return acc
    cx, cy, fx, fy = camera
    x, y, z, w = acc.unbind(-1)
    if rand_f is None:
        return torch.stack([fx * x + cx * w, fy * y + cy * w, z, w], -1)
    f = rand_f.to(T.dtype).view(-1, 1)
    return torch.stack([x * f * fx + cx, y * f * fy + cy, z, torch.ones_like(z)], -1)


def synthetic_table():
    """A 70-vertex table over the hand's 17 bones with every shape of row the kernels branch on: rows without an entry
    (vertices 3, 40 and 69, the last), a row of 17 entries (5: every bone but bone 1, and bone 16 twice -- a row that held
    bone 1 too would contradict the next item), a row naming bone 4 twice (7), and bone 1 unused: its gradient is an
    exact zero.  Entries of a vertex in ascending bone order, as hand_model.sparse_skin writes them."""
    rng = np.random.RandomState(70)
    NV, NB = 70, 17
    start, bone, wv = [0], [], []
    for v in range(NV):
        if v in (3, 40, 69):
            bones = []
        elif v == 5:
            bones = [k for k in range(NB) if k != 1] + [16]
        elif v == 7:
            bones = [2, 4, 4, 9]
        else:
            bones = sorted(rng.choice([k for k in range(NB) if k != 1], size=rng.randint(1, 5), replace=False).tolist())
        assert 1 not in bones
        w = rng.uniform(0.1, 1.0, len(bones))
        w = w / max(w.sum(), 1e-9)
        p = np.append(rng.uniform(-60, 60, 3), 1.0)
        for k, wk in zip(bones, w):
            bone.append(k)
            wv.append((wk * p).astype(np.float32))
        start.append(len(bone))
    return (np.asarray(start, np.int32), np.asarray(bone, np.int32),
            np.ascontiguousarray(np.asarray(wv, np.float32).reshape(-1, 4)))
