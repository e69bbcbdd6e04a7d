"""Vertex normals without a GPU: the host-built tables against their O(NV F) definition, the restatements of
tests/tri_normals_ref.py against each other (fp32 accuracy, fp64 gradient against central differences, the tilt fit),
and the new unit's code-object resources."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tri_interp_ref
import tri_normals_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.mark.parametrize("seed", [0, 1])
def test_tables_on_random_meshes(seed):
    from spherehand_amd import ops
    v, faces = ref.random_mesh(1, 40, 30, seed)
    NV = v.shape[1]
    faces = faces.copy()
    faces[5, 1], faces[9, 0] = NV + 3, -1                       # two faces with an id out of range: in no table
    T = ops.tri_vertex_tables(faces, NV)
    assert ref.check_tables(T, faces, NV) == NV
    assert np.array_equal(T.inc, T.own) and np.array_equal(T.inc_start, T.own_start)       # without welding they coincide
    assert np.array_equal(T.copy, np.arange(NV)) and np.array_equal(T.point, np.arange(NV))
    # an integer weld map that merges vertices in pairs, and the face soup welded by position bits
    weld = (np.arange(NV) // 2) * 7
    assert ref.check_tables(ops.tri_vertex_tables(faces, NV, weld), faces, NV, weld) == (NV + 1) // 2
    good = faces[np.all((faces >= 0) & (faces < NV), axis=1)]
    sv, sf = ref.soup_of(v, good)
    Ts = ops.tri_vertex_tables(sf, sv.shape[1], sv[0, :, :3])
    NP = ref.check_tables(Ts, sf, sv.shape[1], sv[0, :, :3])
    assert NP < sv.shape[1]
    # welded copies share entries: the same rows of inc and copy
    same = np.nonzero(Ts.point == Ts.point[0])[0]
    assert len(same) >= 1 and all(Ts.point[c] == Ts.point[0] for c in Ts.copy[Ts.copy_start[Ts.point[0]]:Ts.copy_start[Ts.point[0] + 1]])


def test_tables_on_the_hand_at_both_weldings():
    from spherehand_amd import ops
    v, faces, rest, index, first = ref.hand(1)
    NV = v.shape[1]
    assert NV == 10144
    T = ops.tri_vertex_tables(faces, NV, rest)
    assert ref.check_tables(T, faces, NV, rest) == 1721
    # welding by rest position is unique_skin's partition
    assert len(set(zip(T.point.tolist(), index.tolist()))) == 1721
    fd = index[faces.astype(np.int64)].astype(np.int32)
    Td = ops.tri_vertex_tables(fd, 1721)
    assert ref.check_tables(Td, fd, 1721) == 1721
    # copies share their point's entries: the welded mesh's incidence per point is the distinct mesh's per vertex
    for vtx in (0, 17, 5000, NV - 1):
        p, d = T.point[vtx], index[vtx]
        assert np.array_equal(T.inc[T.inc_start[p]:T.inc_start[p + 1]], Td.inc[Td.inc_start[d]:Td.inc_start[d + 1]])


def test_table_builder_rejects_bad_arguments():
    from spherehand_amd import ops
    with pytest.raises(RuntimeError, match="faces"):
        ops.tri_vertex_tables(np.zeros((4, 2), np.int32), 5)
    with pytest.raises(RuntimeError, match="weld"):
        ops.tri_vertex_tables(np.zeros((4, 3), np.int32), 5, np.zeros(4, np.int64))
    with pytest.raises(RuntimeError, match="NV"):
        ops.tri_vertex_tables(np.zeros((0, 3), np.int32), 0)


def test_fp32_restatement_is_within_4_ulp_of_fp64():
    """n from the fp32 restatement against N / |N| in fp64 from the SAME fp32 N: three roundings in s, halved by the
    root, the root's and the division's: below 3.5 u of a component of at most 1."""
    v, faces = ref.random_mesh(3, 64, 48, 2, quirks=False)
    hv, hf, rest, _, _ = ref.hand(2)
    worst = 0.0
    for P, f, weld in ((v, faces, None), (hv, hf, rest)):
        N, n, live = ref.normals32(P, f, weld)
        assert live.any()
        N64 = N.astype(np.float64)
        want = N64 / np.sqrt((N64 * N64).sum(-1, keepdims=True))
        err = np.abs(n.astype(np.float64) - want)[live].max()
        worst = max(worst, err)
        assert err <= 4 * U, err
        assert np.all(n[~live] == 0)
    print("fp32 restatement: max |n - fp64| = %.3g u" % (worst / U))


def test_fp64_gradient_matches_central_differences():
    rs = np.random.RandomState(3)
    v, faces = ref.fan_mesh(1, 5, spokes=7)
    v, faces = np.concatenate([v, ref.coincident_mesh(1)[0] + 100], 1), \
        np.concatenate([faces, ref.coincident_mesh(1)[1] + v.shape[1]])
    weld = np.arange(v.shape[1])
    weld[3] = weld[2]                                               # two vertices welded by an integer map
    g = rs.standard_normal((1, v.shape[1], 3))
    got = ref.normals_grad(v, faces, weld, g)
    assert np.abs(got).max() > 1e-3
    P0 = torch.from_numpy(v[..., :3]).double()
    gt = torch.from_numpy(g)
    h = 1e-4
    worst = 0.0
    live = ref.normals32(v, faces, weld)[2]
    assert live.any() and (~live).any()
    for vi in range(v.shape[1]):
        for d in range(3):
            Pp, Pm = P0.clone(), P0.clone()
            Pp[0, vi, d] += h
            Pm[0, vi, d] -= h
            # the zero rule's decisions are those of the unperturbed fp32 points in both evaluations
            fd = ((ref.normals64(Pp, faces, weld, live) * gt).sum() -
                  (ref.normals64(Pm, faces, weld, live) * gt).sum()).item() / (2 * h)
            worst = max(worst, abs(fd - got[0, vi, d]))
    print("fp64 gradient against central differences: max |diff| %.3g of %.3g" % (worst, np.abs(got).max()))
    assert worst <= 1e-6 * np.abs(got).max() + 1e-9, worst


def test_tilt_fit_on_the_restatement(oracle):
    """The fit of tests/test_tri_normals_gpu.py on restatement (b): it recovers (a*, b*) to 0.01."""
    v0, faces = ref.tilt_grid(0.0, 0.0)
    f = faces.astype(np.int64)
    depth = oracle.tri_raster_fwd(np.ascontiguousarray(v0.numpy()[:, f, 0:3], np.float32), 48, 48)
    owner = tri_interp_ref.cpu_owners(depth, v0.numpy().astype(np.float32), faces)
    assert (owner >= 0).all()
    got = ref.tilt_fit(lambda v: ref.module64(v, owner, faces), torch.float64)
    print("tilt fit on the restatement:", got, "want", ref.FIT_TARGET)
    assert np.abs(got - np.array(ref.FIT_TARGET)).max() <= 0.01, got


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    """tests/test_kernel_resources_cpu.py's reading of the resource notes: every kernel of tri_normals.hip reports
    ScratchSize 0 and no spills."""
    from spherehand_amd import build
    out = str(tmp_path / "tri_normals.s")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                                                   "-I", os.path.join(build.PKG, "csrc"), "-o", out,
                                                   os.path.join(build.PKG, "csrc", "tri_normals.hip")],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = [int(s) for s in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(sizes) == 8 and max(sizes) == 0, sizes
    meta = text[text.index("amdhsa.kernels:"):]
    names = re.findall(r"\.name:\s+(\S+)", meta)
    assert len([n for n in names if "vertex_normals" in n]) == 4 and len([n for n in names if "unit3_maps" in n]) == 4, names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        vals = [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % key, meta)]
        assert len(vals) == 8 and max(vals) == 0, (key, vals)
