"""GPU tests of the mesh clean-up kernels (voge_mesh_components, voge_mesh_clean_scan / _emit, voge_vertex_normals; an extension, the
reference and the oracle have none) and of VoGE.Meshing's connected_components, clean_mesh and vertex_normals on the device.

labels, faces  torch.equal against the definitions (Aggregation.mesh_components / mesh_clean on the host) on every case of
               mesh_clean_cases; verts' bit for bit;
normals        against the fp64 reference at mesh_clean_cases' NORMAL_BOUND (derived in that module's header), leaving out only the
               vertices whose sum cancels below 1 / 32 of its terms, at most 1 % of a case's used vertices;
and the same bits on a second run, under a permutation of the faces, with the inputs unchanged."""
import numpy as np
import pytest
import torch

import mesh_clean_cases as cc
from util import log_line
from voge_amd import Aggregation, ops
from voge_amd.Meshing import clean_mesh, connected_components, vertex_normals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CHOICES = [(None, 1), (1, 1), (3, 2), (None, 50), (250, 1)]


def on_device(name):
    verts, faces = cc.case(name)
    return verts.to(DEV), faces.to(torch.int32).to(DEV)


def test_the_cases_know_the_scan_sizes():
    assert cc.SCAN_BLOCK == ops.MESH_CLEAN_BLOCK and cc.SCAN_TOP == ops.MESH_CLEAN_TOP


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_components_labels_and_repeat_runs(name):
    verts, faces = cc.case(name)
    ref_v, ref_f, ref_n = Aggregation.mesh_components(faces, len(verts))
    dv, df = on_device(name)
    before = df.clone()
    vert_label, face_label, n = connected_components(df, len(verts))
    assert vert_label.is_cuda and vert_label.dtype == torch.int32 and face_label.dtype == torch.int32 and isinstance(n, int)
    assert torch.equal(vert_label.cpu(), ref_v.to(torch.int32)) and torch.equal(face_label.cpu(), ref_f.to(torch.int32)) and n == ref_n
    again = connected_components(df, len(verts))
    assert torch.equal(again[0], vert_label) and torch.equal(again[1], face_label) and again[2] == n
    count = ops.mesh_components(df, len(verts), return_count=True)[3]
    assert torch.equal(count.cpu().long(), torch.bincount(ref_f, minlength=len(verts)))
    assert torch.equal(df, before)
    if len(faces):
        assert connected_components(df)[2] == n      # num_verts from the largest index


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_clean_mesh_against_the_definition(name):
    verts, faces = cc.case(name)
    dv, df = on_device(name)
    keep_v, keep_f = dv.clone(), df.clone()
    choices = CHOICES if len(faces) < 150000 else CHOICES[1:4]
    for keep_largest, min_faces in choices:
        ref = Aggregation.mesh_clean(verts, faces, keep_largest, min_faces)
        out = clean_mesh(dv, df, keep_largest, min_faces, return_index=True)
        assert all(t.is_cuda for t in out) and out[0].dtype == torch.float32 and all(t.dtype == torch.int32 for t in out[1:])
        label = f"{name}, keep_largest {keep_largest}, min_faces {min_faces}"
        for got, want in zip(out[1:], ref[1:]):
            assert torch.equal(got.cpu(), want.to(torch.int32)), label
        assert out[0].cpu().numpy().tobytes() == ref[0].numpy().tobytes(), label
        again = clean_mesh(dv, df, keep_largest, min_faces, return_index=True)
        assert all(torch.equal(a, b) for a, b in zip(again, out)), label
        assert len(clean_mesh(dv, df, keep_largest, min_faces)) == 2
    assert torch.equal(dv, keep_v) and torch.equal(df, keep_f)


def test_keep_all_returns_the_input_bit_for_bit():
    for name in ("sphere", "two spheres", "strip permuted", "fan, hub last"):
        dv, df = on_device(name)
        v2, f2, vi, fi = clean_mesh(dv, df, return_index=True)
        assert torch.equal(v2, dv) and torch.equal(f2, df)
        assert torch.equal(vi.long().cpu(), torch.arange(len(dv))) and torch.equal(fi.long().cpu(), torch.arange(len(df)))


@pytest.mark.parametrize("name", ["two spheres", "soup", "strip permuted", "fan, hub last", "crumbs", "sized V 257 F 255",
                                  "sized V 262145 F 262143"])
def test_a_permutation_of_the_faces(name):
    verts, faces = cc.case(name)
    dv, df = on_device(name)
    perm = torch.from_numpy(np.random.default_rng(7).permutation(len(faces)))
    pf = df[perm.to(DEV)].contiguous()
    vert_label, face_label, n = connected_components(df, len(verts))
    p_vert, p_face, p_n = connected_components(pf, len(verts))
    assert torch.equal(p_vert, vert_label) and torch.equal(p_face, face_label[perm.to(DEV)]) and p_n == n
    assert torch.equal(vertex_normals(dv, pf), vertex_normals(dv, df))
    ref = Aggregation.mesh_clean(verts, faces[perm], 3, 1)
    out = clean_mesh(dv, pf, 3, 1, return_index=True)
    assert out[0].cpu().numpy().tobytes() == ref[0].numpy().tobytes()
    assert all(torch.equal(g.cpu(), w.to(torch.int32)) for g, w in zip(out[1:], ref[1:]))


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_vertex_normals_at_the_derived_bound(name):
    verts, faces = cc.case(name)
    dv, df = on_device(name)
    keep_v, keep_f = dv.clone(), df.clone()
    got = vertex_normals(dv, df)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (len(verts), 3)
    assert torch.equal(vertex_normals(dv, df), got)
    assert torch.equal(dv, keep_v) and torch.equal(df, keep_f)
    if len(verts) == 0:
        return
    if name in cc.EXTRACTION_COMPONENTS:      # the bound speaks about every vertex of an extraction
        _, _, compared, used = cc.normal_bound(verts.numpy(), faces.numpy())
        assert compared.sum() == used.sum() == len(verts)
    cc.check_normals(name, got.cpu().numpy(), verts.numpy(), faces.numpy(), log=log_line)


def test_vertex_normals_special_values():
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [9, 9, 9], [float("nan"), 0, 0], [3, 3, 3]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 1], [1, 2, 3], [3, 5, 6]])
    want = Aggregation.mesh_vertex_normals(verts.double(), faces)
    got = vertex_normals(verts.to(DEV), faces.to(torch.int32).to(DEV)).cpu()
    assert torch.isfinite(got).all()
    for v in (0, 3, 4, 5, 6):      # cancelled, a NaN term, unused, a NaN term twice
        assert torch.equal(got[v], torch.zeros(3)) and torch.equal(want[v], torch.zeros(3, dtype=torch.float64))
    assert float((got.double() - want).abs().max()) < 1e-6
    # no faces at all: zeros
    assert torch.equal(vertex_normals(verts.to(DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV)).cpu(), torch.zeros(7, 3))


def test_invalid_indices_raise():
    verts, faces = cc.case("one face")
    dv = verts.to(DEV)
    for bad in ([[0, 1, 4]], [[0, -1, 2]]):
        df = torch.tensor(bad, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError):
            connected_components(df, 4)
        with pytest.raises(ValueError):
            clean_mesh(dv, df)
    with pytest.raises(ValueError):
        clean_mesh(dv, faces.to(torch.int32).to(DEV), keep_largest=0)
    with pytest.raises(ValueError):
        clean_mesh(dv, faces.to(torch.int32).to(DEV), min_faces=0)
    # the other dtypes take the definitions, on the device
    out = clean_mesh(dv.double(), faces.to(DEV), return_index=True)
    assert out[0].dtype == torch.float64 and out[0].is_cuda and all(t.dtype == torch.int32 for t in out[1:])
    assert connected_components(faces.to(DEV), 4)[0].dtype == torch.int32
