"""CPU tests of the mesh clean-up definitions (Aggregation.mesh_components, mesh_clean, mesh_vertex_normals) and of the host route of
VoGE.Meshing's connected_components, clean_mesh and vertex_normals, against mesh_clean_cases' independent reference (a plain
union-find, a brute-force ranking) and its derived normal bound.  Integers are compared exactly."""
import numpy as np
import pytest
import torch

import mesh_clean_cases as cc
from util import log_line
from voge_amd import Aggregation
from voge_amd.Meshing import clean_mesh, connected_components, vertex_normals


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_components_against_the_union_find(name):
    verts, faces = cc.case(name)
    ref_v, ref_f, ref_n = cc.reference_components(name)
    vert_label, face_label, n = Aggregation.mesh_components(faces, len(verts))
    assert vert_label.dtype == torch.int64 and face_label.dtype == torch.int64
    assert np.array_equal(vert_label.numpy(), ref_v) and np.array_equal(face_label.numpy(), ref_f) and n == ref_n
    if name in cc.EXTRACTION_COMPONENTS:
        assert n == cc.EXTRACTION_COMPONENTS[name]
    if name.startswith(("strip", "fan")):
        assert n == 1 and int(vert_label.max()) == 0
    # unused vertices carry their own index and are no component
    used = np.zeros(len(verts), bool)
    used[faces.numpy().reshape(-1)] = True
    assert np.array_equal(vert_label.numpy()[~used], np.nonzero(~used)[0])
    assert n == len(np.unique(vert_label.numpy()[used]))


def assert_clean(label, verts, faces, out, keep_largest, min_faces):
    ref_v, ref_f, ref_vi, ref_fi = cc.clean(verts.numpy(), faces.numpy(), keep_largest, min_faces)
    v2, f2, vi, fi = (t.cpu().numpy() for t in out)
    assert np.array_equal(fi, ref_fi) and np.array_equal(vi, ref_vi), label
    assert np.array_equal(f2, ref_f), label
    assert v2.tobytes() == ref_v.tobytes(), label
    # the properties, from the outputs alone
    assert v2.tobytes() == verts.numpy()[vi].tobytes()
    assert np.array_equal(vi[f2.reshape(-1)].reshape(-1, 3), faces.numpy()[fi])
    assert (np.diff(vi) > 0).all() and (np.diff(fi) > 0).all()
    assert len(f2) == 0 or len(np.unique(f2)) == len(v2)


CHOICES = [(None, 1), (1, 1), (2, 1), (3, 2), (None, 2), (None, 50), (250, 1), (10 ** 6, 1), (1, 10 ** 6)]


@pytest.mark.parametrize("name", ["two spheres", "random field", "soup", "strip permuted", "fan, hub last", "crumbs", "no faces", "no vertices",
                                  "one face", "sized V 255 F 257", "sized V 257 F 255"])
def test_clean_against_the_brute_force_ranking(name):
    verts, faces = cc.case(name)
    for keep_largest, min_faces in CHOICES:
        out = Aggregation.mesh_clean(verts, faces, keep_largest, min_faces)
        assert out[0].dtype == verts.dtype and all(t.dtype == torch.int64 for t in out[1:])
        assert_clean(f"{name}, keep_largest {keep_largest}, min_faces {min_faces}", verts, faces, out, keep_largest, min_faces)


def test_keep_all_is_the_identity_and_ties_go_to_the_lower_label():
    for name in ("sphere", "two spheres", "strip descending"):
        verts, faces = cc.case(name)
        v2, f2, vi, fi = Aggregation.mesh_clean(verts, faces)
        assert v2.numpy().tobytes() == verts.numpy().tobytes() and torch.equal(f2, faces)
        assert torch.equal(vi, torch.arange(len(verts))) and torch.equal(fi, torch.arange(len(faces)))
    # three components of two faces each, at the labels 0, 4 and 8, and one of one face
    faces = torch.tensor([[8, 9, 10], [0, 1, 2], [4, 5, 6], [2, 1, 3], [12, 13, 14], [6, 5, 7], [10, 9, 11]])
    verts = torch.arange(45, dtype=torch.float32).reshape(15, 3)
    for k, labels in ((1, [0]), (2, [0, 4]), (3, [0, 4, 8]), (4, [0, 4, 8, 12])):
        _, _, vi, fi = Aggregation.mesh_clean(verts, faces, keep_largest=k)
        comp = Aggregation.mesh_components(faces, 15)[1]
        assert sorted(set(comp[fi].tolist())) == labels
        assert cc.brute_force_keep(comp.numpy(), 15, k) == set(labels)
    # crumbs: 19 600 single triangles tie at one face; the first of them by label wins the last place
    verts, faces = cc.case("crumbs")
    _, face_label, n = Aggregation.mesh_components(faces, len(verts))
    assert n == 1 + 200 + 19600
    _, _, _, fi = Aggregation.mesh_clean(verts, faces, keep_largest=203)
    singles = sorted(l for l, c in zip(*np.unique(face_label.numpy(), return_counts=True)) if c == 1)
    assert set(face_label[fi].tolist()) == cc.brute_force_keep(face_label.numpy(), len(verts), 203) and singles[0] in face_label[fi].tolist() \
        and singles[1] in face_label[fi].tolist() and singles[2] not in face_label[fi].tolist()


@pytest.mark.parametrize("name", ["sphere", "torus", "two spheres", "random field", "soup", "strip permuted", "fan, hub first", "fan, hub last",
                                  "crumbs", "one face", "sized V 257 F 255"])
def test_vertex_normals_fp32_against_fp64_at_the_derived_bound(name):
    verts, faces = cc.case(name)
    got = Aggregation.mesh_vertex_normals(verts, faces)
    assert got.dtype == torch.float32 and got.shape == verts.shape
    if name in cc.EXTRACTION_COMPONENTS:      # the bound speaks about every vertex of an extraction
        _, _, compared, used = cc.normal_bound(verts.numpy(), faces.numpy())
        assert compared.sum() == used.sum() == len(verts)
    cc.check_normals(f"{name} (fp32 definition)", got.numpy(), verts.numpy(), faces.numpy(), fixed_point=False, log=log_line)
    # the fp64 definition is the reference's formula
    ref, _, compared, _ = cc.normal_bound(verts.numpy(), faces.numpy())
    got64 = Aggregation.mesh_vertex_normals(verts.double(), faces).numpy()
    assert np.abs(got64 - ref)[compared].max(initial=0.0) < 1e-12


def test_vertex_normals_special_values_and_gradient():
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [9, 9, 9], [float("nan"), 0, 0], [3, 3, 3]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 1], [1, 2, 3], [3, 5, 6]])
    n = Aggregation.mesh_vertex_normals(verts, faces)
    assert torch.equal(n[0], torch.zeros(3)) and torch.equal(n[4], torch.zeros(3))      # cancelled, unused
    assert torch.equal(n[3], torch.zeros(3)) and torch.equal(n[5], torch.zeros(3)) and torch.equal(n[6], torch.zeros(3))      # a NaN term
    assert torch.isfinite(n).all() and abs(float(n[1].norm()) - 1) < 1e-6
    # a face that names a vertex twice has no area and adds nothing; a sphere's normals point outwards
    v, f = cc.case("sphere")
    n = Aggregation.mesh_vertex_normals(v, f)
    centre = torch.tensor([5.3, 5.6, 5.45])
    assert ((n * (v - centre)).sum(-1) > 0).all()
    assert torch.equal(Aggregation.mesh_vertex_normals(v, torch.cat([f, f[:5, [0, 0, 1]]])), n)
    vd = v.double().requires_grad_(True)
    Aggregation.mesh_vertex_normals(vd, f)[:, 0].sum().backward()
    assert torch.isfinite(vd.grad).all() and float(vd.grad.abs().max()) > 0


def test_every_value_error():
    verts, faces = cc.case("one face")
    for bad in (torch.tensor([[0, 1, 4]]), torch.tensor([[0, -1, 2]])):
        with pytest.raises(ValueError):
            Aggregation.mesh_components(bad, 4)
        with pytest.raises(ValueError):
            connected_components(bad, 4)
        with pytest.raises(ValueError):
            clean_mesh(verts, bad)
    with pytest.raises(ValueError):
        connected_components(faces, 0)
    for kw in (dict(keep_largest=0), dict(min_faces=0), dict(keep_largest=-1), dict(keep_largest=2, min_faces=-3)):
        with pytest.raises(ValueError):
            clean_mesh(verts, faces, **kw)
        with pytest.raises(ValueError):
            Aggregation.mesh_clean(verts, faces, **kw)
    for fn in (clean_mesh, vertex_normals):
        with pytest.raises(ValueError):
            fn(verts[:, :2], faces)
        with pytest.raises(ValueError):
            fn(verts, faces[:, :2])
        with pytest.raises(ValueError):
            fn(verts, faces.float())
    with pytest.raises(ValueError):
        connected_components(faces.reshape(-1))


@pytest.mark.parametrize("face_dtype", [torch.int32, torch.int64])
def test_host_route_returns_the_documented_dtypes(face_dtype):
    verts, faces = cc.case("two spheres")
    faces = faces.to(face_dtype)
    vert_label, face_label, n = connected_components(faces)
    assert vert_label.dtype == torch.int32 and face_label.dtype == torch.int32 and isinstance(n, int) and n == 2
    assert vert_label.shape == (len(verts),) and face_label.shape == (len(faces),)
    assert torch.equal(connected_components(faces, len(verts) + 3)[0][-3:], torch.arange(len(verts), len(verts) + 3, dtype=torch.int32))
    for v in (verts, verts.double()):
        out = clean_mesh(v, faces, keep_largest=1)
        assert len(out) == 2 and out[0].dtype == v.dtype and out[1].dtype == torch.int32
        out = clean_mesh(v, faces, keep_largest=1, return_index=True)
        assert len(out) == 4 and all(t.dtype == torch.int32 for t in out[1:])
        assert connected_components(out[1])[2] == 1
        assert_clean("host route", verts, faces, (out[0].float(),) + out[1:], 1, 1)
        normals = vertex_normals(v, faces)
        assert normals.dtype == torch.float32 and normals.shape == (len(verts), 3)
    assert not clean_mesh(verts.requires_grad_(True), faces)[0].requires_grad
    verts.requires_grad_(False)
    import VoGE.Meshing
    assert all(hasattr(VoGE.Meshing, k) for k in ("connected_components", "clean_mesh", "vertex_normals"))
    assert {"connected_components", "clean_mesh", "vertex_normals"} <= set(VoGE.Meshing.__all__)
