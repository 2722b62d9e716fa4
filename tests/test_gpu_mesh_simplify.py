"""GPU tests of the mesh simplification kernels (voge_mesh_simplify_scan / _emit / _attr; an extension, the reference and the oracle
have none) and of VoGE.Meshing.simplify_mesh on the device, against Aggregation.mesh_simplify, the definition, on the host.

integers   faces', vert_index, face_index, V' and F' torch.equal on every case of mesh_simplify_cases, under both placements;
values     verts' and attr' within POSITION_BOUND / ATTR_BOUND (derived in that module's header from the kernels' arithmetic); a
           cluster of one vertex bit for bit; the share of the bound used is logged;
and the same bits on a second run, under a permutation of the faces, over a workspace filled with 0x00, 0x7F and 0xFF, and the
three ValueErrors that come from the error word.  No test provokes a fault: the caps are reached through the error word only."""
import functools

import numpy as np
import pytest
import torch

import dirty as D
import mesh_simplify_cases as sc
from util import log_line
from voge_amd import Aggregation, ops
from voge_amd.Meshing import simplify_mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLACEMENTS = ("mean", "quadric")


@functools.lru_cache(maxsize=None)
def definition(name, placement, C):
    """Aggregation.mesh_simplify on the host, once per (case, placement, channels); nobody writes to what it returns"""
    v, f, h = sc.case(name)
    return Aggregation.mesh_simplify(v, f, h, placement, sc.attr_of(v, C) if C else None)


def on_device(name, C=0):
    v, f, h = sc.case(name)
    return v.to(DEV), f.to(torch.int32).to(DEV), h, (sc.attr_of(v, C).to(DEV) if C else None)


def check(name, placement, C, out, label=None):
    """out = simplify_mesh(..., return_index=True) on the device against the definition -> the shares of the two bounds used"""
    v, f, h = sc.case(name)
    rv, rf, ra, rvi, rfi = definition(name, placement, C)
    label = label or f"{name}, {placement}, C {C}"
    assert all(t.is_cuda for t in out) and out[0].dtype == torch.float32 and out[1].dtype == torch.int32
    got_v, got_f = out[0].cpu(), out[1].cpu()
    got_a = out[2].cpu() if C else None
    got_vi, got_fi = out[-2].cpu(), out[-1].cpu()
    assert got_vi.dtype == torch.int32 and got_fi.dtype == torch.int32
    assert got_v.shape == rv.shape and got_f.shape == rf.shape, (label, got_v.shape, rv.shape, got_f.shape, rf.shape)
    assert torch.equal(got_vi, rvi.to(torch.int32)), label
    assert torch.equal(got_fi, rfi.to(torch.int32)), label
    assert torch.equal(got_f, rf.to(torch.int32)), label
    on = rvi >= 0
    count = np.bincount(rvi[on].numpy(), minlength=len(rv))
    corners = np.bincount(rvi[f.reshape(-1)][rvi[f.reshape(-1)] >= 0].numpy(), minlength=len(rv)) if len(f) else np.zeros(len(rv), np.int64)
    bound = sc.position_bound(rv.numpy(), count, corners, v.numpy(), len(f), h, placement)
    s_v, err_v = sc.share(got_v.numpy(), rv.numpy(), bound)
    s_a = err_a = 0.0
    if C:
        assert got_a.shape == ra.shape
        s_a, err_a = sc.share(got_a.numpy(), ra.numpy(), sc.attr_bound(ra.numpy(), count, sc.attr_of(v, C).numpy(), len(v), channels=ops.MESH_SIMPLIFY_CHANNELS))
    log_line(f"[parity] simplify_mesh {label}: V {len(v)} -> {len(rv)}, F {len(f)} -> {len(rf)}, position error {err_v:.3e}, {s_v:.3f} of the "
             f"bound" + (f"; attr error {err_a:.3e}, {s_a:.3f} of the bound" if C else ""))
    assert s_v <= 1.0 and s_a <= 1.0, label
    return s_v, s_a


def run(name, placement, C=0):
    dv, df, h, da = on_device(name, C)
    return simplify_mesh(dv, df, h, placement, attr=da, return_index=True)


def test_the_cases_know_the_constants():
    assert ops.MESH_SIMPLIFY_BLOCK == sc.mcc.SCAN_BLOCK and ops.MESH_SIMPLIFY_TOP == sc.mcc.SCAN_TOP
    assert ops.MESH_SIMPLIFY_MAX_CELLS == sc.MAX_CELLS == Aggregation.MESH_SIMPLIFY_MAX_CELLS
    assert ops.MESH_SIMPLIFY_LAMBDA == sc.LAMBDA == Aggregation.MESH_SIMPLIFY_LAMBDA
    assert ops.mesh_simplify_scales(1024, 700) == (60 - sc._bits(1024), 60 - sc._bits(2100))
    # the table's capacity steps where the stepped cases put their vertex counts
    assert [ops.mesh_simplify_capacity(V, 700) for V in (1023, 1024, 1025)] == [2048, 2048, 4096]
    assert ops.mesh_simplify_capacity(4096, 6000) == 16384 and ops.mesh_simplify_capacity(20002, 64) == 65536


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_against_the_definition(name, placement):
    dv, df, h, da = on_device(name, 3)
    keep_v, keep_f, keep_a = dv.clone(), df.clone(), da.clone()
    out = simplify_mesh(dv, df, h, placement, attr=da, return_index=True)
    check(name, placement, 3, out)
    again = simplify_mesh(dv, df, h, placement, attr=da, return_index=True)      # the same bits on two runs
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(again, out))
    assert torch.equal(dv, keep_v) and torch.equal(df, keep_f) and torch.equal(da, keep_a)
    plain = simplify_mesh(dv, df, h, placement)
    assert len(plain) == 2 and torch.equal(plain[0], out[0]) and torch.equal(plain[1], out[1])


@pytest.mark.parametrize("C", [1, 8, 11])
def test_attribute_channels(C):
    for name, placement in (("torus, cell 2.0", "mean"), ("soup", "quadric")):
        out = run(name, placement, C)
        check(name, placement, C, out)
        assert torch.equal(out[0], run(name, placement)[0])      # the attribute does not touch the geometry


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_identity_and_empty_on_the_device(placement):
    v, f, h = sc.sphere24()
    dv, df, da = v.to(DEV), f.to(torch.int32).to(DEV), sc.attr_of(v, 3).to(DEV)
    v2, f2, a2, vi, fi = simplify_mesh(dv, df, 0.01 * h, placement, attr=da, return_index=True)
    assert torch.equal(v2, dv) and torch.equal(f2, df) and torch.equal(a2, da)
    assert torch.equal(vi.cpu().long(), torch.arange(len(v))) and torch.equal(fi.cpu().long(), torch.arange(len(f)))
    v2, f2, a2, vi, fi = simplify_mesh(dv, df, 100.0, placement, attr=da, return_index=True)
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and a2.shape == (0, 3) and fi.shape == (0,) and v2.is_cuda and f2.dtype == torch.int32
    assert vi.shape == (len(v),) and bool((vi == -1).all())
    z = torch.zeros((0, 3), device=DEV)
    for vv, ff in ((z, z.int()), (dv, z.int())):
        v2, f2 = simplify_mesh(vv, ff, 1.0, placement)
        assert v2.shape == (0, 3) and f2.shape == (0, 3)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", ["random field, cell 2.0", "soup", "one triple", "sized V 257 F 255"])
def test_a_permutation_of_the_faces(name, placement):
    """The same vertex bits and the same face SET (the survivor of a repeated triple is the first in the given order)"""
    dv, df, h, da = on_device(name, 3)
    base = simplify_mesh(dv, df, h, placement, attr=da, return_index=True)
    perm = torch.from_numpy(np.random.default_rng(11).permutation(len(df))).to(DEV)
    out = simplify_mesh(dv, df[perm].contiguous(), h, placement, attr=da, return_index=True)
    assert out[0].cpu().numpy().tobytes() == base[0].cpu().numpy().tobytes() and torch.equal(out[2], base[2]) and torch.equal(out[3], base[3])
    rot = lambda t: sorted(min((a, b, c), (b, c, a), (c, a, b)) for a, b, c in t.cpu().tolist())
    assert rot(out[1]) == rot(base[1])


@pytest.mark.parametrize("pattern", [0x00, 0x7F, 0xFF], ids=D.pattern_id)
def test_dirty_workspace(pattern):
    for name, placement in (("two spheres, cell 2.0", "quadric"), ("stepped V 1025", "mean")):
        clean = run(name, placement, 11)
        with D.dirty(pattern) as d:
            out = run(name, placement, 11)
            assert d.filled > 0 and len(d.taken) == 1 and d.taken[0][0] <= D.GROW, d.taken
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(out, clean)), (name, D.pattern_id(pattern))


def test_the_errors_of_the_error_word():
    v, f = sc.small_soup()
    dv, df = v.to(DEV), f.to(torch.int32).to(DEV)
    bad = df.clone()
    bad[2, 1] = 8
    with pytest.raises(ValueError, match="outside"):
        simplify_mesh(dv, bad, 1.0)
    bad[2, 1] = -1
    with pytest.raises(ValueError, match="outside"):
        simplify_mesh(dv, bad, 1.0, "quadric")
    nan = dv.clone()
    nan[3, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        simplify_mesh(nan, df, 1.0)
    nan[3, 1] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        simplify_mesh(nan, df, 1.0)
    with pytest.raises(ValueError, match="cells"):
        simplify_mesh(dv, df, 1e-7)
    assert len(simplify_mesh(dv, df, 1.0)[1]) == 3      # and the next call is as good as ever
