"""GPU tests of the mesh regularisers (voge_amd.Losses.mesh_regularisers -> ops._MeshReg: voge_mesh_reg_fwd / _bwd; an extension,
the reference and the oracle have none).

The reference is the DEFINITION (Aggregation.mesh_edge_term / mesh_laplacian_term / mesh_normal_term) in fp64 on the host from the
fp32-rounded inputs; tests/test_mesh_reg_cpu.py pins it against an independent numpy restatement and central differences.

Meshes: demo/ShapeFitting.ico_sphere(level) scaled radially by 1 + noise * U(-1, 1), np.random.default_rng(3), one draw of shape
(V, 1); noise 0.15 / 0.15 / 0.1 at levels 1 / 2 / 3 (V = 42 / 162 / 642; level 3 has 4 482 items: 18 workgroups, the last one
ragged).  Target length 0.25.  On these inputs every face angle's sine is >= 0.52 and min |L_i| >= 0.011 x the longest edge
(fp64); each sphere test asserts sine >= 0.3 and |L_i| >= 0.005 x the longest edge on its own inputs before it compares, so no
case is masked out.

Values (derived from rounding counts, not tuned; eps = 2^-23):
  edge       |got - ref| <= 32 eps mean(len^2 + t^2)      an item is ~8 fp32 roundings of terms <= len^2 + t^2
  laplacian  |got - ref| <= (d_max + 8) eps (longest edge)  a sum of d differences, a norm
  normal     |got - ref| <= 64 eps                         two cross products, two norms, a quotient of terms <= 1
  The reduction adds 8 fp32 additions to a partial (a butterfly of 6 over the wave, 2 over the four waves) and is fp64 from there:
  well under the ~20 the constants allow for, so they stand.  (The kernel evaluates the laplacian and the pairs in fp64, so those
  two are good to the one fp32 rounding of an item, about eps / 2 of the scale.)
Gradients: of each term ALONE, seeded with 1: |got - want| <= 1e-5 max|want| -- the project's bar for an fp64 chain on fp32 inputs,
  relative to the gradient's OWN maximum and not max(1, .): these gradients are ~1 / V.  A gradient whose reference is all zero
  must be all zero.  The measured ratios go to util.log_line.

The fan around a vertex of degree 300 is a SMOOTH surface (ring radius 1 + 0.1 sin 5a, height 0.2 sin 3a, the hub lifted off it):
its faces are slivers of angle 2 pi / 300 at the hub, whose normals amplify every rounding by 1 / sin = 48; the kernel's pairs
are fp64, so the stated bounds hold there too."""
import numpy as np
import pytest
import torch

from test_mesh_reg_cpu import definition, hand_cases, noisy_sphere, shape_fitting_demo
from util import log_line

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23
T = 0.25
NODE = "_MeshRegBackward"
NAMES = ("edge", "laplacian", "normal")
SPHERES = {1: 0.15, 2: 0.15, 3: 0.1}


def dev(a, rg=False, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=rg)


def topology(faces, num_verts=None):
    from voge_amd.Losses import MeshTopology
    return MeshTopology(faces=faces, num_verts=num_verts, device=DEV)


REFS = {}


def reference(key, verts32, topo, t):
    """fp64 definition on the host from the fp32-rounded inputs -> (values [3], gradients [3][..,V,3]); once per case."""
    if key not in REFS:
        REFS[key] = definition(np.asarray(verts32, np.float32).astype(np.float64), topo.to("cpu"), t)
    return REFS[key]


def run_kernel(verts32, topo, t, terms=NAMES):
    """one fused forward -> (values [3] fp32 array, gradient of each term alone, the output tensors)"""
    from voge_amd.Losses import mesh_regularisers
    v = dev(verts32, rg=True)
    out = mesh_regularisers(v, topo, t, terms)
    assert all(type(o.grad_fn).__name__ == NODE for o in out), [type(o.grad_fn).__name__ for o in out]      # the kernel, not the definition
    grads = [torch.autograd.grad(o, v, retain_graph=True)[0].cpu().numpy() for o in out]
    return np.asarray([float(o.detach()) for o in out], np.float32), grads, out


def scales(verts32, topo, t):
    """the three value bounds and the longest edge, from the fp32-rounded inputs in fp64"""
    v = np.asarray(verts32, np.float32).astype(np.float64)
    v = v.reshape(-1, v.shape[-2], 3)
    e = topo.to("cpu").edges.numpy()
    length = np.linalg.norm(v[:, e[:, 0]] - v[:, e[:, 1]], axis=-1) if len(e) else np.zeros((1, 1))
    longest = float(length.max())
    return (32 * EPS * float((length ** 2 + t * t).mean()), (topo.max_degree + 8) * EPS * longest, 64 * EPS), longest


def compare(label, verts32, topo, t):
    want, want_g = reference(label, verts32, topo, t)
    got, got_g, _ = run_kernel(verts32, topo, t)
    bound, _ = scales(verts32, topo, t)
    assert np.isfinite(got).all() and all(np.isfinite(g).all() for g in got_g)
    for k, name in enumerate(NAMES):
        err = abs(float(got[k]) - want[k])
        gmax = float(np.abs(want_g[k]).max()) if want_g[k].size else 0.0
        gerr = float(np.abs(got_g[k] - want_g[k]).max()) if want_g[k].size else 0.0
        log_line(f"[parity] mesh_reg {label} {name}: value error {err:.2e} = {err / bound[k]:.3f} of its bound {bound[k]:.2e}; "
                 f"gradient error {gerr:.2e} = {gerr / gmax if gmax else 0.0:.2e} of max|want| {gmax:.2e} (tolerance 1.0e-05)")
        assert err <= bound[k], (label, name, float(got[k]), want[k], bound[k])
        assert gerr <= 1e-5 * gmax, (label, name, gerr, gmax)
    return got, got_g


def well_conditioned(verts32, faces, topo):
    """(min sine of a face angle, min |L_i| / longest edge) of one mesh in fp64"""
    v = np.asarray(verts32, np.float64)
    sines = []
    for k in range(3):
        a, b = v[faces[:, (k + 1) % 3]] - v[faces[:, k]], v[faces[:, (k + 2) % 3]] - v[faces[:, k]]
        sines.append(np.linalg.norm(np.cross(a, b), axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1)))
    host = topo.to("cpu")
    off, nbr = host.nbr_off.numpy(), host.nbr.numpy()
    L = np.stack([(v[nbr[off[i]:off[i + 1]]] - v[i]).mean(0) for i in range(v.shape[0])])
    return float(np.min(sines)), float(np.linalg.norm(L, axis=-1).min() / scales(verts32, topo, T)[1])


@pytest.fixture(scope="module")
def spheres(hip_lib):
    """level -> (verts32, faces, topology on the device)"""
    out = {}
    for level, noise in SPHERES.items():
        v, f = noisy_sphere(level, noise)
        out[level] = (v, f, topology(f))
    return out


# ---- values and gradients ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 3])
def test_noisy_spheres(spheres, level):
    v, f, topo = spheres[level]
    assert topo.num_verts == {1: 42, 2: 162, 3: 642}[level] and topo.num_edges == topo.num_pairs == 3 * (topo.num_verts - 2)
    sine, lap = well_conditioned(v, f, topo)
    log_line(f"[parity] mesh_reg sphere {level}: min sine {sine:.3f}, min |L| / longest edge {lap:.4f}")
    assert sine >= 0.3 and lap >= 0.005
    compare(f"sphere{level}", v, topo, T)


@pytest.mark.parametrize("name", list(hand_cases()))
def test_hand_cases(hip_lib, name):
    verts, faces, nv, t = hand_cases()[name]
    got, got_g = compare(name, verts.astype(np.float32), topology(faces, nv), t)
    if name == "zero_area":
        assert got[2] == 1.0 and (got_g[2] == 0).all()
    if name.startswith("fold"):
        assert got[2] == {"fold_flat": 0.0, "fold_right_angle": 1.0, "fold_back": 2.0}[name]
    if name == "fold_flat":
        assert (got_g[2] == 0).all()
    if name == "hexagon_hub":
        assert (got_g[1][0] == 0).all()
    if name == "lone_triangle":
        assert got[2] == 0.0 and (got_g[2] == 0).all()      # no pairs
    if name == "unused_vertex":
        assert all((g[4] == 0).all() for g in got_g)


def test_hub_of_degree_300(hip_lib):
    n = 300
    a = 2 * np.pi * np.arange(n) / n
    r = 1 + 0.1 * np.sin(5 * a)
    ring = np.stack([r * np.cos(a), r * np.sin(a), 0.2 * np.sin(3 * a)], -1)
    verts = np.concatenate([[(0.05, 0.02, 0.3)], ring]).astype(np.float32)
    faces = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], -1)
    topo = topology(faces)
    assert (topo.max_degree, topo.num_edges, topo.num_pairs) == (300, 600, 300)
    compare("hub300", verts, topo, T)


def test_translated_mesh_keeps_the_bounds(spheres):
    """Level 2 moved by (1000, 1000, 1000) BEFORE the rounding to fp32: positions carry 6e-5 of rounding, edges are 0.3 long.  The
    bounds are the same, on the edge-length scale -- what a Laplacian that sums positions (d terms of 1000, minus d * 1000) misses
    by three orders of magnitude."""
    v, f = noisy_sphere(2, SPHERES[2], shift=1000.0)
    topo = spheres[2][2]
    assert np.abs(v).min() > 998
    sine, lap = well_conditioned(v, f, topo)
    assert sine >= 0.3 and lap >= 0.005
    compare("sphere2+1000", v, topo, T)


def test_batch_is_the_mean_of_its_meshes(spheres):
    _, f, topo = spheres[2]
    batch = np.stack([noisy_sphere(2, noise, seed=3 + i)[0] for i, noise in enumerate((0.15, 0.1, 0.05))])
    got, got_g = compare("batch3", batch, topo, T)
    singles = [run_kernel(x, topo, T) for x in batch]
    bound, _ = scales(batch, topo, T)
    for k in range(3):
        assert abs(float(got[k]) - np.mean([float(s[0][k]) for s in singles])) <= bound[k]
        want = np.stack([s[1][k] for s in singles]) / 3
        assert np.abs(got_g[k] - want).max() <= 1e-5 * np.abs(want).max()


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def test_single_terms_equal_the_fused_call_bit_for_bit(spheres):
    from voge_amd.Losses import mesh_edge_loss, mesh_laplacian_smoothing, mesh_normal_consistency, mesh_regularisers
    verts, _, topo = spheres[3]
    fused, fused_g, _ = run_kernel(verts, topo, T)
    for k, fn in enumerate((lambda x: mesh_edge_loss(x, topo, T), lambda x: mesh_laplacian_smoothing(x, topo),
                            lambda x: mesh_normal_consistency(x, topo))):
        v = dev(verts, rg=True)
        out = fn(v)
        assert type(out.grad_fn).__name__ == NODE and out.dim() == 0
        out.backward()
        assert float(out.detach()) == float(fused[k]) and np.array_equal(v.grad.cpu().numpy(), fused_g[k]), NAMES[k]
    # a term left out: an exact 0, and a zero gradient from it; the others keep their bits
    for k, name in enumerate(NAMES):
        terms = tuple(x for x in NAMES if x != name)
        v = dev(verts, rg=True)
        out = mesh_regularisers(v, topo, T, terms)
        assert float(out[k].detach()) == 0.0
        g = torch.autograd.grad(out[k], v, retain_graph=True, allow_unused=True)[0]
        assert g is None or (g == 0).all()
        for j in range(3):
            if j != k:
                assert float(out[j].detach()) == float(fused[j])
                assert np.array_equal(torch.autograd.grad(out[j], v, retain_graph=True)[0].cpu().numpy(), fused_g[j])
    # all three at once, weighted: the sum of the single gradients to the rounding of the sum
    v = dev(verts, rg=True)
    e, lap, nrm = mesh_regularisers(v, topo, T)
    (1.0 * e + 0.1 * lap + 0.5 * nrm).backward()
    want = fused_g[0].astype(np.float64) + 0.1 * fused_g[1] + 0.5 * fused_g[2]
    assert np.abs(v.grad.cpu().numpy() - want).max() <= 4 * EPS * np.abs(want).max()


def test_two_runs_give_identical_bits(spheres):
    verts, _, topo = spheres[3]
    a, b = run_kernel(verts, topo, T), run_kernel(verts, topo, T)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    batch = np.stack([verts, verts * 1.25, verts * 0.5])
    a, b = run_kernel(batch, topo, T), run_kernel(batch, topo, T)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_fused_call_is_one_autograd_node(spheres):
    from voge_amd.Losses import mesh_regularisers
    verts, _, topo = spheres[1]
    v = dev(verts, rg=True)
    e, lap, nrm = mesh_regularisers(v, topo, T)
    seen, todo = set(), [(e + 0.1 * lap + nrm).grad_fn]
    while todo:
        fn = todo.pop()
        if fn is not None and fn not in seen:
            seen.add(fn)
            todo += [n for n, _ in fn.next_functions]
    assert [type(fn).__name__ for fn in seen].count(NODE) == 1
    with pytest.raises(RuntimeError):      # once_differentiable: no double backward
        g, = torch.autograd.grad(e, v, create_graph=True)
        g.sum().backward()


def test_graph_capture_and_replay(spheres):
    """Level 2 captured once and replayed twice after the vertices were changed in place: the eager bits each time."""
    from voge_amd.Losses import mesh_regularisers
    _, _, topo = spheres[2]
    sets = [noisy_sphere(2, 0.15, seed=s)[0] for s in (3, 4, 5)]
    eager = [run_kernel(x, topo, T) for x in sets]
    v = dev(sets[0], rg=True)
    vals, grad = torch.zeros(3, device=DEV), torch.zeros_like(v)

    def step():
        out = mesh_regularisers(v, topo, T)
        g, = torch.autograd.grad(out[0] + out[1] + out[2], v)
        vals.copy_(torch.stack([o.detach() for o in out]))
        grad.copy_(g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in (1, 2, 0):
        with torch.no_grad():
            v.copy_(dev(sets[k]))
        graph.replay()
        torch.cuda.synchronize()
        x = dev(sets[k], rg=True)
        out = mesh_regularisers(x, topo, T)
        want_g, = torch.autograd.grad(out[0] + out[1] + out[2], x)
        assert np.array_equal(vals.cpu().numpy(), eager[k][0]), k
        assert torch.equal(grad, want_g), k


def test_other_dtypes_and_host_tensors_take_the_definition(spheres):
    from voge_amd.Losses import mesh_regularisers
    verts, _, topo = spheres[1]
    want, want_g = reference("sphere1", verts, topo, T)
    for v, tp in ((dev(verts, rg=True, dtype=torch.float64), topo), (torch.tensor(verts, dtype=torch.float64, requires_grad=True), topo),
                  (dev(verts, rg=True, dtype=torch.float64), topo.to("cpu"))):
        out = mesh_regularisers(v, tp, T)
        assert all(type(o.grad_fn).__name__ != NODE and o.dtype == torch.float64 and o.device == v.device for o in out)
        np.testing.assert_allclose([float(o.detach()) for o in out], want, rtol=1e-12)
        g, = torch.autograd.grad(out[0] + out[1] + out[2], v)
        np.testing.assert_allclose(g.cpu().numpy(), want_g[0] + want_g[1] + want_g[2], rtol=0, atol=1e-12)
    out = mesh_regularisers(torch.tensor(verts), topo, T)      # fp32 on the host: the definition in fp32
    np.testing.assert_allclose([float(o) for o in out], want, rtol=1e-5)
    empty = mesh_regularisers(torch.zeros((0, topo.num_verts, 3), device=DEV, requires_grad=True), topo, T)
    assert [float(o.detach()) for o in empty] == [0.0, 0.0, 0.0]


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def test_shape_fitting_loop_with_regularisers(hip_lib):
    """BatchedIteration at level 2, 64 x 64, 150 iterations, without and with the default regularisers (edge 1.0, laplacian 0.1,
    normal 0): the silhouette loss falls in both runs, and the final Laplacian term is lower with them.  Inequalities only."""
    from voge_amd.Losses import MeshTopology, mesh_laplacian_smoothing
    demo = shape_fitting_demo()
    topo = MeshTopology(faces=demo.ico_sphere(2)[1])
    final = {}
    for label, reg in (("plain", None), ("regularised", dict(demo.REGULARISER_WEIGHTS))):
        h = demo.fit(iters=150, level=2, size=64, quiet=True, regularise=reg)
        sil = np.asarray(h["silhouette"])
        assert np.isfinite(sil).all() and np.isfinite(h["final_verts"]).all()
        assert sil[-20:].mean() < sil[:5].mean(), (label, sil[:5].mean(), sil[-20:].mean())
        final[label] = float(mesh_laplacian_smoothing(torch.tensor(h["final_verts"], dtype=torch.float64), topo))
        log_line(f"[parity] mesh_reg loop {label}: silhouette {sil[:5].mean():.5f} -> {sil[-20:].mean():.5f}, laplacian {final[label]:.5f}")
    assert final["regularised"] < final["plain"], final
