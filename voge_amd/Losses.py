"""Mesh regularisers for shape fitting (an extension: the reference's demo/ShapeFitting.py imports mesh_edge_loss,
mesh_laplacian_smoothing and mesh_normal_consistency from PyTorch3D, which is not available here).

A MeshTopology is built ONCE on the host from the faces (or from a plain edge list) and holds int32 tables on the device;
mesh_regularisers evaluates the three terms of a vertex set over it as ONE autograd node.  The terms are defined in torch in
Aggregation.mesh_edge_term / mesh_laplacian_term / mesh_normal_term; fp32 vertices on the HIP device that holds the tables take
the kernels of voge_amd/csrc/mesh_reg.hip (ops._MeshReg: two launches forward, one backward, no atomics, the same bits on every
run), everything else -- host tensors, other dtypes, vertices on another device than the tables -- takes the definitions.
The cotangent ("cot", "cotcurv") Laplacians of PyTorch3D and a normal term on per-vertex normals are out of scope.

chamfer_distance is the fourth loss that demo imports: the score of a fit against the points it should reach.  Its definition is
Aggregation.chamfer_term; fp32 clouds on a HIP device take the kernels of voge_amd/csrc/chamfer.hip (ops._Chamfer: exact nearest
points over a grid chosen on the device, fp64 sums in a fixed order, an integer-atomic backward -- the same bits on every run and
nothing read back on the host, so it runs inside a captured iteration).

sample_points_from_meshes is what feeds that loss in practice: area-weighted points (and normals) on a mesh's surface, redrawn
every iteration, with gradients to the three vertices of each sampled face.  A SurfaceSampler is built ONCE on the host from the
faces; the definition is Aggregation.mesh_surface_points, and fp32 vertices on the HIP device of the sampler's tables take the
kernels of voge_amd/csrc/mesh_sample.hip (ops._MeshSample: three launches forward, an integer-atomic backward, the same bits on
every run, capturable).

point_mesh_face_distance measures a mesh against a cloud exactly -- every point to its nearest triangle, every triangle to its
nearest point --, point_mesh_edge_distance the same over segments, and closest_faces is the search alone, the score of an
extracted mesh against ground-truth points.  The definitions are Aggregation.point_triangle_closest / point_mesh_term; fp32
tensors on a HIP device take the kernels of voge_amd/csrc/point_mesh.hip (ops._PointMesh: two exact searches through LDS, fp64
sums in a fixed order, an integer-atomic backward -- the same bits on every run, capturable)."""
import weakref

import numpy as np
import torch

from . import Aggregation, ops

TERMS = ("edge", "laplacian", "normal")      # bit k of the kernels' mask


def _index_array(x, width, name):
    """x as an int64 numpy array [n, width]; ValueError for anything that is not an integer table of that width."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.size == 0:
        x = np.zeros((0, width), np.int64)
    if x.ndim != 2 or x.shape[1] != width or not np.issubdtype(x.dtype, np.integer):
        raise ValueError(f"MeshTopology: {name} must be an integer array [n,{width}], got {x.dtype} {tuple(x.shape)}")
    return x.astype(np.int64)


def _csr(owner, n):
    """offsets [n+1] of a sorted owner array"""
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(owner, minlength=n), out=off[1:])
    return off


class MeshTopology:
    """The connectivity the mesh regularisers need, built once on the host with numpy (never per step).

    MeshTopology(faces=[F,3]) takes a triangle mesh, MeshTopology(edges=[E,2]) a plain graph -- e.g. the symmetrised
    Converters.knn_points neighbours of a point cloud --, which has no face pairs: its normal term is 0.  num_verts defaults to
    the largest index + 1; a vertex nothing uses is allowed (degree 0).  ValueError: an index out of range, a face (or an edge)
    that names a vertex twice, both faces and edges given, or neither.

    The tables are int32 tensors on `device` (default: the host) in this fixed order:
      edges   [E,2]   the unique undirected pairs i < j, sorted lexicographically;
      nbr_off [V+1], nbr [2E]   the adjacency as CSR: nbr[nbr_off[i] : nbr_off[i+1]] are i's neighbours, ascending;
      pairs   [P,4] = (v0, v1, a, b)   one row for every pair of faces that share the edge (v0, v1), v0 < v1; a and b are the
              opposite vertices of the first and the second face.  An edge with m faces gives m (m - 1) / 2 rows, a boundary edge
              none.  Rows are sorted by (edge, first face index, second face index);
      inc_off [V+1], inc [4P]   per vertex the entries pair * 4 + role (role = the column of `pairs` that names it), ascending.
    num_verts, num_edges, num_pairs and max_degree are Python ints; .to(device) gives the same tables on another device."""

    _TABLES = ("edges", "nbr_off", "nbr", "pairs", "inc_off", "inc")

    def __init__(self, faces=None, num_verts=None, edges=None, device=None):
        if (faces is None) == (edges is None):
            raise ValueError("MeshTopology: give faces or edges, not both and not neither")
        given = _index_array(faces, 3, "faces") if faces is not None else _index_array(edges, 2, "edges")
        V = int(given.max()) + 1 if num_verts is None and given.size else int(num_verts or 0)
        if V < 0 or V > 2 ** 31 - 1 or (given.size and (given.min() < 0 or given.max() >= V)):
            raise ValueError(f"MeshTopology: indices must lie in [0, {V})")
        s = np.sort(given, axis=1)
        if (s[:, 1:] == s[:, :-1]).any():
            raise ValueError(f"MeshTopology: {'a face' if faces is not None else 'an edge'} names a vertex twice")

        if faces is not None:
            F = given.shape[0]
            # the three edges of every face with the vertex opposite: (lo, hi, opposite, face)
            corner = np.concatenate([given[:, [0, 1, 2]], given[:, [1, 2, 0]], given[:, [2, 0, 1]]])
            lo, hi = np.minimum(corner[:, 0], corner[:, 1]), np.maximum(corner[:, 0], corner[:, 1])
            opp, face = corner[:, 2], np.tile(np.arange(F), 3)
            und = np.stack([lo, hi], 1)
        else:
            und = s
        key, edge_of = np.unique(und[:, 0] * V + und[:, 1], return_inverse=True)      # (lexicographic: lo * V + hi, below 2^62)
        uniq = np.stack([key // max(V, 1), key % max(V, 1)], 1)
        E = uniq.shape[0]

        owner = np.concatenate([uniq[:, 0], uniq[:, 1]])
        other = np.concatenate([uniq[:, 1], uniq[:, 0]])
        order = np.lexsort((other, owner))
        nbr, nbr_off = other[order], _csr(owner[order], V)

        pairs = np.zeros((0, 4), np.int64)
        if faces is not None and E:
            edge_of = edge_of.reshape(-1)
            order = np.lexsort((face, edge_of))                       # the faces of every edge, by face index
            e_s, f_s, o_s = edge_of[order], face[order], opp[order]
            count = np.bincount(e_s, minlength=E)
            start = _csr(e_s, E)[:-1]
            rows = []
            for m in np.unique(count[count >= 2]):
                first, second = np.triu_indices(int(m), 1)
                base = start[count == m][:, None]
                i0, i1 = (base + first[None, :]).ravel(), (base + second[None, :]).ravel()
                rows.append(np.stack([e_s[i0], f_s[i0], f_s[i1], o_s[i0], o_s[i1]], 1))
            if rows:
                r = np.concatenate(rows)
                r = r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]
                pairs = np.concatenate([uniq[r[:, 0]], r[:, 3:5]], 1)
        P = pairs.shape[0]
        if E > 2 ** 30 - 1 or P > 2 ** 29 - 1:
            raise ValueError("MeshTopology: too many edges or face pairs for the int32 tables")
        vert = pairs.ravel()
        inc = np.argsort(vert, kind="stable")                         # entry = pair * 4 + role, ascending inside a vertex
        inc_off = _csr(vert, V)

        self.num_verts, self.num_edges, self.num_pairs = V, E, P
        self.max_degree = int((nbr_off[1:] - nbr_off[:-1]).max()) if V else 0
        self._host = {"edges": uniq.reshape(E, 2), "nbr_off": nbr_off, "nbr": nbr, "pairs": pairs, "inc_off": inc_off, "inc": inc}
        self._place(torch.device("cpu" if device is None else device))

    def _place(self, device):
        for name in self._TABLES:
            setattr(self, name, torch.from_numpy(np.ascontiguousarray(self._host[name], dtype=np.int32)).to(device))
        self.device = self.edges.device

    def to(self, device):
        """The same topology with its tables on `device` (self when they are there already)."""
        device = torch.device(device)
        if device == self.edges.device:
            return self
        other = object.__new__(MeshTopology)
        other.num_verts, other.num_edges, other.num_pairs, other.max_degree = self.num_verts, self.num_edges, self.num_pairs, self.max_degree
        other._host = self._host
        other._place(device)
        return other


def _terms_mask(terms):
    if isinstance(terms, str):
        terms = (terms,)
    mask = 0
    for t in terms:
        if t not in TERMS:
            raise ValueError(f"mesh_regularisers: unknown term {t!r} (one of {TERMS})")
        mask |= 1 << TERMS.index(t)
    return mask


def mesh_regularisers(verts, topo, target_length=0.0, terms=TERMS):
    """(edge, laplacian, normal) of verts [V,3] | [B,V,3] over a MeshTopology, as 0-dim tensors; for a batch each term is the
    mean over the B meshes, which share the topology.  A term that is not in `terms` is not computed, is returned as an exact 0
    and passes no gradient.  Definitions: Aggregation.mesh_edge_term (target_length is a Python float), mesh_laplacian_term
    (uniform weights; PyTorch3D's "cot" and "cotcurv" are out of scope) and mesh_normal_term.  Only verts get a gradient.
    fp32 verts on the HIP device of the tables: ONE autograd node (ops._MeshReg), no double backward; otherwise the definitions,
    with the tables moved to the vertices' device."""
    mask = _terms_mask(terms)
    if verts.dim() not in (2, 3) or tuple(verts.shape[-2:]) != (topo.num_verts, 3):
        raise ValueError(f"mesh_regularisers: verts [{topo.num_verts},3] or [B,{topo.num_verts},3] expected, got {tuple(verts.shape)}")
    if verts.is_cuda and verts.dtype == torch.float32 and topo.edges.device == verts.device:
        return ops.mesh_reg(verts, topo, float(target_length), mask)
    t = topo.to(verts.device)
    zero = verts.new_zeros(())
    return (Aggregation.mesh_edge_term(verts, t.edges, float(target_length)) if mask & 1 else zero,
            Aggregation.mesh_laplacian_term(verts, t.nbr_off, t.nbr) if mask & 2 else zero,
            Aggregation.mesh_normal_term(verts, t.pairs) if mask & 4 else zero)


def mesh_edge_loss(verts, topo, target_length=0.0):
    """(1 / E) sum_e (|v_i - v_j| - target_length)^2: mesh_regularisers with the edge term alone."""
    return mesh_regularisers(verts, topo, target_length, ("edge",))[0]


def mesh_laplacian_smoothing(verts, topo):
    """(1 / V) sum_i |L_i| with uniform weights: mesh_regularisers with the laplacian term alone ("cot" / "cotcurv": out of scope)."""
    return mesh_regularisers(verts, topo, 0.0, ("laplacian",))[1]


def mesh_normal_consistency(verts, topo):
    """(1 / P) sum (1 - cos) over the pairs of faces that share an edge: mesh_regularisers with the normal term alone."""
    return mesh_regularisers(verts, topo, 0.0, ("normal",))[2]


def _normals_term(n_own, n_other, nn, reduce):
    """PyTorch3D's normal term of one direction: reduce(1 - |cos(n_own_i, n_other_nn(i))|), cosine_similarity with eps 1e-6"""
    cos = torch.nn.functional.cosine_similarity(n_own, n_other[nn.long()], dim=-1, eps=1e-6)
    return reduce(1 - cos.abs())


def _chamfer_pair(x, y, x_normals, y_normals, single_directional, point_reduction):
    if x.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32 and y.device == x.device:
        loss, nn_x, nn_y = ops.chamfer(x, y, point_reduction == "sum", single_directional)
    else:
        loss, nn_x, nn_y = Aggregation.chamfer_term(x, y, single_directional, point_reduction, return_indices=True)
    loss_normals = None
    if x_normals is not None:
        reduce = torch.mean if point_reduction == "mean" else torch.sum
        loss_normals = _normals_term(x_normals, y_normals, nn_x, reduce)
        if not single_directional:
            loss_normals = loss_normals + _normals_term(y_normals, x_normals, nn_y, reduce)
    return loss, loss_normals


def chamfer_distance(x, y, x_normals=None, y_normals=None, single_directional=False, point_reduction="mean", **unsupported):
    """(loss, loss_normals) of two clouds x [Nx,3] and y [Ny,3] -- PyTorch3D's return shape, `loss, _ = chamfer_distance(a, b)`:

        loss = (1 / Nx) sum_i min_j |x_i - y_j|^2 + (1 / Ny) sum_j min_i |y_j - x_i|^2,

    point_reduction="sum" without the two divisors, single_directional the first sum alone.  Both clouds get gradients.  The
    definition is Aggregation.chamfer_term, and what host tensors and other dtypes get; fp32 clouds on one HIP device are ONE
    autograd node (ops._Chamfer, no double backward) with no host synchronisation.  A batch x [B,Nx,3], y [B,Ny,3] is a HOST LOOP
    over the B pairs whose losses are averaged (PyTorch3D's batch_reduction="mean"): the kernels handle one pair of clouds.
    loss_normals is None without normals; with x_normals [.., Nx,3] and y_normals [.., Ny,3] it is PyTorch3D's 1 - |cos| between a
    point's normal and the normal at its nearest point, reduced and summed over the directions like the loss -- a plain torch
    expression on the node's saved indices, differentiable in the normals only.
    Out of scope, ValueError by name: norm=1, x_lengths / y_lengths, weights, batch_reduction other than "mean", and
    point_reduction other than "mean" / "sum"; wrong shapes and an empty cloud raise ValueError too."""
    for name, value in unsupported.items():
        if name not in ("norm", "x_lengths", "y_lengths", "weights", "batch_reduction", "abs_cosine"):
            raise TypeError(f"chamfer_distance: unexpected argument {name!r}")
        if value is not None and not (name == "norm" and value == 2) and not (name == "batch_reduction" and value == "mean") \
                and not (name == "abs_cosine" and value is True):
            raise ValueError(f"chamfer_distance: {name}={value!r} is out of scope")
    if point_reduction not in ("mean", "sum"):
        raise ValueError(f"chamfer_distance: point_reduction must be 'mean' or 'sum', got {point_reduction!r}")
    if not torch.is_tensor(x) or not torch.is_tensor(y) or x.dim() not in (2, 3) or y.dim() != x.dim() or x.shape[-1] != 3 \
            or y.shape[-1] != 3 or (x.dim() == 3 and x.shape[0] != y.shape[0]):
        raise ValueError("chamfer_distance: x [Nx,3] and y [Ny,3], or [B,Nx,3] and [B,Ny,3], expected")
    if x.shape[-2] == 0 or y.shape[-2] == 0 or (x.dim() == 3 and x.shape[0] == 0):
        raise ValueError("chamfer_distance: an empty cloud")
    if (x_normals is None) != (y_normals is None):
        raise ValueError("chamfer_distance: give both x_normals and y_normals, or neither")
    if x_normals is not None and (x_normals.shape != x.shape or y_normals.shape != y.shape):
        raise ValueError("chamfer_distance: the normals must have their clouds' shapes")
    if x.dim() == 2:
        return _chamfer_pair(x, y, x_normals, y_normals, single_directional, point_reduction)
    pairs = [_chamfer_pair(x[b], y[b], None if x_normals is None else x_normals[b], None if y_normals is None else y_normals[b],
                           single_directional, point_reduction) for b in range(x.shape[0])]
    loss = torch.stack([p[0] for p in pairs]).mean()
    return loss, (None if x_normals is None else torch.stack([p[1] for p in pairs]).mean())


class SurfaceSampler:
    """What sample_points_from_meshes needs of a mesh's connectivity, built once on the host with numpy (never per step).

    SurfaceSampler(faces=[F,3]); num_verts defaults to the largest index + 1, and a vertex no face uses is allowed.  ValueError
    (MeshTopology's): an index out of range, a face that names a vertex twice.  int32 tensors on `device` (default: the host):
      faces      [F,3]   the faces as given;
      corner_off [V+1], corner [3F]   per vertex the entries face * 3 + role (role = the column of `faces` that names it),
                 ascending: corner[corner_off[v] : corner_off[v+1]] are the corners at v -- what the backward of the normals walks.
    num_verts and num_faces are Python ints; .to(device) gives the same tables on another device."""

    _TABLES = ("faces", "corner_off", "corner")

    def __init__(self, faces, num_verts=None, device=None):
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        given = np.asarray(faces)
        if given.size == 0:
            given = np.zeros((0, 3), np.int64)
        if given.ndim != 2 or given.shape[1] != 3 or not np.issubdtype(given.dtype, np.integer):
            raise ValueError(f"SurfaceSampler: faces must be an integer array [F,3], got {given.dtype} {tuple(given.shape)}")
        given = given.astype(np.int64)
        V = int(given.max()) + 1 if num_verts is None and given.size else int(num_verts or 0)
        if V < 0 or V > 2 ** 28 - 1 or (given.size and (given.min() < 0 or given.max() >= V)):
            raise ValueError(f"SurfaceSampler: indices must lie in [0, {V})")
        s = np.sort(given, axis=1)
        if (s[:, 1:] == s[:, :-1]).any():
            raise ValueError("SurfaceSampler: a face names a vertex twice")
        F = given.shape[0]
        if F > 2 ** 28 - 1:
            raise ValueError("SurfaceSampler: too many faces for the int32 tables")
        vert = given.ravel()
        self.num_verts, self.num_faces = V, F
        self._host = {"faces": given, "corner_off": _csr(vert, V), "corner": np.argsort(vert, kind="stable")}
        self._place(torch.device("cpu" if device is None else device))

    def _place(self, device):
        for name in self._TABLES:
            setattr(self, name, torch.from_numpy(np.ascontiguousarray(self._host[name], dtype=np.int32)).to(device))
        self.device = self.faces.device

    def to(self, device):
        """The same sampler with its tables on `device` (self when they are there already)."""
        device = torch.device(device)
        if device == self.faces.device:
            return self
        other = object.__new__(SurfaceSampler)
        other.num_verts, other.num_faces, other._host = self.num_verts, self.num_faces, self._host
        other._place(device)
        return other


def _sample_one(verts, sampler, u, return_normals):
    if verts.is_cuda and verts.dtype == torch.float32 and sampler.faces.device == verts.device:
        return ops.mesh_sample(verts, sampler, u.to(device=verts.device, dtype=torch.float32), return_normals)
    return Aggregation.mesh_surface_points(verts, sampler.to(verts.device).faces, u.to(verts.device), return_normals)


def sample_points_from_meshes(verts, faces_or_sampler, num_samples=10000, return_normals=False, generator=None, u=None,
                              return_faces=False):
    """Points on the surface of the mesh (verts [V,3], faces), each face chosen with probability proportional to its area --
    PyTorch3D's name and return shape: points [S,3], or (points, normals) with return_normals=True; return_faces=True appends
    face_idx [S] and bary [S,3], what a caller needs to interpolate anything else at the samples (face_idx is int32 from the
    kernels, int64 from the definition; -1 everywhere for a mesh without area).  The definition is
    Aggregation.mesh_surface_points.  verts get gradients through the three vertices of every sampled face (and through the
    normals); the face choice and the random numbers are constants.

    u [S,3] in [0,1) is the random table (column 0 chooses the face, 1 and 2 the point inside it); u=None draws
    torch.rand((num_samples, 3)) on the vertices' device with `generator` -- one more launch, and capturable: every replay draws
    anew (the default generator is known to a captured graph; one of the caller's own has to be registered with the graph first,
    CUDAGraph.register_generator_state(generator), and then draws in a replay what an eager call draws after the same seed).  A captured step must keep no output of an earlier step alive with its grad_fn.
    faces_or_sampler: a SurfaceSampler, or a faces tensor / array [F,3], from which a sampler is built ON THE SPOT -- a host round
    trip (the faces are copied to the host, sorted with numpy and copied back): a loop builds the SurfaceSampler once and passes it.
    fp32 verts on the HIP device of the sampler's tables are ONE autograd node (ops._MeshSample, no double backward, no host
    synchronisation); everything else -- host tensors, other dtypes, a sampler on another device -- takes the definition.
    verts [B,V,3] is a HOST LOOP over the B meshes, which share the faces, with u [B,S,3]: the kernels handle one mesh.
    S = 0 returns empty tensors; a mesh without faces raises ValueError, and so do wrong shapes."""
    if not torch.is_tensor(verts) or verts.dim() not in (2, 3) or verts.shape[-1] != 3:
        raise ValueError("sample_points_from_meshes: verts [V,3] or [B,V,3] expected")
    sampler = faces_or_sampler
    if not isinstance(sampler, SurfaceSampler):
        sampler = SurfaceSampler(faces_or_sampler, num_verts=verts.shape[-2], device=verts.device)
    if sampler.num_faces == 0:
        raise ValueError("sample_points_from_meshes: a mesh without faces")
    if verts.shape[-2] != sampler.num_verts:
        raise ValueError(f"sample_points_from_meshes: the sampler was built for {sampler.num_verts} vertices, verts has {verts.shape[-2]}")
    lead = tuple(verts.shape[:-2])
    if u is None:
        u = torch.rand(lead + (int(num_samples), 3), generator=generator, device=verts.device,
                       dtype=verts.dtype if verts.dtype in (torch.float32, torch.float64) else torch.float32)
    elif not torch.is_tensor(u) or tuple(u.shape[:-2]) != lead or u.dim() != verts.dim() or u.shape[-1] != 3:
        raise ValueError(f"sample_points_from_meshes: u {list(lead) + ['S', 3]} expected, got {tuple(u.shape) if torch.is_tensor(u) else u}")
    if verts.dim() == 2:
        out = _sample_one(verts, sampler, u, return_normals)
    else:
        if verts.shape[0] == 0:
            raise ValueError("sample_points_from_meshes: an empty batch")
        per = [_sample_one(verts[b], sampler, u[b], return_normals) for b in range(verts.shape[0])]
        out = tuple(None if per[0][k] is None else torch.stack([p[k] for p in per]) for k in range(4))
    points, normals, face_idx, bary = out
    res = (points, normals) if return_normals else (points,)
    if return_faces:
        res = res + (face_idx, bary)
    return res[0] if len(res) == 1 else res


_FACES_CHECKED = {}      # id of a faces tensor -> (weak reference to it, its version when it passed, the V it passed for)


def _checked_faces(faces, V, what, width=3):
    """faces as an integer tensor [F,width] whose entries lie in [0, V); ValueError otherwise.  The range check of a device tensor
    reads two numbers back, so it is made once per tensor and never inside a stream capture: the kernels themselves skip a face
    that names a vertex out of range.  "Once per tensor" is the tensor OBJECT at its version, held by weak reference as
    cameras._INTR holds its pair: an address says nothing (the allocator hands a freed tensor's block to the next one of its
    size, whose version is 0 again), so a new tensor, a new view of one or an array wrapped afresh is always checked, and an
    in-place edit of a tensor or of the base of a view bumps the version they share."""
    if isinstance(faces, np.ndarray):
        faces = torch.from_numpy(faces)
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != width or faces.dtype.is_floating_point or faces.dtype == torch.bool \
            or faces.dtype.is_complex:
        raise ValueError(f"{what}: an integer tensor [n,{width}] expected, got "
                         f"{(faces.dtype, tuple(faces.shape)) if torch.is_tensor(faces) else type(faces).__name__}")
    if faces.shape[0] == 0:
        raise ValueError(f"{what}: an empty mesh")
    hit = _FACES_CHECKED.get(id(faces))
    if hit is not None and hit[0]() is faces and hit[1:] == (faces._version, V):
        return faces
    if not (faces.is_cuda and torch.cuda.is_current_stream_capturing()):
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= V:
            raise ValueError(f"{what}: indices must lie in [0, {V}), got [{lo}, {hi}]")
        if len(_FACES_CHECKED) > 64:
            _FACES_CHECKED.clear()
        _FACES_CHECKED[id(faces)] = (weakref.ref(faces), faces._version, V)
    return faces


_POINT_MESH_ROUTES = (None, "brute", "grid")


def _checked_route(route, what):
    if route not in _POINT_MESH_ROUTES:
        raise ValueError(f"{what}: route must be None, 'brute' or 'grid', got {route!r}")
    return route


def closest_faces(points, verts, faces, route=None):
    """For every row of points [P,3] the nearest triangle of the mesh (verts [V,3], faces [F,3] of any integer dtype) ->
    (d2 [P], face_idx [P], bary [P,3]) without gradient: the squared distance of Aggregation.point_triangle_closest, the lowest
    face index among exact ties (int32 from the kernels, int64 from the definition) and the weights of the closest point on the
    face's (a, b, c).  What an extracted mesh is scored with against ground-truth points: sqrt(d2).mean() is the accuracy of a
    reconstruction's points against a reference mesh, (d2 <= tau^2).float().mean() its precision at tau, and the same with the
    roles swapped completeness and recall.  fp32 tensors on one HIP device take the kernels of ops.closest_faces (no host
    synchronisation): route "brute" meets all P F pairs, at most ops.POINT_MESH_MAX_PAIRS of them; "grid" searches a uniform grid
    chosen on the device, returns the same bits and has no pair cap -- a million faces against half a million points --; None takes
    the brute force below ops.POINT_MESH_GRID_MIN_PAIRS pairs and the grid above, and still refuses more than the cap.  Everything
    else takes the definition in chunks of points, which has no routes.  P = 0 returns empty tensors; wrong shapes, an empty mesh,
    an unknown route or a face that names a vertex outside [0, V) raise ValueError."""
    _checked_route(route, "closest_faces")
    if not torch.is_tensor(points) or not torch.is_tensor(verts) or points.dim() != 2 or verts.dim() != 2 or points.shape[1] != 3 \
            or verts.shape[1] != 3:
        raise ValueError("closest_faces: points [P,3] and verts [V,3] expected")
    if verts.shape[0] == 0:
        raise ValueError("closest_faces: an empty mesh")
    faces = _checked_faces(faces, verts.shape[0], "closest_faces: faces")
    points, verts = points.detach(), verts.detach()
    if verts.is_cuda and verts.dtype == torch.float32 and points.dtype == torch.float32 and points.device == verts.device:
        return ops.closest_faces(points, verts, faces.to(verts.device), route)
    f = faces.to(verts.device).long()
    points = points.to(verts.dtype)
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    P, F = points.shape[0], f.shape[0]
    face_idx = torch.empty((P,), dtype=torch.long, device=verts.device)
    ar = torch.arange(F, device=verts.device)
    chunk = max(1, (1 << 20) // F)
    for s in range(0, P, chunk):
        d = Aggregation.point_triangle_closest(points[s:s + chunk, None], a[None], b[None], c[None])[0]
        face_idx[s:s + chunk] = torch.where(d == d.min(dim=1).values[:, None], ar[None, :], F).min(dim=1).values
    d2, bary = Aggregation.point_triangle_closest(points, a[face_idx], b[face_idx], c[face_idx])
    return d2, face_idx, bary


_POINT_MESH_UNSUPPORTED = ("min_triangle_area", "meshes", "pcls", "weights", "norm", "batch_reduction", "x_lengths", "y_lengths")


def _point_mesh_pair(verts, faces, points, single_directional, point_reduction, route=None):
    if verts.is_cuda and verts.dtype == torch.float32 and points.dtype == torch.float32 and points.device == verts.device:
        return ops.point_mesh(verts, faces.to(verts.device), points, point_reduction == "sum", single_directional, route)[0]
    return Aggregation.point_mesh_term(verts, faces.to(verts.device), points.to(verts.device), single_directional, point_reduction)


def _point_mesh_distance(what, verts, faces, points, single_directional, point_reduction, unsupported, route=None):
    for name, value in unsupported.items():
        if name not in _POINT_MESH_UNSUPPORTED:
            raise TypeError(f"{what}: unexpected argument {name!r}")
        raise ValueError(f"{what}: {name}={value!r} is out of scope" + (
            " (there is no area threshold: a triangle without area is its three segments)" if name == "min_triangle_area" else ""))
    if point_reduction not in ("mean", "sum"):
        raise ValueError(f"{what}: point_reduction must be 'mean' or 'sum', got {point_reduction!r}")
    _checked_route(route, what)
    if not torch.is_tensor(verts) or not torch.is_tensor(points) or verts.dim() not in (2, 3) or points.dim() != verts.dim() \
            or verts.shape[-1] != 3 or points.shape[-1] != 3 or (verts.dim() == 3 and verts.shape[0] != points.shape[0]):
        raise ValueError(f"{what}: verts [V,3] and points [P,3], or [B,V,3] and [B,P,3], expected")
    if points.shape[-2] == 0 or (verts.dim() == 3 and verts.shape[0] == 0):
        raise ValueError(f"{what}: an empty cloud")
    if verts.shape[-2] == 0:
        raise ValueError(f"{what}: an empty mesh")
    if verts.dim() == 2:
        return _point_mesh_pair(verts, faces, points, single_directional, point_reduction, route)
    return torch.stack([_point_mesh_pair(verts[b], faces, points[b], single_directional, point_reduction, route)
                        for b in range(verts.shape[0])]).mean()


def point_mesh_face_distance(verts, faces, points, single_directional=False, point_reduction="mean", route=None, **unsupported):
    """The distance between a mesh (verts [V,3], faces [F,3] of any integer dtype; an int32 tensor on the vertices' device is used
    as it is) and a cloud points [P,3] -- PyTorch3D's point_mesh_face_distance on tensors, a 0-dim tensor:

        loss = (1 / P) sum_i min_f d2(p_i, T_f) + (1 / F) sum_f min_i d2(p_i, T_f),

    d2 the squared distance to the closest point of the triangle (Aggregation.point_triangle_closest), point_reduction="sum"
    without the two divisors, single_directional the first sum alone.  Unlike the chamfer distance of surface samples it is 0 on
    a perfect fit, does not change with a draw and moves no vertex along the surface.  verts and points get gradients.  The
    definition is Aggregation.point_mesh_term, and what host tensors and other dtypes get; fp32 tensors on one HIP device are ONE
    autograd node (ops._PointMesh, no double backward) with no host synchronisation, so it runs inside a captured iteration.  Both
    searches are exact on either route: "brute" meets all P F pairs and is capped (ops.POINT_MESH_MAX_PAIRS), "grid" searches a
    uniform grid chosen on the device, returns the same bits -- loss, pairs, weights and both gradients -- and is bound by the
    sizes alone; None takes the brute force below ops.POINT_MESH_GRID_MIN_PAIRS pairs, the grid above, and refuses more than the
    cap (pass route="grid" there).  The grid's weak cases are a mesh of mostly large triangles and lopsided pairs (correct, slow);
    a hierarchy for wildly mixed triangle sizes is out of scope.  verts [B,V,3] with points [B,P,3] is a HOST LOOP over the B pairs, which share
    the faces, averaged.  There is NO min_triangle_area: it depends on the scale of the mesh; a triangle without area is its
    three segments.  That and every other PyTorch3D keyword (meshes, pcls, weights, norm, ...) is rejected by name (ValueError);
    wrong shapes, an empty cloud, an empty mesh or a face that names a vertex outside [0, V) raise ValueError too."""
    what = "point_mesh_face_distance"
    if torch.is_tensor(verts) and verts.dim() in (2, 3):
        faces = _checked_faces(faces, verts.shape[-2], what + ": faces")
    return _point_mesh_distance(what, verts, faces, points, single_directional, point_reduction, unsupported, route)


def point_mesh_edge_distance(verts, edges, points, single_directional=False, point_reduction="mean", route=None, **unsupported):
    """PyTorch3D's point_mesh_edge_distance on tensors: point_mesh_face_distance with the segments edges [E,2] (an integer
    tensor, or a MeshTopology, whose unique edges are taken) in the triangles' place.  A segment (i, j) is the triangle (i, j, j),
    which point_triangle_closest's rule for a triangle without area makes exactly the segment: the same node on the index table
    [i, j, j], no kernel of its own; route as in point_mesh_face_distance."""
    what = "point_mesh_edge_distance"
    if isinstance(edges, MeshTopology):
        edges = edges.edges
    if torch.is_tensor(verts) and verts.dim() in (2, 3):
        edges = _checked_faces(edges, verts.shape[-2], what + ": edges", width=2)
        edges = edges[:, [0, 1, 1]]
    return _point_mesh_distance(what, verts, edges, points, single_directional, point_reduction, unsupported, route)
