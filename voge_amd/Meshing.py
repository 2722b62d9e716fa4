"""Mesh extraction (an extension: the reference has none; the step the 2D Gaussian splatting pipeline ends with).

    vol = TSDFVolume(lo, hi=None, voxel_size=None, resolution=None, device=...)
    vol.integrate(depth, cameras, trunc, max_weight=None)      # in place, returns vol
    verts, faces = extract_mesh(vol, level=0.0)
    verts, faces = extract_mesh(values, weight=None, level=0.0, lo=(0, 0, 0), voxel_size=1.0)

TSDFVolume fuses depth maps -- what Renderer.get_depth returns: the distance along the unit pixel ray, under the cameras of
cameras.pixel_rays -- into a truncated signed distance volume; extract_mesh turns the volume, or any scalar field such as an
analytic SDF, into verts [V,3] fp32 and faces [F,3] int32 by marching tetrahedra, ready for Losses.MeshTopology,
mesh_regularisers, sample_points_from_meshes, chamfer_distance and Converter.IO.save_off.  Aggregation.tsdf_integrate and
Aggregation.marching_tets ARE the definitions; fp32 tensors on a HIP device take the kernels of csrc/meshing.hip, everything
else (host tensors, other dtypes) the definitions.

NEITHER STEP IS DIFFERENTIABLE, by design: the fusion chooses a nearest pixel and the extraction a topology.  Gradients reach
a surface here through the renderer (get_depth, get_normals) or through a mesh's vertices (Losses), not through this module.

extract_mesh on the device reads TWO integers back on the host, the vertex and the face count, to size its outputs: one
synchronisation per call.  Extraction is a one-off step after a fit, not a step of an iteration, and cannot be captured into a
graph; integrate reads nothing back.

Mesh clean-up, what the same pipeline runs on the extracted mesh before it scores or saves it (a TSDF fused from rendered depth
carries floaters: small closed blobs where a few views disagree, shells behind silhouettes):

    vert_label, face_label, n = connected_components(faces, num_verts=None)
    verts, faces = clean_mesh(verts, faces, keep_largest=None, min_faces=1, return_index=False)
    normals = vertex_normals(verts, faces)

Aggregation.mesh_components, Aggregation.mesh_clean and Aggregation.mesh_vertex_normals ARE the definitions; fp32 / int32 tensors on
one HIP device take the kernels of csrc/mesh_clean.hip, everything else the definitions.  NONE OF THE THREE IS DIFFERENTIABLE
either (Aggregation.mesh_vertex_normals is, through autograd, for whoever needs that).  connected_components reads ONE pair of
integers back on the host (the error word and the number of components: one synchronisation); clean_mesh that pair and then
the three that size its outputs (V', F' and an error word: a second synchronisation) -- like extraction, one-off steps that
cannot be captured into a graph.  vertex_normals reads nothing back and can be.

Attributes -- colour, rendered normals, any [B,H,W,C] image a renderer makes -- go through both steps beside the geometry:

    vol = TSDFVolume(lo, ..., channels=C)                       # vol.attr [nz,ny,nx,C] fp32, channel last
    vol.integrate(depth, cameras, trunc, attr=images)           # images [B,H,W,C]; in every call of such a volume
    verts, faces, vert_attr = extract_mesh(vol, attr=True)      # vert_attr [V,C] fp32
    verts, faces, vert_attr = extract_mesh(values, ..., attr=field)      # any field [nz,ny,nx,C] beside any scalar field

One rule each (Aggregation.tsdf_integrate, step 6, and Aggregation.marching_tets): where a view updates a grid point its attribute
becomes (attr w + pixel) / (w + 1) with the depth's own nearest pixel and the weight the distance is averaged by; the vertex on an
edge gets attr_a + t (attr_b - attr_a) with the edge's own t.  On a HIP device: voge_tsdf_integrate_attr, still ONE launch with
the C running averages in registers (16 + 8 C bytes a grid point however many views), and voge_mtet_attr, one launch after the
emit on its tables; tsdf, weight, verts and faces keep the bits of the calls without an attribute.  The kernels are compiled for
C <= 8: a volume of more channels on the device is fused by the definition (torch, on the device), a field of more channels is
carried to the vertices eight channels a launch.

Simplification, the step between extraction and use (marching tetrahedra makes about eight faces a surface cell, and everything
downstream pays per face or per vertex):

    verts, faces = simplify_mesh(verts, faces, cell_size, placement="mean")
    verts, faces, colours = simplify_mesh(verts, faces, cell_size, placement="quadric", attr=colours)
    ..., vert_index, face_index = simplify_mesh(..., return_index=True)

Vertex clustering on a uniform grid: the vertices of one cell of size cell_size become one vertex at their mean, or where the
planes of the faces around them meet (placement="quadric": corners and creases survive); faces that collapse or repeat go.
Aggregation.mesh_simplify IS the definition and states the rule in five steps; fp32 verts and int32 faces on one HIP device take
the kernels of csrc/mesh_simplify.hip -- equal connectivity and index tables, positions and attributes within the bounds that
file's header derives, the same bits on every run and in every order of the faces --, everything else the definition.  ONE
synchronisation per call (V', F' and an error word), a one-off step like extraction, not capturable and NOT DIFFERENTIABLE.
Vertex clustering does not promise a manifold result: two sheets closer than a cell merge.  It gives no target face count either:
a count is reached by trying cell sizes.

Depth maps of a mesh, the arrow back from a mesh to an image:

    frags = rasterize_mesh(verts, faces, cameras, image_size, cull_backfaces=False, route=None)
    frags.pix_to_face [B,H,W] int32 (-1: nothing hit), frags.bary [B,H,W,3], frags.depth [B,H,W]
    image = interpolate_vertex_attr(frags, faces, vert_attr, background=0.0)      # [B,H,W,C]

The nearest face under every pixel by an exact ray-triangle test: Aggregation.mesh_rasterize IS the definition, seven steps.  depth
is get_depth's -- the distance along the unit pixel ray, under the cameras integrate reads -- so it goes unchanged into integrate,
get_normals and a loss against get_depth; pix_to_face is the visibility test for colouring a mesh from images.  fp32 verts, int32 or
int64 faces and cameras on one HIP device take the kernels of csrc/mesh_raster.hip: the definition's fp32 bits on both routes --
"brute", two launches, nothing read back, capturable: the meshes of a fitting loop; "bins", per-tile lists and ONE synchronisation:
large meshes; None chooses by ops.MESH_RASTER_BINS_MIN_WORK (brute won at every measured size).  depth IS DIFFERENTIABLE to verts there
(integer atomics, the same bits on every run); pix_to_face and bary carry no gradient and the cameras take none.  Everything else
-- host tensors, other dtypes -- takes the definition, differentiable through depth and bary by autograd.  No soft silhouettes, one
face a pixel, no near plane, one mesh a call.

Not here: gradients through any of the other steps, bilinear pixel sampling, per-view confidence weights, textures and UV maps,
edge-collapse decimation, a target_faces= argument and boundary preservation for the simplification.
"""
import collections

import torch

from . import Aggregation, cameras as _cameras, ops

__all__ = ["TSDFVolume", "extract_mesh", "connected_components", "clean_mesh", "vertex_normals", "simplify_mesh", "MeshFragments",
           "rasterize_mesh", "interpolate_vertex_attr"]


def _triple(v, name, integer=False):
    t = torch.as_tensor(v, dtype=torch.float64, device="cpu").reshape(-1)
    if t.numel() == 1:
        t = t.expand(3)
    if t.numel() != 3:
        raise ValueError(f"{name}: a scalar or three values (x, y, z) expected, got {tuple(t.shape)}")
    return [int(x) for x in t.tolist()] if integer else [float(x) for x in t.tolist()]


def _check_dims(nx, ny, nz, what):
    if min(nx, ny, nz) < 2:
        raise ValueError(f"{what}: every grid dimension must be >= 2, got (nx, ny, nz) = ({nx}, {ny}, {nz})")
    if nx * ny * nz * 7 >= 2 ** 31:
        raise ValueError(f"{what}: nx ny nz 7 = {nx * ny * nz * 7} does not fit the 32-bit indices of the extraction")


class TSDFVolume:
    """A truncated signed distance volume over a box.  Exactly two of hi / voxel_size / resolution:

      hi + resolution       h = (hi - lo) / (resolution - 1): the last grid point sits at hi;
      hi + voxel_size       resolution = floor((hi - lo) / h + 1e-6) + 1: the grid ends at or before hi;
      voxel_size + resolution   as given.

    voxel_size and resolution are scalars or (x, y, z).  Grid point (ix,iy,iz) sits at lo + (ix hx, iy hy, iz hz);
    tsdf and weight are [nz,ny,nx] fp32 (index order [iz,iy,ix]) and start at 0.  lo and voxel_size are kept as the fp32
    numbers the kernels see.  channels = C > 0: the volume also fuses an attribute of C floats a pixel (a colour, a normal) in
    attr [nz,ny,nx,C] fp32, channel last, zeros at the start, and integrate takes attr= in every call; C = 0: attr is None."""

    def __init__(self, lo, hi=None, voxel_size=None, resolution=None, device="cpu", channels=0):
        if isinstance(channels, bool) or not isinstance(channels, int) or channels < 0:
            raise ValueError(f"TSDFVolume: channels must be an integer >= 0, got {channels!r}")
        if sum(a is not None for a in (hi, voxel_size, resolution)) != 2:
            raise ValueError("TSDFVolume: exactly two of hi / voxel_size / resolution")
        lo = _triple(lo, "lo")
        if voxel_size is not None:
            h = _triple(voxel_size, "voxel_size")
            if not all(x > 0 and x < float("inf") for x in h):
                raise ValueError(f"TSDFVolume: voxel_size must be positive and finite, got {h}")
        if resolution is not None:
            res = _triple(resolution, "resolution", integer=True)
        if hi is not None:
            hi = _triple(hi, "hi")
            if not all(b > a for a, b in zip(lo, hi)):
                raise ValueError(f"TSDFVolume: hi {hi} must lie above lo {lo}")
            if resolution is not None:
                if min(res) < 2:
                    raise ValueError(f"TSDFVolume: resolution must be >= 2, got {res}")
                h = [(b - a) / (r - 1) for a, b, r in zip(lo, hi, res)]
            else:
                res = [int((b - a) / s + 1e-6) + 1 for a, b, s in zip(lo, hi, h)]
        _check_dims(res[0], res[1], res[2], "TSDFVolume")
        f32 = lambda xs: tuple(float(x) for x in torch.tensor(xs, dtype=torch.float32).tolist())
        self.lo, self.voxel_size, self.resolution = f32(lo), f32(h), tuple(res)
        self.device = torch.device(device)
        nx, ny, nz = self.resolution
        self.tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.channels = channels
        self.attr = torch.zeros((nz, ny, nx, channels), dtype=torch.float32, device=self.device) if channels else None

    @property
    def hi(self):
        return tuple(a + (r - 1) * s for a, s, r in zip(self.lo, self.voxel_size, self.resolution))

    def to(self, device):
        self.device = torch.device(device)
        self.tsdf, self.weight = self.tsdf.to(self.device), self.weight.to(self.device)
        if self.attr is not None:
            self.attr = self.attr.to(self.device)
        return self

    def integrate(self, depth, cameras, trunc, max_weight=None, attr=None):
        """Fuse depth [B,H,W] (get_depth's: the distance along the unit pixel ray; not finite or <= 0: no surface) seen by
        `cameras` (R, T, focal_length, principal_point, as cameras.pixel_rays reads them; B views or one for all) into the
        volume, in place, the views in their order: Aggregation.tsdf_integrate's rule.  rows= bands and distributed.Stripes
        are not taken.  One launch on a HIP device, nothing read back (the call can be captured into a graph; R is therefore not checked
        there: a singular R, which raises on the host, gives a centre that is not finite and poisons what its view updates); not
        differentiable.  Returns the volume.
        attr [B,H,W,C] -- the layout of the renderer's images and of interpolate_attr's outputs -- is required if and only if the
        volume has channels = C > 0: the attribute of the depth's own nearest pixel enters vol.attr as a running average under the
        weight of the distance, wherever the view updates the grid point (step 6 of the rule).  Its VALUES ARE NOT EXAMINED: a NaN
        pixel poisons the grid points that read it.  ValueError for a missing or an unexpected attr, one that is no tensor, a wrong
        C or a wrong B, H, W.  C <= 8 on a HIP device: still one launch (voge_tsdf_integrate_attr); more channels there: the
        definition in torch, on the device.  No bilinear sampling, no per-view confidence weights, no gradients."""
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise ValueError(f"integrate: depth [B,H,W] expected, got {tuple(getattr(depth, 'shape', ()))}")
        if not float(trunc) > 0 or float(trunc) == float("inf"):
            raise ValueError(f"integrate: trunc must be positive and finite, got {trunc}")
        if max_weight is not None and not float(max_weight) >= 1:
            raise ValueError(f"integrate: max_weight must be >= 1, got {max_weight}")
        B = depth.shape[0]
        dev = self.device
        if self.channels == 0 and attr is not None:
            raise ValueError("integrate: attr given, but the volume has channels = 0")
        if self.channels > 0:
            if not isinstance(attr, torch.Tensor):
                raise ValueError(f"integrate: a volume with channels = {self.channels} takes attr [B,H,W,{self.channels}] in every call, got "
                                 f"{type(attr).__name__}")
            if tuple(attr.shape) != tuple(depth.shape) + (self.channels,):
                raise ValueError(f"integrate: attr {list(depth.shape) + [self.channels]} expected, got {tuple(attr.shape)}")
        R = torch.as_tensor(cameras.R, device=dev).detach().to(torch.float32).reshape(-1, 3, 3)
        T = torch.as_tensor(cameras.T, device=dev).detach().to(torch.float32).reshape(-1, 3)
        Bc = max(R.shape[0], T.shape[0])
        if Bc not in (1, B) or R.shape[0] not in (1, Bc) or T.shape[0] not in (1, Bc):
            raise ValueError(f"integrate: {B} depth maps but {R.shape[0]} rotations and {T.shape[0]} translations")
        if B == 0:
            return self
        try:
            focal = _cameras._as_b2(torch.as_tensor(cameras.focal_length).detach(), B, dev)
            pp = _cameras._as_b2(torch.as_tensor(cameras.principal_point).detach(), B, dev)
        except RuntimeError as e:
            raise ValueError(f"integrate: {B} depth maps do not match the cameras' focal_length / principal_point") from e
        R, T = R.expand(B, 3, 3), T.expand(B, 3)
        depth = depth.detach().to(dev)
        # the centres in fp64, rounded once: what |x - c| is measured from
        centre = Aggregation.camera_centres(R.double(), T.double()).to(torch.float32)
        if self.channels > 0:
            attr = attr.detach().to(device=dev, dtype=torch.float32)
            if dev.type == "cuda" and self.channels <= ops.MTET_MAX_CHANNELS:
                ops.tsdf_integrate(self.tsdf, self.weight, depth, R, T, centre, focal, pp, self.lo, self.voxel_size, float(trunc), max_weight,
                                   attr=self.attr, attr_image=attr)
            else:      # (the host, or more channels than the kernel is compiled for: the definition, on the volume's device)
                t, w, a = Aggregation.tsdf_integrate(self.tsdf, self.weight, depth, R, T, focal, pp, self.lo, self.voxel_size, float(trunc),
                                                     max_weight, centre=centre, attr=self.attr, attr_image=attr)
                self.tsdf.copy_(t)
                self.weight.copy_(w)
                self.attr.copy_(a)
        elif dev.type == "cuda":
            ops.tsdf_integrate(self.tsdf, self.weight, depth, R, T, centre, focal, pp, self.lo, self.voxel_size, float(trunc), max_weight)
        else:
            t, w = Aggregation.tsdf_integrate(self.tsdf, self.weight, depth, R, T, focal, pp, self.lo, self.voxel_size, float(trunc),
                                              max_weight, centre=centre)
            self.tsdf.copy_(t)
            self.weight.copy_(w)
        return self


def extract_mesh(values, weight=None, level=0.0, lo=(0.0, 0.0, 0.0), voxel_size=1.0, attr=None):
    """(verts [V,3] fp32, faces [F,3] int32) of the level set of a TSDFVolume (its own weight, lo and voxel_size; the grid
    points no view has seen are unobserved) or of any scalar field values [nz,ny,nx] -- an analytic SDF for example -- with
    grid point (ix,iy,iz) at lo + (ix hx, iy hy, iz hz): Aggregation.marching_tets' rule, inside <=> value < level, normals from
    inside to outside.  An empty result is a pair of [0,3] tensors.  Raises ValueError when a dimension is < 2 or
    nx ny nz 7 >= 2^31.  On a HIP device: three launches, the two totals read back on the host (ONE synchronisation, see the
    module's header), one launch that writes the mesh.  Not differentiable.
    attr=True with a TSDFVolume of channels > 0 (its own attr), or attr=field [nz,ny,nx,C] beside any scalar field (an analytic
    colour beside an analytic SDF): the result is (verts, faces, vert_attr [V,C] fp32), the vertex on an edge getting
    attr_a + t (attr_b - attr_a) with the edge's own t -- Aggregation.marching_tets' rule; verts and faces are those of the call
    without attr, and an empty mesh has a vert_attr of [0,C].  On a HIP device: one more launch (voge_mtet_attr; one per eight
    channels).  ValueError for attr=True without a volume that has channels.  Not differentiable either; no textures or UV maps,
    and no colouring of an existing mesh by projecting its vertices into images."""
    if isinstance(values, TSDFVolume):
        vol = values
        values, weight, lo, voxel_size = vol.tsdf, vol.weight, vol.lo, vol.voxel_size
        if attr is True:
            if vol.channels == 0:
                raise ValueError("extract_mesh: attr=True, but the volume has channels = 0")
            attr = vol.attr
    if attr is True:
        raise ValueError("extract_mesh: attr=True needs a TSDFVolume with channels > 0; give the field [nz,ny,nx,C] itself")
    if not isinstance(values, torch.Tensor) or values.dim() != 3:
        raise ValueError(f"extract_mesh: a TSDFVolume or values [nz,ny,nx] expected, got {tuple(getattr(values, 'shape', ()))}")
    nz, ny, nx = values.shape
    _check_dims(nx, ny, nz, "extract_mesh")
    if weight is not None and (not isinstance(weight, torch.Tensor) or weight.shape != values.shape):
        raise ValueError(f"extract_mesh: weight must match values {tuple(values.shape)}")
    if attr is not None and (not isinstance(attr, torch.Tensor) or attr.dim() != 4 or attr.shape[:3] != values.shape or attr.shape[3] < 1):
        raise ValueError(f"extract_mesh: attr [nz,ny,nx,C] over values {tuple(values.shape)} expected, got {tuple(getattr(attr, 'shape', ()))}")
    lo, h = _triple(lo, "lo"), _triple(voxel_size, "voxel_size")
    values = values.detach()
    w = None if weight is None else weight.detach().to(values.device)
    if attr is not None:
        attr = attr.detach().to(values.device)
    if values.is_cuda and values.dtype == torch.float32:
        return ops.marching_tets(values, w, float(level), lo, h, attr=attr)
    out = Aggregation.marching_tets(values, w, float(level), lo, h, attr=attr)
    return (out[0].to(torch.float32), out[1].to(torch.int32)) + tuple(a.to(torch.float32) for a in out[2:])


def _check_faces(faces, what):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
        raise ValueError(f"{what}: faces [F,3] of integers expected, got {tuple(getattr(faces, 'shape', ()))}")


def _check_mesh(verts, faces, what):
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or not verts.dtype.is_floating_point:
        raise ValueError(f"{what}: verts [V,3] of floats expected, got {tuple(getattr(verts, 'shape', ()))}")
    _check_faces(faces, what)


def _on_device(verts, faces):
    return verts.is_cuda and verts.dtype == torch.float32 and faces.dtype == torch.int32 and faces.device == verts.device


def connected_components(faces, num_verts=None):
    """(vert_label [V] int32, face_label [F] int32, num_components: int) of faces [F,3]: Aggregation.mesh_components' rule.  Two
    vertices are connected when a chain of faces links them, each face joining its three vertices: VERTEX connectivity.  On the
    manifold output of extract_mesh that is edge connectivity too; it differs where two surfaces touch in a vertex without
    sharing an edge there (two cones tip to tip, the pinch of a non-manifold vertex): one component here, two for a clustering over
    shared edges.  A component's label is its smallest vertex index; a vertex no face names is labelled with its own index and is
    not counted in num_components; face_label[f] = vert_label[faces[f, 0]].  num_verts=None: 1 + the largest index (read back on
    the host).  An index outside [0, V) raises ValueError; a face may name a vertex twice, it just joins fewer vertices.  int32
    faces on a HIP device: three launches and ONE synchronisation (see the module's header).  Not differentiable."""
    _check_faces(faces, "connected_components")
    faces = faces.detach()
    if num_verts is None:
        num_verts = int(faces.max()) + 1 if faces.shape[0] else 0
    if int(num_verts) < 0:
        raise ValueError(f"connected_components: num_verts {num_verts}")
    if faces.is_cuda and faces.dtype == torch.int32:
        return ops.mesh_components(faces, int(num_verts))
    vert_label, face_label, n = Aggregation.mesh_components(faces, int(num_verts))
    return vert_label.to(torch.int32), face_label.to(torch.int32), n


def clean_mesh(verts, faces, keep_largest=None, min_faces=1, return_index=False):
    """(verts' [V',3], faces' [F',3] int32[, vert_index [V'] int32, face_index [F'] int32]) -- the mesh without its small components:
    Aggregation.mesh_clean's rule.  A component of connected_components stays when it has at least min_faces faces and is among the
    keep_largest components (None: all), ranked by face count descending, then by label ascending, so ties have one answer.  Kept
    faces keep their order and are renumbered; vertices no kept face names are dropped, the others keep their order and their
    bits; vert_index and face_index give the old indices, so colours or any other attribute can follow (colours[vert_index]).
    keep_largest=None, min_faces=1 on a mesh without unused vertices returns its input bit for bit.  keep_largest < 1 or
    min_faces < 1 raise ValueError, and so does an index outside [0, V).  fp32 verts and int32 faces on one HIP device: the
    components' launches, the ranking as torch calls on the device, five launches of the filter and TWO synchronisations (see
    the module's header); no float atomics, the same bits on every run.  Not differentiable."""
    _check_mesh(verts, faces, "clean_mesh")
    if (keep_largest is not None and int(keep_largest) < 1) or int(min_faces) < 1:
        raise ValueError(f"clean_mesh: keep_largest (None or >= 1) and min_faces >= 1 expected, got {keep_largest} / {min_faces}")
    verts, faces = verts.detach(), faces.detach()
    if _on_device(verts, faces):
        _, face_label, _, count = ops.mesh_components(faces, verts.shape[0], return_count=True)
        keep = Aggregation.mesh_keep_roots(count, keep_largest, min_faces)
        out = ops.mesh_clean(verts, faces, face_label, keep)
    else:
        out = Aggregation.mesh_clean(verts, faces.to(verts.device), keep_largest, min_faces)
        out = (out[0],) + tuple(t.to(torch.int32) for t in out[1:])
    return out if return_index else out[:2]


def vertex_normals(verts, faces):
    """normals [V,3] fp32: PyTorch3D's verts_normals_packed, the normalised sum of (b - a) x (c - a) over the faces at a vertex, which
    weights them by area -- Aggregation.mesh_vertex_normals' rule; what Converters.normal_mesh_converter(..., oriented=True) takes.
    (0, 0, 0) where the sum is zero or not finite, and for a vertex no face names.  The faces' indices must lie in [0, V) (nothing
    is read back to check them: the kernels skip such a face, the definition raises).  fp32 verts and int32 faces on one HIP
    device: four launches, fixed-point sums with integer atomics -- the same bits on every run and in every order of the faces --,
    nothing read back, capturable.  Not differentiable."""
    _check_mesh(verts, faces, "vertex_normals")
    verts, faces = verts.detach(), faces.detach()
    if _on_device(verts, faces):
        return ops.vertex_normals(verts, faces)
    return Aggregation.mesh_vertex_normals(verts, faces.to(verts.device)).to(torch.float32)


def simplify_mesh(verts, faces, cell_size, placement="mean", attr=None, return_index=False):
    """(verts' [V',3] fp32, faces' [F',3] int32[, attr' [V',C] fp32][, vert_index [V] int32, face_index [F'] int32]) -- the mesh with
    the vertices of every grid cell merged into one: Aggregation.mesh_simplify's rule, five steps.  cell_size, a scalar or
    (x, y, z), positive and finite, is kept as the fp32 numbers the kernels see; cells start at the vertices' per-axis minimum, and
    a vertex on a cell boundary belongs to the upper cell (floor((v - lo) / h) in fp32, the same decision on every route).  A
    cluster's vertex sits at the mean of its vertices (placement="mean") or where the planes of all the faces at its vertices
    meet, pulled towards the mean with weight 1e-3 and kept inside the cell (placement="quadric": a box keeps its corners); a
    cluster of one vertex keeps its bits.  Faces with two corners in one cluster are dropped; of the faces that become the same
    oriented triple the first stays; two faces of opposite orientation both stay; surviving faces keep their order, and only
    clusters they name become vertices, in the order of their smallest vertex index.  attr [V,C] (colours[, normals, ...]) comes
    back as the clusters' means.  vert_index[v] is the output row of input vertex v or -1, face_index the input faces that stay.
    A cell smaller than every gap between vertices returns the input bit for bit; a cell larger than the mesh returns [0,3]
    tensors (and [0,C]).  ValueError for a cell_size that is not positive and finite, a placement other than "mean" / "quadric", an
    attr that is not [V,C], a vertex that is not finite, a face index outside [0, V) and more than 2^21 - 1 cells on an axis.
    Vertex clustering does NOT promise a manifold result -- two sheets closer than a cell merge -- and has NO target face count:
    a count is reached by trying cell sizes.  Edge-collapse decimation, target_faces=, boundary preservation and gradients are out
    of scope.  fp32 verts and int32 faces on one HIP device: the launches of csrc/mesh_simplify.hip and ONE synchronisation (see the
    module's header); integer atomics only, the same bits on every run and in every order of the faces.  Not differentiable."""
    _check_mesh(verts, faces, "simplify_mesh")
    if placement not in ("mean", "quadric"):
        raise ValueError(f"simplify_mesh: placement 'mean' or 'quadric' expected, got {placement!r}")
    try:
        h = torch.tensor(_triple(cell_size, "cell_size"), dtype=torch.float32)
    except (TypeError, RuntimeError) as e:
        raise ValueError(f"simplify_mesh: cell_size must be a scalar or (x, y, z), got {cell_size!r}") from e
    if not bool((torch.isfinite(h) & (h > 0)).all()):
        raise ValueError(f"simplify_mesh: cell_size must be positive and finite as fp32, got {cell_size}")
    h = tuple(h.tolist())
    if attr is not None and (not isinstance(attr, torch.Tensor) or attr.dim() != 2 or attr.shape[0] != verts.shape[0]
                             or not attr.dtype.is_floating_point):
        raise ValueError(f"simplify_mesh: attr [{verts.shape[0]},C] of floats expected, got {tuple(getattr(attr, 'shape', ()))}")
    verts, faces = verts.detach(), faces.detach()
    if attr is not None:
        attr = attr.detach().to(verts.device)
    if _on_device(verts, faces):
        v, f, a, vi, fi = ops.mesh_simplify(verts, faces, h, placement, attr)
    else:
        v, f, a, vi, fi = Aggregation.mesh_simplify(verts, faces.to(verts.device), h, placement, attr)
        f, vi, fi = f.to(torch.int32), vi.to(torch.int32), fi.to(torch.int32)
    return (v, f) + (() if attr is None else (a,)) + ((vi, fi) if return_index else ())


MeshFragments = collections.namedtuple("MeshFragments", ["pix_to_face", "bary", "depth"])


def rasterize_mesh(verts, faces, cameras, image_size, cull_backfaces=False, route=None):
    """MeshFragments(pix_to_face [B,H,W] int32, bary [B,H,W,3] fp32, depth [B,H,W] fp32) of the mesh verts [V,3], faces [F,3] seen
    by `cameras` (R, T, focal_length, principal_point, as TSDFVolume.integrate reads them; B views or one) at image_size (H, W):
    Aggregation.mesh_rasterize's rule, the nearest face under every pixel centre by an exact ray-triangle test, ties to the lower
    index.  pix_to_face is -1, bary and depth are 0 where nothing is hit; depth is get_depth's, the distance along the unit pixel
    ray.  cull_backfaces keeps only the fronts of faces whose normal (b - a) x (c - a) points at the camera.  route: None, "brute"
    or "bins" (the module's header); host tensors and other dtypes take the definition whatever the route.  ValueError for verts or
    faces of another shape, an image_size that is not two integers >= 1, an unknown route, cameras whose counts do not match, a
    face index outside [0, V) (the definition; on the device such a face hits nothing) and, on the bins route, lists longer than
    2^31 - 1.  depth is differentiable to verts; on the device nothing else is."""
    _check_mesh(verts, faces, "rasterize_mesh")
    try:
        H, W = (int(x) for x in image_size)
    except (TypeError, ValueError) as e:
        raise ValueError(f"rasterize_mesh: image_size (H, W) expected, got {image_size!r}") from e
    if H < 1 or W < 1:
        raise ValueError(f"rasterize_mesh: image_size (H, W) >= 1 expected, got ({H}, {W})")
    if route not in ops.MESH_RASTER_ROUTES:
        raise ValueError(f"rasterize_mesh: route None, 'brute' or 'bins' expected, got {route!r}")
    dev = verts.device
    R = torch.as_tensor(cameras.R, device=dev).detach().to(torch.float32).reshape(-1, 3, 3)
    T = torch.as_tensor(cameras.T, device=dev).detach().to(torch.float32).reshape(-1, 3)
    B = max(R.shape[0], T.shape[0])
    if R.shape[0] not in (1, B) or T.shape[0] not in (1, B):
        raise ValueError(f"rasterize_mesh: {R.shape[0]} rotations and {T.shape[0]} translations")
    if B == 0:
        empty = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        return MeshFragments(empty(0, H, W, dt=torch.int32), empty(0, H, W, 3, dt=verts.dtype), empty(0, H, W, dt=verts.dtype))
    try:
        focal = _cameras._as_b2(torch.as_tensor(cameras.focal_length).detach(), B, dev)
        pp = _cameras._as_b2(torch.as_tensor(cameras.principal_point).detach(), B, dev)
    except RuntimeError as e:
        raise ValueError(f"rasterize_mesh: {B} views do not match the cameras' focal_length / principal_point") from e
    R, T = R.expand(B, 3, 3), T.expand(B, 3)
    faces = faces.detach().to(dev)
    if verts.is_cuda and verts.dtype == torch.float32 and faces.dtype in (torch.int32, torch.int64):
        return MeshFragments(*ops.mesh_rasterize(verts, faces, R, T, focal, pp, H, W, bool(cull_backfaces), route))
    dt = verts.dtype
    pix, bary, depth = Aggregation.mesh_rasterize(verts, faces, R.to(dt), T.to(dt), focal.to(dt), pp.to(dt), H, W, bool(cull_backfaces))
    return MeshFragments(pix.to(torch.int32), bary, depth)


def interpolate_vertex_attr(fragments, faces, vert_attr, background=0.0):
    """[B,H,W,C]: vert_attr [V,C] of the hit face's three vertices weighted by fragments.bary, `background` (a number or [C]) where
    pix_to_face < 0 -- the image integrate(attr=) and a colour comparison take.  Plain torch, differentiable to vert_attr (and to
    bary where it carries a gradient).  ValueError for faces that are not [F,3] integers or a vert_attr that is not [V,C] floats."""
    _check_faces(faces, "interpolate_vertex_attr")
    if not isinstance(vert_attr, torch.Tensor) or vert_attr.dim() != 2 or not vert_attr.dtype.is_floating_point:
        raise ValueError(f"interpolate_vertex_attr: vert_attr [V,C] of floats expected, got {tuple(getattr(vert_attr, 'shape', ()))}")
    pix, bary = fragments.pix_to_face, fragments.bary
    covered = pix >= 0
    if faces.shape[0] == 0:
        tri = torch.zeros(tuple(pix.shape) + (3,), dtype=torch.long, device=pix.device)
    else:
        tri = faces.to(pix.device).long()[pix.long().clamp(min=0)]                      # [B,H,W,3]
    if vert_attr.shape[0] == 0:
        image = torch.zeros(tuple(pix.shape) + (vert_attr.shape[1],), dtype=vert_attr.dtype, device=vert_attr.device)
    else:
        image = (vert_attr[tri] * bary.to(vert_attr.dtype)[..., None]).sum(-2)      # [B,H,W,3,C] -> [B,H,W,C]
    bg = torch.as_tensor(background, dtype=vert_attr.dtype, device=vert_attr.device)
    return torch.where(covered[..., None], image, bg.expand_as(image))
