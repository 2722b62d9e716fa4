"""Cases, an independent fp64 restatement and the derived bounds shared by tests/test_mesh_raster_cpu.py and
tests/test_gpu_mesh_raster.py.

Every bound here restates voge_amd/csrc/mesh_raster.hip's header (ACCURACY and BACKWARD) and is derived from the roundings of the
seven steps of Aggregation.mesh_rasterize, never fitted to what the kernels return.  With u = 2^-24, for the face a pixel chose:

  P    the largest |x0 R0k| + |x1 R1k| + |x2 R2k| + |Tk| over its corners       M    its largest squared corner norm (view space)
  e_p = 4 u P                           e_n = 2 u M + 2 sqrt(2) e_p sqrt(M)          e_w = |d| (5 u M + sqrt(3) e_n)
  e_b = 4 e_w / |det| + 3 u             e_z = 2 e_b (zmax - zmin) + e_p + 8 u zmax   depth: |d| (e_z + 3 u z)

gradients   the kernels evaluate the nine terms g |d| bary_i N_k / det of a pixel in fp64 from the fp32 inputs, so what separates
            them from fp64 autograd is fp64 roundings (2^-45 of sum |terms| covers them with room), the fixed point -- a vertex
            that m pixels of a view name is off by m q / 2 per view-space component, q = 2^-s, s = 62 - L - e with 2^L >= B H W
            and 2^e > D = max |term|; the rotation back spreads that by at most sqrt(3) -- and one rounding to fp32."""
import functools
import math

import numpy as np
import torch

import meshing_cases as mc
import sample_meshes

U = 2.0 ** -24
MARK = (16, 1e-4)      # the marks of step 7 every test takes out: c = 16, rho = 1e-4
MARK_CAP = 0.02        # and the share of the pixels they may cover


class Case:
    def __init__(self, name, verts, faces, eyes, size, focal, pp):
        self.name, self.verts, self.faces, self.H, self.W = name, verts.float().contiguous(), faces.long().contiguous(), size[0], size[1]
        RT = [mc.look_at(e) for e in eyes]
        self.R = torch.from_numpy(np.stack([r for r, _ in RT]))
        self.T = torch.from_numpy(np.stack([t for _, t in RT]))
        B = len(eyes)
        self.focal = torch.tensor([focal] * B, dtype=torch.float32)
        self.pp = torch.tensor([pp] * B, dtype=torch.float32)

    def cameras(self, device="cpu"):
        return mc.Cams(self.R.to(device), self.T.to(device), self.focal.to(device), self.pp.to(device))

    def args(self, dtype=torch.float32, device="cpu"):
        return tuple(t.to(device=device, dtype=dtype) for t in (self.R, self.T, self.focal, self.pp)) + (self.H, self.W)


def centred_grid():
    v, f = sample_meshes.grid_mesh(23, 13, jitter=0.3)
    return v - torch.tensor([0.5, 0.5, 0.0]), f


@functools.lru_cache(maxsize=None)
def main_cases():
    """Two or three look-at views, 37 x 29 (no multiple of the tile) and 48 x 40 images, intrinsics that are no integers, at least
    half of every image covered"""
    sphere, grid, tet = sample_meshes.level2_sphere(), centred_grid(), sample_meshes.tetrahedron()
    return (
        Case("sphere 29x37", *sphere, [(2.1, 0.9, 1.4), (-1.2, -1.9, 1.3), (0.4, 2.5, -0.6)], (29, 37), (41.3, 40.2), (18.3, 14.6)),
        Case("sphere 40x48", *sphere, [(2.6, 0.3, -0.8), (-0.7, 1.1, 2.4)], (40, 48), (57.7, 59.1), (24.4, 19.7)),
        Case("grid 29x37", *grid, [(0.2, -0.3, 1.5), (0.5, 0.4, -1.4)], (29, 37), (47.3, 61.9), (18.8, 14.1)),
        Case("grid 40x48", *grid, [(-0.3, 0.2, 1.3), (0.1, -0.5, 1.2), (0.3, 0.3, -1.6)], (40, 48), (55.3, 72.6), (23.7, 20.4)),
        Case("tetrahedron 29x37", *tet, [(0.9, 0.5, 0.7), (-0.6, -0.8, -0.5)], (29, 37), (52.6, 51.1), (18.1, 14.9)),
        Case("tetrahedron 40x48", *tet, [(0.2, -1.1, 0.4), (-0.7, 0.3, 0.9), (0.8, 0.6, -0.4)], (40, 48), (61.4, 63.2), (24.6, 20.3)),
    )


# ---- the independent restatement ------------------------------------------------------------------------------------------------

def rasterize_numpy(verts, faces, R, T, focal, pp, H, W, cull_backfaces=False):
    """The rule in fp64, face by face: the ray of a pixel centre against the triangle by scalar triple products; the nearest hit,
    ties to the lower index -> (pix_to_face [B,H,W] int64, bary [B,H,W,3], depth [B,H,W])"""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    R, T, focal, pp = (np.asarray(t, np.float64) for t in (R, T, focal, pp))
    B = R.shape[0]
    pix = np.full((B, H, W), -1, np.int64)
    bary = np.zeros((B, H, W, 3))
    best = np.full((B, H, W), np.inf)
    for b in range(B):
        p = v @ R[b] + T[b]
        d = np.stack(np.broadcast_arrays(((pp[b, 0] - (np.arange(W) + 0.5)) / focal[b, 0])[None, :],
                                         ((pp[b, 1] - (np.arange(H) + 0.5)) / focal[b, 1])[:, None], np.ones((H, W))), -1)      # [H,W,3]
        for k, (ia, ib, ic) in enumerate(f):
            A, Bc, C = p[ia], p[ib], p[ic]
            w = np.stack([d @ np.cross(Bc, C), d @ np.cross(C, A), d @ np.cross(A, Bc)], -1)
            det = w.sum(-1)
            with np.errstate(all="ignore"):
                front = (w >= 0).all(-1) & (det > 0)
                back = (w <= 0).all(-1) & (det < 0)
                bw = w / det[..., None]
                z = bw @ np.array([A[2], Bc[2], C[2]])
                hit = (back if cull_backfaces else (front | back)) & (z > 0) & (z < best[b])
            pix[b][hit] = k
            best[b][hit] = z[hit]
            bary[b][hit] = bw[hit]
        dn = np.linalg.norm(d, axis=-1)
        best[b] = np.where(pix[b] >= 0, best[b] * dn, 0.0)
    return pix, bary, best


# ---- per-pixel quantities and bounds --------------------------------------------------------------------------------------------

@torch.no_grad()
def pixel_geometry(verts, faces, R, T, focal, pp, H, W, pix_to_face):
    """fp64 quantities of the face every pixel chose (all [B,H,W,...], garbage where pix_to_face < 0): corners in view space
    a, b, c, the ray d0, d1, |d|, the edge values w [..,3], det, N = (b - a) x (c - a), P of the docstring"""
    v, f = verts.double(), faces.long()
    R, T, focal, pp = R.double(), T.double(), focal.double(), pp.double()
    B = R.shape[0]
    tri = f[pix_to_face.long().clamp(min=0)]                                          # [B,H,W,3]
    p = torch.einsum("vj,bjk->bvk", v, R) + T[:, None]
    Pabs = (torch.einsum("vj,bjk->bvk", v.abs(), R.abs()) + T.abs()[:, None]).max(-1).values      # [B,V]
    view = torch.arange(B).view(B, 1, 1)
    a, b, c = (p[view, tri[..., i]] for i in range(3))
    P = torch.stack([Pabs[view, tri[..., i]] for i in range(3)], -1).max(-1).values
    d0 = ((pp[:, 0:1] - (torch.arange(W).double() + 0.5)) / focal[:, 0:1])[:, None, :].expand(B, H, W)
    d1 = ((pp[:, 1:2] - (torch.arange(H).double() + 0.5)) / focal[:, 1:2])[:, :, None].expand(B, H, W)
    dn = (d0 * d0 + d1 * d1 + 1).sqrt()
    d = torch.stack((d0, d1, torch.ones_like(d0)), -1)
    n = [torch.linalg.cross(b, c), torch.linalg.cross(c, a), torch.linalg.cross(a, b)]
    w = torch.stack([(d * x).sum(-1) for x in n], -1)
    return dict(a=a, b=b, c=c, d0=d0, d1=d1, dn=dn, w=w, det=w.sum(-1), N=n[0] + n[1] + n[2], P=P, tri=tri)


@torch.no_grad()
def forward_bounds(verts, faces, R, T, focal, pp, H, W, pix_to_face):
    """(bary bound [B,H,W], depth bound [B,H,W]) of the module's docstring at the faces pix_to_face names"""
    g = pixel_geometry(verts, faces, R, T, focal, pp, H, W, pix_to_face)
    zs = torch.stack((g["a"][..., 2], g["b"][..., 2], g["c"][..., 2]), -1)
    M = torch.stack([(g[k] ** 2).sum(-1) for k in "abc"], -1).max(-1).values
    zmax, zr = zs.max(-1).values, zs.max(-1).values - zs.min(-1).values
    e_p = 4 * U * g["P"]
    e_n = 2 * U * M + 2 * math.sqrt(2) * e_p * M.sqrt()
    e_w = g["dn"] * (5 * U * M + math.sqrt(3) * e_n)
    e_b = 4 * e_w / g["det"].abs() + 3 * U
    z = ((g["w"] / g["det"][..., None]) * zs).sum(-1)
    e_z = 2 * e_b * zr + e_p + 8 * U * zmax
    return e_b, g["dn"] * (e_z + 3 * U * z.abs())


@torch.no_grad()
def closed_form_grad(verts, faces, R, T, focal, pp, H, W, pix_to_face, g_depth):
    """(g_verts fp64 [V,3], bound [V,3]): the gradient of (depth * g_depth).sum() to verts at the faces pix_to_face names by the closed
    form d depth / d p_i = |d| bary_i N / det, rotated back through R^T, and the bound of the module's docstring per element"""
    g = pixel_geometry(verts, faces, R, T, focal, pp, H, W, pix_to_face)
    B, V = R.shape[0], verts.shape[0]
    covered = pix_to_face >= 0
    G = torch.where(covered, g_depth.double() * g["dn"], torch.zeros((), dtype=torch.float64))
    det = torch.where(covered, g["det"], torch.ones((), dtype=torch.float64))
    term = G[..., None, None] * (g["w"] / det[..., None])[..., :, None] * (g["N"] / det[..., None])[..., None, :]      # [B,H,W,3 corners,3]
    term = torch.where(covered[..., None, None], term, torch.zeros((), dtype=torch.float64))
    Rd = R.double()
    out, mag = torch.zeros(V, 3, dtype=torch.float64), torch.zeros(V, 3, dtype=torch.float64)
    count = torch.zeros(B, V, dtype=torch.float64)
    for b in range(B):
        view = torch.zeros(V, 3, dtype=torch.float64)
        vmag = torch.zeros(V, 3, dtype=torch.float64)
        for i in range(3):
            idx = g["tri"][b][..., i][covered[b]]
            view.index_add_(0, idx, term[b][covered[b]][:, i])
            vmag.index_add_(0, idx, term[b][covered[b]][:, i].abs())
            count[b].index_add_(0, idx, torch.ones(idx.shape[0], dtype=torch.float64))
        out += view @ Rd[b].T
        mag += vmag @ Rd[b].abs().T
    D = float(term.abs().max()) if term.numel() else 0.0
    L = max(B * H * W - 1, 0).bit_length()
    q = 2.0 ** -(62 - L - math.frexp(D * (1 + 2.0 ** -23))[1])      # (D is rounded UP to fp32 on the device)
    bound = math.sqrt(3) * count.sum(0)[:, None] * q / 2 + 2.0 ** -45 * mag
    bound = bound + U * (out.abs() + bound) + 1e-45
    return out, bound


def workspace_bytes(B, V, F, H, W):
    """voge_mesh_raster_workspace_bytes restated: the larger of the forward's fields -- records of 64 bytes, then the tile counters,
    the cursors, 16 bytes of total, the prefixes and the block totals, each rounded up to 16 -- and the backward's 16-byte head and
    accumulators [B][V][4] of 8 bytes"""
    up16 = lambda n: (n + 15) // 16 * 16
    nt = B * ((W + 15) // 16) * ((H + 15) // 16)
    nb = (nt + 255) // 256
    fwd = B * F * 64 + 3 * up16(4 * nt) + 16 + up16(4 * nb)
    return max(fwd, 16 + B * V * 32)
