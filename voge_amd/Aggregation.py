"""Host-side mirror of VoGE/Aggregation.py (aggregation :82-107, merge_final :111-141,
expend_sigma :144-175, inverse_cumsum :7-8).  The K x K occlusion integral and the attribute
merge run as fused HIP kernels (voge_amd.ops); nothing here builds a [pixels,K,K] tensor."""
import torch

from . import ops


def inverse_cumsum(x, dim):
    return x + torch.sum(x, dim=dim, keepdim=True) - torch.cumsum(x, dim=dim)


def aggregation(sel_idx: torch.Tensor, sel_act: torch.Tensor, sel_len: torch.Tensor, sel_dsd: torch.Tensor,
                occupation_weight: float = 1.):
    """[..., K] hit lists -> (weight [..., K] f32, sel_idx (same tensor), valid_num [...] int64,
    sel_len (same tensor)), as Aggregation.py:82-107."""
    weight, valid_num = ops.composite(sel_idx, sel_act, sel_len, sel_dsd, occupation_weight)
    return weight, sel_idx, valid_num, sel_len


def merge_final(vert_attr: torch.Tensor, weight: torch.Tensor, vert_assign: torch.Tensor, valid_num: torch.Tensor):
    """out[..., c] = sum over the first valid_num slots of vert_attr[idx] * weight; vert_assign is
    updated in place (-1 -> 0) like Aggregation.py:131."""
    assert vert_attr.dim() == 2
    return ops.merge(vert_attr, weight, vert_assign, valid_num)


def expend_sigma(sigma, rotation_matrix=None):
    """(N,) -> s*R, (N,3) -> diag(s)-scaled R rows, (N,3,3) passthrough; R defaults to identity
    (Aggregation.py:144-175)."""
    if sigma.dim() == 3:
        if tuple(sigma.shape[1:]) == (3, 3):
            return sigma
        raise Exception('Got unexpected sigma, which has shape: ' + str(sigma.shape))
    if rotation_matrix is None:
        rotation_matrix = torch.eye(3, device=sigma.device).unsqueeze(0)
    rotation_matrix = rotation_matrix[..., :3, :3]
    if rotation_matrix.dim() == 2:
        rotation_matrix = rotation_matrix.unsqueeze(0)
    if sigma.dim() == 1:
        return sigma[:, None, None] * rotation_matrix
    if sigma.dim() == 2:
        return sigma[:, :, None] * rotation_matrix
    raise Exception('Got unexpected sigma, which has shape: ' + str(sigma.shape))


# quaternion_to_matrix's constant: R - I as a linear map of the 16 products q_a q_b (a, b over w, x, y, z), two terms per entry
_QUAT_TERMS = (((2, 2, -2.0), (3, 3, -2.0)), ((1, 2, 2.0), (0, 3, -2.0)), ((1, 3, 2.0), (0, 2, 2.0)),
               ((1, 2, 2.0), (0, 3, 2.0)), ((1, 1, -2.0), (3, 3, -2.0)), ((2, 3, 2.0), (0, 1, -2.0)),
               ((1, 3, 2.0), (0, 2, -2.0)), ((2, 3, 2.0), (0, 1, 2.0)), ((1, 1, -2.0), (2, 2, -2.0)))


_QUAT_CONSTS = {}


def _quat_consts(like):
    """(the [16,9] map, the 3x3 identity) in a tensor's dtype on its device, made once each (no upload per call)."""
    key = (like.dtype, like.device)
    c = _QUAT_CONSTS.get(key)
    if c is None:
        m = torch.zeros((16, 9), dtype=like.dtype)
        for col, terms in enumerate(_QUAT_TERMS):
            for a, b, coef in terms:
                m[4 * a + b, col] = coef
        c = _QUAT_CONSTS[key] = (m.to(like.device), torch.eye(3, dtype=like.dtype, device=like.device))
    return c


def quaternion_to_matrix(quats):
    """[..., 4] quaternions (w, x, y, z), not necessarily unit -> [..., 3, 3] rotation matrices of q / |q|:
    [[1-2(y^2+z^2), 2(xy-wz), 2(xz+wy)], [2(xy+wz), 1-2(x^2+z^2), 2(yz-wx)], [2(xz-wy), 2(yz+wx), 1-2(x^2+y^2)]].  A quaternion
    whose squared norm is not a positive finite number is the identity rotation and gets a zero gradient.  Differentiable torch,
    any device / dtype, a handful of launches each way (the products q_a q_b through one constant [16,9] map): the definition the
    oriented frame path (ops.frame_trace_ori) is tested against, and its fallback."""
    assert quats.shape[-1] == 4, 'quats[..,4] expected, got shape: ' + str(tuple(quats.shape))
    n2 = (quats * quats).sum(-1, keepdim=True)
    ok = (n2 > 0) & torch.isfinite(n2)
    unit = torch.zeros_like(quats)
    unit[..., 0] = 1
    qs = torch.where(ok, quats, unit)      # (a constant where the norm is unusable: nothing flows back to such a quaternion)
    qh = qs / torch.sqrt((qs * qs).sum(-1, keepdim=True))
    outer = (qh[..., :, None] * qh[..., None, :]).reshape(quats.shape[:-1] + (16,))
    qmap, eye = _quat_consts(quats)
    return (outer @ qmap).reshape(quats.shape[:-1] + (3, 3)) + eye


def oriented_sigma(scales, quats):
    """S = R(q) diag(scales) R(q)^T [..., N, 3, 3]: what an (N,3,3) `sigmas` holds for the oriented Gaussians (scales [..,N,3],
    quats [..,N,4]); S_ij = sum_k (s_k R_ik) R_jk, the upper triangle mirrored, so S is bitwise symmetric."""
    assert scales.shape[-1] == 3 and quats.shape[-1] == 4 and scales.shape[:-1] == quats.shape[:-1], \
        'scales[..,3] and quats[..,4] with the same leading dims expected, got ' + str(tuple(scales.shape)) + ' / ' + str(tuple(quats.shape))
    R = quaternion_to_matrix(quats)
    p = (scales[..., None, :] * R)[..., :, None, :] * R[..., None, :, :]      # [.., i, j, k] = (s_k R_ik) R_jk
    S = (p[..., 0] + p[..., 1]) + p[..., 2]
    return torch.triu(S) + torch.triu(S, 1).transpose(-1, -2)


def gaussian_normals_shapes(scales, quats, verts, cam_center):
    """(B, N) of gaussian_normals' arguments, checked: scales [N,3] | [B,N,3], quats [N,4] | [B,N,4] with the same leading
    dimensions, verts [N,3] | [B,N,3], cam_center [B,3]."""
    if (scales.dim() not in (2, 3) or scales.shape[-1] != 3 or quats.shape[-1:] != (4,) or quats.shape[:-1] != scales.shape[:-1]):
        raise ValueError('scales[N,3] or [B,N,3] and quats[N,4] or [B,N,4] with the same leading dims expected, got '
                         + str(tuple(scales.shape)) + ' / ' + str(tuple(quats.shape)))
    if cam_center.dim() != 2 or cam_center.shape[-1] != 3 or verts.shape[-1:] != (3,) or verts.dim() not in (2, 3):
        raise ValueError('verts[N,3] or [B,N,3] and cam_center[B,3] expected, got ' + str(tuple(verts.shape)) + ' / ' + str(tuple(cam_center.shape)))
    B, N = cam_center.shape[0], scales.shape[-2]
    if verts.shape[-2] != N or (verts.dim() == 3 and verts.shape[0] != B) or (scales.dim() == 3 and scales.shape[0] != B):
        raise ValueError(f'verts {tuple(verts.shape)} do not match scales {tuple(scales.shape)} and cam_center {tuple(cam_center.shape)}')
    return B, N


def gaussian_normals(scales, quats, verts, cam_center, inverse_sigma=False):
    """Per-view normals [B*N, 3] (row b*N + n: what the fragments of a B-view render index) of oriented Gaussians: scales [N,3]
    or [B,N,3]; quats [N,4] or [B,N,4] (w, x, y, z; not necessarily unit; the leading dimensions of scales); verts [N,3] or
    [B,N,3]; cam_center [B,3].  An extension: the reference has none.

    The oriented Gaussian S = R diag(s) R^T, R = quaternion_to_matrix(quats), stands for a flat surface element, and its normal
    is its thinnest axis -- a COLUMN of R, the axes of S being the columns of R.  S stands where a `sigmas` would: with
    inverse_sigma=False the trace uses A = 2 S, so a LARGER s_k is a thinner extent; with inverse_sigma=True it uses
    A = R diag(2 / s) R^T, so a SMALLER s_k is thinner.  The axis k*: start at k = 0; for j = 1, 2 in that order take j if
    s_j > s_k (inverse_sigma=False) or s_j < s_k (True) -- exact ties keep the lowest index, a NaN never wins, a NaN in s_0 stays
    chosen.  n0 = R[:, k*].  For view b, delta = v - c_b and t = n0 . delta: the output is -n0 where t > 0 and n0 otherwise, the
    side get_normals picks (n . delta <= 0: towards the camera); t == 0, delta == 0 and a NaN t keep n0.

    Only quats get a gradient: through the chosen column of R, orthogonal to quats, summed over the views when the quaternions
    are shared, zero for a quaternion without a usable norm (the identity rotation).  The axis and the sign are constants, so
    scales, verts and cam_center get none (no graph edge).  Differentiable torch on any device / dtype: the definition the kernel
    (ops._GaussNormals, Renderer.gaussian_normals) is tested against, and the route for everything the kernel does not take."""
    B, N = gaussian_normals_shapes(scales, quats, verts, cam_center)
    R = quaternion_to_matrix(quats)                                              # [.., N, 3, 3]
    sc = scales.detach()
    s0, s1, s2 = sc[..., 0], sc[..., 1], sc[..., 2]
    better = torch.lt if inverse_sigma else torch.gt
    take1 = better(s1, s0)
    take2 = better(s2, torch.where(take1, s1, s0))
    k = torch.where(take2, torch.full_like(take1, 2, dtype=torch.long), take1.long())
    n0 = torch.gather(R, -1, k[..., None, None].expand(k.shape + (3, 1))).squeeze(-1)      # [.., N, 3]: column k* of R
    n0 = n0 if n0.dim() == 3 else n0[None]
    delta = ((verts if verts.dim() == 3 else verts[None]) - cam_center[:, None, :]).detach()
    t = (n0.detach() * delta).sum(-1, keepdim=True)                              # [B, N, 1]
    return torch.where(t > 0, -n0, n0).reshape(B * N, 3)


# The orthonormal real spherical harmonics of degree <= 3 as polynomials of a unit vector (x, y, z), in the order and with the
# signs trained Gaussian scenes store their colour coefficients in.
_SH_C0 = 0.28209479177387814
_SH_C1 = 0.4886025119029199
_SH_C2 = (1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
_SH_C3 = (0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277)


def _sh_basis(d, count):
    """[..., 3] unit vectors -> the first `count` (1, 4, 9 or 16) basis values, a list of [...] tensors."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = [torch.full_like(x, _SH_C0)]
    if count > 1:
        Y += [-_SH_C1 * y, _SH_C1 * z, -_SH_C1 * x]
    if count > 4:
        xx, yy, zz = x * x, y * y, z * z
        a, b, c = _SH_C2
        Y += [a * (x * y), -a * (y * z), b * (2 * zz - xx - yy), -a * (x * z), c * (xx - yy)]
    if count > 9:
        a, b, c, e, f = _SH_C3
        q = 4 * zz - xx - yy
        Y += [-a * (y * (3 * xx - yy)), b * (x * y * z), -c * (y * q), e * (z * (2 * zz - 3 * xx - 3 * yy)), -c * (x * q),
              f * (z * (xx - yy)), -a * (x * (xx - 3 * yy))]
    return Y


def sh_degree(sh, degree=None):
    """The active degree of sh [N, M, C] (M in {1, 4, 9, 16}: maximum degree L = sqrt(M) - 1), checked: `degree`, or L."""
    if sh.dim() != 3 or sh.shape[1] not in (1, 4, 9, 16):
        raise ValueError('sh[N, M, C] with M in (1, 4, 9, 16) expected, got shape: ' + str(tuple(sh.shape)))
    L = (1, 4, 9, 16).index(sh.shape[1])
    if degree is None:
        return L
    if int(degree) != degree or not 0 <= degree <= L:
        raise ValueError(f'degree must be an integer in 0..{L} for sh of shape {tuple(sh.shape)}, got {degree!r}')
    return int(degree)


def sh_colors(sh, verts, cam_center, degree=None, clamp=True):
    """View-dependent colours [B*N, C] (row b*N + n: what the fragments of a B-view render index) from spherical-harmonic
    coefficients sh [N, M, C], M in {1, 4, 9, 16}; verts [N,3] or [B,N,3]; cam_center [B,3].  An extension: the reference has none.

    For view b and Gaussian n: delta = v - c_b, d = delta / |delta| -- the direction from the camera to the Gaussian; where
    |delta|^2 <= 1e-20, d = 0: only the constant term survives and verts gets no gradient --
        pre[b,n,:] = sum_{m < (degree+1)^2} Y_m(d) sh[n,m,:] + 0.5,      out = relu(pre) if clamp else pre.
    `degree` (default: the maximum, sqrt(M) - 1) is the ACTIVE degree: the coefficients above it are not read and get a zero
    gradient (progressive training).  Y_m, the +0.5 and the clamp at 0 are the convention trained Gaussian scenes are stored in.

    Differentiable torch on any device / dtype (sh, verts and cam_center all get autograd's gradient): the definition the kernel
    (ops._ShColors, Renderer.sh_to_colors) is tested against, and the route for everything the kernel does not take."""
    degree = sh_degree(sh, degree)
    if cam_center.dim() != 2 or cam_center.shape[-1] != 3 or verts.shape[-1] != 3 or verts.dim() not in (2, 3):
        raise ValueError('verts[N,3] or [B,N,3] and cam_center[B,3] expected, got ' + str(tuple(verts.shape)) + ' / ' + str(tuple(cam_center.shape)))
    B, N = cam_center.shape[0], sh.shape[0]
    if verts.shape[-2] != N or (verts.dim() == 3 and verts.shape[0] != B):
        raise ValueError(f'verts {tuple(verts.shape)} do not match sh {tuple(sh.shape)} and cam_center {tuple(cam_center.shape)}')
    delta = (verts if verts.dim() == 3 else verts[None]) - cam_center[:, None, :]
    n2 = (delta * delta).sum(-1, keepdim=True)
    ok = n2 > 1e-20
    inv = torch.where(ok, torch.rsqrt(torch.where(ok, n2, torch.ones_like(n2))), torch.zeros_like(n2))
    active = (degree + 1) ** 2
    Y = torch.stack(_sh_basis(delta * inv, active), dim=-1)                      # [B, N, active]
    pre = torch.einsum('bnm,nmc->bnc', Y, sh[:, :active]) + 0.5
    return (torch.relu(pre) if clamp else pre).reshape(B * N, sh.shape[2])


def _shifted(x, dim, k):
    """y[.., i, ..] = x[.., i + k, ..] along `dim` for k = +-1, zeros (False) where i + k falls outside."""
    n = x.shape[dim]
    if n == 0:
        return x
    pad = torch.zeros_like(x.narrow(dim, 0, 1))
    return torch.cat([x.narrow(dim, 1, n - 1), pad], dim) if k > 0 else torch.cat([pad, x.narrow(dim, 0, n - 1)], dim)


def _stencil_difference(P, d, valid, dim, edge):
    """The finite difference of P [B,h,W,3] along `dim` (1: rows, 2: columns) by the rule of depth_normals -> (D, exists)."""
    up, um = _shifted(valid, dim, 1), _shifted(valid, dim, -1)
    if edge is not None:
        up = up & ((_shifted(d, dim, 1) - d).abs() <= edge * d)
        um = um & ((_shifted(d, dim, -1) - d).abs() <= edge * d)
    Pp, Pm = _shifted(P, dim, 1), _shifted(P, dim, -1)
    up3, um3 = up[..., None], um[..., None]
    D = torch.where(up3 & um3, Pp - Pm, torch.where(up3, Pp - P, torch.where(um3, P - Pm, torch.zeros_like(P))))
    return D, up | um


def depth_normals(depth, rays, edge=None):
    """Surface normals [B,h,W,3] of a depth map (an extension: the reference has neither): depth [B,h,W] is the distance along
    each pixel's UNIT ray -- what Renderer.get_depth returns, not view-space z --, rays [B,h,W,3] the unit world-space directions
    of the same pixels (cameras.pixel_rays).  The normal of the rendered surface from finite differences of the back-projected
    points; the camera centre cancels in every difference and is not needed.

        valid = isfinite(depth) & (depth > 0),      P = depth * ray
        a neighbour (i, j +- 1) is USABLE if it lies inside [0, W), is valid and -- with an `edge`, a relative depth jump that
            cuts the stencil at occlusion boundaries -- |depth_nb - depth| <= edge * depth
        D_x = P(j+1) - P(j-1) if both are usable, P(j+1) - P(j) or P(j) - P(j-1) if one is, undefined if neither;
        D_y the same along i inside [0, h) (rows outside the band do not exist)
        c = D_x x D_y;  the pixel is DEFINED iff it is valid, both differences exist and 0 < |c|^2 < inf
        n = c / |c|, negated where n . ray > 0 (the normal faces the camera: no handedness convention leaks out); (0, 0, 0)
            at every pixel that is not defined.

    The gradient flows through P, the cross product and the normalisation to `depth` (and to `rays`); the choice of stencil,
    the edge test and the sign are constants.  A pixel that is not defined gives its upstream gradient to nothing, and a depth
    that is not valid gets exactly zero; NaN and inf in such depths reach no output and no gradient (every masked quantity is
    replaced BEFORE it is used: no sqrt(0), no 0/0 under a where).

    fp32: the differences cancel, so the error is about 2^-23 * depth / pixel footprint -- 2e-6 to 5e-6 at focal lengths of 30
    to 60 pixels, 3.3e-5 at 500, 1.2e-4 at 2000 and distance 6 (against fp64, on the same depth values).  That is the floor of
    the problem in this number format: the kernels avoid it in their own arithmetic (normals.hip), nobody avoids it for the
    rounding the fp32 depth values already carry.

    Differentiable torch on any device / dtype: the definition the kernels (ops._DepthNormals, Renderer.get_normals) are tested
    against, and the route for everything they do not take."""
    if depth.dim() != 3 or tuple(rays.shape) != tuple(depth.shape) + (3,):
        raise ValueError(f'depth[B,h,W] and rays[B,h,W,3] expected, got {tuple(depth.shape)} / {tuple(rays.shape)}')
    if edge is not None:
        edge = float(edge)
        if not 0.0 <= edge < float('inf'):
            raise ValueError(f'edge must be None or a finite relative depth jump >= 0, got {edge!r}')
    valid = torch.isfinite(depth) & (depth > 0)
    d = torch.where(valid, depth, torch.zeros_like(depth))
    P = d[..., None] * rays
    Dx, has_x = _stencil_difference(P, d.detach(), valid, 2, edge)
    Dy, has_y = _stencil_difference(P, d.detach(), valid, 1, edge)
    c = torch.cross(Dx, Dy, dim=-1)
    c2 = (c * c).sum(-1).detach()
    defined = valid & has_x & has_y & (c2 > 0) & torch.isfinite(c2)
    c = torch.where(defined[..., None], c, torch.zeros_like(c))
    n = c * torch.rsqrt(torch.where(defined, (c * c).sum(-1), torch.ones_like(c2)))[..., None]
    away = (n.detach() * rays.detach()).sum(-1, keepdim=True) > 0
    return torch.where(away, -n, n)


def distortion(weight, hit_length, valid_num, normalize=False):
    """Depth-distortion regulariser [..] of composited fragments (an extension: the reference has none): weight, hit_length
    [.., K], valid_num [..].  Over the n = min(max(valid_num, 0), K) live slots of a pixel, with w = weight and t = hit_length,

        L = sum_i sum_j w_i w_j |t_i - t_j|

    evaluated WITHOUT a [.., K, K] tensor: a stable sort of the live slots by t puts them in the total order (t_k, k) -- ascending
    t, exact ties by slot position --, u_k = t_k - t_first recentres them on the smallest live t (L is translation invariant; in
    fp32 the closed form on t itself loses 2e-4 at t = 1000, on u it holds 2e-7 at any offset) and, with the exclusive prefix
    sums W<_i = sum_{j before i} w_j and X<_i = sum_{j before i} w_j u_j,

        L = 2 sum_i w_i (u_i W<_i - X<_i).

    Autograd through this form yields dL/dw_i = 2 [u_i (W<_i - W>_i) - (X<_i - X>_i)] and dL/dt_i = 2 w_i (W<_i - W>_i) (W>, X>:
    the same sums over the slots after i) -- at an exact tie the POSITIONAL subgradient, the earlier slot counting as nearer: tied
    i before j get -2 w_i w_j and +2 w_i w_j, not the sign(0) = 0 of the pairwise expression.  Dead slots get exactly zero.

    normalize=False: L (0 where nothing is hit).  normalize=True: L / S^2 with S = sum_k w_k where S > 0 -- the distortion of the
    weights rescaled to sum to 1 --, 0 with zero gradient elsewhere.

    Differentiable torch on any device / dtype, O(K) memory a pixel: the definition the kernels (ops._Distortion,
    Renderer.get_distortion) are tested against, and the route for everything they do not take."""
    if hit_length.shape != weight.shape or valid_num.shape != weight.shape[:-1]:
        raise ValueError(f'weight {tuple(weight.shape)}, hit_length {tuple(hit_length.shape)} and valid_num {tuple(valid_num.shape)} '
                         'do not describe the same fragments')
    K = weight.shape[-1]
    live = torch.arange(K, device=weight.device) < valid_num.clamp(0, K)[..., None]
    key = torch.where(live, hit_length.detach(), torch.full_like(hit_length, float('inf')))      # (dead slots sort last)
    order = torch.sort(key, dim=-1, stable=True)[1]
    w = torch.gather(torch.where(live, weight, torch.zeros_like(weight)), -1, order)
    t = torch.gather(torch.where(live, hit_length, torch.zeros_like(hit_length)), -1, order)
    live = torch.gather(live, -1, order)
    u = torch.where(live, t - t[..., :1].detach(), torch.zeros_like(t))
    x = w * u
    zero = torch.zeros_like(w[..., :1])
    w_before = torch.cat([zero, w[..., :-1]], -1).cumsum(-1)      # (exclusive prefix sums)
    x_before = torch.cat([zero, x[..., :-1]], -1).cumsum(-1)
    L = 2 * (w * (u * w_before - x_before)).sum(-1)
    if not normalize:
        return L
    S = w.sum(-1)
    hit = S > 0
    return torch.where(hit, L / torch.where(hit, S * S, torch.ones_like(S)), torch.zeros_like(L))


def _safe_norm(x):
    """|x| over the last axis and the mask of the rows where it is positive; a zero row gives 0 and passes a ZERO gradient
    (torch.linalg.norm gives NaN there)."""
    s = (x * x).sum(-1)
    ok = s.detach() > 0
    return torch.where(ok, torch.sqrt(torch.where(ok, s, torch.ones_like(s))), torch.zeros_like(s)), ok


def mesh_edge_term(verts, edges, target_length=0.0):
    """Edge-length regulariser (PyTorch3D's mesh_edge_loss; an extension here): verts [V,3] | [B,V,3], edges [E,2] integer,

        (1 / E) sum_e (|v_i - v_j| - t)^2,

    the mean over the B meshes for a batch.  Where |v_i - v_j| = 0 the term is t^2 and the gradient 0, not torch's NaN; E = 0
    (or an empty batch) gives 0.  Differentiable torch on any device / dtype: the definition ops._MeshReg is tested against and
    the route for everything it does not take."""
    if edges.shape[0] == 0 or verts.numel() == 0:
        return verts.new_zeros(())
    e = edges.long()
    length, _ = _safe_norm(verts[..., e[:, 0], :] - verts[..., e[:, 1], :])
    return ((length - target_length) ** 2).mean()


def mesh_laplacian_term(verts, nbr_off, nbr):
    """Uniform-weight Laplacian smoothing (PyTorch3D's mesh_laplacian_smoothing(method="uniform"); an extension here): verts
    [V,3] | [B,V,3], the adjacency as CSR (nbr_off [V+1], nbr [2E] integer),

        L_i = (1 / d_i) sum_{j in N(i)} (v_j - v_i)   (0 where d_i = 0),        (1 / V) sum_i |L_i|,

    the norm and not its square, the mean over the B meshes for a batch.  The DIFFERENCES are summed, not the positions: a fine
    mesh far from the origin would otherwise lose its Laplacian to cancellation.  Where L_i is exactly 0 the gradient through it
    is 0.  PyTorch3D's "cot" and "cotcurv" weightings are out of scope.  Differentiable torch on any device / dtype (on a GPU its
    index_add_ uses float atomics, so the bits may differ from run to run; ops._MeshReg has none)."""
    V = verts.shape[-2]
    if verts.numel() == 0:
        return verts.new_zeros(())
    off, nb = nbr_off.long(), nbr.long()
    deg = off[1:] - off[:-1]
    owner = torch.repeat_interleave(torch.arange(V, device=verts.device), deg, output_size=nb.shape[0])      # (no host round trip)
    diff = verts[..., nb, :] - verts[..., owner, :]
    L = torch.zeros_like(verts).index_add_(-2, owner, diff) / deg.clamp(min=1).to(verts.dtype)[:, None]
    return _safe_norm(L)[0].mean()


def mesh_normal_term(verts, pairs):
    """Normal consistency of neighbouring faces (PyTorch3D's mesh_normal_consistency; an extension here): verts [V,3] | [B,V,3],
    pairs [P,4] = (v0, v1, a, b) integer, one row for two faces that share the edge (v0, v1) with the opposite vertices a, b,

        n0 = (v1 - v0) x (a - v0),   n1 = -(v1 - v0) x (b - v0),        (1 / P) sum (1 - n0 . n1 / (|n0| |n1|)),

    independent of the faces' winding; the mean over the B meshes for a batch.  A pair with a zero-area face contributes 1 and
    passes no gradient; P = 0 gives 0.  Differentiable torch on any device / dtype."""
    if pairs.shape[0] == 0 or verts.numel() == 0:
        return verts.new_zeros(())
    p = pairs.long()
    v0 = verts[..., p[:, 0], :]
    e, a, b = verts[..., p[:, 1], :] - v0, verts[..., p[:, 2], :] - v0, verts[..., p[:, 3], :] - v0
    n0, n1 = torch.cross(e, a, dim=-1), torch.cross(b, e, dim=-1)
    l0, ok0 = _safe_norm(n0)
    l1, ok1 = _safe_norm(n1)
    ok = ok0 & ok1
    one = torch.ones_like(l0)
    cos = (torch.where(ok[..., None], n0, torch.zeros_like(n0)) * n1).sum(-1) / torch.where(ok, l0 * l1, one)
    return (1 - cos).mean()


def nearest_rows(queries, points):
    """For every row of queries [Nq,3] the lexicographically smallest (d2, index) over points [Np,3] (Np >= 1) -> (idx [Nq] int64,
    d2 [Nq]), in the tensors' own dtype and not differentiable: d2 = (dx*dx + dy*dy) + dz*dz, each a single operation of that
    dtype, rows of the Nq x Np matrix in chunks, an exact tie keeps the LOWER index (the minimum over the indices that attain the
    row's minimum: no reliance on which of several equal entries torch.min reports)."""
    q, p = queries.detach(), points.detach()
    Nq, Np = q.shape[0], p.shape[0]
    idx = torch.empty((Nq,), dtype=torch.long, device=q.device)
    d2 = torch.empty((Nq,), dtype=q.dtype, device=q.device)
    chunk = max(1, (1 << 24) // max(Np, 1))
    ar = torch.arange(Np, device=q.device)
    for s in range(0, Nq, chunk):
        e = min(s + chunk, Nq)
        dx, dy, dz = q[s:e, None, 0] - p[None, :, 0], q[s:e, None, 1] - p[None, :, 1], q[s:e, None, 2] - p[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        m = d.min(dim=1).values
        d2[s:e] = m
        idx[s:e] = torch.where(d == m[:, None], ar[None, :], Np).min(dim=1).values
    return idx, d2


def chamfer_term(x, y, single_directional=False, point_reduction="mean", return_indices=False):
    """Chamfer distance of two clouds (PyTorch3D's chamfer_distance at norm=2, without lengths and weights; an extension here):
    x [Nx,3], y [Ny,3],

        (1 / Nx) sum_i min_j |x_i - y_j|^2 + (1 / Ny) sum_j min_i |y_j - x_i|^2,

    point_reduction="sum" without the two divisors, single_directional the first sum alone.  The nearest indices come from
    nearest_rows (a tie keeps the lower index) and are constants of the graph, as the argmin of a min is; the distances are
    recomputed from them, so both clouds get gradients.  return_indices=True: (loss, nn_x, nn_y | None), int64.  Differentiable torch
    on any device / dtype: the definition ops._Chamfer is tested against and the route for everything it does not take."""
    if point_reduction not in ("mean", "sum"):
        raise ValueError(f"chamfer_term: point_reduction must be 'mean' or 'sum', got {point_reduction!r}")
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != 3 or y.shape[1] != 3 or x.shape[0] == 0 or y.shape[0] == 0:
        raise ValueError(f"chamfer_term: non-empty x [Nx,3] and y [Ny,3] expected, got {tuple(x.shape)} / {tuple(y.shape)}")
    y = y.to(x.dtype)
    reduce = torch.mean if point_reduction == "mean" else torch.sum
    nn_x = nearest_rows(x, y)[0]
    loss = reduce(((x - y[nn_x]) ** 2).sum(-1))
    nn_y = None
    if not single_directional:
        nn_y = nearest_rows(y, x)[0]
        loss = loss + reduce(((y - x[nn_y]) ** 2).sum(-1))
    return (loss, nn_x, nn_y) if return_indices else loss


def _face_cross(e1, e2):
    """e1 x e2 over the last axis, each component (p * q) - (r * s) as separate operations"""
    return torch.stack(((e1[..., 1] * e2[..., 2]) - (e1[..., 2] * e2[..., 1]),
                        (e1[..., 2] * e2[..., 0]) - (e1[..., 0] * e2[..., 2]),
                        (e1[..., 0] * e2[..., 1]) - (e1[..., 1] * e2[..., 0])), -1)


def _ieee_sqrt(x):
    """sqrt(x), correctly rounded for fp32: torch's vectorised fp32 sqrt on the host is not always (a last-bit difference in
    about 0.6 % of random arguments on an AVX-512 build), its fp64 one rounded to fp32 is -- the square root of a 24-bit number
    never lies within 2^-53 of the midpoint of two fp32 numbers, so the second rounding changes nothing.  Other dtypes: torch.sqrt."""
    return torch.sqrt(x.double()).to(x.dtype) if x.dtype == torch.float32 else torch.sqrt(x)


def mesh_face_areas2(verts, faces):
    """A2 [F]: the doubled area of every face of verts [V,3], faces [F,3] integer, in the vertices' dtype and not differentiable:
    e1 = b - a, e2 = c - a (positions are differenced first), cr = e1 x e2, A2 = sqrt((crx^2 + cry^2) + crz^2), every operation a
    separate torch op (the square root through _ieee_sqrt) -- what mesh_surface_points chooses faces by, and bit for bit what voge_mesh_sample_fwd computes."""
    v, f = verts.detach(), faces.long()
    a = v[f[:, 0]]
    cr = _face_cross(v[f[:, 1]] - a, v[f[:, 2]] - a)
    return _ieee_sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])


def mesh_surface_points(verts, faces, u, return_normals=False, face_idx=None):
    """Points on the surface of a triangle mesh, faces chosen by area (PyTorch3D's sample_points_from_meshes for one mesh and a
    GIVEN random table; an extension here): verts [V,3], faces [F,3] integer (F >= 1), u [S,3] in [0,1) ->
    (points [S,3], normals [S,3] | None, face_idx [S] int64, bary [S,3]).

      faces   A2 = mesh_face_areas2 in the vertices' dtype; cdf = its inclusive cumulative sum in fp64, total = cdf[F-1];
              t_s = float64(u_s0) * total; face_idx_s = the smallest f with cdf[f] > t_s, strictly -- a face of area 0 is never
              chosen, wherever it sits.  u is clamped to [0, 1 - 2^-24] first and a NaN becomes 0;
      points  PyTorch3D's _rand_barycentric_coords: r = sqrt(u_s1), w0 = 1 - r, w1 = r (1 - u_s2), w2 = r u_s2,
              p = a + (w1 e1 + w2 e2), bary = (w0, w1, w2);
      normals cr / A2 of the chosen face.

    total == 0 or not finite (every face degenerate, a NaN vertex): every face_idx is -1, points, normals and bary are 0 and
    verts get a zero gradient; nothing raises and nothing is read back on the host.  The face choice and u are constants of the
    graph; verts get gradients through a, e1, e2 and through the normals.  face_idx (integer [S]) overrides the choice -- the
    expression evaluated at given faces, what the tests compare a kernel's output with; an entry below 0 gives a zero sample.
    Every operation is a separate torch op, so the host result is plain IEEE arithmetic of the vertices' dtype.  Differentiable
    torch on any device / dtype: the definition ops._MeshSample is tested against and the route for everything it does not take."""
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or u.dim() != 2 or u.shape[1] != 3:
        raise ValueError(f"mesh_surface_points: verts [V,3], faces [F,3], u [S,3] expected, got {tuple(verts.shape)} / "
                         f"{tuple(faces.shape)} / {tuple(u.shape)}")
    F = faces.shape[0]
    if F == 0:
        raise ValueError("mesh_surface_points: a mesh without faces")
    f = faces.long()
    u = u.detach().to(verts.dtype)
    u = torch.where(torch.isnan(u), torch.zeros_like(u), u).clamp(0.0, 1.0 - 2.0 ** -24)
    cdf = torch.cumsum(mesh_face_areas2(verts, f).double(), 0)
    total = cdf[-1]
    ok = (total > 0) & torch.isfinite(total)
    if face_idx is None:
        idx = torch.searchsorted(cdf, u[:, 0].double() * total, right=True).clamp(max=F - 1)
        valid = ok.expand(idx.shape)
    else:
        valid = ok & (face_idx >= 0)
        idx = face_idx.long().clamp(0, F - 1)
    # a degenerate mesh is evaluated on zeros: finite values everywhere, and `where` passes the vertices a zero gradient
    v = torch.where(ok, verts, torch.zeros_like(verts))
    tri = f[idx]
    a = v[tri[:, 0]]
    e1, e2 = v[tri[:, 1]] - a, v[tri[:, 2]] - a
    r = _ieee_sqrt(u[:, 1])
    w0, w1, w2 = 1 - r, r * (1 - u[:, 2]), r * u[:, 2]
    p = a + (w1[:, None] * e1 + w2[:, None] * e2)
    zero = torch.zeros_like(p)
    points = torch.where(valid[:, None], p, zero)
    bary = torch.where(valid[:, None], torch.stack((w0, w1, w2), -1), zero)
    normals = None
    if return_normals:
        cr = _face_cross(e1, e2)
        s = (cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2]
        pos = s.detach() > 0
        A2 = _ieee_sqrt(torch.where(pos, s, torch.ones_like(s)))
        normals = torch.where((valid & pos)[:, None], cr / A2[:, None], zero)
    return points, normals, torch.where(valid, idx, torch.full_like(idx, -1)), bary


def _dot3(x, y):
    """(x0 y0 + x1 y1) + x2 y2 over the last axis, every operation a separate torch op"""
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _recip_or_zero(x):
    """1 / x where x > 0 and the reciprocal is finite, else 0 -- the zero cases of point_triangle_closest, folded into the factor"""
    pos = x > 0
    r = 1 / torch.where(pos, x, torch.ones_like(x))
    return torch.where(pos & torch.isfinite(r), r, torch.zeros_like(r))


def point_triangle_closest(points, a, b, c):
    """The closest point of the triangle (a, b, c) to every point (PyTorch3D's point-to-face distance without its
    min_triangle_area; an extension here): points, a, b, c [..., 3], broadcast against each other -> (d2 [...], bary [..., 3]).

    Differences first: e0 = b - a, e1 = c - a, v = p - a -- nothing below sees a position, so a mesh at (1000, 1000, 1000) keeps
    the bounds of one at the origin.  Four candidates, each a point of the triangle, in this order:

      interior  n = e0 x e1, nn = n.n; w2 = ((e0 x v).n) (1 / nn), w1 = ((v x e1).n) (1 / nn), w0 = (1 - w1) - w2; it EXISTS only if
                nn > 0 and w0, w1, w2 >= 0; r = v - (w1 e0 + w2 e1), weights (w0, w1, w2);
      ab        t = clamp((v.e0) (1 / e0.e0), 0, 1), r = v - t e0, weights (1 - t, t, 0);
      bc        vb = v - e0, eb = e1 - e0, t = clamp((vb.eb) (1 / eb.eb), 0, 1), r = vb - t eb, weights (0, 1 - t, t);
      ca        walked from a: t = clamp((v.e1) (1 / e1.e1), 0, 1), r = v - t e1, weights (1 - t, 0, t);

    d2 = (rx rx + ry ry) + rz rz of the candidate, every operation one operation of the tensors' dtype; a reciprocal is taken
    once and multiplied with (what the kernels do: no division per pair), and is 0 where its argument is 0 or where it would
    not be finite -- t = 0 on an edge of length 0, no interior candidate on a triangle without area.  The result is the smallest
    d2; an exact tie keeps the EARLIER candidate.  The minimum over all four, not a walk through Voronoi regions: every candidate
    is a point of the triangle, so a candidate whose weights are poor (a sliver's interior) can only lose.  Two consequences:
    a zero-area triangle is the union of its three segments, and a zero-length edge is a point (a = b = c: the point a, weights
    (1, 0, 0)).  Nothing is NaN for finite inputs whose squares do not overflow, and there is NO area threshold: PyTorch3D's
    min_triangle_area depends on the scale of the mesh and is the one deliberate deviation.

    The weights are constants of the graph, as the argmin of a min is: q minimises over the triangle, so their derivative drops
    out (the envelope theorem) and d d2 / dp = 2 (p - q), d d2 / d(a, b, c) = -2 w_r (p - q).  bary carries no gradient."""
    pd, ad, bd, cd = points.detach(), a.detach(), b.detach(), c.detach()
    e0, e1, v = bd - ad, cd - ad, pd - ad
    n = _face_cross(e0, e1)
    inn = _recip_or_zero(_dot3(n, n))
    w2 = _dot3(_face_cross(e0, v), n) * inn
    w1 = _dot3(_face_cross(v, e1), n) * inn
    w0 = (1 - w1) - w2
    inside = (inn > 0) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
    t_ab = (_dot3(v, e0) * _recip_or_zero(_dot3(e0, e0))).clamp(0, 1)
    vb, eb = v - e0, e1 - e0
    t_bc = (_dot3(vb, eb) * _recip_or_zero(_dot3(eb, eb))).clamp(0, 1)
    t_ca = (_dot3(v, e1) * _recip_or_zero(_dot3(e1, e1))).clamp(0, 1)
    # the same residuals once more on the attached inputs, the weights as constants
    e0, e1, v = b - a, c - a, points - a
    r = v - (w1[..., None] * e0 + w2[..., None] * e1)
    d_in = _dot3(r, r)
    r = v - t_ab[..., None] * e0
    d_ab = _dot3(r, r)
    r = (v - e0) - t_bc[..., None] * (e1 - e0)
    d_bc = _dot3(r, r)
    r = v - t_ca[..., None] * e1
    d_ca = _dot3(r, r)
    zero = torch.zeros_like(t_ab)
    take = ~inside | (d_ab.detach() < d_in.detach())
    d2 = torch.where(take, d_ab, d_in)
    bary = torch.where(take[..., None], torch.stack((1 - t_ab, t_ab, zero), -1), torch.stack((w0, w1, w2), -1))
    for d, w in ((d_bc, torch.stack((zero, 1 - t_bc, t_bc), -1)), (d_ca, torch.stack((1 - t_ca, zero, t_ca), -1))):
        take = d.detach() < d2.detach()
        d2 = torch.where(take, d, d2)
        bary = torch.where(take[..., None], w, bary)
    return d2, bary


POINT_MESH_CHUNK_PAIRS = 1 << 20      # pairs of one chunk of point_mesh_term's P x F matrix


def point_mesh_term(verts, faces, points, single_directional=False, point_reduction="mean", return_indices=False):
    """Point-to-mesh distance (PyTorch3D's point_mesh_face_distance for one mesh and one cloud; an extension here):
    verts [V,3], faces [F,3] integer, points [P,3], with d2(p, T) of point_triangle_closest,

        (1 / P) sum_i min_f d2(p_i, T_f) + (1 / F) sum_f min_i d2(p_i, T_f),

    point_reduction="sum" without the two divisors, single_directional the first sum alone.  The P x F matrix is evaluated in
    chunks of points and never exists whole; an exact tie keeps the LOWER index in both directions, and the chosen pairs are
    constants of the graph: the distances are evaluated once more on them, so verts and points get gradients.
    return_indices=True: (loss, face_idx [P], point_idx [F] | None), int64.  Differentiable torch on any device / dtype: the
    definition ops._PointMesh is tested against and the route for everything it does not take."""
    if point_reduction not in ("mean", "sum"):
        raise ValueError(f"point_mesh_term: point_reduction must be 'mean' or 'sum', got {point_reduction!r}")
    if verts.dim() != 2 or points.dim() != 2 or faces.dim() != 2 or verts.shape[1] != 3 or points.shape[1] != 3 or faces.shape[1] != 3 \
            or 0 in (verts.shape[0], faces.shape[0], points.shape[0]):
        raise ValueError(f"point_mesh_term: non-empty verts [V,3], faces [F,3] and points [P,3] expected, got {tuple(verts.shape)} / "
                         f"{tuple(faces.shape)} / {tuple(points.shape)}")
    points = points.to(verts.dtype)
    f = faces.long()
    P, F = points.shape[0], f.shape[0]
    vd, pd = verts.detach(), points.detach()
    a, b, c = vd[f[:, 0]], vd[f[:, 1]], vd[f[:, 2]]
    face_idx = torch.empty((P,), dtype=torch.long, device=verts.device)
    best_f = torch.full((F,), float("inf"), dtype=verts.dtype, device=verts.device)
    point_idx = torch.zeros((F,), dtype=torch.long, device=verts.device)
    ar_f = torch.arange(F, device=verts.device)
    chunk = max(1, POINT_MESH_CHUNK_PAIRS // F)
    for s in range(0, P, chunk):
        e = min(s + chunk, P)
        d = point_triangle_closest(pd[s:e, None], a[None], b[None], c[None])[0]      # [e - s, F]
        m = d.min(dim=1).values
        face_idx[s:e] = torch.where(d == m[:, None], ar_f[None, :], F).min(dim=1).values
        if not single_directional:
            m = d.min(dim=0).values
            first = torch.where(d == m[None, :], torch.arange(s, e, device=d.device)[:, None], P).min(dim=0).values
            better = m < best_f                                                     # (strictly: an earlier chunk keeps a tie)
            best_f = torch.where(better, m, best_f)
            point_idx = torch.where(better, first, point_idx)
    reduce = torch.mean if point_reduction == "mean" else torch.sum
    tri = f[face_idx]
    loss = reduce(point_triangle_closest(points, verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]])[0])
    if single_directional:
        return (loss, face_idx, None) if return_indices else loss
    loss = loss + reduce(point_triangle_closest(points[point_idx], verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]])[0])
    return (loss, face_idx, point_idx) if return_indices else loss


def camera_centres(R, T):
    """C [B,3] = -T @ R^-1 in the tensors' dtype (row vectors, X_view = X_world @ R + T): the point every pixel ray of a view leaves.
    On a device R^-1 is the closed form adj(R) / det(R) from elementwise operations: torch.linalg.inv reads its status word back on
    the host, a synchronisation that TSDFVolume.integrate promises not to make and that a stream capture refuses.  In fp64 the two
    agree to a few 2^-53, the same fp32 centre once rounded; a singular R raises on the host and gives a centre that is not finite
    on a device."""
    if R.is_cuda:
        return _camera_centres_closed_form(R, T)
    return -torch.einsum("bj,bjk->bk", T, torch.linalg.inv(R))


def _camera_centres_closed_form(R, T):
    """camera_centres from elementwise operations alone: column k of det(R) R^-1 is the cross product of the other two rows of R"""
    r0, r1, r2 = R[:, 0], R[:, 1], R[:, 2]
    adj = torch.stack((torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)), -1)      # [B,j,k] = det(R) R^-1
    det = (r0 * adj[:, :, 0]).sum(-1, keepdim=True)
    return -(T[:, :, None] * adj).sum(1) / det


def tsdf_integrate(tsdf, weight, depth, R, T, focal, pp, lo, voxel_size, trunc, max_weight=None, centre=None, mark=None, *, attr=None,
                   attr_image=None):
    """Fuse depth maps into a truncated signed distance volume (an extension here: the last step of the 2D Gaussian splatting
    pipeline, whose depth maps get_depth renders) -> (tsdf, weight), new tensors; not differentiable.

      tsdf, weight [nz,ny,nx]   the running average and its count; grid point (ix,iy,iz) sits at lo + (ix hx, iy hy, iz hz);
      depth [B,H,W]             what get_depth returns: the distance along the UNIT pixel ray from the camera centre (not view z);
      R [B,3,3], T [B,3], focal [B,2], pp [B,2]   the cameras of cameras.pixel_rays: X_view = X_world @ R + T, pixel (i,j) looks
                                along ((px - j - 0.5)/fx, (py - i - 0.5)/fy, 1); centre [B,3] = camera_centres(R, T) unless given.

    For the grid point x and the views b = 0 .. B-1 IN THAT ORDER, every operation a separate operation of the volume's dtype:
      1. p = x @ R_b + T_b, each component ((x0 R0k + x1 R1k) + x2 R2k) + Tk; the view is skipped unless p_z > 0;
      2. u = px - (fx p_x) / p_z, v = py - (fy p_y) / p_z, j = floor(u), i = floor(v); skipped unless 0 <= j < W and 0 <= i < H;
      3. d = depth[b,i,j], the nearest pixel, no interpolation; skipped unless d is finite and d > 0;
      4. sdf = d - sqrt((dx dx + dy dy) + dz dz) with dx = x - c_b; skipped if sdf < -trunc;
      5. t = min(1, sdf / trunc);
      6. tsdf <- (tsdf w + t) / (w + 1); and with attr [nz,ny,nx,C], the running attribute volume, and attr_image [B,H,W,C] (both or
         neither, channel last), for every channel, with the same w -- the weight before step 7 -- and the same nearest pixel:
         attr <- (attr w + attr_image[b,i,j]) / (w + 1), wherever the view updates the grid point and under no other condition;
      7. w <- w + 1, or min(w + 1, max_weight) when max_weight is given.
    attr is appended to the result, a new tensor.  tsdf and attr share ONE weight, which is why a volume takes an attribute in every
    call or in none.  The values of attr_image are not examined: a NaN pixel poisons the grid points that read it.
    The update is sequential in b: the same bits on every run, and one call with three views gives the bits of three calls with
    one view each.  mark = (delta, rho) appends a bool volume of the grid points whose decisions a lower precision may take the
    other way: in some view with p_z > 0, u or v within delta of an integer, or |sdf + trunc| or |sdf - trunc| within
    rho * |x - c_b| at a valid pixel.  torch on any device / dtype: the definition voge_tsdf_integrate is tested against and the
    route for everything it does not take."""
    if tsdf.dim() != 3 or weight.shape != tsdf.shape:
        raise ValueError(f"tsdf_integrate: tsdf and weight [nz,ny,nx] expected, got {tuple(tsdf.shape)} / {tuple(weight.shape)}")
    if depth.dim() != 3:
        raise ValueError(f"tsdf_integrate: depth [B,H,W] expected, got {tuple(depth.shape)}")
    B, H, W = depth.shape
    if R.shape != (B, 3, 3) or T.shape != (B, 3) or focal.shape != (B, 2) or pp.shape != (B, 2):
        raise ValueError(f"tsdf_integrate: {B} depth maps need R [{B},3,3], T [{B},3], focal [{B},2], pp [{B},2], got "
                         f"{tuple(R.shape)} / {tuple(T.shape)} / {tuple(focal.shape)} / {tuple(pp.shape)}")
    if not trunc > 0:
        raise ValueError(f"tsdf_integrate: trunc must be > 0, got {trunc}")
    dt, dev = tsdf.dtype, tsdf.device
    nz, ny, nx = tsdf.shape
    cast = lambda a: torch.as_tensor(a, device=dev).detach().to(dt)
    depth, R, T, focal, pp = cast(depth), cast(R), cast(T), cast(focal), cast(pp)
    centre = camera_centres(R, T) if centre is None else cast(centre)
    lo, hs = cast(lo).reshape(3), cast(voxel_size).reshape(-1).expand(3)
    trunc_t = cast(float(trunc))
    x0 = (lo[0] + torch.arange(nx, device=dev).to(dt) * hs[0]).view(1, 1, nx).expand(nz, ny, nx)
    x1 = (lo[1] + torch.arange(ny, device=dev).to(dt) * hs[1]).view(1, ny, 1).expand(nz, ny, nx)
    x2 = (lo[2] + torch.arange(nz, device=dev).to(dt) * hs[2]).view(nz, 1, 1).expand(nz, ny, nx)
    if (attr is None) != (attr_image is None):
        raise ValueError("tsdf_integrate: attr and attr_image go together")
    if attr is not None:
        if attr.dim() != 4 or attr.shape[:3] != tsdf.shape or attr_image.shape != (B, H, W, attr.shape[3]):
            raise ValueError(f"tsdf_integrate: attr [nz,ny,nx,C] and attr_image [{B},{H},{W},C] expected, got {tuple(attr.shape)} / "
                             f"{tuple(attr_image.shape)}")
        attr, attr_image = cast(attr).clone(), cast(attr_image)
    tsdf, w = tsdf.detach().clone(), weight.detach().clone()
    marked = torch.zeros(tsdf.shape, dtype=torch.bool, device=dev)
    one, zero = torch.ones((), dtype=dt, device=dev), torch.zeros((), dtype=dt, device=dev)
    for b in range(B):
        p = [((x0 * R[b, 0, k] + x1 * R[b, 1, k]) + x2 * R[b, 2, k]) + T[b, k] for k in range(3)]
        front = p[2] > 0
        pz = torch.where(front, p[2], one)
        u = pp[b, 0] - (focal[b, 0] * p[0]) / pz
        v = pp[b, 1] - (focal[b, 1] * p[1]) / pz
        inside = front & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        j = torch.where(inside, torch.floor(u), zero).long()
        i = torch.where(inside, torch.floor(v), zero).long()
        d = depth[b][i, j]
        valid = inside & torch.isfinite(d) & (d > 0)
        dx, dy, dz = x0 - centre[b, 0], x1 - centre[b, 1], x2 - centre[b, 2]
        dist = _ieee_sqrt((dx * dx + dy * dy) + dz * dz)
        sdf = torch.where(valid, d, zero) - dist
        upd = valid & ~(sdf < -trunc_t)
        t = torch.minimum(one, sdf / trunc_t)
        if attr is not None:
            attr = torch.where(upd[..., None], (attr * w[..., None] + attr_image[b][i, j]) / (w + 1)[..., None], attr)
        tsdf = torch.where(upd, (tsdf * w + t) / (w + 1), tsdf)
        w1 = w + 1
        if max_weight is not None:
            w1 = torch.minimum(w1, cast(float(max_weight)))
        w = torch.where(upd, w1, w)
        if mark is not None:
            delta, rho = mark
            near = lambda a: (a - torch.round(a)).abs() <= delta
            marked |= front & (near(u) | near(v))
            marked |= valid & (((sdf + trunc_t).abs() <= rho * dist) | ((sdf - trunc_t).abs() <= rho * dist))
    out = (tsdf, w) if mark is None else (tsdf, w, marked)
    return out if attr is None else out + (attr,)


def _mtet_tables():
    """Kuhn's split of the unit cell and the 16 cases of a tetrahedron (marching_tets' header): corners [6][4] cell corner masks
    (bit 0 = +x, bit 1 = +y, bit 2 = +z), positively oriented; count [16] triangles of a case (bit j of the case: local corner j
    inside); tri [6][16][2][3][2]: the edge of every triangle vertex as (low cell corner, direction mask d), -1 where there is none."""
    import itertools
    vec = lambda c: [(c >> k) & 1 for k in range(3)]
    det = lambda a, b, c: (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))
    corners = []
    for perm in itertools.permutations(range(3)):
        c1 = 1 << perm[0]
        c2 = c1 | (1 << perm[1])
        if det(vec(c1), vec(c2), vec(7)) < 0:
            c1, c2 = c2, c1
        corners.append([0, c1, c2, 7])
    even = {0: (0, 1, 2, 3), 1: (1, 0, 3, 2), 2: (2, 0, 1, 3), 3: (3, 0, 2, 1)}

    def odd(seq):
        return sum(1 for m in range(4) for n in range(m + 1, 4) if seq[m] > seq[n]) % 2 == 1

    local = []      # per case: triangles of local edges (m, n)
    for case in range(16):
        ins = [j for j in range(4) if (case >> j) & 1]
        out = [j for j in range(4) if not (case >> j) & 1]
        if len(ins) == 1:
            a, b, c, d = even[ins[0]]
            tris = [((a, b), (a, c), (a, d))]
        elif len(ins) == 3:
            a, b, c, d = even[out[0]]
            tris = [((a, b), (a, d), (a, c))]
        elif len(ins) == 2:
            (a, b), (c, d) = ins, out
            if odd((a, b, c, d)):
                c, d = d, c
            q = ((a, c), (a, d), (b, d), (b, c))
            tris = [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
        else:
            tris = []
        local.append(tris)
    count = [len(t) for t in local]
    tri = [[[[[-1, -1] for _ in range(3)] for _ in range(2)] for _ in range(16)] for _ in range(6)]
    for tet in range(6):
        for case in range(16):
            for k, t in enumerate(local[case]):
                for r, (m, n) in enumerate(t):
                    ca, cb = corners[tet][m], corners[tet][n]
                    tri[tet][case][k][r] = [min(ca, cb), ca ^ cb]      # (one corner's bits contain the other's: the edge's direction)
    return corners, count, tri


_MTET = {}


def marching_tets(values, weight=None, level=0.0, lo=(0.0, 0.0, 0.0), voxel_size=1.0, *, attr=None):
    """The level set of a scalar field on a regular grid as a triangle mesh: marching tetrahedra on Kuhn's six-tetrahedron
    split of every cell (an extension here) -> (verts [V,3] in the field's dtype, faces [F,3] int64); not differentiable.
    values [nz,ny,nx] (every dimension >= 2, nx ny nz 7 < 2^31), weight of the same shape or None; grid point (ix,iy,iz) sits at
    lo + (ix hx, iy hy, iz hz) and has the linear index (iz ny + iy) nx + ix.

      observed  isfinite(value), and weight > 0 when a weight is given.  inside <=> value < level, strictly;
      tetrahedra  cell corners are bit masks (bit 0 = +x, bit 1 = +y, bit 2 = +z); one tetrahedron per permutation pi of the axes, in
                the order of itertools.permutations(range(3)): c0 = 0, c1 = bit(pi_1), c2 = c1 | bit(pi_2), c3 = 7, c1 and c2 swapped
                when det[c1 - c0, c2 - c0, c3 - c0] < 0; emitted only when its four corners are observed;
      vertices  a grid point owns the edges of directions d = 1 .. 7 (bit masks: three axes, three face diagonals, the body
                diagonal) that stay inside the grid; an edge carries a vertex iff both ends are observed and exactly one is inside:
                p_a + t (p_b - p_a), t = (level - v_a) / (v_b - v_a), a the owner (the end of the lower linear index), every
                operation a separate one and p = lo + i h; ordered by ascending (linear index of the owner, d);
      faces     ordered by ascending (cell, tetrahedron, triangle), the cell by the linear index of its low corner.  With the local
                corners 0 .. 3 of a tetrahedron and `mn` the vertex on the edge between m and n:
                one inside, a: (a,b,c,d) the even permutation {0: 0123, 1: 1032, 2: 2013, 3: 3021}[a], the triangle (ab, ac, ad);
                three inside, a outside: (ab, ad, ac);
                two inside, a < b, and c < d outside, c and d swapped when (a,b,c,d) is odd: the quad (ac, ad, bd, bc) as
                (q0,q1,q2), (q0,q2,q3).
    The geometric normal of every face points from inside to outside.  Kuhn's split is invariant under translation, so the cells
    agree on their shared faces: on a fully observed grid whose border is outside the mesh is closed and every vertex is used; a
    value exactly at the level gives coincident vertices and faces of no area; next to unobserved points the mesh has a boundary
    and a vertex there may belong to no face.  attr [nz,ny,nx,C] (channel last: a colour, or anything else a grid point carries)
    appends vert_attr [V,C] in the field's dtype: for the vertex on the edge (a, b), with its own t, attr_a + t (attr_b - attr_a), every
    operation a separate one; both ends of such an edge are observed by construction.  Vectorised torch on any device / dtype: the
    definition voge_mtet_* are tested against and the route for everything they do not take."""
    v = values.detach()
    if v.dim() != 3 or min(v.shape) < 2:
        raise ValueError(f"marching_tets: values [nz,ny,nx] with every dimension >= 2 expected, got {tuple(v.shape)}")
    nz, ny, nx = v.shape
    n = nx * ny * nz
    if n * 7 >= 2 ** 31:
        raise ValueError(f"marching_tets: nx ny nz 7 = {n * 7} does not fit 32-bit indices")
    if weight is not None and weight.shape != v.shape:
        raise ValueError(f"marching_tets: weight {tuple(weight.shape)} does not match values {tuple(v.shape)}")
    if attr is not None and (attr.dim() != 4 or attr.shape[:3] != v.shape):
        raise ValueError(f"marching_tets: attr {tuple(attr.shape)} does not match values {tuple(v.shape)}")
    dt, dev = v.dtype, v.device
    if not _MTET:
        _MTET["t"] = _mtet_tables()
    corners, count, tri = _MTET["t"]
    obs = torch.isfinite(v)
    if weight is not None:
        obs = obs & (weight.detach() > 0)
    ins = v < level
    off = lambda c: (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
    sl = lambda a, c, m: a[((c >> 2) & 1):nz - m + ((c >> 2) & 1), ((c >> 1) & 1):ny - m + ((c >> 1) & 1), (c & 1):nx - m + (c & 1)]
    # the edges that carry a vertex, as a table over the keys 7 q + (d - 1)
    has = torch.zeros((nz, ny, nx, 7), dtype=torch.bool, device=dev)
    for d in range(1, 8):
        bx, by, bz = d & 1, (d >> 1) & 1, (d >> 2) & 1
        a = (slice(0, nz - bz), slice(0, ny - by), slice(0, nx - bx))
        b = (slice(bz, nz), slice(by, ny), slice(bx, nx))
        has[a + (d - 1,)] = obs[a] & obs[b] & (ins[a] != ins[b])
    has = has.reshape(-1)
    vid = torch.cumsum(has, 0) - 1
    keys = torch.nonzero(has)[:, 0]
    q, d = torch.div(keys, 7, rounding_mode="floor"), keys % 7 + 1
    bits = torch.stack((d & 1, (d >> 1) & 1, (d >> 2) & 1), -1)
    ia = torch.stack((q % nx, torch.div(q, nx, rounding_mode="floor") % ny, torch.div(q, nx * ny, rounding_mode="floor")), -1)
    flat = v.reshape(-1)
    va, vb = flat[q], flat[q + bits[:, 0] + bits[:, 1] * nx + bits[:, 2] * (nx * ny)]
    lo_t = torch.as_tensor(lo, device=dev).to(dt).reshape(3)
    hs = torch.as_tensor(voxel_size, device=dev).to(dt).reshape(-1).expand(3)
    t = (torch.as_tensor(level, device=dev).to(dt) - va) / (vb - va)
    pa, pb = lo_t + ia.to(dt) * hs, lo_t + (ia + bits).to(dt) * hs
    verts = pa + t[:, None] * (pb - pa)
    if attr is not None:
        rows = attr.detach().to(device=dev, dtype=dt).reshape(n, -1)
        aa, ab = rows[q], rows[q + bits[:, 0] + bits[:, 1] * nx + bits[:, 2] * (nx * ny)]
        vert_attr = aa + t[:, None] * (ab - aa)
    # the faces: every cell, six tetrahedra, up to two triangles
    lin = torch.arange(n, device=dev).view(nz, ny, nx)[:-1, :-1, :-1].reshape(-1)
    cins = [sl(ins, c, 1).reshape(-1) for c in range(8)]
    cobs = [sl(obs, c, 1).reshape(-1) for c in range(8)]
    count_t = torch.tensor(count, device=dev)
    tri_t = torch.tensor(tri, device=dev)      # [6,16,2,3,2]
    slot = torch.arange(2, device=dev)
    all_faces, all_keep = [], []
    for tet in range(6):
        cs = corners[tet]
        case = sum(cins[cs[j]].long() << j for j in range(4))
        whole = cobs[cs[0]] & cobs[cs[1]] & cobs[cs[2]] & cobs[cs[3]]
        keep = whole[:, None] & (slot[None, :] < count_t[case][:, None])      # [cells,2]
        e = tri_t[tet][case]      # [cells,2,3,2]
        cm, dd = e[..., 0].clamp(min=0), e[..., 1].clamp(min=1)
        key = (lin[:, None, None] + off(cm)) * 7 + (dd - 1)
        all_faces.append(vid[key])
        all_keep.append(keep)
    faces = torch.stack(all_faces, 1)[torch.stack(all_keep, 1)]      # [cells,6,2,3] under [cells,6,2]: the order of the faces
    faces = faces.reshape(-1, 3)
    return (verts, faces) if attr is None else (verts, faces, vert_attr)


def mesh_components(faces, num_verts):
    """Connected components of a triangle mesh (an extension here) -> (vert_label [V] int64, face_label [F] int64,
    num_components: int).  Two vertices are connected when a chain of faces links them, each face joining its three vertices; a
    component's label is its SMALLEST VERTEX INDEX; a vertex no face names keeps its own index and is no component;
    face_label[f] = vert_label[faces[f, 0]].  Min-label propagation to a fixed point: label[faces].amin(1) scattered with amin to
    the three vertices and to their present labels, then label = label[label] until flat, until nothing changes -- every label
    stays a vertex of the same component that is not above its owner, and at the fixed point a face's vertices agree, so a
    component carries one label, an index of its own not above any of them: its smallest.  An index outside [0, V) raises
    ValueError; a face may name a vertex twice.  Torch on any device, with one comparison read back per round: the definition
    voge_mesh_components is tested against and the route for everything it does not take."""
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"mesh_components: faces [F,3] expected, got {tuple(faces.shape)}")
    V, F = int(num_verts), faces.shape[0]
    f = faces.detach().long()
    if V < 0 or (F > 0 and (V == 0 or int(f.min()) < 0 or int(f.max()) >= V)):
        raise ValueError(f"mesh_components: a face names a vertex outside [0, {V})")
    label = torch.arange(V, dtype=torch.int64, device=f.device)
    corners = f.reshape(-1)
    while F > 0:
        low = label[f].amin(1).repeat_interleave(3)
        new = label.scatter_reduce(0, corners, low, "amin", include_self=True)
        # the corners' present labels take it too (a label is a vertex of the same component, not below the minimum): whole
        # trees hang under one another, and a long strip with shuffled indices takes tens of rounds, not tens of thousands
        new = new.scatter_reduce(0, label[corners], low, "amin", include_self=True)
        while True:
            nxt = new[new]
            if torch.equal(nxt, new):
                break
            new = nxt
        if torch.equal(new, label):
            break
        label = new
    face_label = label[f[:, 0]]
    return label, face_label, int(torch.unique(face_label).numel())


def mesh_keep_roots(count, keep_largest=None, min_faces=1):
    """keep [V] bool: the labels of the components that stay, from count [V] (the faces of a component at its label, 0 elsewhere):
    at least min_faces faces, and among the keep_largest first when the components are ranked by face count descending, then by
    label ascending (None: all).  The rank is a topk over the int64 key (count << 32) | (2^32 - 1 - label), -1 for what min_faces
    drops.  Torch on the counts' device, nothing read back."""
    V = count.shape[0]
    c = count.long()
    keep = c >= max(int(min_faces), 1)
    if keep_largest is None or V == 0:
        return keep
    idx = torch.arange(V, dtype=torch.int64, device=c.device)
    key = torch.where(keep, (c << 32) | (0xffffffff - idx), torch.full_like(c, -1))
    top_val, top_idx = torch.topk(key, min(int(keep_largest), V))
    return torch.zeros_like(keep).scatter_(0, top_idx, top_val >= 0)


def mesh_clean(verts, faces, keep_largest=None, min_faces=1):
    """The mesh without its small components (an extension here: the filter the 2D Gaussian splatting pipeline runs on an extracted
    mesh) -> (verts' [V',3], faces' [F',3] int64, vert_index [V'] int64, face_index [F'] int64).  A component (mesh_components)
    stays when mesh_keep_roots says so; kept faces keep their order and are renumbered; vertices no kept face names are dropped,
    the others keep their order and their bits; the index tables give the old indices.  keep_largest or min_faces below 1 raise
    ValueError.  Torch on any device: the definition voge_mesh_clean_* are tested against and the route for everything they do
    not take."""
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"mesh_clean: verts [V,3] and faces [F,3] expected, got {tuple(verts.shape)} / {tuple(faces.shape)}")
    if (keep_largest is not None and int(keep_largest) < 1) or int(min_faces) < 1:
        raise ValueError(f"mesh_clean: keep_largest (None or >= 1) and min_faces >= 1 expected, got {keep_largest} / {min_faces}")
    V = verts.shape[0]
    f = faces.detach().long()
    _, face_label, _ = mesh_components(f, V)
    keep = mesh_keep_roots(torch.bincount(face_label, minlength=V), keep_largest, min_faces)
    face_index = torch.nonzero(keep[face_label])[:, 0]
    kept = f[face_index]
    used = torch.zeros((V,), dtype=torch.bool, device=f.device)
    used[kept.reshape(-1)] = True
    vert_index = torch.nonzero(used)[:, 0]
    new_id = torch.cumsum(used, 0) - 1
    return verts[vert_index], new_id[kept], vert_index, face_index


def mesh_vertex_normals(verts, faces):
    """Area-weighted vertex normals [V,3] in the vertices' dtype (PyTorch3D's verts_normals_packed; an extension here): the
    normalised sum, over the corners that name a vertex, of cr = (b - a) x (c - a) of the corner's face -- a face that names a
    vertex twice counts twice there.  cr is _face_cross of the rounded differences in the vertices' dtype (for fp32 the bits of
    voge_mesh_sample_fwd's and voge_vertex_normals'); the sum, its norm sqrt((x^2 + y^2) + z^2) and the quotient are fp64, rounded
    once.  (0, 0, 0) where the sum is zero or not finite, and for a vertex no face names.  Differentiable torch on any device: the
    definition voge_vertex_normals is tested against and the route for everything it does not take."""
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"mesh_vertex_normals: verts [V,3] and faces [F,3] expected, got {tuple(verts.shape)} / {tuple(faces.shape)}")
    f = faces.detach().long()
    a = verts[f[:, 0]]
    cr = _face_cross(verts[f[:, 1]] - a, verts[f[:, 2]] - a)
    acc = torch.zeros((verts.shape[0], 3), dtype=torch.float64, device=verts.device).index_add(0, f.reshape(-1), cr.double().repeat_interleave(3, 0))
    ok = torch.isfinite(acc.detach()).all(-1, keepdim=True) & (acc.detach() != 0).any(-1, keepdim=True)
    acc = torch.where(ok, acc, torch.ones_like(acc))
    n = torch.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])[:, None]
    return torch.where(ok, acc / n, torch.zeros_like(acc)).to(verts.dtype)


MESH_SIMPLIFY_MAX_CELLS = 2 ** 21 - 1      # cells on an axis: three cell indices share one 63-bit key
MESH_SIMPLIFY_LAMBDA = 1e-3                # the quadric placement's pull towards the cluster mean


def _det3(m00, m01, m02, m10, m11, m12, m20, m21, m22):
    return (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20)


def mesh_simplify(verts, faces, cell_size, placement="mean", attr=None):
    """Vertex clustering on a uniform grid with mean or quadric placement (an extension here: the decimation step between
    extracting a mesh and using it; Rossignac-Borrel cells, Lindstrom's placement) -> (verts' [V',3] fp32, faces' [F',3] int64,
    attr' [V',C] fp32 or None, vert_index [V] int64, face_index [F'] int64).  Integers are int64, positions fp64 computed from the
    fp32 vertices.  THE RULE, in five steps:

      1 cells     lo = the per-axis minimum of verts in fp32; cell(v) = floor((v - lo) / h) per axis as three separate IEEE fp32
                  operations (h = cell_size as fp32 numbers).  Every vertex takes part, whether a face names it or not.  More than
                  2^21 - 1 cells on an axis, a vertex that is not finite and a face index outside [0, V) raise ValueError.
      2 clusters  the vertices of one cell are one cluster; its label is its smallest vertex index (mesh_components' convention).
      3 faces     a face's corners are replaced by their labels; the face is dropped when two labels are equal; the triple is
                  rotated so that its smallest label comes first (the orientation stays) to name it; among the faces with the
                  same rotated triple the one with the smallest face index stays, in its own corner order (two faces of opposite orientation are different triples and
                  both stay).  Surviving faces keep their order.
      4 outputs   the output vertices are the clusters a surviving face names, in ascending order of their labels.  vert_index[v]
                  is the output row of the cluster of v, -1 where that cluster was dropped; face_index holds the input indices of
                  the surviving faces.
      5 values    a cluster of one vertex keeps that vertex's bits (and its attribute row's) under both placements.  Otherwise
                  attr' is the mean of the cluster's attribute rows (NaN where one of them is not finite), and the position is
                  "mean"     the mean of the cluster's vertices;
                  "quadric"  in cell coordinates x = (p - c) / h per axis, c = lo + (cell + 1/2) h the cell's centre: every input
                             face -- those that collapse too -- adds at each of its three corners, to that corner's cluster, the
                             plane quadric of its unit normal n through that corner: n n^T to A, n d to b with d = -n . x_corner.
                             n is e1 x e2 normalised with e1 = (b - a) / h, e2 = (c - a) / h per axis (cell coordinates as well:
                             for a scalar cell_size the face's own unit normal); a face whose cross product is zero or not
                             finite adds nothing.  With m contributions and mu the cluster's mean in the same coordinates,
                             (A + lambda m I) x = -b + lambda m mu, lambda = 1e-3 (it bounds the condition number by
                             (1 + lambda) / lambda and pulls the directions the planes leave free to the mean), by Cramer's rule;
                             x is clamped to [-1/2, 1/2]^3 and the result is c + x h, rounded once to fp32.  m = 0: the mean.
    A corner of a cell lies inside it, so every entry of a term is bounded by about 1: what lets the kernels add them in fixed point.
    Vertex clustering does not promise a manifold result (two sheets closer than a cell merge) and has no target face count.  Not
    differentiable.  Torch on any device: the definition voge_mesh_simplify_* are tested against and the route for everything
    they do not take."""
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"mesh_simplify: verts [V,3] and faces [F,3] expected, got {tuple(verts.shape)} / {tuple(faces.shape)}")
    if placement not in ("mean", "quadric"):
        raise ValueError(f"mesh_simplify: placement 'mean' or 'quadric' expected, got {placement!r}")
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    if attr is not None and (attr.dim() != 2 or attr.shape[0] != V):
        raise ValueError(f"mesh_simplify: attr [{V},C] expected, got {tuple(attr.shape)}")
    h32 = torch.as_tensor(cell_size, dtype=torch.float32, device="cpu").reshape(-1)
    if h32.numel() == 1:
        h32 = h32.expand(3)
    if h32.numel() != 3 or not bool((torch.isfinite(h32) & (h32 > 0)).all()):
        raise ValueError(f"mesh_simplify: cell_size must be one or three positive finite numbers, got {cell_size}")
    h32 = h32.to(dev)
    v32 = verts.detach().to(torch.float32)
    f = faces.detach().long().to(dev)
    if not bool(torch.isfinite(v32).all()):
        raise ValueError("mesh_simplify: a vertex is not finite")
    if F > 0 and (V == 0 or int(f.min()) < 0 or int(f.max()) >= V):
        raise ValueError(f"mesh_simplify: a face names a vertex outside [0, {V})")
    C = 0 if attr is None else attr.shape[1]
    a32 = None if attr is None else attr.detach().to(device=dev, dtype=torch.float32)
    idx = lambda n: torch.arange(n, dtype=torch.int64, device=dev)
    none = (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev),
            None if attr is None else torch.zeros((0, C), dtype=torch.float32, device=dev),
            torch.full((V,), -1, dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.int64, device=dev))
    if V == 0:
        return none
    # 1 cells
    lo32 = v32.amin(0)
    cellf = torch.floor((v32 - lo32) / h32)
    if not bool((cellf <= MESH_SIMPLIFY_MAX_CELLS - 1).all()):
        raise ValueError(f"mesh_simplify: more than {MESH_SIMPLIFY_MAX_CELLS} cells on an axis")
    cell = cellf.long()
    # 2 clusters
    _, inv = torch.unique((cell[:, 2] << 42) | (cell[:, 1] << 21) | cell[:, 0], return_inverse=True)
    first = torch.full((int(inv.max()) + 1,), V, dtype=torch.int64, device=dev).scatter_reduce(0, inv, idx(V), "amin")
    label = first[inv]
    if F == 0:
        return none
    # 3 faces
    lab = label[f]
    dropped = (lab[:, 0] == lab[:, 1]) | (lab[:, 1] == lab[:, 2]) | (lab[:, 2] == lab[:, 0])
    turn = (lab.argmin(1)[:, None] + idx(3)[None]) % 3
    tri = torch.gather(lab, 1, turn)
    cand = torch.nonzero(~dropped)[:, 0]
    keep = torch.zeros((F,), dtype=torch.bool, device=dev)
    if cand.numel():
        _, tinv = torch.unique(tri[cand], dim=0, return_inverse=True)
        tfirst = torch.full((int(tinv.max()) + 1,), F, dtype=torch.int64, device=dev).scatter_reduce(0, tinv, cand, "amin")
        keep[cand] = tfirst[tinv] == cand
    face_index = torch.nonzero(keep)[:, 0]
    if face_index.numel() == 0:
        return none
    # 4 outputs
    used = torch.zeros((V,), dtype=torch.bool, device=dev)
    used[tri[face_index].reshape(-1)] = True
    out_label = torch.nonzero(used)[:, 0]
    row_of = torch.where(used, torch.cumsum(used, 0) - 1, torch.full((V,), -1, dtype=torch.int64, device=dev))
    vert_index = row_of[label]
    new_faces = row_of[lab[face_index]]      # (in the face's own corner order: the rotation only names the triple)
    # 5 values
    Vk = out_label.numel()
    member = vert_index >= 0
    rows = vert_index[member]
    count = torch.bincount(rows, minlength=Vk)
    single = count == 1
    p = v32.double()
    mean = torch.zeros((Vk, 3), dtype=torch.float64, device=dev).index_add(0, rows, p[member]) / count[:, None]
    if placement == "quadric":
        h, lo = h32.double(), lo32.double()
        centre = lo + (cell[out_label].double() + 0.5) * h
        mu = torch.zeros((Vk, 3), dtype=torch.float64, device=dev).index_add(0, rows, (p[member] - centre[rows]) / h) / count[:, None]
        pa, pb, pc = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        e1, e2 = (pb - pa) / h, (pc - pa) / h
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        norm = torch.sqrt((cx * cx + cy * cy) + cz * cz)
        good = torch.isfinite(norm) & (norm > 0)
        n = torch.stack([cx, cy, cz], -1)[good] / norm[good][:, None]
        fg = f[good]
        A = torch.zeros((Vk, 6), dtype=torch.float64, device=dev)
        b = torch.zeros((Vk, 3), dtype=torch.float64, device=dev)
        m = torch.zeros((Vk,), dtype=torch.float64, device=dev)
        for k in range(3):
            r = vert_index[fg[:, k]]
            on = r >= 0
            r, nk = r[on], n[on]
            x = (p[fg[:, k]][on] - centre[r]) / h
            d = -((nk[:, 0] * x[:, 0] + nk[:, 1] * x[:, 1]) + nk[:, 2] * x[:, 2])
            A.index_add_(0, r, torch.stack([nk[:, 0] * nk[:, 0], nk[:, 0] * nk[:, 1], nk[:, 0] * nk[:, 2], nk[:, 1] * nk[:, 1],
                                            nk[:, 1] * nk[:, 2], nk[:, 2] * nk[:, 2]], -1))
            b.index_add_(0, r, nk * d[:, None])
            m.index_add_(0, r, torch.ones_like(d))
        lm = MESH_SIMPLIFY_LAMBDA * m
        solve = m > 0
        lm1 = torch.where(solve, lm, torch.ones_like(lm))      # (the rows without a contribution: any regular system)
        a00, a01, a02, a11, a12, a22 = A[:, 0] + lm1, A[:, 1], A[:, 2], A[:, 3] + lm1, A[:, 4], A[:, 5] + lm1
        r0, r1, r2 = (lm[:, None] * mu - b).unbind(-1)
        det = _det3(a00, a01, a02, a01, a11, a12, a02, a12, a22)
        x = torch.stack([_det3(r0, a01, a02, r1, a11, a12, r2, a12, a22) / det, _det3(a00, r0, a02, a01, r1, a12, a02, r2, a22) / det,
                         _det3(a00, a01, r0, a01, a11, r1, a02, a12, r2) / det], -1)
        x = torch.minimum(torch.maximum(x, torch.full_like(x, -0.5)), torch.full_like(x, 0.5))
        pos = torch.where(solve[:, None], centre + x * h, mean)
    else:
        pos = mean
    new_verts = torch.where(single[:, None], v32[out_label], pos.to(torch.float32))
    new_attr = None
    if attr is not None:
        am = torch.zeros((Vk, C), dtype=torch.float64, device=dev).index_add(0, rows, a32.double()[member]) / count[:, None]
        am = torch.where(torch.isfinite(am), am, torch.full_like(am, float("nan")))      # (a value that is not finite: NaN)
        new_attr = torch.where(single[:, None], a32[out_label], am.to(torch.float32))
    return new_verts, new_faces, new_attr, vert_index, face_index


MESH_RASTER_CHUNK_PAIRS = 1 << 21      # (pixel, face) pairs of one chunk of mesh_rasterize's walk over the faces


def _view_space(verts, R, T):
    """p [B,V,3] = verts @ R_b + T_b, each component ((x0 R0k + x1 R1k) + x2 R2k) + Tk: step 1 of tsdf_integrate"""
    x0, x1, x2 = verts[None, :, 0, None], verts[None, :, 1, None], verts[None, :, 2, None]
    return ((x0 * R[:, None, 0, :] + x1 * R[:, None, 1, :]) + x2 * R[:, None, 2, :]) + T[:, None, :]


def _pixel_dirs(focal, pp, H, W):
    """(d0 [B,W], d1 [B,H]): pixel (i, j) looks along ((px - (j + 0.5)) / fx, (py - (i + 0.5)) / fy, 1)"""
    dt, dev = focal.dtype, focal.device
    cj = torch.arange(W, device=dev).to(dt) + 0.5
    ci = torch.arange(H, device=dev).to(dt) + 0.5
    return (pp[:, 0:1] - cj[None, :]) / focal[:, 0:1], (pp[:, 1:2] - ci[None, :]) / focal[:, 1:2]


def _edge_values(d0, d1, n):
    """w = (d0 n_0 + d1 n_1) + n_2 of rays d0, d1 against records n [..., 3] (broadcast)"""
    return (d0 * n[..., 0] + d1 * n[..., 1]) + n[..., 2]


def mesh_rasterize(verts, faces, R, T, focal, pp, H, W, cull_backfaces=False, mark=None):
    """The nearest face of a mesh under every pixel (an extension: PyTorch3D's rasterize_meshes with one face a pixel and an exact
    ray-triangle test) -> (pix_to_face [B,H,W] int64, -1 where nothing is hit; bary [B,H,W,3] and depth [B,H,W] in the vertices'
    dtype, zeros where nothing is hit).

      verts [V,3], faces [F,3] integer                the mesh, one for all views;
      R [B,3,3], T [B,3], focal [B,2], pp [B,2]       the cameras of cameras.pixel_rays and of tsdf_integrate.

    depth is get_depth's: the distance along the UNIT pixel ray from the camera centre, not view z.  Every operation below is a
    separate operation of the vertices' dtype, in this order:
      1. view space: p = x @ R_b + T_b, each component ((x0 R0k + x1 R1k) + x2 R2k) + Tk (step 1 of tsdf_integrate);
      2. pixel ray: pixel (i, j) looks along d = ((px - (j + 0.5)) / fx, (py - (i + 0.5)) / fy, 1) -- the centre of the pixel that
         tsdf_integrate's floor(u), floor(v) names, so a grid point on the rasterised surface reads its own pixel;
      3. face records: for the corners a, b, c in view space n_a = b x c, n_b = c x a, n_c = a x b, each component (p q) - (r s);
      4. edge values: w_i = (d0 n_i0 + d1 n_i1) + n_i2, det = (w_a + w_b) + w_c.  a x b and b x a are exact negatives in IEEE
         arithmetic, so two faces that share an edge get exactly opposite w on it: a ray on a shared edge is inside both faces,
         and a closed mesh has no cracks;
      5. hit test: hit <=> (w_a, w_b, w_c >= 0 and det > 0) or (w_a, w_b, w_c <= 0 and det < 0); with cull_backfaces only the
         second arm, the front of a face whose normal (b - a) x (c - a) points at the camera for det R > 0.  bary_i = w_i / det,
         z = (bary_a a_z + bary_b b_z) + bary_c c_z, and a hit needs z > 0.  A ray-triangle test in 3-D: a face that crosses the
         camera plane needs no clipping; a face with a NaN corner hits nothing, every comparison being written positively;
         infinite coordinates are out of contract;
      6. winner: the lexicographically smallest (z, face index) -- an exact tie keeps the lower index;
         depth = z * sqrt((d0 d0 + d1 d1) + 1), IEEE square root and division;
      7. marks: mark = (c, rho) appends a bool [B,H,W] of the pixels whose decision a lower precision may take the other way: some
         face with z > 0 has its smallest bary within c 2^-23 M |d| / |det| of zero, M the largest squared corner norm of the face
         in view space; or the second-nearest hit lies within rho z of the nearest.
    The faces are walked in chunks of MESH_RASTER_CHUNK_PAIRS / (B H W), so memory stays bounded; the choice is made without
    autograd, bary and depth are then evaluated at the chosen face with it: differentiable to verts (and the cameras) through
    depth and bary.  torch on any device / dtype: the definition csrc/mesh_raster.hip is tested against and the route for
    everything it does not take."""
    if verts.dim() != 2 or verts.shape[1] != 3 or not verts.dtype.is_floating_point:
        raise ValueError(f"mesh_rasterize: verts [V,3] of floats expected, got {tuple(verts.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
        raise ValueError(f"mesh_rasterize: faces [F,3] of integers expected, got {tuple(faces.shape)}")
    B, H, W = R.shape[0], int(H), int(W)
    if R.shape != (B, 3, 3) or T.shape != (B, 3) or focal.shape != (B, 2) or pp.shape != (B, 2):
        raise ValueError(f"mesh_rasterize: R [B,3,3], T [B,3], focal [B,2], pp [B,2] expected, got {tuple(R.shape)} / {tuple(T.shape)} / "
                         f"{tuple(focal.shape)} / {tuple(pp.shape)}")
    if H < 1 or W < 1:
        raise ValueError(f"mesh_rasterize: image_size (H, W) >= 1 expected, got ({H}, {W})")
    dt, dev = verts.dtype, verts.device
    V, F = verts.shape[0], faces.shape[0]
    faces = faces.to(dev).long()
    if F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise ValueError(f"mesh_rasterize: a face names a vertex outside [0, {V})")
    R, T, focal, pp = (torch.as_tensor(t, device=dev).to(dt) for t in (R, T, focal, pp))
    p = _view_space(verts, R, T)                                                           # step 1 [B,V,3]
    d0, d1 = _pixel_dirs(focal, pp, H, W)                                                  # step 2
    dn = _ieee_sqrt((d0 * d0)[:, None, :] + (d1 * d1)[:, :, None] + 1)                      # |d| [B,H,W]
    best_z = torch.full((B, H, W), float("inf"), dtype=dt, device=dev)
    second_z = best_z.clone()
    best_f = torch.full((B, H, W), -1, dtype=torch.long, device=dev)
    marked = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    chunk = max(1, MESH_RASTER_CHUNK_PAIRS // max(1, B * H * W))
    with torch.no_grad():
        pd = p.detach()
        D0, D1 = d0[:, None, None, :].detach(), d1[:, None, :, None].detach()
        for f0 in range(0, F if B else 0, chunk):
            f = faces[f0:f0 + chunk]
            a, b, c = pd[:, f[:, 0]], pd[:, f[:, 1]], pd[:, f[:, 2]]                       # [B,Fc,3]
            w = [_edge_values(D0, D1, n[:, :, None, None, :]) for n in (_face_cross(b, c), _face_cross(c, a), _face_cross(a, b))]      # steps 3, 4
            det = (w[0] + w[1]) + w[2]
            back = (w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0) & (det < 0)
            hit = back if cull_backfaces else (back | ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (det > 0)))
            bary = [x / det for x in w]
            z = (bary[0] * a[:, :, None, None, 2] + bary[1] * b[:, :, None, None, 2]) + bary[2] * c[:, :, None, None, 2]
            hit = hit & (z > 0)                                                            # step 5
            zh = torch.where(hit, z, torch.full_like(z, float("inf")))
            z1 = zh.min(1).values
            ids = torch.arange(f0, f0 + f.shape[0], device=dev).view(1, -1, 1, 1)
            first = torch.where(hit & (zh == z1[:, None]), ids, torch.full_like(ids, F)).min(1).values      # the lowest index at z1, F: no hit
            z2 = torch.where(ids == first[:, None], torch.full_like(zh, float("inf")), zh).min(1).values
            take = (first < F) & ((best_f < 0) | (z1 < best_z))                            # step 6 (the chunks ascend: a tie keeps the earlier)
            second_z = torch.minimum(torch.maximum(best_z, z1), torch.minimum(second_z, z2))
            best_z = torch.where(take, z1, best_z)
            best_f = torch.where(take, first, best_f)
            if mark is not None:
                M = torch.stack(((a * a).sum(-1), (b * b).sum(-1), (c * c).sum(-1)), 0).max(0).values[:, :, None, None]
                low = torch.minimum(torch.minimum(bary[0], bary[1]), bary[2]).abs()
                marked |= ((z > 0) & (low <= (mark[0] * 2.0 ** -23) * M * dn[:, None] / det.abs())).any(1)
        if mark is not None:
            marked |= (best_f >= 0) & (second_z - best_z <= mark[1] * best_z)
    # bary and depth at the chosen face, with the operations of steps 3 - 6 (and with autograd)
    covered = best_f >= 0
    tri = faces[best_f.clamp(min=0)] if F else torch.zeros((B, H, W, 3), dtype=torch.long, device=dev)
    view = torch.arange(B, device=dev).view(B, 1, 1)
    if V:
        a, b, c = p[view, tri[..., 0]], p[view, tri[..., 1]], p[view, tri[..., 2]]         # [B,H,W,3]
    else:
        a = b = c = torch.zeros((B, H, W, 3), dtype=dt, device=dev)
    D0, D1 = d0[:, None, :], d1[:, :, None]
    w = [_edge_values(D0, D1, n) for n in (_face_cross(b, c), _face_cross(c, a), _face_cross(a, b))]
    det = (w[0] + w[1]) + w[2]
    det = torch.where(covered, det, torch.ones_like(det))
    bary = [x / det for x in w]
    z = (bary[0] * a[..., 2] + bary[1] * b[..., 2]) + bary[2] * c[..., 2]
    zero = torch.zeros((), dtype=dt, device=dev)
    depth = torch.where(covered, z * dn, zero)
    bary = torch.where(covered[..., None], torch.stack(bary, -1), zero)
    out = (best_f, bary, depth)
    return out if mark is None else out + (marked,)
