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
