"""Gaussian parameter containers with the interface of VoGE/Meshes.py:5-57: calling one
returns (verts, sigmas, radians).  The Oriented* classes (no reference counterpart) return
(verts, scales, quats) and carry `oriented = True`."""
import torch
import torch.nn as nn


class GaussianMeshesNaive:
    """Plain references to tensors (Meshes.py:5-27)."""

    def __init__(self, verts, sigmas, radians=None):
        self.verts, self.sigmas, self.radians = verts, sigmas, radians

    def to(self, device):
        self.verts = self.verts.to(device)
        self.sigmas = self.sigmas.to(device)
        if self.radians is not None:
            self.radians = self.radians.to(device)
        return self

    def __call__(self):
        return self.verts, self.sigmas, self.radians

    def __getitem__(self, item):
        rad = None if self.radians is None else self.radians[item]
        return GaussianMeshesNaive(self.verts[item], self.sigmas[item], rad)


class GaussianMeshes(nn.Module):
    """Parameters with per-argument requires_grad switches (Meshes.py:30-54)."""

    def __init__(self, verts, sigmas, radians=None, gradianted_args=None):
        super().__init__()
        flags = [True, True, True] if gradianted_args is None else list(gradianted_args)
        self.verts = nn.Parameter(verts, requires_grad=flags[0])
        self.sigmas = nn.Parameter(sigmas, requires_grad=flags[1])
        if radians is None:
            self.radians = None
            flags[2] = False
        else:
            self.radians = nn.Parameter(radians, requires_grad=flags[2])
        self.gradianted_args = flags

    def grad_parameters(self):
        params = (self.verts, self.sigmas, self.radians)
        return tuple(p for p, f in zip(params, self.gradianted_args) if f)

    def forward(self):
        return self.verts, self.sigmas, self.radians


DeformedGaussianMeshes = GaussianMeshes


def _check_oriented(verts, scales, quats):
    if scales.shape[-1] != 3 or quats.shape[-1] != 4 or scales.shape[:-1] != quats.shape[:-1] or verts.shape[-1] != 3 \
            or verts.shape[-2] != scales.shape[-2]:
        raise ValueError('oriented Gaussians take verts[..,N,3], scales[..,N,3] and quats[..,N,4] (w, x, y, z) with the same leading '
                         f'dims for scales and quats; got {tuple(verts.shape)}, {tuple(scales.shape)}, {tuple(quats.shape)}')


class OrientedGaussianMeshesNaive:
    """Plain references to the tensors of oriented Gaussians: calling one returns (verts, scales [..,N,3], quats [..,N,4]);
    S = R(q) diag(scales) R(q)^T stands where an (N,3,3) `sigmas` would (Aggregation.oriented_sigma).  No counterpart in the
    reference, whose `radians` slot is never consumed."""
    oriented = True

    def __init__(self, verts, scales, quats):
        _check_oriented(verts, scales, quats)
        self.verts, self.scales, self.quats = verts, scales, quats

    def to(self, device):
        self.verts, self.scales, self.quats = self.verts.to(device), self.scales.to(device), self.quats.to(device)
        return self

    def __call__(self):
        return self.verts, self.scales, self.quats

    def __getitem__(self, item):
        return OrientedGaussianMeshesNaive(self.verts[item], self.scales[item], self.quats[item])


class OrientedGaussianMeshes(nn.Module):
    """Oriented Gaussians as parameters with per-argument requires_grad switches (verts, scales, quats), as GaussianMeshes."""
    oriented = True

    def __init__(self, verts, scales, quats, gradianted_args=None):
        super().__init__()
        _check_oriented(verts, scales, quats)
        flags = [True, True, True] if gradianted_args is None else list(gradianted_args)
        self.verts = nn.Parameter(verts, requires_grad=flags[0])
        self.scales = nn.Parameter(scales, requires_grad=flags[1])
        self.quats = nn.Parameter(quats, requires_grad=flags[2])
        self.gradianted_args = flags

    def grad_parameters(self):
        params = (self.verts, self.scales, self.quats)
        return tuple(p for p, f in zip(params, self.gradianted_args) if f)

    def __getitem__(self, item):
        return OrientedGaussianMeshesNaive(self.verts[item], self.scales[item], self.quats[item])

    def forward(self):
        return self.verts, self.scales, self.quats
