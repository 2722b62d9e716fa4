"""CPU tests of Renderer.get_distortion (an extension: the reference has no distortion regulariser): the import path and what
the docstring promises, the two C-ABI entries and their host-side argument validation (no GPU here: anything that reached HIP
would fail differently), and Aggregation.distortion -- the definition the kernels are tested against -- in fp64 against the
pairwise sum  L = sum_i sum_j w_i w_j |t_i - t_j|  and autograd through it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "voge_hip.h")
ENTRIES = {"voge_distortion_fwd": 9, "voge_distortion_bwd": 12}


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_get_distortion_is_importable_through_the_alias_package():
    from VoGE.Renderer import get_distortion
    from voge_amd import Renderer
    assert get_distortion is Renderer.get_distortion
    doc = get_distortion.__doc__
    assert "POSITIONAL subgradient" in doc and "sign(0)" in doc      # the tie rule
    assert "1 / (far - near)" in doc                                   # no distance mapping: the user's own scale


def test_the_two_entries_are_declared_exported_and_typed(lib):
    from voge_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s*" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in voge_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.voge_abi_version() == 7
    text = open(HEADER).read()
    assert "Depth-distortion regulariser of composited fragments (EXTENSION" in text
    assert "(t[..., :, None] - t[..., None, :]).abs()" in text      # which torch expression they replace


def test_entries_validate_before_any_hip_call(lib):
    P = 1234      # (a non-NULL pointer value: nothing is dereferenced before validation is through)
    assert lib.voge_distortion_fwd(None, None, None, 10, 8, 1, None, None, None) == -1
    assert lib.voge_distortion_fwd(P, P, P, 10, 8, 0, P, None, None) == -1
    assert lib.voge_distortion_fwd(P, P, P, -1, 8, 1, P, P, None) == -1
    assert lib.voge_distortion_fwd(P, P, P, 10, 0, 1, P, P, None) == -1
    assert lib.voge_distortion_fwd(P, P, P, 10, 257, 1, P, P, None) == -3
    assert lib.voge_distortion_fwd(P, P, P, 0, 8, 1, P, P, None) == 0
    assert lib.voge_distortion_bwd(P, P, P, P, P, None, 10, 8, 1, P, P, None) == -1
    assert lib.voge_distortion_bwd(P, P, P, P, P, P, 10, 8, 0, P, None, None) == -1
    assert lib.voge_distortion_bwd(P, P, P, None, None, P, 10, 8, 1, P, P, None) == -1      # the normalised form needs dist and wsum
    assert lib.voge_distortion_bwd(P, P, P, P, P, P, -1, 8, 1, P, P, None) == -1
    assert lib.voge_distortion_bwd(P, P, P, P, P, P, 10, 0, 1, P, P, None) == -1
    assert lib.voge_distortion_bwd(P, P, P, P, P, P, 10, 257, 1, P, P, None) == -3
    assert lib.voge_distortion_bwd(P, P, P, P, P, P, 0, 8, 1, P, P, None) == 0
    assert lib.voge_distortion_bwd(None, None, None, None, None, None, 0, 8, 0, None, None, None) == 0


# ---- the pairwise definition, in torch so that autograd differentiates it ---------------------------------------------------
def pairwise(w, t, vn, normalize):
    K = w.shape[-1]
    live = torch.arange(K) < vn.clamp(0, K)[..., None]
    wl = torch.where(live, w, torch.zeros_like(w))
    tl = torch.where(live, t, torch.zeros_like(t))
    L = (wl[..., :, None] * wl[..., None, :] * (tl[..., :, None] - tl[..., None, :]).abs()).sum((-1, -2))
    if not normalize:
        return L
    S = wl.sum(-1)
    return torch.where(S > 0, L / torch.where(S > 0, S * S, torch.ones_like(S)), torch.zeros_like(L))


def case(P=50, K=13, seed=0):
    """P pixels of K slots: valid_num from [0, K + 2] plus one negative entry, distinct sorted live len, garbage in the dead slots."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 0.4, (P, K))
    w[rng.uniform(size=(P, K)) < 0.1] = 0.0
    t = np.sort(rng.uniform(3.0, 4.0, (P, K)), axis=-1)
    vn = rng.integers(0, K + 3, P)
    vn[:6] = [0, 1, K - 1, K, K + 2, -3]
    dead = np.arange(K)[None] >= np.clip(vn, 0, K)[:, None]
    t[dead] = 1e10
    w[dead & (rng.uniform(size=dead.shape) < 0.5)] = 0.25      # (garbage in dead slots must not count)
    return torch.tensor(w), torch.tensor(t), torch.tensor(vn), dead


@pytest.mark.parametrize("normalize", [False, True])
def test_definition_equals_the_pairwise_sum_and_its_autograd_gradients(normalize):
    from voge_amd.Aggregation import distortion
    w, t, vn, dead = case()
    g = torch.tensor(np.random.default_rng(1).normal(size=w.shape[0]))
    outs = []
    for fn in (distortion, pairwise):
        wi, ti = w.clone().requires_grad_(True), t.clone().requires_grad_(True)
        out = fn(wi, ti, vn, normalize)
        (out * g).sum().backward()
        outs.append((out.detach(), wi.grad, ti.grad))
    (d, gw, gt), (d_ref, gw_ref, gt_ref) = outs
    assert d.dtype == torch.float64 and d.shape == vn.shape
    assert (d - d_ref).abs().max().item() <= 1e-12
    assert (gw - gw_ref).abs().max().item() <= 1e-12 and (gt - gt_ref).abs().max().item() <= 1e-12
    assert gw_ref.abs().max().item() > 0.1 and gt_ref.abs().max().item() > 0.1
    assert (gw[torch.tensor(dead)] == 0).all() and (gt[torch.tensor(dead)] == 0).all()
    empty = vn.clamp(0, w.shape[-1]) == 0
    assert empty.sum() >= 2 and (d[empty] == 0).all()
    assert (d[vn == 1] == 0).all()      # (one live slot: no pair)


@pytest.mark.parametrize("normalize", [False, True])
def test_a_shuffled_row_gives_the_value_of_its_sorted_copy(normalize):
    from voge_amd.Aggregation import distortion
    w, t, vn, _ = case(seed=2)
    K = w.shape[-1]
    ws, ts = w.clone(), t.clone()
    rng = np.random.default_rng(3)
    for p in range(w.shape[0]):
        n_ = int(np.clip(int(vn[p]), 0, K))
        perm = torch.tensor(rng.permutation(n_), dtype=torch.long)
        ws[p, :n_], ts[p, :n_] = w[p, :n_][perm], t[p, :n_][perm]
    a, b = distortion(w, t, vn, normalize), distortion(ws, ts, vn, normalize)
    assert not torch.equal(ts, t)
    assert (a - b).abs().max().item() <= 1e-12
    assert (b - pairwise(ws, ts, vn, normalize)).abs().max().item() <= 1e-12


def test_a_three_slot_tie_gets_the_positional_subgradient():
    """t = (1, 1, 2): L = 2 (w0 w2 + w1 w2).  Slot 0 counts as nearer than slot 1: dL/dt = 2 w_i (W<_i - W>_i) exactly, so the
    tie hands -2 w0 w1 to t0 and +2 w0 w1 to t1 on top of what the pair with slot 2 gives (torch's |.| gives the tie nothing)."""
    from voge_amd.Aggregation import distortion
    w = torch.tensor([[0.5, 0.25, 0.125]], dtype=torch.float64, requires_grad=True)
    t = torch.tensor([[1.0, 1.0, 2.0]], dtype=torch.float64, requires_grad=True)
    L = distortion(w, t, torch.tensor([3]))
    assert L.item() == 2 * (0.5 * 0.125 + 0.25 * 0.125)
    L.sum().backward()
    w0, w1, w2 = 0.5, 0.25, 0.125
    assert t.grad.tolist() == [[2 * w0 * (0 - (w1 + w2)), 2 * w1 * (w0 - w2), 2 * w2 * (w0 + w1)]]
    assert t.grad[0, 0].item() == -2 * w0 * w1 - 2 * w0 * w2 and t.grad[0, 1].item() == 2 * w0 * w1 - 2 * w1 * w2
    # dL/dw_i = 2 [u_i (W< - W>) - (X< - X>)] with u = (0, 0, 1)
    assert w.grad.tolist() == [[2 * w2, 2 * w2, 2 * (w0 + w1)]]
    # the pairwise expression differs exactly by the tie's two terms
    wp, tp = w.detach().clone().requires_grad_(True), t.detach().clone().requires_grad_(True)
    pairwise(wp, tp, torch.tensor([3]), False).sum().backward()
    assert (t.grad - tp.grad).tolist() == [[-2 * w0 * w1, 2 * w0 * w1, 0.0]]


def test_fp32_recentring_holds_the_value_at_an_offset():
    """The same pixels shifted by 1000 (exactly: the len are multiples of 2^-13): the fp32 definition stays within 2e-6 of the fp64
    pairwise sum; the closed form on t itself would be off by about 2e-4 there."""
    from voge_amd.Aggregation import distortion
    w, t, vn, _ = case(seed=4)
    t = torch.where(t < 1e9, torch.round(t * 8192) / 8192, t)
    ref = pairwise(w, t, vn, False)
    for off in (0.0, 1000.0):
        t32 = torch.where(t < 1e9, t + off, t).float()
        assert torch.equal(t32.double(), torch.where(t < 1e9, t + off, t))
        got = distortion(w.float(), t32, vn).double()
        assert ((got - ref).abs() <= 2e-6 * ref.clamp(min=1.0)).all(), off


def test_host_fp32_fragments_take_the_torch_definition(lib, monkeypatch):
    from voge_amd.Renderer import Fragments, get_distortion

    def boom(*a):
        raise AssertionError("a HIP entry was called on host tensors")
    monkeypatch.setattr(lib, "voge_distortion_fwd", boom, raising=True)
    monkeypatch.setattr(lib, "voge_distortion_bwd", boom, raising=True)
    torch.manual_seed(0)
    w = torch.rand(4, 5, 3, requires_grad=True)
    ln = torch.sort(torch.rand(4, 5, 3) + 2, dim=-1)[0].requires_grad_(True)
    frag = Fragments(w, torch.zeros(4, 5, 3, dtype=torch.int32), torch.randint(0, 5, (4, 5)), ln)
    for normalize in (False, True):
        d = get_distortion(frag, normalize=normalize)
        assert d.shape == (4, 5) and d.dtype == torch.float32 and torch.isfinite(d).all() and (d >= 0).all()
    d.sum().backward()
    assert torch.isfinite(w.grad).all() and torch.isfinite(ln.grad).all() and ln.grad.abs().max().item() > 0
