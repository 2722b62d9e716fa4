"""The frame form of the forward composite (composite.hip: compositen_kernel<..., FRAME = true>) against the generic instantiation,
bit for bit.

The host gives a launch of the one-pass entries (shade stage C = 3, 4 from scalar, per-axis or full records; depth stage) the frame
form when K is a multiple of four and every offset fits 32 bits; every other launch keeps the generic instantiation.  The two are
run on the SAME lists by a route the code already has: a list of K slots and the same list with dead slots appended up to the next
K' take different instantiations when exactly one of K, K' is a multiple of four, and a dead slot (index -1, len 1e10, beyond the
count) contributes nothing to any sum -- the scans' association is a function of the lane's index in the pixel alone and a pixel's
result does not depend on where it sits in a wave (composite_core.h).  So

  K in 4, 8, 40, 44, 128 (LP = 1, 2, 10, 11, 32 lanes per pixel): frame form, against K + 1 padded (generic);
  K = 256 (LP = 64; 257 is beyond the entries' limit): frame form on lists of at most 255 hits, against K = 255 (generic);
  K in 5, 25, 41: generic, against 8, 28, 44 padded (frame form)

must agree in every output: weight, valid_num, the rewritten index list, rgb, img, wsum, sil, depth, the kept act / dsd, and the
zeroed accumulator of the backward.  Compared with np.array_equal on the bit patterns.

Lists (ctypes entries): 48 (8 x 6), 256 (16 x 16) and 241 pixels -- a prime, no multiple of the pixels per wave unless a pixel
fills the wave -- over 300 Gaussians; hit counts 0, 1, 2, 3, K - 1, K and random ones; the first wave's pixels all full and the
second wave's all empty; one pixel out of order (the unsorted arm: the K x K scan); colour ids at and beyond the table's rows;
thr = 0 and 0.4; a background component of 1.5; sil asked for or not; an accumulator the launch covers and one it does not (the fill
fallback).  Then two frames through the public renderer (8 x 6 and 16 x 16, 60 and 300 Gaussians) at K = 40 and K = 41."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OCC = 1.0
P = 300           # Gaussians
NATTR = 280       # rows of the colour table: ids 280 .. 299 are beyond it
SIZES = (48, 256, 241)      # 8 x 6, 16 x 16, and a prime: no multiple of any number of pixels per wave but 1
FILL = -7.0
FORMS = ("iso3", "iso4", "axis3", "axis4", "full3", "full4", "depth", "depth_sum")
# (K run, K of the other instantiation, which of the two is the frame form)
PAIRS = [(4, 5), (8, 9), (40, 41), (44, 45), (128, 129), (256, 255), (5, 8), (25, 28), (41, 44)]


def t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def bits(x):
    a = np.ascontiguousarray(x.detach().cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def pixels_per_wave(K):
    return 64 // ((K + 3) // 4)


@functools.lru_cache(maxsize=None)
def lists(K, npix, cap):
    """idx / cnt / len [npix, K] with at most `cap` hits per pixel, rays, and the three record forms of 300 Gaussians."""
    rng = np.random.default_rng(1000 * K + npix)
    pw = pixels_per_wave(K)
    cnt = rng.integers(0, cap + 1, npix)
    special = [0, 1, 2, 3, cap - 1, cap, 5 if cap >= 5 else cap, 0]
    cnt[2 * pw:2 * pw + len(special)] = special[:max(0, min(len(special), npix - 2 * pw))]
    cnt[:pw] = cap                      # a full wave ...
    cnt[pw:min(2 * pw, npix)] = 0       # ... next to an empty one
    idx = np.full((npix, K), -1, np.int32)
    ln = np.full((npix, K), 1e10, np.float32)
    for p in range(npix):
        c = int(cnt[p])
        idx[p, :c] = rng.integers(0, P, c)
        ln[p, :c] = np.sort(rng.uniform(1.0, 3.0, c).astype(np.float32))
    uns = next(p for p in range(npix - 1, -1, -1) if cnt[p] >= 2)      # one pixel out of order
    ln[uns, [0, cnt[uns] - 1]] = ln[uns, [cnt[uns] - 1, 0]]
    if cnt[0] >= 1:
        idx[0, 0] = NATTR               # the first id beyond the table, and the last one
        idx[0, cnt[0] - 1] = P - 1
    rays = np.concatenate([rng.uniform(-0.3, 0.3, (npix, 2)), np.ones((npix, 1))], 1).astype(np.float32)
    mu = rng.uniform(-0.3, 0.3, (P, 3)).astype(np.float32) + np.float32([0, 0, 2.0])
    a = rng.uniform(1.0, 6.0, (P, 1)).astype(np.float32)
    ax = (a * rng.uniform(0.6, 1.6, (P, 3))).astype(np.float32)
    L = np.tril(rng.uniform(-1, 1, (P, 3, 3)))
    L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.5
    A = (L @ L.transpose(0, 2, 1) * a[:, :, None]).astype(np.float32)
    rec = {"iso": np.concatenate([mu, a], 1), "axis": np.concatenate([mu, ax, np.zeros((P, 2), np.float32)], 1),
           "full": np.concatenate([mu, A.reshape(P, 9)], 1)}
    colors = rng.uniform(0, 1, (NATTR, 4)).astype(np.float32)
    return dict(idx=idx, cnt=cnt.astype(np.int32), len=ln, rays=rays, rec=rec, colors=colors, uns=uns)


def widen(a, K2, fill):
    """the same lists with dead slots appended (K2 > K) or the dead last slots cut (K2 < K)"""
    K = a.shape[1]
    if K2 <= K:
        return np.ascontiguousarray(a[:, :K2])
    return np.concatenate([a, np.full((a.shape[0], K2 - K), fill, a.dtype)], 1)


def run(form, K, L, thr, want_sil, acc_floats):
    """One launch through the C ABI; every output pre-filled."""
    from voge_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    npix = L["idx"].shape[0]
    idx, cnt, ln, rays = t(widen(L["idx"], K, -1), torch.int32), t(L["cnt"], torch.int32), t(widen(L["len"], K, 1e10)), t(L["rays"])
    weight = torch.full((npix, K), FILL, device=DEV)
    vn = torch.full((npix,), int(FILL), dtype=torch.int64, device=DEV)
    wsum, sil = torch.full((npix,), FILL, device=DEV), (torch.full((npix,), FILL, device=DEV) if want_sil else None)
    acc = torch.full((acc_floats,), FILL, device=DEV) if acc_floats else None
    pa = lambda x: None if x is None else x.data_ptr()
    out = dict(weight=weight, valid_num=vn, wsum=wsum)
    if form.startswith("depth"):
        depth = torch.full((npix,), FILL, device=DEV)
        rc = lib.voge_frame_depth_fwd_iso(pa(idx), pa(cnt), pa(ln), pa(t(L["rec"]["iso"])), pa(rays), OCC, int(form == "depth"), 7.5, npix, K,
                                          pa(weight), pa(vn), pa(depth), pa(wsum), pa(sil), pa(acc), 4 * acc_floats, st)
        out["depth"] = depth
    else:
        kind, C = form[:-1], int(form[-1])
        colors, bg = t(L["colors"][:, :C]), t([1.5, 0.25, 0.0, 0.5][:C])
        rgb, img = torch.full((npix, C), FILL, device=DEV), torch.full((npix, C), FILL, device=DEV)
        rec = t(L["rec"][kind])
        shade = (OCC, pa(colors), pa(bg), thr, npix, K, C, NATTR, pa(weight), pa(vn), pa(rgb), pa(img), pa(wsum))
        if kind == "iso" and not want_sil and not acc_floats:
            rc = lib.voge_composite_shade_fwd_iso(pa(idx), pa(cnt), pa(ln), pa(rec), pa(rays), *shade, st)
        elif kind == "iso":
            rc = lib.voge_frame_shade_fwd_iso(pa(idx), pa(cnt), pa(ln), pa(rec), pa(rays), *shade, pa(sil), pa(acc), 4 * acc_floats, st)
        else:
            act, dsd = torch.full((npix, K), FILL, device=DEV), torch.full((npix, K), FILL, device=DEV)
            rc = lib.voge_frame_shade_fwd_rec(1 if kind == "axis" else 2, pa(idx), pa(cnt), pa(ln), pa(rec), pa(rays), *shade, pa(sil), pa(act), pa(dsd),
                                              pa(acc), 4 * acc_floats, st)
            out.update(act=act, dsd=dsd)
        out.update(rgb=rgb, img=img, idx=idx)
    assert rc == 0, (form, K, rc)
    torch.cuda.synchronize()
    if want_sil:
        out["sil"] = sil
    if acc_floats:
        out["acc"] = acc
    return out


def cases():
    out = []
    for i, (K, K2) in enumerate(PAIRS):
        for j, form in enumerate(FORMS):
            if form.startswith("depth") and K2 > 128:      # (the depth entry takes K <= 128: 128 against 127, lists of at most 127 hits)
                if K > 128:
                    continue
                K2 = K - 1
            # thr, sil, and the accumulator's size dealt over the grid so that every form meets every setting
            out.append((K, K2, form, SIZES[(i + j) % 3], (0.0, 0.4)[(i + j // 2) % 2], (i + j // 3) % 3 != 0, (0, 4 * 50, 4 * 100000)[(i + 2 * j) % 3]))
    return out


def test_the_grid_of_cases_covers_what_it_claims():
    cs = cases()
    for form in FORMS:
        mine = [c for c in cs if c[2] == form]
        assert {c[3] for c in mine} == set(SIZES) and {c[5] for c in mine} == {True, False} and {c[6] for c in mine} == {0, 200, 400000}, form
        if not form.startswith("depth"):
            assert {c[4] for c in mine} == {0.0, 0.4}, form
    assert all(c[0] <= 128 and c[1] <= 128 for c in cs if c[2].startswith("depth"))
    for K, K2 in PAIRS:
        assert (K % 4 == 0) != (K2 % 4 == 0) and (K % 4 == 0) != ((K - 1) % 4 == 0)
        pw = pixels_per_wave(K)
        assert pw == 1 or any(s % pw for s in SIZES), K
    # the larger accumulator is beyond what the smallest launch covers (its grid x 64 float4s), the smaller one inside every launch
    assert 400000 // 4 > 256 * 64 and 200 // 4 <= 64


@pytest.mark.parametrize("K,K2,form,npix,thr,want_sil,acc_floats", cases())
def test_frame_form_and_generic_instantiation_give_the_same_bits(hip_lib, K, K2, form, npix, thr, want_sil, acc_floats):
    cap = min(K, K2)
    L = lists(max(K, K2) if K2 < K else K, npix, cap)
    if K2 < K:      # (K = 256 against 255: the lists hold at most 255 hits; both runs see slices / the whole of the same arrays)
        assert L["cnt"].max() <= K2
    a, b = run(form, K, L, thr, want_sil, acc_floats), run(form, K2, L, thr, want_sil, acc_floats)
    lo = min(K, K2)
    cnt = L["cnt"]
    assert (a["valid_num"].cpu().numpy() == cnt).all() and (b["valid_num"].cpu().numpy() == cnt).all()
    for name in a:
        x, y = a[name], b[name]
        if x.dim() == 2 and x.shape[1] in (K, K2) and name not in ("rgb", "img"):
            if name in ("act", "dsd"):      # kept for the live slots only: the others keep the fill in both
                live = torch.arange(lo, device=DEV)[None, :] < t(cnt, torch.int64)[:, None]
                assert (x[:, :lo][~live] == FILL).all() and (y[:, :lo][~live] == FILL).all(), (name, K, K2)
            else:
                assert (x[:, lo:] == 0).all() and (y[:, lo:] == 0).all(), (name, K, K2)
            x, y = x[:, :lo], y[:, :lo]
        assert np.array_equal(bits(x), bits(y)), (form, K, K2, name, int((bits(x) != bits(y)).sum()))
        if name != "acc" and name not in ("act", "dsd"):
            assert (x != FILL).all(), (form, K, name, "not every element written")
    if acc_floats:
        assert (a["acc"] == 0).all() and (b["acc"] == 0).all()
    # the lists are what the docstring says, and the outputs say so
    w = a["weight"].cpu().numpy()
    assert np.isfinite(w).all() and (w[cnt == 0] == 0).all() and (w >= 0).all() and (w[cnt > 0] > 0).any()
    if "idx" in a:
        i2 = a["idx"].cpu().numpy()[:, :lo]
        dead = np.arange(lo)[None, :] >= cnt[:, None]
        assert (i2[dead] == 0).all() and (i2[~dead] == L["idx"][:, :lo][~dead]).all()
        empty = cnt == 0
        bg = np.float32([1.5, 0.25, 0.0, 0.5][:a["img"].shape[1]])
        assert (a["rgb"].cpu().numpy()[empty] == 0).all() and (a["img"].cpu().numpy()[empty] == np.minimum(bg, 1.0)).all()
    if want_sil:
        assert np.array_equal(bits(a["sil"]), bits(torch.clamp(a["wsum"], max=1.0)))


@pytest.mark.parametrize("H,W,N", [(6, 8, 60), (16, 16, 300)])
def test_public_renderer_at_k40_and_k41(hip_lib, H, W, N):
    """The frame path itself: the same scene rendered with 40 (frame form) and 41 (generic) slots per pixel, no pixel with more than
    40 hits -- image over a background with a component above 1, silhouette and depth have the same bits."""
    import test_gpu_depth as dpt
    from oracle import camera_np
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import get_depth, get_silhouette, to_colored_background
    rng = np.random.default_rng(N)
    verts = (rng.uniform(-1, 1, (N, 3)) * 0.5).astype(np.float32)
    r = rng.uniform(0.07, 0.12, N)
    sig = (1.0 / (r * r / (2 * np.log(1 / 0.6)))).astype(np.float32)
    cols = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    R, T = camera_np.look_at_view_transform(4.0, 10.0, 70.0)
    got = {}
    for K in (40, 41):
        renderer = dpt.renderer_for(H, W, K, 30.0 * W / 16.0)
        gm = GaussianMeshes(t(verts), t(sig)).to(DEV)
        frag = renderer(gm, R=t(R), T=t(T))
        img = to_colored_background(frag, t(cols), background_color=(1.5, 0.25, 0.0))
        sil = get_silhouette(frag)
        frag_d = renderer(gm, R=t(R), T=t(T))
        depth = get_depth(frag_d, normalize=True, background=7.5)
        torch.cuda.synchronize()
        got[K] = dict(img=img, sil=sil, depth=depth, weight=frag.vert_weight[..., :40], idx=frag.vert_index[..., :40], vn=frag.valid_num)
    vn = got[40]["vn"].cpu().numpy()
    assert vn.max() <= 40 and vn.max() >= 4 and (vn == 0).any(), (vn.max(), vn.min())
    for name in got[40]:
        assert np.array_equal(bits(got[40][name]), bits(got[41][name])), (H, W, name)
