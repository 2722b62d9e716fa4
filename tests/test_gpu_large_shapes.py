"""The large-shape arms: the 64-bit-offset instantiations of the composite and of the fused backward (npix * K >= 2^30), their
32-bit forms at their largest launches, the gate between the two at few slots and very many pixels, the sweep's plain-store
epilogue (W * K >= 2^26) and the consumers' long indexing on 2^30 slots.  The cases, the gates and the tiling rule are
tests/large_shape_cases.py's; its docstring says why a large input is THREE different base tiles repeated, never one.

Every test builds its base fragments once per module at the small shape through ops._Fragments (the renderer's own trace +
composite chain; scalar forms with VOGE_FRAGMENTS_KEEP_ACT_DSD=1 so that act / dsd exist), holds them to the fp64 oracle there
(TOL of scale on the pixels whose index lists the oracle chose alike, at least 90 % of them -- tests/test_gpu_fragment_bwd_entries.py's
bound; a quarter of TOL for the depth form), tiles them on the device and calls the entry at the large shape directly -- the
Python layer above the entries takes no tiled fragments.  Deterministic outputs of the large call must equal the SMALL call of the
same entry on base t mod 3 bit for bit in every tile; per-Gaussian gradients (floating-point atomics: no fixed order) must pass
grad_close against the fp64 reference of base t mod 3 in every tile's block -- the worst tile per base is the one reported.  The
consumers and the sweep go through their public ops functions; a spy on the loaded library checks every entry and its sizes.

Each test checks torch.cuda.mem_get_info() against the case's need first and frees everything in a finally."""
import contextlib
import gc
import os
import time
import types

import numpy as np
import pytest
import torch

import large_shape_cases as ls
from util import TOL, compare_trace_strict, grad_close, log_line

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADROOM = 4 << 30      # the fills' temporaries, the comparisons' masks and copies (3.1 GiB measured at most), torch's own context


def t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def n(x):
    return x.detach().cpu().numpy()


def p(x):
    return None if x is None else x.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


# ---- the base fragments: once per module -----------------------------------------------------------------------------------------
_BASES = {}


def base_fragments(case):
    """[3 x dict] of base b's fragments on the device (flat pixels): mus, p1, rays [pix0,3], colors [P0,4], idx, len, weight, act,
    dsd [pix0,K], cnt [pix0] int32, valid [pix0] int64, records [P0,4] | None; ref = the fp64 oracle's dict; same [pix0] bool: the
    pixels whose index list is the oracle's.  Held to the oracle here, once."""
    from voge_amd import ops
    key = (case.K, case.H0, case.W0, case.form)
    if key in _BASES:
        return _BASES[key]
    out = []
    for b, tile in enumerate(ls.case_bases(case)):
        mus, p1 = t(tile["mus"]), t(tile["a"] if case.form == "scalar" else tile["isigmas"])
        rays = t(tile["rays"])[None]
        with torch.no_grad(), env("VOGE_FRAGMENTS_KEEP_ACT_DSD", "1"):
            weight, idx, valid, ln, cnt, records, act, dsd = ops._Fragments.apply(1 if case.form == "scalar" else 0, mus, p1, None, rays, None,
                                                                                  ls.THR_ACT, case.K, 0, 1.0)
        K = case.K
        d = dict(mus=mus, p1=p1, rays=rays.reshape(-1, 3), colors=t(tile["colors"]), idx=idx.reshape(-1, K), len=ln.reshape(-1, K),
                 weight=weight.reshape(-1, K), act=act.reshape(-1, K), dsd=dsd.reshape(-1, K), cnt=cnt.reshape(-1),
                 valid=valid.reshape(-1), records=records, tile=tile)
        ref = ls.oracle_forward(tile, K)
        ridx = ref["idx"].numpy()
        same = (n(d["idx"]) == ridx).all(-1)
        label = f"[large shapes] base {b} of K={K} {case.H0}x{case.W0} {case.form}"
        assert same.mean() >= 0.9, f"{label}: only {same.mean():.3f} of the pixels have the oracle's index list"
        assert (n(d["cnt"])[same] == ref["vn"].numpy()[same]).all() and (n(d["valid"]) == n(d["cnt"])).all(), label
        w_ref = ref["w"].detach().numpy()
        err = np.abs(n(d["weight"]) - w_ref)[same].max()
        log_line(f"{label}: {int((~same).sum())} of {same.size} pixels differ from the oracle's lists; weights off by {err:.2e} (bound {TOL:.0e} of scale)")
        assert err <= TOL * max(1.0, np.abs(w_ref).max()), (label, err)
        vn = n(d["cnt"])
        assert (vn == 0).any() and (vn == K).any() and (K == 1 or ((vn > 0) & (vn < K)).any()), label
        d.update(ref=ref, same=same)
        out.append(d)
    _BASES[key] = out
    return out


# ---- one large case: memory check, timing, clean-up -----------------------------------------------------------------------------
def run_case(case, body, with_bases=True):
    """body(case, A, bases): A is the dict that holds every large tensor; it is emptied, and the allocator's cache released, whatever
    happens."""
    bases = base_fragments(case) if with_bases else None
    need = ls.CASES[case.short_of].need_bytes() if case.short_of else case.need_bytes()
    assert need <= ls.CAP_BYTES
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if need + HEADROOM > free:
        pytest.skip(f"{case.name} needs {need + HEADROOM} bytes ({need / 2**30:.1f} GiB in its arrays), {free} are free of {total}")
    A = {}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    try:
        body(case, A, bases)
        torch.cuda.synchronize()
        log_line(f"[large shapes] {case.name}: {case.arm}; {case.slots} slots, {case.npix} pixels ({case.nrows} x {case.W}), {case.P} Gaussians, {need / 2**30:.1f} GiB "
                 f"planned, peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB, {time.perf_counter() - t0:.1f} s")
    finally:
        A.clear()
        from voge_amd import ops
        ops.release_workspaces()
        gc.collect()
        torch.cuda.empty_cache()


def tiled(case, bases, key, tail=(), dtype=torch.float32, offset=None, T=None, src=None, per="pix"):
    """The large array of bases[b][key] (or src[b]), tile t = base t mod 3: [T * pix0, *tail] (per "pix") | [T * P0, *tail] ("gauss")."""
    T = case.T if T is None else T
    n0 = case.pix0 if per == "pix" else ls.P0
    small = [(bases[b][key] if src is None else src[b]).reshape((n0,) + tuple(tail)).to(dtype) for b in range(3)]
    out = torch.empty((T * n0,) + tuple(tail), dtype=dtype, device=DEV)
    ls.fill_tiles(out.view((T, n0) + tuple(tail)), small, offset)
    return out


def lit_counts(case, bases, T=None):
    """cnt of the large input: the bases' counts in the lit tiles, zero elsewhere."""
    T = case.T if T is None else T
    if case.lit == "all":
        return tiled(case, bases, "cnt", dtype=torch.int32, T=T)
    out = torch.zeros((T * case.pix0,), dtype=torch.int32, device=DEV)
    ls.fill_tiles(out.view(T, case.pix0), [bases[b]["cnt"] for b in range(3)], tiles=case.lit_tiles())
    return out


def assert_tiles_equal(label, big, small, n0, T, tiles=None):
    """big [>= T * n0, ...] == small[t mod 3] bit for bit in every tile (or in `tiles`), compared on the device."""
    v = big.reshape((-1, n0) + tuple(big.shape[1:]))[:T]
    for b in range(3):
        s = small[b].reshape((n0,) + tuple(big.shape[1:]))
        sel = v[b::3] if tiles is None else v[[t_ for t_ in tiles if t_ % 3 == b]]
        if sel.shape[0] == 0:
            continue
        bad = ((sel != s[None]) & ~(torch.isnan(sel) & torch.isnan(s[None]))).reshape(sel.shape[0], -1).any(1)
        nbad = int(bad.sum())
        if nbad:
            first = int(torch.nonzero(bad)[0])
            diff = (sel[first].double() - s.double()).abs().max()
            raise AssertionError(f"{label}: {nbad} of {sel.shape[0]} tiles of base {b} differ from the small call; the first is number {first} "
                                 f"of them, largest difference {float(diff):.3e}")


def tiles_grad_close(label, g_big, refs, tol, T, tiles=None, dark_zero=False):
    """Every tile's block of a per-Gaussian gradient [T * P0, ...] against the fp64 reference of base t mod 3: the reduction (max over
    the tiles of the error) runs on the device, the worst tile of each base goes through grad_close.  -> the largest scaled error."""
    v = g_big.reshape((-1, ls.P0) + tuple(g_big.shape[1:]))[:T]
    worst = 0.0
    for b in range(3):
        ref = torch.tensor(np.asarray(refs[b]), dtype=torch.float64, device=DEV).reshape((ls.P0,) + tuple(g_big.shape[1:]))
        ids = list(range(b, T, 3)) if tiles is None else [t_ for t_ in tiles if t_ % 3 == b]
        if not ids:
            continue
        sel = v[b::3] if tiles is None else v[ids]
        err = torch.zeros(sel.shape[0], dtype=torch.float64, device=DEV)
        for i0 in range(0, sel.shape[0], 4096):
            err[i0:i0 + 4096] = (sel[i0:i0 + 4096].double() - ref[None]).abs().reshape(min(4096, sel.shape[0] - i0), -1).amax(1)
        assert bool(torch.isfinite(err).all()), f"{label}: a non-finite gradient in base {b}'s tiles"
        w = int(torch.argmax(err))
        scale = max(1.0, float(ref.abs().max()))
        worst = max(worst, float(err[w]) / scale)
        grad_close(f"[large shapes] {label}, base {b}: the worst of {len(ids)} tiles (tile {ids[w]})", n(sel[w]), np.asarray(refs[b]), tol)
    if dark_zero and tiles is not None:
        dark = torch.ones(T, dtype=torch.bool, device=DEV)
        dark[tiles] = False
        assert float(v[dark].abs().max()) == 0.0, f"{label}: a Gaussian of a tile without hits got a gradient"
    return worst


def spy(monkeypatch, lib, names):
    calls = []
    for name in names:
        def wrap(*a, _real=getattr(lib, name), _name=name):
            calls.append((_name, a))
            return _real(*a)
        monkeypatch.setattr(lib, name, wrap, raising=True)
    return calls


def entry(lib, calls, name, **kw):
    """Call a fused-backward entry by its parameter names (tests/test_fragment_bwd_args_cpu.ARGS); the call is kept in `calls`."""
    from test_fragment_bwd_args_cpu import ARGS
    names = ARGS[name].split()
    assert set(kw) == set(names), (name, sorted(set(names) ^ set(kw)))
    calls.append((name, dict(kw)))
    rc = getattr(lib, name)(*[kw[k] for k in names])
    assert rc == 0, (name, rc)


def close_on(label, got, want, same, tol=TOL):
    """|got - want| <= tol * max(1, |want|_max) on the pixels of `same`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = float(np.abs(got - want)[same].max(initial=0.0))
    scale = max(1.0, float(np.abs(want[same]).max(initial=0.0)))
    log_line(f"[large shapes] {label}: off by {err / scale:.2e} of scale from the fp64 oracle (bound {tol:.1e})")
    assert err <= tol * scale, (label, err, scale)


# ---- 1. voge_composite_fwd / _bwd from act / dsd ------------------------------------------------------------------------------
def _composite_body(lib, with_bwd):
    def body(case, A, bases):
        K, T, npix, pix0 = case.K, case.T, case.npix, case.pix0
        for key in ("act", "len", "dsd"):
            A[key] = tiled(case, bases, key, (K,))
        A["idx"] = tiled(case, bases, "idx", (K,), torch.int32)
        A["cnt"] = lit_counts(case, bases)
        A["weight"] = torch.empty((npix, K), device=DEV)
        A["valid"] = torch.empty((npix,), dtype=torch.int64, device=DEV)
        assert A["idx"].numel() >= ls.SLOT_GATE

        def fwd(d, n_, w, v):
            rc = lib.voge_composite_fwd(p(d["idx"]), p(d["cnt"]), p(d["act"]), p(d["len"]), p(d["dsd"]), 1.0, n_, K, p(w), p(v), stream())
            assert rc == 0, rc
        small = []
        for b in range(3):
            w, v = torch.empty((pix0, K), device=DEV), torch.empty((pix0,), dtype=torch.int64, device=DEV)
            fwd(bases[b], pix0, w, v)
            close_on(f"{case.name} base {b} weights", n(w), bases[b]["ref"]["w"].detach().numpy(), bases[b]["same"])
            assert torch.equal(v, bases[b]["valid"])
            small.append((w, v))
        fwd(A, npix, A["weight"], A["valid"])
        assert_tiles_equal(f"{case.name} weights", A["weight"], [s[0] for s in small], pix0, T)
        assert_tiles_equal(f"{case.name} valid_num", A["valid"], [s[1] for s in small], pix0, T)
        if not with_bwd:
            return
        from oracle import torch_ref
        G = [ls.upstream(case, b, "weight") * bases[b]["same"][:, None] for b in range(3)]
        A["g_weight"] = tiled(case, bases, None, (K,), src=[t(g) for g in G])
        for key in ("g_act", "g_len", "g_dsd"):
            A[key] = torch.empty((npix, K), device=DEV)

        def bwd(d, w, gw, n_, outs):
            rc = lib.voge_composite_bwd(p(d["act"]), p(d["len"]), p(d["dsd"]), p(w), p(d["cnt"]), p(gw), 1.0, n_, K, *[p(o) for o in outs], stream())
            assert rc == 0, rc
        smallg = []
        for b in range(3):
            outs = [torch.empty((pix0, K), device=DEV) for _ in range(3)]
            bwd(bases[b], small[b][0], t(G[b]), pix0, outs)
            ref = bases[b]["ref"]
            leaves = [ref[k].detach().clone().requires_grad_(True) for k in ("act", "len", "dsd")]
            w64, _ = torch_ref.aggregation(ref["idx"], leaves[0], leaves[1], leaves[2], 1.0)
            (w64 * torch.tensor(G[b], dtype=torch.float64)).sum().backward()
            live = (np.arange(K)[None] < ref["vn"].numpy()[:, None]) & bases[b]["same"][:, None]
            for o, leaf, what in zip(outs, leaves, ("g_act", "g_len", "g_dsd")):
                close_on(f"{case.name} base {b} {what}", np.where(live, n(o), 0.0), np.where(live, leaf.grad.numpy(), 0.0), bases[b]["same"])
            smallg.append(outs)
        bwd(A, A["weight"], A["g_weight"], npix, [A["g_act"], A["g_len"], A["g_dsd"]])
        for i, what in enumerate(("g_act", "g_len", "g_dsd")):
            assert_tiles_equal(f"{case.name} {what}", A[what], [s[i] for s in smallg], pix0, T)
    return body


@pytest.mark.parametrize("name", ["composite_K4", "composite_K130"])
def test_composite_from_act_dsd_at_2_30_slots(hip_lib, monkeypatch, name):
    case = ls.CASES[name]
    calls = spy(monkeypatch, hip_lib, ["voge_composite_fwd", "voge_composite_bwd"])
    run_case(case, _composite_body(hip_lib, name == "composite_K4"))      # (the backward's three more outputs fit the cap at K = 4: run there)
    big = [(nm, a) for nm, a in calls if a[6 if nm == "voge_composite_fwd" else 7] == case.npix]
    assert [nm for nm, _ in big] == list(case.entries), [nm for nm, _ in calls]
    assert all(a[7 if nm == "voge_composite_fwd" else 8] == case.K for nm, a in big)


# ---- 2, 3, 5, 8. the forward from the records, its largest 32-bit launch, the consumers, the one-pass shade --------------------
def _distortion64(w, ln, vn):
    K = w.shape[-1]
    live = (torch.arange(K)[None] < vn[:, None]).to(w.dtype)
    wl, tl = w * live, torch.where(live > 0, ln, torch.zeros_like(ln))
    return (wl[:, :, None] * wl[:, None, :] * (tl[:, :, None] - tl[:, None, :]).abs()).sum((1, 2))


def test_forward_from_records_consumers_and_one_pass_shade_at_2_30_slots(hip_lib, monkeypatch):
    from oracle import torch_ref
    from voge_amd import ops
    case, short = ls.CASES["records_K256"], ls.CASES["records_K256_short"]
    lib = hip_lib
    calls = spy(monkeypatch, lib, list(case.entries))
    C, bg = case.C, t(ls.BACKGROUND[:case.C])

    def body(case, A, bases):
        K, T, npix, pix0, P = case.K, case.T, case.npix, case.pix0, case.P
        A["idx"] = tiled(case, bases, "idx", (K,), torch.int32, offset=ls.P0)
        A["len"] = tiled(case, bases, "len", (K,))
        A["cnt"] = lit_counts(case, bases)
        A["rays"] = tiled(case, bases, "rays", (3,))
        A["records"] = tiled(case, bases, "records", (4,), per="gauss")
        A["colors"] = tiled(case, bases, None, (C,), src=[bases[b]["colors"][:, :C].contiguous() for b in range(3)], per="gauss")
        A["weight"] = torch.empty((npix, K), device=DEV)
        A["weight2"] = torch.full((npix, K), 7.0, device=DEV)
        A["valid"] = torch.empty((npix,), dtype=torch.int64, device=DEV)
        assert int(A["idx"].max()) == P - 1 or int(A["idx"].max()) >= P - ls.P0

        def fwd(d, recs, n_, w, v):
            rc = lib.voge_composite_fwd_iso(p(d["idx"]), p(d["cnt"]), p(d["len"]), p(recs), p(d["rays"]), 1.0, n_, K, p(w), p(v), stream())
            assert rc == 0, rc
        small = []
        for b in range(3):
            w, v = torch.empty((pix0, K), device=DEV), torch.empty((pix0,), dtype=torch.int64, device=DEV)
            fwd(bases[b], bases[b]["records"], pix0, w, v)
            close_on(f"{case.name} base {b} weights from the records", n(w), bases[b]["ref"]["w"].detach().numpy(), bases[b]["same"])
            small.append((w, v))
        # case 2: 2^30 slots, the size_t form
        fwd(A, A["records"], npix, A["weight"], A["valid"])
        assert_tiles_equal(f"{case.name} weights", A["weight"], [s[0] for s in small], pix0, T)
        assert_tiles_equal(f"{case.name} valid_num", A["valid"], [s[1] for s in small], pix0, T)
        # case 5: one tile short, the 32-bit form's largest launch, into a buffer whose last tile must stay as it was
        fwd(A, A["records"], short.npix, A["weight2"], A["valid"])
        assert_tiles_equal(f"{short.name} weights", A["weight2"], [s[0] for s in small], pix0, short.T)
        assert bool((A["weight2"][short.npix:] == 7.0).all()), f"{short.name}: wrote past its last pixel"
        log_line(f"[large shapes] {short.name}: {short.arm}; {short.slots} slots, {short.npix} pixels, last byte offset {short.slots * 4 - 1}")
        # case 8: the consumers on the 2^30-slot fragments, forwards (merge rewrites the index list: it runs after the others)
        refs = [bases[b]["ref"] for b in range(3)]
        col64 = [torch.tensor(bases[b]["tile"]["colors"][:, :C], dtype=torch.float64) for b in range(3)]
        bg64 = torch.tensor(ls.BACKGROUND[:C], dtype=torch.float64)
        w64 = [r["w"].detach() for r in refs]
        merged64 = [torch_ref.merge_final(col64[b], w64[b], refs[b]["vn"], refs[b]["idx"]) for b in range(3)]
        depth64 = [ls.oracle_outputs(refs[b], "depth")[0].detach() for b in range(3)]
        consumers = [
            ("get_silhouette", lambda d, w, rgb: ops.silhouette(w), [torch.minimum(w64[b].sum(-1), torch.ones((), dtype=torch.float64)) for b in range(3)]),
            ("get_depth", lambda d, w, rgb: ops.depth(w, d["len"], d["valid"], True, 0.0), depth64),
            ("get_distortion", lambda d, w, rgb: ops.distortion(w, d["len"], d["valid"], False),
             [_distortion64(w64[b], refs[b]["len"].detach(), refs[b]["vn"]) for b in range(3)]),
            ("interpolate_attr", lambda d, w, rgb: ops.merge(d["colors"], w, d["idx"], d["valid"]), merged64),
            ("to_colored_background", lambda d, w, rgb: ops.blend(rgb, w, bg, -1.0),
             [torch_ref.to_colored_background(merged64[b], w64[b], bg64) for b in range(3)]),
        ]
        sm = [dict(idx=bases[b]["idx"].clone(), len=bases[b]["len"], valid=small[b][1], colors=bases[b]["colors"][:, :C].contiguous()) for b in range(3)]
        rgb_small, rgb_big = [None] * 3, None
        with torch.no_grad():
            for what, fn, want in consumers:
                outs = []
                for b in range(3):
                    o = fn(sm[b], small[b][0], rgb_small[b])
                    close_on(f"{case.name} base {b} {what}", n(o), want[b].numpy(), bases[b]["same"])
                    outs.append(o)
                A[what] = fn(A, A["weight"], rgb_big)
                assert_tiles_equal(f"{case.name} {what}", A[what], outs, pix0, T)
                if what == "interpolate_attr":
                    rgb_small, rgb_big = outs, A[what]
        # case 3: the one-pass composite + shade, C = 3: not the FRAME form at this size; weights, rgb, weight sum and image
        def shade(d, recs, cols, n_, nattr, w, v, rgb, img, ws):
            rc = lib.voge_composite_shade_fwd_iso(p(d["idx"]), p(d["cnt"]), p(d["len"]), p(recs), p(d["rays"]), 1.0, p(cols), p(bg), -1.0, n_, K, C,
                                                  nattr, p(w), p(v), p(rgb), p(img), p(ws), stream())
            assert rc == 0, rc
        sh_small = []
        for b in range(3):
            o = dict(w=torch.empty((pix0, K), device=DEV), v=torch.empty((pix0,), dtype=torch.int64, device=DEV), rgb=torch.empty((pix0, C), device=DEV),
                     img=torch.empty((pix0, C), device=DEV), ws=torch.empty((pix0,), device=DEV))
            d = dict(bases[b], idx=bases[b]["idx"].clone())
            shade(d, bases[b]["records"], sm[b]["colors"], pix0, ls.P0, o["w"], o["v"], o["rgb"], o["img"], o["ws"])
            assert torch.equal(o["w"], small[b][0]), f"base {b}: the one-pass weights differ from the composite's"
            close_on(f"{case.name} base {b} one-pass image", n(o["img"]), torch_ref.to_colored_background(merged64[b], w64[b], bg64).numpy(), bases[b]["same"])
            close_on(f"{case.name} base {b} one-pass rgb", n(o["rgb"]), merged64[b].numpy(), bases[b]["same"])
            close_on(f"{case.name} base {b} one-pass weight sum", n(o["ws"]), w64[b].sum(-1).numpy(), bases[b]["same"])
            sh_small.append(o)
        A["rgb"], A["img"], A["wsum"] = torch.empty((npix, C), device=DEV), torch.empty((npix, C), device=DEV), torch.empty((npix,), device=DEV)
        shade(A, A["records"], A["colors"], npix, P, A["weight2"], A["valid"], A["rgb"], A["img"], A["wsum"])
        assert torch.equal(A["weight2"], A["weight"]), f"{case.name}: the one-pass weights differ from the composite's at the large shape"
        for key, k2 in (("rgb", "rgb"), ("img", "img"), ("wsum", "ws"), ("valid", "v")):
            assert_tiles_equal(f"{case.name} one-pass {key}", A[key], [o[k2] for o in sh_small], pix0, T)
        assert int(A["idx"].min()) == 0      # (merge_final's rewrite of the empty slots, -1 -> 0)
    run_case(case, body)
    big = [(nm, a) for nm, a in calls if case.npix in a or short.npix in a]
    assert [nm for nm, _ in big] == ["voge_composite_fwd_iso", "voge_composite_fwd_iso", "voge_silhouette_fwd", "voge_depth_fwd", "voge_distortion_fwd",
                                     "voge_merge_fwd", "voge_blend_fwd", "voge_composite_shade_fwd_iso"], [nm for nm, _ in calls]
    assert big[0][1][6:8] == (case.npix, case.K) and big[1][1][6:8] == (short.npix, case.K) and big[-1][1][9:13] == (case.npix, case.K, 3, case.P)


# ---- 4 - 6. the fused backward ---------------------------------------------------------------------------------------------------
def _fb_common(case, A, bases, T, weight=True):
    K = case.K
    A["idx"] = tiled(case, bases, "idx", (K,), torch.int32, offset=ls.P0)
    A["len"] = tiled(case, bases, "len", (K,))
    if weight:      # (the one-pass forms tile the weights of their own forward instead)
        A["weight"] = tiled(case, bases, "weight", (K,))
    A["cnt"] = lit_counts(case, bases)
    A["rays"] = tiled(case, bases, "rays", (3,))
    if case.form == "scalar":
        A["records"] = tiled(case, bases, "records", (4,), per="gauss")
        A["p1"] = tiled(case, bases, "p1", (), per="gauss")
        A["g1"] = torch.full((case.P,), 7.0, device=DEV)
    else:
        A["mus"] = tiled(case, bases, "mus", (3,), per="gauss")
        A["p1"] = tiled(case, bases, "p1", (3, 3), per="gauss")
        A["g1"] = torch.full((case.P, 3, 3), 7.0, device=DEV)
    A["g0"] = torch.full((case.P, 3), 7.0, device=DEV)
    A["ws"] = torch.empty((case.P * 112,), dtype=torch.uint8, device=DEV)


def _fb_weights_call(lib, calls, case, d, g, P, nrows, with_ad, ws, g0, g1):
    K = case.K
    common = dict(rays=p(d["rays"]), idx=p(d["idx"]), cnt=p(d["cnt"]), weight=p(d["weight"]), act=p(d["act"]) if with_ad else None, len=p(d["len"]),
                  dsd=p(d["dsd"]) if with_ad else None, g=p(g), gs0=K, gs1=1, g_hitlen=None, occ=1.0, nrows=nrows, W=case.W0, K=K, ws=p(ws),
                  ws_bytes=ws.numel(), g_verts=p(g0), g_sigmas=p(g1), stream=stream())
    if case.form == "scalar":
        entry(lib, calls, "voge_fragment_bwd_iso", records=p(d["records"]), sigmas=p(d["p1"]), shared=0, sigma_mode=0, B=1, N=P, **common)
    else:
        entry(lib, calls, "voge_fragment_bwd", mus=p(d["mus"]), isigmas=p(d["p1"]), P=P, **common)


def _small_ws():
    return torch.empty((ls.P0 * 112,), dtype=torch.uint8, device=DEV)


def _fb_weights(lib, calls, case, shorter=None):
    """The weights' own gradient at the large shape (and, `shorter`, again on the first tiles of the same arrays)."""
    def body(case, A, bases):
        K, T = case.K, case.T
        ref = [ls.oracle_gradients(case, b, bases[b]["same"]) for b in range(3)]
        _fb_common(case, A, bases, T)
        if case.keep_ad:
            A["act"], A["dsd"] = tiled(case, bases, "act", (K,)), tiled(case, bases, "dsd", (K,))
        A["g"] = tiled(case, bases, None, (K,), src=[t(r["G"][0]) for r in ref])
        assert A["idx"].numel() >= ls.SLOT_GATE or case.lit == "ends"
        for b in range(3):      # the small call of the same entry against the oracle
            g0, g1 = torch.empty_like(bases[b]["mus"]), torch.empty_like(bases[b]["p1"])
            _fb_weights_call(lib, [], case, bases[b], t(ref[b]["G"][0]), ls.P0, case.H0, case.keep_ad, _small_ws(), g0, g1)
            grad_close(f"[large shapes] {case.name} base {b} small call, means", n(g0), ref[b]["grads"]["mus"], TOL)
            grad_close(f"[large shapes] {case.name} base {b} small call, second parameter", n(g1), ref[b]["grads"]["p1"], TOL)
        for c in [case] + ([shorter] if shorter else []):
            A["g0"].fill_(7.0)
            A["g1"].fill_(7.0)
            _fb_weights_call(lib, calls, case, A, A["g"], case.P, c.T * c.H0, case.keep_ad, A["ws"], A["g0"], A["g1"])
            tiles = None if c.lit == "all" else c.lit_tiles()
            e0 = tiles_grad_close(f"{c.name} means", A["g0"], [r["grads"]["mus"] for r in ref], TOL, c.T, tiles, dark_zero=True)
            e1 = tiles_grad_close(f"{c.name} second parameter", A["g1"], [r["grads"]["p1"] for r in ref], TOL, c.T, tiles, dark_zero=True)
            if c.T < case.T:      # the Gaussians of the tiles behind the launch's last row: written, and zero
                assert float(A["g0"][c.T * ls.P0:].abs().max()) == 0.0 and float(A["g1"][c.T * ls.P0:].abs().max()) == 0.0, c.name
            log_line(f"[large shapes] {c.name}: {c.arm}; {c.slots} slots, {c.npix} pixels; largest scaled gradient error {max(e0, e1):.2e} (tolerance {TOL:.1e})")
    return body


@pytest.mark.parametrize("name,short", [("fb_weights_K256", "fb_weights_K256_short"), ("fb_weights_K5_full_ad", None)])
def test_fused_backward_weights_form_at_2_30_slots(hip_lib, name, short):
    case, calls = ls.CASES[name], []
    run_case(case, _fb_weights(hip_lib, calls, case, ls.CASES[short] if short else None))
    want = case.entries[0]
    assert [nm for nm, _ in calls] == [want] * (2 if short else 1)
    a = calls[0][1]
    assert a["K"] == case.K and a["W"] == case.W0 and a["nrows"] == case.nrows and a.get("P", a.get("N")) == case.P
    assert (a["act"] is not None) == case.keep_ad and a["nrows"] * a["W"] * a["K"] >= ls.SLOT_GATE
    if short:
        assert calls[1][1]["nrows"] * case.W0 * case.K < ls.SLOT_GATE <= (calls[1][1]["nrows"] + case.H0) * case.W0 * case.K


def _shade_body(lib, calls):
    def body(case, A, bases):
        K, C, T, pix0 = case.K, case.C, case.T, case.pix0
        bg = t(ls.BACKGROUND[:C])
        ref = [ls.oracle_gradients(case, b, bases[b]["same"]) for b in range(3)]
        fw = []
        for b in range(3):      # the forward's image, merged colours and weight sums: the one-pass entry at the small shape
            o = dict(w=torch.empty((pix0, K), device=DEV), v=torch.empty((pix0,), dtype=torch.int64, device=DEV), rgb=torch.empty((pix0, C), device=DEV),
                     img=torch.empty((pix0, C), device=DEV), ws=torch.empty((pix0,), device=DEV), colors=bases[b]["colors"][:, :C].contiguous())
            rc = lib.voge_composite_shade_fwd_iso(p(bases[b]["idx"].clone()), p(bases[b]["cnt"]), p(bases[b]["len"]), p(bases[b]["records"]),
                                                  p(bases[b]["rays"]), 1.0, p(o["colors"]), p(bg), -1.0, pix0, K, C, ls.P0, p(o["w"]), p(o["v"]),
                                                  p(o["rgb"]), p(o["img"]), p(o["ws"]), stream())
            assert rc == 0, rc
            close_on(f"{case.name} base {b} image", n(o["img"]), ref[b]["outs"][0], bases[b]["same"])
            fw.append(o)
        _fb_common(case, A, bases, T, weight=False)
        A["weight"] = tiled(case, bases, None, (K,), src=[o["w"] for o in fw])
        A["rgb"] = tiled(case, bases, None, (C,), src=[o["rgb"] for o in fw])
        A["wsum"] = tiled(case, bases, None, (), src=[o["ws"] for o in fw])
        A["colors"] = tiled(case, bases, None, (C,), src=[o["colors"] for o in fw], per="gauss")
        A["g"] = tiled(case, bases, None, (C,), src=[t(r["G"][0]) for r in ref])
        A["g_attr"] = torch.full((case.P, C), 7.0, device=DEV)

        def call(cl, d, o, g, P, nrows, ws, g0, g1, ga):
            entry(lib, cl, "voge_fragment_shade_bwd_iso", records=p(d["records"]), sigmas=p(d["p1"]), shared=0, sigma_mode=0, rays=p(d["rays"]),
                  attr=p(o["colors"]), idx=p(d["idx"]), cnt=p(d["cnt"]), weight=p(o["weight"]), act=None, len=p(d["len"]), dsd=None, rgb=p(o["rgb"]),
                  wsum=p(o["wsum"]), bg=p(bg), thr=-1.0, g=p(g), gs0=C, gs1=1, occ=1.0, B=1, N=P, nrows=nrows, W=case.W0, K=K, C=C, Nattr=P,
                  ws=p(ws), ws_bytes=ws.numel(), g_verts=p(g0), g_sigmas=p(g1), g_attr=p(ga), stream=stream())
        for b in range(3):
            g0, g1, ga = torch.empty_like(bases[b]["mus"]), torch.empty_like(bases[b]["p1"]), torch.empty((ls.P0, C), device=DEV)
            call([], bases[b], dict(colors=fw[b]["colors"], weight=fw[b]["w"], rgb=fw[b]["rgb"], wsum=fw[b]["ws"]), t(ref[b]["G"][0]), ls.P0, case.H0,
                 _small_ws(), g0, g1, ga)
            for what, got in (("mus", g0), ("p1", g1), ("colors", ga)):
                grad_close(f"[large shapes] {case.name} base {b} small call, {what}", n(got), ref[b]["grads"][what], TOL)
        call(calls, A, A, A["g"], case.P, case.nrows, A["ws"], A["g0"], A["g1"], A["g_attr"])
        tiles = None if case.lit == "all" else case.lit_tiles()
        errs = [tiles_grad_close(f"{case.name} {what}", A[key], [r["grads"][what] for r in ref], TOL, T, tiles, dark_zero=True)
                for what, key in (("mus", "g0"), ("p1", "g1"), ("colors", "g_attr"))]
        log_line(f"[large shapes] {case.name}: largest scaled gradient error {max(errs):.2e} (tolerance {TOL:.1e})")
    return body


def test_fused_backward_shade_form_at_2_30_slots(hip_lib):
    case, calls = ls.CASES["fb_shade_K128_C3"], []
    run_case(case, _shade_body(hip_lib, calls))
    assert [nm for nm, _ in calls] == ["voge_fragment_shade_bwd_iso"]
    a = calls[0][1]
    assert (a["K"], a["C"], a["W"], a["nrows"], a["N"], a["Nattr"]) == (128, 3, case.W0, case.nrows, case.P, case.P) and a["act"] is None


def test_fused_backward_depth_form_at_2_30_slots(hip_lib):
    case, calls, lib = ls.CASES["fb_depth_K128"], [], hip_lib
    tol = 0.25 * TOL      # (the one-pass depth's bound: tests/test_gpu_fragment_bwd_entries.py)

    def body(case, A, bases):
        K, T, pix0 = case.K, case.T, case.pix0
        ref = [ls.oracle_gradients(case, b, bases[b]["same"]) for b in range(3)]
        fw = []
        for b in range(3):      # get_depth's one-pass forward at the small shape
            o = dict(w=torch.empty((pix0, K), device=DEV), v=torch.empty((pix0,), dtype=torch.int64, device=DEV), depth=torch.empty((pix0,), device=DEV),
                     ws=torch.empty((pix0,), device=DEV), sil=torch.empty((pix0,), device=DEV))
            rc = lib.voge_frame_depth_fwd_iso(p(bases[b]["idx"]), p(bases[b]["cnt"]), p(bases[b]["len"]), p(bases[b]["records"]), p(bases[b]["rays"]), 1.0,
                                              1, 0.0, pix0, K, p(o["w"]), p(o["v"]), p(o["depth"]), p(o["ws"]), p(o["sil"]), None, 0, stream())
            assert rc == 0, rc
            close_on(f"{case.name} base {b} depth", n(o["depth"]), ref[b]["outs"][0], bases[b]["same"], tol)
            close_on(f"{case.name} base {b} silhouette", n(o["sil"]), ref[b]["outs"][1], bases[b]["same"], tol)
            fw.append(o)
        _fb_common(case, A, bases, T, weight=False)
        A["weight"] = tiled(case, bases, None, (K,), src=[o["w"] for o in fw])
        A["depth"] = tiled(case, bases, None, (), src=[o["depth"] for o in fw])
        A["wsum"] = tiled(case, bases, None, (), src=[o["ws"] for o in fw])
        A["g"] = tiled(case, bases, None, (), src=[t(r["G"][0]) for r in ref])
        A["g_sil"] = tiled(case, bases, None, (), src=[t(r["G"][1]) for r in ref])

        def call(cl, d, o, g, gs, P, nrows, acc, g0, g1):
            entry(lib, cl, "voge_frame_depth_bwd_iso", records=p(d["records"]), sigmas=p(d["p1"]), shared=0, sigma_mode=0, rays=p(d["rays"]), idx=p(d["idx"]),
                  cnt=p(d["cnt"]), weight=p(o["weight"]), len=p(d["len"]), depth=p(o["depth"]), wsum=p(o["wsum"]), g=p(g), gs0=1, g_sil=p(gs),
                  normalize=1, occ=1.0, B=1, N=P, nrows=nrows, W=case.W0, K=K, ws=p(acc), ws_bytes=acc.numel() * 4, g_verts=p(g0), g_sigmas=p(g1),
                  stream=stream())
        for b in range(3):
            g0, g1 = torch.empty_like(bases[b]["mus"]), torch.empty_like(bases[b]["p1"])
            call([], bases[b], dict(weight=fw[b]["w"], depth=fw[b]["depth"], wsum=fw[b]["ws"]), t(ref[b]["G"][0]), t(ref[b]["G"][1]), ls.P0, case.H0,
                 torch.zeros((ls.P0 * 4,), device=DEV), g0, g1)
            grad_close(f"[large shapes] {case.name} base {b} small call, means", n(g0), ref[b]["grads"]["mus"], tol)
            grad_close(f"[large shapes] {case.name} base {b} small call, a", n(g1), ref[b]["grads"]["p1"], tol)
        A["acc"] = torch.zeros((case.P * 4,), device=DEV)      # (the frame path's accumulator arrives zeroed)
        call(calls, A, A, A["g"], A["g_sil"], case.P, case.nrows, A["acc"], A["g0"], A["g1"])
        e0 = tiles_grad_close(f"{case.name} means", A["g0"], [r["grads"]["mus"] for r in ref], tol, T)
        e1 = tiles_grad_close(f"{case.name} a", A["g1"], [r["grads"]["p1"] for r in ref], tol, T)
        log_line(f"[large shapes] {case.name}: largest scaled gradient error {max(e0, e1):.2e} (tolerance {tol:.1e})")
    run_case(case, body)
    assert [nm for nm, _ in calls] == ["voge_frame_depth_bwd_iso"] and calls[0][1]["nrows"] == case.nrows and calls[0][1]["K"] == 128


# ---- 6. the gate: few slots, very many pixels ------------------------------------------------------------------------------------
def test_gate_one_slot_lists_past_the_rays_32_bit_range(hip_lib, monkeypatch):
    """K = 1 and more than 2^32 / 12 pixels: the ray of a pixel in the last tiles lies past byte 2^32 while npix * K is far below
    2^30.  The fused backward (weights form) and the composite from the records, at that shape and at the largest one whose rays
    still fit 32 bits; hit counts are zero but in the first tile and the last four."""
    case, short, lib = ls.CASES["gate_fb_weights_K1"], ls.CASES["gate_fb_weights_K1_short"], hip_lib
    calls = []
    comp = spy(monkeypatch, lib, ["voge_composite_fwd_iso"])
    fb = _fb_weights(lib, calls, case, short)

    def body(case, A, bases):
        K, pix0 = case.K, case.pix0
        # every wrapped offset stays inside its array: it is smaller than the offset it stands for
        assert (case.npix * 12) % ls.U32 < case.npix * 12 and case.npix * 12 < 2 * ls.U32
        fb(case, A, bases)
        A["w_out"] = torch.full((case.npix, K), 7.0, device=DEV)
        A["valid"] = torch.full((case.npix,), -7, dtype=torch.int64, device=DEV)
        small = []
        for b in range(3):
            w, v = torch.empty((pix0, K), device=DEV), torch.empty((pix0,), dtype=torch.int64, device=DEV)
            assert lib.voge_composite_fwd_iso(p(bases[b]["idx"]), p(bases[b]["cnt"]), p(bases[b]["len"]), p(bases[b]["records"]), p(bases[b]["rays"]), 1.0,
                                              pix0, K, p(w), p(v), stream()) == 0
            close_on(f"{case.name} base {b} weights from the records", n(w), bases[b]["ref"]["w"].detach().numpy(), bases[b]["same"])
            small.append((w, v))
        for c in (case, short):
            A["w_out"].fill_(7.0)
            assert lib.voge_composite_fwd_iso(p(A["idx"]), p(A["cnt"]), p(A["len"]), p(A["records"]), p(A["rays"]), 1.0, c.npix, K, p(A["w_out"]),
                                              p(A["valid"]), stream()) == 0
            assert_tiles_equal(f"{c.name} composite weights", A["w_out"], [s[0] for s in small], pix0, c.T, c.lit_tiles())
            assert_tiles_equal(f"{c.name} composite valid_num", A["valid"], [s[1] for s in small], pix0, c.T, c.lit_tiles())
            dark = torch.ones(c.T, dtype=torch.bool, device=DEV)
            dark[c.lit_tiles()] = False
            assert float(A["w_out"].view(-1, pix0)[:c.T][dark].abs().max()) == 0.0 and bool((A["w_out"][c.npix:] == 7.0).all()), c.name
    run_case(case, body)
    assert [nm for nm, _ in calls] == ["voge_fragment_bwd_iso"] * 2 and [c_[1]["nrows"] for c_ in calls] == [case.nrows, short.nrows]
    assert [a[6] for _, a in comp if a[6] > case.pix0] == [case.npix, short.npix]
    assert calls[0][1]["nrows"] * case.W0 > ls.PIX_GATE + case.pix0 and calls[1][1]["nrows"] * case.W0 * 12 <= ls.U32


def test_gate_three_slot_lists_past_the_rgb_32_bit_range(hip_lib):
    """K = 3, C = 4 with a background, npix just below 2^30 / 3: the forward's rgb of a pixel past 2^28 lies past byte 2^32."""
    case, calls = ls.CASES["gate_fb_shade_K3_C4"], []
    assert (case.npix * 16) % ls.U32 < case.npix * 16      # a wrapped rgb offset stays inside the array
    run_case(case, _shade_body(hip_lib, calls))
    a = calls[0][1]
    assert (a["K"], a["C"], a["nrows"]) == (3, 4, case.nrows) and a["bg"] is not None and a["nrows"] * a["W"] * 3 < ls.SLOT_GATE


# ---- 7. the sweep's plain-store epilogue ----------------------------------------------------------------------------------------
def _delta_of(tb, tc):
    """trace_bound_cases.case_delta's figure for a bundle of our own: the relative width of the band around a decision (the K-th
    len, the threshold) inside which the kernels' fp32 evaluation may decide otherwise, from the error bound over ALL pairs."""
    d = tc.rays.astype(np.float64).reshape(-1, 3)
    T = tb.pair_terms(tc, d[:, None, :], np.arange(tc.N)[None, :])
    with np.errstate(all="ignore"):
        hit = np.isfinite(T["len"]) & np.isfinite(T["act"]) & (np.abs(T["len"]) < 2e10)
        near = hit & (T["act"] < 2 * tc.thr_act)
        band = near & (T["act"] > tc.thr_act / 2)
        d_len = float((2 * T["b_len"][near] / np.maximum(1.0, np.abs(T["len"][near]))).max()) if near.any() else 0.0
        d_act = float((T["b_act"][band] / tc.thr_act).max()) if band.any() else 0.0
    return max(d_len, d_act, 2.0 ** -20)


def _sweep_scene(case):
    """About 300 Gaussians shared by every tile, and three base bundles of width 64."""
    tiles = ls.case_bases(case)
    return tiles[0]["mus"], tiles[0]["a"], [tl["rays"] for tl in tiles]


@pytest.mark.parametrize("name,keep", [("sweep_W262144", False), ("sweep_W262144", True), ("sweep_W262080", False)])
def test_sweep_epilogue_on_both_sides_of_its_store_switch(hip_lib, monkeypatch, name, keep):
    import trace_bound_cases as tb
    from voge_amd import ops
    case, lib = ls.CASES[name], hip_lib
    K, H0, W0, T = case.K, case.H0, case.W0, case.T
    mus_np, a_np, rays_np = _sweep_scene(case)
    mus, a = t(mus_np), t(a_np)
    calls = spy(monkeypatch, lib, ["voge_fragments_fwd_iso", "voge_trace_topk_fwd_iso"])

    def trace(rays):
        with torch.no_grad():
            if keep:
                idx, ln, act, dsd = ops._RayTraceVoGEIso.apply(mus, a, rays, None, ls.THR_ACT, K)
                return idx, ln, ops.hit_count_of(idx), act, dsd
            idx, ln, cnt, _ = ops._TraceLean.apply(1, mus, a, None, rays, None, ls.THR_ACT, K, 0)
            return idx, ln, cnt, None, None

    def body(case, A, bases_unused):
        small = []
        for b in range(3):
            got = trace(t(rays_np[b])[None])
            # (what trace_bound_cases' bound and oracle read of a case: the Gaussians, the bundle)
            tc = types.SimpleNamespace(mus=mus_np, a=a_np, A=None, rays=rays_np[b][None], N=ls.P0, thr_act=ls.THR_ACT,
                                       isigmas=lambda: (a_np[:, None, None] * np.eye(3, dtype=np.float32)[None]).astype(np.float32))
            delta = _delta_of(tb, tc)
            assert delta <= 1e-4
            compare_trace_strict(tuple(None if x is None else n(x) for x in (got[0], got[1], got[3], got[4], got[2])), tb.oracle_fn(tc), K, ls.THR_ACT,
                                 delta, tb.CAP, f"{case.name} base {b}" + (", act / dsd kept" if keep else ""), bounds=tb.bounds_fn(tc),
                                 n_per_batch=ls.P0)
            small.append(got)
        A["rays"] = torch.empty((1, H0, T * W0, 3), device=DEV)
        ls.fill_tiles(ls.tiles_view(A["rays"][0], case, (3,)), [t(r) for r in rays_np])
        A["out"] = trace(A["rays"])
        names = ("idx", "len", "cnt", "act", "dsd")
        for i, what in enumerate(names):
            if A["out"][i] is None:
                continue
            tail = () if what == "cnt" else (K,)
            v = ls.tiles_view(A["out"][i][0], case, tail)
            for b in range(3):
                bad = (v[b::3] != small[b][i][0][None]).reshape(v[b::3].shape[0], -1).any(1)
                assert not bool(bad.any()), f"{case.name} {what}: {int(bad.sum())} tiles of base {b} differ from the 8 x 64 trace, the first at {int(torch.nonzero(bad)[0])}"

    run_case(case, body, with_bases=False)
    want = "voge_trace_topk_fwd_iso" if keep else "voge_fragments_fwd_iso"
    big = [a_ for nm, a_ in calls if nm == want and case.W in a_]
    assert len(big) == 1 and [nm for nm, _ in calls] == [want] * 4
    assert ls.sweep_write_through(case.W, K) == dict(case.sides)["sweep write-through"]
