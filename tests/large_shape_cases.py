"""The large-shape cases of tests/test_gpu_large_shapes.py: which entry each reaches, on which side of which host gate, how much
device memory it takes -- and the rule by which a large input is laid out from SMALL base tiles, so that the fp64 oracle
(oracle/torch_ref.py) only ever runs on a base tile.  Importable without a GPU (tests/test_large_shape_cases_cpu.py checks it).

The gates, restated from the host code:
  * composite.hip comp_plan / fragment_bwd.hip fb_launch: the 32-bit-offset instantiation (OffT = uint32_t) is taken when EVERY
    byte offset the kernel forms in OffT is below 2^32: npix * 4 K into the [pix][K] arrays, npix * 12 into the rays, npix * 4 C
    into the shade form's rgb (addressed through OffT only with a background), npix * 4 into cnt / wsum / bg.  Before this was
    written down the test was npix * K < 2^30 alone (old_narrow), which lets pix * 12 wrap for K <= 2 and pix * 16 for K = 3, C = 4.
  * comp_plan's FRAME form: a one-pass entry (shade / depth stage), K % 4 == 0 and the 32-bit form.
  * sweep_iso.h, the epilogue: write-through buffer stores while W * K < 2^26, plain stores from there on.

THREE different base tiles, not one.  Tile t of a large input is base t mod 3; the bases differ in seed, camera and hit counts
(0 .. K).  A read that a wrapped 32-bit offset displaces by a multiple of 2^32 bytes moves by 2^32 / tile_bytes tiles: a power of
two where the tile's bytes divide 2^32, no whole number of tiles otherwise -- never a multiple of 3 -- so it lands on ANOTHER base
and shows.  With identical tiles such a read would find the very bytes it should have read, and the wrap these cases exist to
catch would pass unseen.  Tile t also refers to its OWN Gaussians: live indices are offset by t * P0, and records, colours and
rays are tiled alike, so a gradient that lands in the wrong tile is seen and tile t's per-Gaussian sums stay comparable with the
base's reference.  (The sweep case shares its Gaussians between the tiles: it is one image.)

Tiles are stacked along the rows (nrows = T * H0, W = W0) for the entries that take (nrows, W), flat for those that take npix,
and along W for the sweep (base width a multiple of 8, the sweep's tile)."""
import math
from dataclasses import dataclass

import numpy as np

SLOT_GATE = 1 << 30      # npix * K (the test before the fix; still what "2^30 slots" means below)
SWEEP_GATE = 1 << 26     # W * K
U32 = 1 << 32
CAP_BYTES = 48 << 30     # no case may need more device memory than this
P_LIMIT = 1 << 26        # the entries' own limits: Gaussians ...
ATTR_LIMIT = 1 << 30     # ... and Nattr * C
THR_ACT = -math.log(0.01 + 1e-10)
NBASE = 3
P0 = 300                 # Gaussians per base tile: lists of 256 slots fill


# ---- the gates -------------------------------------------------------------------------------------------------------------------
def old_narrow(npix, K):
    return npix * K < SLOT_GATE


def fb_bytes_per_pixel(K, C=0, shade_bg=False):
    """The largest per-pixel stride fragment_bwd_kernel multiplies a pixel number by in OffT."""
    return max(4 * K, 12, 4 * C if shade_bg else 0)


def fb_narrow(npix, K, C=0, shade_bg=False):
    return npix * fb_bytes_per_pixel(K, C, shade_bg) < U32


def comp_narrow(npix, K, from_records):
    return npix * (12 if (from_records and K < 3) else 4 * K) < U32


def comp_frame(npix, K, onepass):
    return bool(onepass and K % 4 == 0 and comp_narrow(npix, K, True))


def sweep_write_through(W, K):
    return W * K < SWEEP_GATE


def byte_offsets(npix, K, C=0):
    """{array kind: one past the largest byte offset} of a launch -- what has to stay below 2^32 for the 32-bit form."""
    return {"slots": npix * K * 4, "rays": npix * 12, "rgb": npix * 4 * C, "per pixel": npix * 4}


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    entries: tuple          # the C entries it calls at the large shape
    arm: str                # the template arm it must reach
    K: int
    C: int                  # colour channels (0: none)
    form: str               # "scalar" | "full" records
    keep_ad: bool           # act / dsd kept and handed in
    H0: int
    W0: int
    T: int                  # tiles
    stack: str              # "rows" | "flat" | "W"
    arrays: tuple           # ((name, "slot" | "pix" | "gauss" | "once", bytes per element), ...): what is on the device at once
    sides: tuple            # ((gate name, the side it must fall on), ...)
    lit: str = "all"        # "all" | "ends": hit counts zero but in the first tile and the last `tail` ones
    tail: int = 2
    per_tile_gaussians: bool = True
    short_of: str = ""      # the case whose buffers it views (one tile less): no memory of its own
    smallest: bool = False  # T is the smallest count that reaches 2^30 slots
    gradients: bool = False
    shade_bg: bool = False

    @property
    def pix0(self):
        return self.H0 * self.W0

    @property
    def npix(self):
        return self.T * self.pix0

    @property
    def slots(self):
        return self.npix * self.K

    @property
    def P(self):
        return self.T * P0 if self.per_tile_gaussians else P0

    @property
    def nrows(self):
        return self.H0 if self.stack == "W" else self.T * self.H0

    @property
    def W(self):
        return self.T * self.W0 if self.stack == "W" else self.W0

    def need_bytes(self):
        """Device memory in bytes, summed from the case's arrays."""
        per = {"slot": self.slots, "pix": self.npix, "gauss": self.P, "once": 1}
        return sum(per[kind] * size for _, kind, size in self.arrays)

    def tile_bytes(self):
        """{array: bytes of one tile} of the arrays a wrapped offset could displace a read in."""
        out = {"slots": self.pix0 * self.K * 4, "rays": self.pix0 * 12, "per pixel": self.pix0 * 4}
        if self.C:
            out["rgb"] = self.pix0 * 4 * self.C
        return out

    def gates(self):
        """{gate name: the side the host code takes at this shape}."""
        onepass = "voge_composite_shade_fwd_iso" in self.entries
        return {
            "slots >= 2^30": self.slots >= SLOT_GATE,
            "old gate narrow": old_narrow(self.npix, self.K),
            "fused backward narrow": fb_narrow(self.npix, self.K, self.C, self.shade_bg),
            "composite from records narrow": comp_narrow(self.npix, self.K, True),
            "composite narrow": comp_narrow(self.npix, self.K, False),
            "frame form": comp_frame(self.npix, self.K, onepass),
            "sweep write-through": sweep_write_through(self.W, self.K),
        }

    def lit_tiles(self):
        return list(range(self.T)) if self.lit == "all" else [0] + list(range(self.T - self.tail, self.T))


def tiles_to_reach(K, pix0, slots=SLOT_GATE):
    return -(-slots // (K * pix0))


def _slot(*names):
    return tuple((n, "slot", 4) for n in names)


_PIX_IN = (("rays", "pix", 12), ("cnt", "pix", 4))
_GAUSS_ISO = (("records", "gauss", 16), ("a", "gauss", 4), ("workspace", "gauss", 112), ("g_mus", "gauss", 12), ("g_a", "gauss", 4))
PIX_GATE = -(-U32 // 12)      # 357 913 942: the first pixel whose ray offset pix * 12 does not fit 32 bits


def _cases():
    out = []
    WIDE = (("slots >= 2^30", True), ("old gate narrow", False))
    # 1. voge_composite_fwd / _bwd from act / dsd, at exactly 2^30 slots
    T = tiles_to_reach(4, 64 * 64)
    out.append(Case("composite_K4", ("voge_composite_fwd", "voge_composite_bwd"),
                    "compositen_kernel<0 | 2, NS 4 (fwd) | 2 (bwd), WAVE, size_t>; valid_num reaches byte 2^31", 4, 0, "scalar", True, 64, 64, T,
                    "flat", _slot("idx", "act", "len", "dsd", "weight", "g_weight", "g_act", "g_len", "g_dsd")
                    + (("cnt", "pix", 4), ("valid_num", "pix", 8)), WIDE + (("composite narrow", False),), per_tile_gaussians=False,
                    smallest=True))
    # (four slots per lane cannot leave the wave form at K <= 256 -- compn_lanes(256, 4) = 64 -- so the 256-thread workgroup form
    #  is reached through NS = 2: a K that is no multiple of 4 and above 128)
    T = tiles_to_reach(130, 8 * 32)
    out.append(Case("composite_K130", ("voge_composite_fwd",), "compositen_kernel<0, NS 2, 256-thread form, size_t>", 130, 0, "scalar", True,
                    8, 32, T, "flat", _slot("idx", "act", "len", "dsd", "weight") + (("cnt", "pix", 4), ("valid_num", "pix", 8)),
                    WIDE + (("composite narrow", False),), per_tile_gaussians=False, smallest=True))
    # 2, 3, 8. the forward from the records, the one-pass shade, and the consumers, on ONE set of arrays
    T = tiles_to_reach(256, 8 * 32)
    rec_arrays = (_slot("idx", "len", "weight", "weight (one-pass)") + _PIX_IN
                  + (("valid_num", "pix", 8), ("rgb", "pix", 12), ("img", "pix", 12), ("wsum", "pix", 4), ("consumer outputs", "pix", 12 + 8 + 8 + 8 + 12),
                     ("records", "gauss", 16), ("colours", "gauss", 12)))
    out.append(Case("records_K256", ("voge_composite_fwd_iso", "voge_composite_shade_fwd_iso", "voge_merge_fwd", "voge_silhouette_fwd",
                                     "voge_depth_fwd", "voge_distortion_fwd", "voge_blend_fwd"),
                    "compositen_kernel<0, NS 4, WAVE, size_t, SC 0 | 3> (not FRAME); the consumers' long indexing", 256, 3, "scalar", False,
                    8, 32, T, "flat", rec_arrays, WIDE + (("composite from records narrow", False), ("frame form", False)), smallest=True))
    out.append(Case("records_K256_short", ("voge_composite_fwd_iso",), "compositen_kernel<0, NS 4, WAVE, uint32_t>: its largest launch", 256, 0,
                    "scalar", False, 8, 32, T - 1, "flat", (), (("slots >= 2^30", False), ("composite from records narrow", True)),
                    short_of="records_K256"))
    # 4. the fused backward, size_t form
    fbw = _slot("idx", "weight", "len", "g_weight") + _PIX_IN + _GAUSS_ISO
    out.append(Case("fb_weights_K256", ("voge_fragment_bwd_iso",), "fragment_bwd_kernel<SRC 1, NS 4, size_t, ISO, NOAD>", 256, 0, "scalar", False,
                    8, 32, T, "rows", fbw, WIDE + (("fused backward narrow", False),), smallest=True, gradients=True))
    out.append(Case("fb_weights_K256_short", ("voge_fragment_bwd_iso",), "fragment_bwd_kernel<SRC 1, NS 4, uint32_t, ISO, NOAD>: its largest launch",
                    256, 0, "scalar", False, 8, 32, T - 1, "rows", (), (("slots >= 2^30", False), ("fused backward narrow", True)),
                    short_of="fb_weights_K256", gradients=True))
    T = tiles_to_reach(128, 8 * 32)
    out.append(Case("fb_shade_K128_C3", ("voge_fragment_shade_bwd_iso",), "fragment_bwd_kernel<SRC 0, C 3, NS 2, size_t, ISO, NOAD>", 128, 3, "scalar",
                    False, 8, 32, T, "rows", _slot("idx", "weight", "len") + _PIX_IN + (("rgb", "pix", 12), ("wsum", "pix", 4), ("g_img", "pix", 12))
                    + _GAUSS_ISO + (("colours", "gauss", 12), ("g_colours", "gauss", 12)), WIDE + (("fused backward narrow", False),),
                    smallest=True, gradients=True, shade_bg=True))
    T = tiles_to_reach(5, 50 * 64)
    out.append(Case("fb_weights_K5_full_ad", ("voge_fragment_bwd",),
                    "fragment_bwd_kernel<SRC 1, NS 2, size_t, !ISO, !NOAD>, vec == false: slot-by-slot loads at 2.1e8 pixels", 5, 0, "full", True,
                    50, 64, T, "rows", _slot("idx", "weight", "len", "act", "dsd", "g_weight") + _PIX_IN
                    + (("mus", "gauss", 12), ("isigmas", "gauss", 36), ("workspace", "gauss", 112), ("g_mus", "gauss", 12), ("g_isigmas", "gauss", 36)),
                    WIDE + (("fused backward narrow", False),), smallest=True, gradients=True))
    T = tiles_to_reach(128, 8 * 32)
    out.append(Case("fb_depth_K128", ("voge_frame_depth_bwd_iso",), "fragment_bwd_kernel<SRC 2, NS 2, size_t, ISO, NOAD>", 128, 0, "scalar", False,
                    8, 32, T, "rows", _slot("idx", "weight", "len") + _PIX_IN
                    + (("depth", "pix", 4), ("wsum", "pix", 4), ("g_depth", "pix", 4), ("g_sil", "pix", 4)) + _GAUSS_ISO,
                    WIDE + (("fused backward narrow", False),), smallest=True, gradients=True))
    # 6. the gate: few slots, very many pixels.  Lit: tile 0 and the last two tiles -- of the K = 1 case AND of its companion two
    # tiles shorter (the largest launch whose ray offsets fit 32 bits), which views the same arrays: four lit tiles at the end.
    pix0 = 32 * 1024
    T = -(-PIX_GATE // pix0) + 1      # the smallest tile multiple above 357 913 942, and one more tile
    gate = (("slots >= 2^30", False), ("old gate narrow", True))
    out.append(Case("gate_fb_weights_K1", ("voge_fragment_bwd_iso", "voge_composite_fwd_iso"),
                    "fragment_bwd_kernel<SRC 1, NS 2, size_t> and compositen_kernel<0, NS 2, WAVE, size_t>, where the old gate took uint32_t and pix * 12 wrapped",
                    1, 0, "scalar", False, 32, 1024, T, "rows", _slot("idx", "weight", "len", "g_weight", "weight (composite)") + _PIX_IN
                    + (("valid_num", "pix", 8),) + _GAUSS_ISO,
                    gate + (("fused backward narrow", False), ("composite from records narrow", False)), lit="ends", tail=4, gradients=True))
    out.append(Case("gate_fb_weights_K1_short", ("voge_fragment_bwd_iso", "voge_composite_fwd_iso"),
                    "the same two in the uint32_t form: the largest launch whose ray offsets fit", 1, 0, "scalar", False, 32, 1024, T - 2, "rows", (),
                    gate + (("fused backward narrow", True), ("composite from records narrow", True)), lit="ends",
                    short_of="gate_fb_weights_K1", gradients=True))
    T3 = (SLOT_GATE // 3) // pix0      # npix just below 2^30 / 3
    out.append(Case("gate_fb_shade_K3_C4", ("voge_fragment_shade_bwd_iso",),
                    "fragment_bwd_kernel<SRC 0, C 4, NS 2, size_t>, where the old gate took uint32_t and the rgb's pix * 16 wrapped", 3, 4, "scalar",
                    False, 32, 1024, T3, "rows", _slot("idx", "weight", "len") + _PIX_IN + (("rgb", "pix", 16), ("wsum", "pix", 4), ("g_img", "pix", 16))
                    + _GAUSS_ISO + (("colours", "gauss", 16), ("g_colours", "gauss", 16)), gate + (("fused backward narrow", False),), lit="ends",
                    gradients=True, shade_bg=True))
    # 7. the sweep's plain-store epilogue
    sweep = _slot("idx", "len", "act", "dsd") + _PIX_IN + (("trace workspace (voge_trace_workspace_bytes: 1476 bytes a pixel at this shape)", "pix", 1536),)
    out.append(Case("sweep_W262144", ("voge_fragments_fwd_iso", "voge_trace_topk_fwd_iso"), "sweep_iso.h epilogue, wt_ok == false: st16i<false> / st16f<false>",
                    256, 0, "scalar", True, 8, 64, SWEEP_GATE // 256 // 64, "W", sweep, (("sweep write-through", False),), per_tile_gaussians=False))
    out.append(Case("sweep_W262080", ("voge_fragments_fwd_iso",), "sweep_iso.h epilogue, wt_ok == true: the last width of the write-through stores", 256, 0,
                    "scalar", False, 8, 64, SWEEP_GATE // 256 // 64 - 1, "W", sweep, (("sweep write-through", True),), per_tile_gaussians=False))
    return out


CASES = {c.name: c for c in _cases()}


# ---- the base tiles --------------------------------------------------------------------------------------------------------------
def base_tile(b, K, H0, W0, form="scalar"):
    """Base b (0, 1, 2) of a case: P0 Gaussians around (0, 0, 4) seen from the origin, and an H0 x W0 bundle of unit rays wide
    enough that its outer pixels miss every Gaussian.  The bases differ in seed, focal length and principal point.
    -> dict(mus [P0,3], a [P0] | isigmas [P0,3,3], rays [H0,W0,3], colors [P0,4]) in fp32."""
    rng = np.random.default_rng(4000 + 97 * b + K)
    mus = (rng.uniform(-1, 1, (P0, 3)) * 0.45 + np.array([0.0, 0.0, 4.0])).astype(np.float32)
    r_lo, r_hi = (0.2, 0.32) if K <= 16 else (0.45, 0.9)      # long lists: nearly every Gaussian reaches the central rays
    r = rng.uniform(r_lo, r_hi, P0)
    s = 1.0 / (r * r / (2 * np.log(1 / 0.6)))
    tile = dict(mus=mus, colors=rng.uniform(0, 1, (P0, 4)).astype(np.float32))
    if form == "scalar":
        tile["a"] = (2.0 * s).astype(np.float32)
    else:
        L = np.tril(rng.uniform(-1, 1, (P0, 3, 3)))
        L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.5
        L = L * np.sqrt(s)[:, None, None] * 0.8
        tile["isigmas"] = (2.0 * (L @ L.transpose(0, 2, 1))).astype(np.float32)
    reach = 0.45 + (1.6 if form == "scalar" else 4.0) * r_hi      # act < THR_ACT within about 1.5 r of a centre (3x3 forms: their longest axis)
    half = 1.25 * reach / 4.0 * (1.0 + 0.12 * b)      # tan of the half field of view along x
    cx, cy = (W0 - 1) / 2.0 + (b - 1) * 0.11 * W0, (H0 - 1) / 2.0 + (1 - b) * 0.2 * H0
    x = (np.arange(W0) - cx) / (W0 / 2.0) * half
    y = (np.arange(H0) - cy) / (W0 / 2.0) * half * (2.0 if H0 * 4 <= W0 else 1.0)
    d = np.stack([np.broadcast_to(x[None, :], (H0, W0)), np.broadcast_to(y[:, None], (H0, W0)), np.ones((H0, W0))], -1)
    tile["rays"] = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    return tile


def case_bases(case):
    return [base_tile(b, case.K, case.H0, case.W0, case.form) for b in range(NBASE)]


def upstream(case, b, what):
    """The upstream gradient of base b's output `what` ("weight" [pix0,K] | "image" [pix0,C] | "pixel" [pix0]), fixed by the case."""
    rng = np.random.default_rng(9000 + 31 * b + case.K + {"weight": 0, "image": 1, "pixel": 2, "sil": 3}[what])
    shape = {"weight": (case.pix0, case.K), "image": (case.pix0, max(case.C, 1)), "pixel": (case.pix0,), "sil": (case.pix0,)}[what]
    return rng.normal(size=shape).astype(np.float32)


# ---- the tiling rule -------------------------------------------------------------------------------------------------------------
CHUNK = 1 << 26      # elements written per step of an offset fill (its temporaries stay a few hundred MB)


def fill_tiles(out, bases, offset=None, tiles=None):
    """out [T, ...] (a numpy array or a torch tensor, any strides) <- tile t = bases[t mod 3] (each shaped out.shape[1:]).  offset:
    an index array -- its live entries (>= 0) of tile t get t * offset added, its empty ones stay -1.  tiles: only those t."""
    is_np = isinstance(out, np.ndarray)
    T = out.shape[0]
    if tiles is not None:
        for t in tiles:
            src = bases[t % NBASE]
            if offset is None:
                out[t] = src
            else:
                out[t] = np.where(src >= 0, src + t * offset, -1) if is_np else _torch_where(src, t * offset)
        return out
    per = 1
    for s_ in out.shape[1:]:
        per *= int(s_)
    step = max(1, CHUNK // max(per, 1))
    for b in range(NBASE):
        n = len(range(b, T, NBASE))
        if n == 0:
            continue
        dst, src = out[b::NBASE], bases[b][None]
        if offset is None:
            dst[...] = src
            continue
        for i0 in range(0, n, step):
            i1 = min(n, i0 + step)
            if is_np:
                t = ((b + NBASE * np.arange(i0, i1)) * offset).reshape((-1,) + (1,) * (out.ndim - 1)).astype(src.dtype)
                dst[i0:i1] = np.where(src >= 0, src + t, -1)
            else:
                import torch
                t = ((b + NBASE * torch.arange(i0, i1, device=out.device)) * offset).reshape((-1,) + (1,) * (out.dim() - 1)).to(src.dtype)
                dst[i0:i1] = torch.where(src >= 0, src + t, torch.full_like(src, -1))
    return out


def _torch_where(src, add):
    import torch
    return torch.where(src >= 0, src + add, torch.full_like(src, -1))


def tiles_view(big, case, tail=()):
    """big (numpy | torch, the large array in the entry's own layout) as [T, ...tile shape..., *tail]: a view, never a copy.
    rows / flat: [T * pix0, *tail] -> [T, pix0, *tail]; W: [H0, T * W0, *tail] -> [T, H0, W0, *tail]."""
    tail = tuple(tail)
    if case.stack == "W":
        v = big.reshape((case.H0, -1, case.W0) + tail)
        return v.transpose((1, 0, 2) + tuple(range(3, 3 + len(tail)))) if isinstance(v, np.ndarray) else v.movedim(1, 0)
    return big.reshape((-1, case.pix0) + tail)


# ---- the fp64 oracle on a base tile ---------------------------------------------------------------------------------------------
def oracle_forward(tile, K):
    """fp64 torch_ref on one base tile -> dict(mus, p1 (leaves), idx, len, act, dsd, w, vn); pixels in row-major order."""
    import torch
    from oracle import torch_ref
    mus = torch.tensor(tile["mus"], dtype=torch.float64, requires_grad=True)
    if "a" in tile:
        p1 = torch.tensor(tile["a"], dtype=torch.float64, requires_grad=True)
        isg = p1[:, None, None] * torch.eye(3, dtype=torch.float64)
    else:
        p1 = torch.tensor(tile["isigmas"], dtype=torch.float64, requires_grad=True)
        isg = p1
    rays = torch.tensor(tile["rays"], dtype=torch.float64).reshape(-1, 3)
    idx, ln, act, dsd = torch_ref.trace_dense(mus, isg, rays, K, THR_ACT)
    w, vn = torch_ref.aggregation(idx, act, ln, dsd, 1.0)
    return dict(mus=mus, p1=p1, idx=idx, len=ln, act=act, dsd=dsd, w=w, vn=vn)


def oracle_outputs(ref, consumer, colors=None, bg=None):
    """The consumer's fp64 outputs on a base tile, from oracle_forward's dict: "weight" -> [w]; "shade" -> [image] (colors [P0,C],
    bg [C]); "depth" -> [depth (normalised, background 0), silhouette]."""
    import torch
    from oracle import torch_ref
    w, vn, idx, ln = ref["w"], ref["vn"], ref["idx"], ref["len"]
    if consumer == "weight":
        return [w]
    if consumer == "shade":
        rgb = torch_ref.merge_final(colors, w, vn, idx)
        return [torch_ref.to_colored_background(rgb, w, bg)]
    K = idx.shape[-1]
    live = torch.arange(K)[None] < vn[:, None]
    wl = w * live
    A, S = (wl * torch.where(live, ln, torch.zeros_like(ln))).sum(-1), wl.sum(-1)
    depth = torch.where(S > 0, A / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S))
    return [depth, torch.minimum(w.sum(-1), torch.ones((), dtype=w.dtype))]


def oracle_gradients(case, b, same=None):
    """fp64 autograd on base b of a gradient case: the loss is sum(output * upstream) over the consumer's outputs, with the
    upstream gradient zeroed where `same` [pix0] is False (a pixel whose index list the kernels chose differently).
    -> dict(ref=oracle_forward's dict, outs, grads={"mus", "p1"[, "colors"]} as numpy fp64, G=[upstream arrays, masked, fp32])."""
    import torch
    tile = case_bases(case)[b]
    ref = oracle_forward(tile, case.K)
    m = np.ones(case.pix0, bool) if same is None else np.asarray(same, bool).reshape(-1)
    colors = bg = None
    if case.entries[0] == "voge_fragment_shade_bwd_iso":
        consumer, whats = "shade", ["image"]
        colors = torch.tensor(tile["colors"][:, :case.C], dtype=torch.float64, requires_grad=True)
        bg = torch.tensor(BACKGROUND[:case.C], dtype=torch.float64)
    elif case.entries[0] == "voge_frame_depth_bwd_iso":
        consumer, whats = "depth", ["pixel", "sil"]
    else:
        consumer, whats = "weight", ["weight"]
    outs = oracle_outputs(ref, consumer, colors, bg)
    G = [upstream(case, b, what)[..., :o.shape[-1]] if o.dim() == 2 else upstream(case, b, what) for what, o in zip(whats, outs)]
    G = [g * m.reshape((-1,) + (1,) * (g.ndim - 1)).astype(np.float32) for g in G]
    loss = sum((o * torch.tensor(g, dtype=torch.float64)).sum() for o, g in zip(outs, G))
    loss.backward()
    grads = {"mus": ref["mus"].grad.numpy(), "p1": ref["p1"].grad.numpy()}
    if colors is not None:
        grads["colors"] = colors.grad.numpy()
    return dict(ref=ref, outs=[o.detach().numpy() for o in outs], grads=grads, G=G, tile=tile)


BACKGROUND = (0.9, 0.2, 0.6, 0.4)      # the shade cases' background colour
