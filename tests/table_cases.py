"""Index lists that drive every per-Gaussian accumulation table past its entries and past its probe limit, and a numpy model of
the tables that says, on the CPU, which keys such a list sends down the straight-to-memory path (plain numpy, no GPU).

The tables (voge_amd/csrc/voge_common.h), restated:
  home(id, bits) = ((id * 2654435761) mod 2^32) >> (32 - bits)
  WaveTable<128>:    7 bits, next probe +1 mod 128, at most 16 probes, a claimed slot is never freed; a key whose probes all hit
                     other keys goes to memory, now and in every later look-up.
  WaveDirTable<ND>:  B = log2 ND bits, step ((m >> (32 - 2B)) & (ND - 1)) | 1, at most 16 probes; the 96 value entries are handed
                     out in order of arrival (inside one look-up: the first keys of the lanes, by lane, then the second keys); a
                     key that claims a directory slot after that keeps the slot with no entry and goes to memory every time.
A look-up is one instruction over 64 lanes: its compare-and-swaps of one probe step happen in an order nobody defines.  The model
runs every step's lanes in ASCENDING or DESCENDING order; a case relies only on what holds under both, and on the order BETWEEN
look-ups, which the kernels define:
  trace / shade backward (8 x TH tiles): a tile row is one run of tw * K slots cut into batches of 64, row 0 before row 1;
  fused backward (4 x 3 groups): rounds of consecutive pixels whose ceil(count / NS) lanes fit the wave; a lane holds NS
                     consecutive slots; NS = 4 looks its slots up one after the other, NS = 2 both in one look-up.

Case kinds: see the builders below.  tests/test_table_cases_cpu.py proves each case's claims with the model, and
tests/test_gpu_accumulation_tables.py runs the kernels on the same arrays."""
import functools
import os
import re

import numpy as np

MUL = 2654435761
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voge_amd", "csrc")

# what the cases were built for; tests/test_table_cases_cpu.py compares them with the sources
BUILT_FOR = dict(VOGE_BWD_NE=128, VOGE_BWDI_NE=128, VOGE_SHADE_NE=128, VOGE_FB_NE=128, VOGE_FB_ND=256, VOGE_FB_ND_FRAME=512,
                 VOGE_FB_NEV=96, kWtProbe=16, VOGE_BWD_TH=2, VOGE_SHADE_TH=2, VOGE_FB_GW=4, VOGE_FB_GH=3)
NE, PROBE, TH, GW, GH, NEV, ND = 128, 16, 2, 4, 3, 96, 256
P_ALL = 8192                  # Gaussians / attribute rows of the 8 x 2 kernels' cases
FRAME = (5, 19)               # a partial tile on each edge: tw = 3, th = 1
POOL_HOME = 120               # the one-home pool's slot: probes 120 .. 127, 0 .. 7 -- through the wrap


def source_sizes():
    """The #define defaults (and kWtProbe) as the sources have them -> {name: int}."""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("trace_bwd.hip", "merge_blend.hip", "fragment_bwd.hip", "voge_common.h"))
    out = {}
    for name in BUILT_FOR:
        m = re.search(r"constexpr\s+int\s+kWtProbe\s*=\s*(\d+)\s*;", text) if name == "kWtProbe" else \
            re.search(r"#ifndef\s+" + name + r"\s*\n\s*#define\s+" + name + r"\s+(\d+)", text)
        assert m, f"{name}: no default found in the sources"
        out[name] = int(m.group(1))
    return out


def home(ids, bits):
    return ((np.asarray(ids, np.uint64) * MUL) & 0xFFFFFFFF) >> np.uint64(32 - bits)


def dir_step(ids, bits):
    m = (np.asarray(ids, np.uint64) * MUL) & 0xFFFFFFFF
    return ((m >> np.uint64(32 - 2 * bits)) & np.uint64((1 << bits) - 1)) | np.uint64(1)


def pool(n_ids=P_ALL, slot=POOL_HOME, bits=7, lo=0):
    """ids in [lo, lo + n_ids) whose home is `slot`"""
    ids = np.arange(lo, lo + n_ids)
    return ids[home(ids, bits) == slot]


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def _lanes(n, order):
    return range(n) if order == "asc" else range(n - 1, -1, -1)


class WaveTableModel:
    """wt_find over successive look-ups: tabled (set), memory {key: free slots when it first ran out}, wrapped (a key sits below
    its home); find() returns the lanes whose key went to memory."""

    def __init__(self, order, ne=NE, probe=PROBE):
        self.order, self.ne, self.probe = order, ne, probe
        self.bits = ne.bit_length() - 1
        self.keys = np.full(ne, -1, np.int64)
        self.memory, self.wrapped = {}, False

    def find(self, keys):
        """keys [lanes] (-1: the lane does not take part) -> bool [lanes]: the lane's key goes to memory"""
        keys = np.asarray(keys, np.int64)
        h = home(np.maximum(keys, 0), self.bits).astype(np.int64)
        h0 = h.copy()
        pending = keys >= 0
        asked = pending.copy()
        for _ in range(self.probe):
            if not pending.any():
                break
            for l in _lanes(len(keys), self.order):
                if not pending[l]:
                    continue
                if self.keys[h[l]] == -1:
                    self.keys[h[l]] = keys[l]
                if self.keys[h[l]] == keys[l]:
                    pending[l] = False
                    self.wrapped |= bool(h[l] < h0[l])
                else:
                    h[l] = (h[l] + 1) & (self.ne - 1)
        out = asked & pending
        free = int((self.keys == -1).sum())
        for k in np.unique(keys[out]):
            self.memory.setdefault(int(k), free)
        return out

    @property
    def tabled(self):
        return set(self.keys[self.keys >= 0].tolist())


class WaveDirModel:
    """wd_find2 over successive look-ups of two keys per lane.  memory {key: ("entries" | "probes", free directory slots then)}."""

    def __init__(self, order, nd=ND, nev=NEV, probe=PROBE):
        self.order, self.nd, self.nev, self.probe = order, nd, nev, probe
        self.bits = nd.bit_length() - 1
        self.keys = np.full(nd, -1, np.int64)
        self.eidx = np.full(nd, -1, np.int64)
        self.n = 0
        self.memory = {}

    def find2(self, key0, key1):
        ks = [np.asarray(key0, np.int64), np.asarray(key1, np.int64)]
        n_l = len(ks[0])
        h = [home(np.maximum(k, 0), self.bits).astype(np.int64) for k in ks]
        st = [dir_step(np.maximum(k, 0), self.bits).astype(np.int64) for k in ks]
        pend = [k >= 0 for k in ks]
        asked = [p.copy() for p in pend]
        claimed = [np.zeros(n_l, bool), np.zeros(n_l, bool)]
        for _ in range(self.probe):
            if not (pend[0].any() or pend[1].any()):
                break
            for a in (0, 1):      # (both compare-and-swaps of a step: the first keys' instruction, then the second keys')
                for l in _lanes(n_l, self.order):
                    if not pend[a][l]:
                        continue
                    s = h[a][l]
                    if self.keys[s] == -1:
                        self.keys[s] = ks[a][l]
                        claimed[a][l] = True
                    if self.keys[s] == ks[a][l]:
                        pend[a][l] = False
                    else:
                        h[a][l] = (s + st[a][l]) & (self.nd - 1)
        for a in (0, 1):          # dense entries by a ballot prefix: the first keys' claims by lane, then the second keys'
            for l in np.nonzero(claimed[a])[0]:
                self.eidx[h[a][l]] = self.n if self.n < self.nev else -1
                self.n += 1
        free = int((self.keys == -1).sum())
        out = []
        for a in (0, 1):
            found = asked[a] & ~pend[a]
            none = asked[a] & (pend[a] | (found & (self.eidx[h[a]] < 0)))
            for l in np.nonzero(none)[0]:
                self.memory.setdefault(int(ks[a][l]), ("probes" if pend[a][l] else "entries", free))
            out.append(none)
        return out

    @property
    def tabled(self):
        return set(self.keys[(self.keys >= 0) & (self.eidx >= 0)].tolist())


def tile_batches(nrows, W, K, th_tile=TH):
    """The 64-slot batches of every 8 x th_tile tile, in the kernels' order -> [dict(x0, y0, tw, th, batches=[flat slot index [64], -1 = idle])]"""
    tiles = []
    for y0 in range(0, nrows, th_tile):
        for x0 in range(0, W, 8):
            tw, th = min(8, W - x0), min(th_tile, nrows - y0)
            n_items = tw * K
            batches = []
            for r in range(th):
                for it in range((n_items + 63) // 64):
                    j = it * 64 + np.arange(64)
                    batches.append(np.where(j < n_items, ((y0 + r) * W + x0) * K + j, -1))
            tiles.append(dict(x0=x0, y0=y0, tw=tw, th=th, batches=batches))
    return tiles


def run_tiles(live_keys, nrows, W, K, order):
    """live_keys [nrows * W * K]: the key of every slot that reaches the table, -1 otherwise.
    -> per tile dict(tabled, memory, wrapped), and mem [nrows * W * K] bool: the slot's sums go straight to memory."""
    live_keys = np.asarray(live_keys).reshape(-1)
    mem = np.zeros(live_keys.size, bool)
    out = []
    for tile in tile_batches(nrows, W, K):
        m = WaveTableModel(order)
        for flat in tile["batches"]:
            keys = np.where(flat >= 0, live_keys[np.maximum(flat, 0)], -1)
            if (keys >= 0).any():
                went = m.find(keys)
                mem[flat[went]] = True
        out.append(dict(x0=tile["x0"], y0=tile["y0"], tw=tile["tw"], th=tile["th"], tabled=m.tabled, memory=m.memory, wrapped=m.wrapped,
                        slots=set(np.nonzero(m.keys >= 0)[0].tolist())))
    return out, mem


def group_rounds(nv, H, W, K, NS):
    """The fused backward's lane packing (composite_core.h: pack_round) -> per 4 x 3 group a list of rounds, each an int array
    [lanes, NS] of flat slot indices (pixel * K + k; -1: no live slot there)."""
    nv = np.asarray(nv).reshape(H, W)
    groups = []
    for y0 in range(0, H, GH):
        for x0 in range(0, W, GW):
            pix = [(y0 + g // GW, x0 + g % GW) for g in range(GW * GH)]
            lead = [int(min(K, max(0, nv[y, x]))) if (y < H and x < W) else 0 for y, x in pix]
            need = [(c + NS - 1) // NS for c in lead]
            rounds, pc = [], 0
            while pc < len(pix):
                pe, used = pc, 0
                while pe < len(pix) and used + need[pe] <= 64:
                    used += need[pe]
                    pe += 1
                assert pe > pc
                lanes = []
                for g in range(pc, pe):
                    y, x = pix[g]
                    for q in range(need[g]):
                        lanes.append([(y * W + x) * K + NS * q + a if NS * q + a < lead[g] else -1 for a in range(NS)])
                if lanes:
                    rounds.append(np.array(lanes, np.int64))
                pc = pe
            groups.append(dict(x0=x0, y0=y0, rounds=rounds))
    return groups


def run_groups(live_keys, nv, H, W, K, order, nd=ND):
    """The fused backward's table over every group: K <= 128 two slots per lane (WaveDirTable<nd>), above four (WaveTable<128>).
    -> per group dict(tabled, memory), mem [H * W * K] bool."""
    NS = 2 if K <= 128 else 4
    live_keys = np.asarray(live_keys).reshape(-1)
    mem = np.zeros(live_keys.size, bool)
    out = []
    for grp in group_rounds(nv, H, W, K, NS):
        m = WaveDirModel(order, nd) if NS == 2 else WaveTableModel(order)
        for lanes in grp["rounds"]:
            keys = np.where(lanes >= 0, live_keys[np.maximum(lanes, 0)], -1)
            if NS == 2:
                if (keys >= 0).any():
                    for a, went in enumerate(m.find2(keys[:, 0], keys[:, 1])):
                        mem[lanes[went, a]] = True
            else:
                for a in range(NS):
                    if (keys[:, a] >= 0).any():
                        went = m.find(keys[:, a])
                        mem[lanes[went, a]] = True
        out.append(dict(x0=grp["x0"], y0=grp["y0"], tabled=m.tabled, memory=m.memory))
    return out, mem


# ---- index lists for the 8 x 2 kernels --------------------------------------------------------------------------------------------------
TILE_KINDS = {"capacity40": 40, "capacity13": 13, "probe_runout": 3, "hot": 3, "mixed": 6}


def full_tiles(H, W):
    return [(y0, x0) for y0 in range(0, H - TH + 1, TH) for x0 in range(0, W - 7, 8)]


def _distinct_rows(rng, ids, n, K):
    """n lists of K distinct ids each"""
    return np.stack([rng.permutation(ids)[:K] for _ in range(n)])


def plant_hot(idx, ids, rng, H, W):
    """probe_runout lists [H, W, 3] over the one-home pool `ids` with two planted ids per full tile -> planted [(tile, table id,
    memory id)].  Row 0 of the tile: the table id in slot 1 of all eight pixels, the other 16 slots 15 distinct pool ids (one of
    them twice) -- 16 distinct keys in the tile's first batch, all of them tabled whatever the order, which fills the pool's 16
    slots.  Row 1: the memory id in slot 0 of all eight pixels, the other slots any pool ids but the two planted ones."""
    planted = []
    for y0, x0 in full_tiles(H, W):
        p = rng.permutation(ids)
        t_id, m_id, rest = int(p[0]), int(p[1]), p[2:]
        others = np.concatenate([rest[:15], rest[:1]])       # (the repeated one lands in two different pixels: 0 and 7)
        for x in range(8):
            idx[y0, x0 + x] = (others[x], t_id, others[8 + x])
            idx[y0 + 1, x0 + x] = np.concatenate([[m_id], rng.permutation(rest)[:2]])
        planted.append(((y0, x0), t_id, m_id))
    return planted


def tile_lists(kind, n_ids=P_ALL, lo=0, seed=0, H=FRAME[0], W=FRAME[1]):
    """idx [H, W, K] int32 over ids [lo, lo + n_ids), cnt [H, W] int32 | None, planted (hot) -- see the module docstring's kinds:
    capacity  ids uniform over all (a Gaussian once per list);  capacity13 also has a count array with 0, K and random counts;
    probe_runout  every id from the one-home pool;  hot  plant_hot;  mixed  alternate pixels draw from the pool and from all."""
    K = TILE_KINDS[kind]
    rng = np.random.default_rng(4100 + 13 * K + len(kind) + seed)
    every, one_home = np.arange(lo, lo + n_ids), pool(n_ids, lo=lo)
    cnt, planted = None, []
    if kind.startswith("capacity"):
        idx = _distinct_rows(rng, every, H * W, K).reshape(H, W, K)
        if kind == "capacity13":
            cnt = np.where(rng.random((H, W)) < 0.2, rng.integers(0, K + 1, (H, W)), K)      # (most lists full: the tiles stay over 128 ids)
            cnt[0, :4], cnt[1, :4] = (0, K, 0, K), (K, K, 1, K - 1)
    elif kind == "mixed":
        idx = _distinct_rows(rng, every, H * W, K).reshape(H, W, K)
        alt = (np.arange(H)[:, None] + np.arange(W)[None]) % 2 == 0
        idx[alt] = _distinct_rows(rng, one_home, int(alt.sum()), K)
    else:
        idx = _distinct_rows(rng, one_home, H * W, K).reshape(H, W, K)
        if kind == "hot":
            planted = plant_hot(idx, one_home, rng, H, W)
    return idx.astype(np.int32), (None if cnt is None else cnt.astype(np.int32)), planted


def signed_unit(rng, shape):
    """magnitudes in [0.5, 1.5] with a random sign: no slot's gradient is near zero, so none can hide its own loss"""
    return rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)


def trace_gaussians(P, npix, seed=0, scalar=False):
    """P Gaussians in front of the origin with well-conditioned forms (tests/test_gpu_bwd_walk_accumulators.py: gaussians), a little
    asymmetry on the 3 x 3 ones (the backward does not symmetrise), and npix unit rays in a narrow bundle."""
    rng = np.random.default_rng(4300 + seed)
    mus = (rng.uniform(-1, 1, (P, 3)) + [0, 0, 4]).astype(np.float32)
    if scalar:
        isg = rng.uniform(0.5, 3.0, P).astype(np.float32)
    else:
        L = np.tril(rng.uniform(-1, 1, (P, 3, 3)))
        L[:, [0, 1, 2], [0, 1, 2]] = np.abs(L[:, [0, 1, 2], [0, 1, 2]]) + 0.5
        isg = (L @ L.transpose(0, 2, 1) + rng.normal(size=(P, 3, 3)) * 0.02).astype(np.float32)
    rays = rng.normal(size=(npix, 3)) * 0.2 + [0, 0, 1.0]
    return mus, isg, (rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def trace_case(kind, scalar=False, B=1):
    """Everything ops._trace_bwd takes for one kind -> dict.  B = 2: one set of P_ALL / 2 Gaussians seen by two views (ids b * N + i),
    each from its own origin: the Gaussians of view b are mus - origin[b], rounded to fp32 as the kernel's record pass does."""
    H, W = FRAME
    N = P_ALL // B
    parts = [tile_lists(kind, n_ids=N, lo=b * N, seed=b) for b in range(B)]
    idx = np.stack([p[0] for p in parts])
    cnt = None if parts[0][1] is None else np.stack([p[1] for p in parts])
    K = idx.shape[-1]
    mus, isg, rays = trace_gaussians(N, B * H * W, seed=K + (7 if scalar else 0), scalar=scalar)
    rng = np.random.default_rng(4500 + K + len(kind))
    g_len, g_act = signed_unit(rng, idx.shape).astype(np.float32), signed_unit(rng, idx.shape).astype(np.float32)
    g_dsd = (signed_unit(rng, idx.shape) * 1e-3).astype(np.float32)
    live = np.ones(idx.shape, bool) if cnt is None else np.arange(K) < cnt[..., None]
    origin = np.array([[0.1, -0.05, 0.0], [-0.15, 0.1, 0.05]], np.float32)[:B] * (B > 1)
    return dict(kind=kind, K=K, B=B, N=N, H=H, W=W, idx=idx, cnt=cnt, mus=mus, isg=isg, origin=origin, rays=rays.reshape(B, H, W, 3), g_len=g_len, g_act=g_act,
                g_dsd=g_dsd, live=live, planted=[(b,) + q for b, p in enumerate(parts) for q in p[2]])


def trace_reference_inputs(case):
    """(mus [B * N, 3], isg [B * N, 3, 3]) as oracle.trace_bwd reads them, and the gradients masked to the live slots (the kernel
    skips the slots behind a pixel's count; the oracle skips a slot by its negative index)."""
    B, N = case["B"], case["N"]
    mus = (case["mus"][None] - case["origin"][:, None]).astype(np.float32).reshape(B * N, 3) if "origin" in case else case["mus"]
    isg = case["isg"]
    if isg.ndim == 1:
        isg = isg[:, None, None] * np.eye(3, dtype=np.float32)
    idx = np.where(case["live"], case["idx"], -1).astype(np.int32)
    return mus, np.tile(isg, (B, 1, 1)), idx


def trace_mu_terms(case):
    """The largest component of every slot's own term of g_mu, fp64, from the closed form in the header of trace_bwd.hip:
    g_mu = c1 A d + g_act [(A + A^T) v + t (A^T - A) d], t = mu'A d / d'A d, v = mu - t d, c1 = g_len / d'A d  -> [B, H, W, K]."""
    mus, isg, _ = trace_reference_inputs(case)
    idx = case["idx"].astype(np.int64)
    mu, A = mus.astype(np.float64)[idx], isg.astype(np.float64)[idx]
    d = np.broadcast_to(case["rays"].astype(np.float64)[..., None, :], mu.shape)
    Ad, Atd = np.einsum("...ij,...j->...i", A, d), np.einsum("...ji,...j->...i", A, d)
    dsd = (d * Ad).sum(-1)
    t = (mu * Ad).sum(-1) / dsd
    v = mu - t[..., None] * d
    c1 = case["g_len"].astype(np.float64) / dsd
    sym_v = np.einsum("...ij,...j->...i", A + np.swapaxes(A, -1, -2), v)
    term = c1[..., None] * Ad + case["g_act"].astype(np.float64)[..., None] * (sym_v + t[..., None] * (Atd - Ad))
    return np.abs(term).max(-1) * case["live"]


# ---- fragments for the shade / merge backward ---------------------------------------------------------------------------------------------
SHADE_KINDS = {"capacity40": 40, "capacity13": 13, "probe_runout": 3, "hot": 3}


@functools.lru_cache(maxsize=None)
def shade_case(kind, C, blend=False):
    """test_attr_routes_cpu.attr_case on the 5 x 19 frame with 8192 attribute rows, then: the upstream gradient redrawn by
    signed_unit; every non-zero weight lifted to at least 0.6 of its pixel's largest (the pixel's sum kept), so that no live slot's
    w g can vanish against the tolerance; at K = 13 and K = 3 nine pixels of ten get a full list (attr_case's counts average K / 2,
    which leaves a tile under 128 ids, or under 16 of the pool's); the pool kinds' ids redrawn from the one-home pool, none of them
    -1, which would read row 0 (hot: plant_hot, its pixels with all three slots live); blend: the pixels that came within the clamp's
    margin rescaled until none does."""
    import test_attr_routes_cpu as A
    K = SHADE_KINDS[kind]
    case = A.attr_case((1,) + FRAME, K, C, Nattr=P_ALL, seed=4700 + 7 * K + C + len(kind), blend=blend)
    rng = np.random.default_rng(4800 + 7 * K + C + len(kind))
    case["g"] = signed_unit(rng, case["g"].shape).astype(np.float32)
    idx, vn, w = case["idx"][0], case["valid_num"][0], case["weight"][0].astype(np.float64)
    s = w.sum(-1, keepdims=True)
    case["planted"] = []
    if kind != "capacity40":
        ids = np.arange(P_ALL) if kind == "capacity13" else pool()
        fill = rng.random(vn.shape) < 0.9
        fill[0, 1] = False        # (attr_case's pixel without a live slot stays)
        fresh = _distinct_rows(rng, ids, vn.size, K).reshape(idx.shape)
        idx[...] = fresh if kind != "capacity13" else np.where(fill[..., None], fresh, idx)
        vn[fill] = K
        if kind == "hot":
            case["planted"] = plant_hot(idx, ids, rng, *FRAME)
            for (y0, x0), _, _ in case["planted"]:
                vn[y0:y0 + 2, x0:x0 + 8] = K
                blk = w[y0:y0 + 2, x0:x0 + 8]
                blk[...] = np.where(blk > 0, blk, blk.max(-1, keepdims=True))      # (a planted slot with weight 0 would not be live)
    lifted = np.where(w > 0, 0.6 + 0.4 * w / w.max(-1, keepdims=True), 0.0)
    w = lifted / lifted.sum(-1, keepdims=True) * s
    w32 = w.astype(np.float32)
    if blend:
        flat_i, flat_v = idx.reshape(-1, K), vn.reshape(-1)
        w2 = w32.reshape(-1, K)
        for _ in range(400):
            x = A._blend_x(w2, A._merge_np(case["attr"], w2, flat_v, flat_i), case["bg"])
            sm = w2.astype(np.float64).sum(-1)
            bad = (np.abs(x - 1) < 1.2 * A.MARGIN).any(axis=(0, 2)) | (np.abs(sm - 1) < 1.2 * A.MARGIN)
            if not bad.any():
                break
            w2[bad] = (w2[bad] * (A._draw_target(rng, int(bad.sum())) / sm[bad])[:, None]).astype(np.float32)
        else:
            raise AssertionError("no target keeps every channel of some pixel away from the clamp")
    case["weight"] = w32.reshape(case["weight"].shape)
    case["kind"] = kind
    return case


def shade_live_keys(case, passes=None):
    """The key of every slot that reaches shade_bwd_tile_kernel's table: k < valid_num, a negative index reads row 0, and the
    slot's w g_rgb is not all zero (passes [pixels] bool: the blend's clamp lets some channel of the pixel through)."""
    K = case["K"]
    idx, vn, w = case["idx"].reshape(-1, K), case["valid_num"].reshape(-1), case["weight"].reshape(-1, K)
    live = (np.arange(K)[None] < vn[:, None]) & (w != 0)
    if passes is not None:
        live &= np.asarray(passes).reshape(-1, 1)
    return np.where(live, np.maximum(idx, 0), -1)


# ---- index lists for the fused backward ---------------------------------------------------------------------------------------------------
FUSED_KINDS = {"entries": 40, "directory": 40, "capacity": 130, "probe_runout": 130}
FUSED_P = {"entries": 256, "directory": 4096, "capacity": 4096, "probe_runout": P_ALL}
RUNOUT_LIVE = 40      # live slots per pixel at most, from the one-home pool's 62-66 ids (a list names a Gaussian once)


@functools.lru_cache(maxsize=None)
def fused_case(kind):
    """The lists of tests/test_gpu_bwd_walk_accumulators.py (build_lists: their depth structure stays) with every pixel's ids sent
    through its own injective map into the kind's id set; its gaussians() repeated over that set.
      entries       K = 40: 256 ids in all -- a group holds more than 96 and at most 256 distinct ones;
      directory     K = 40: 4096 ids, and the frame's twelve longest lists moved into the first group: more distinct ids there
                    than the 256 directory keys, so look-ups run out of probes;
      capacity      K = 130: 4096 ids, more than 128 distinct ones per group;
      probe_runout  K = 130: every id from the one-home pool of 8192, lists cut to RUNOUT_LIVE live slots."""
    import test_gpu_bwd_walk_accumulators as Wk
    K, P = FUSED_KINDS[kind], FUSED_P[kind]
    idx, act, ln, dsd, nv = (a.copy() for a in Wk.build_lists(K))
    rng = np.random.default_rng(4900 + K + len(kind))
    if kind == "directory":
        first = [y * Wk.W + x for y in range(GH) for x in range(GW)]
        longest = np.argsort(-nv, kind="stable")[:len(first)].tolist()
        moved = np.empty(Wk.NPIX, np.int64)      # moved[destination] = source
        moved[first] = longest
        moved[[p for p in range(Wk.NPIX) if p not in first]] = [p for p in range(Wk.NPIX) if p not in longest]
        idx, act, ln, dsd, nv = idx[moved], act[moved], ln[moved], dsd[moved], nv[moved]
    if kind == "probe_runout":
        cut = np.arange(K)[None] >= np.minimum(nv, RUNOUT_LIVE)[:, None]
        idx[cut], act[cut], ln[cut], dsd[cut] = -1, 1e10, 1e10, 0.0
        nv = np.minimum(nv, RUNOUT_LIVE)
    ids = pool(P) if kind == "probe_runout" else np.arange(P)
    for p in range(Wk.NPIX):
        c = int(nv[p])
        idx[p, :c] = rng.permutation(ids)[:c]      # injective, this pixel's own: old id in slot j -> the j-th of a fresh draw
    g0 = Wk.gaussians(K)
    rep = np.arange(P) % g0["mus"].shape[0]
    g = dict(mus=g0["mus"][rep], isg=g0["isg"][rep], rays=g0["rays"])
    gw = signed_unit(np.random.default_rng(4950 + K + len(kind)), (Wk.NPIX, K)).astype(np.float32)
    return dict(kind=kind, K=K, P=P, H=Wk.H, W=Wk.W, idx=idx, act=act, ln=ln, dsd=dsd, nv=nv, g=g, gw=gw, occ=Wk.OCC)


def fused_weights(case):
    """the forward's weights of the case's lists (fp64 oracle, rounded to fp32: the fused backward reads them)"""
    import oracle
    return oracle.composite_fwd(case["idx"], case["act"], case["ln"], case["dsd"], case["occ"])[0].astype(np.float32)


def fused_reference(case, precision="f64"):
    """oracle.composite_bwd, then oracle.trace_bwd -> (g_act, g_len, g_dsd) [pixels, K], g_mus [P, 3], g_isigmas [P, 3, 3]"""
    import oracle
    ga, gl, gd = oracle.composite_bwd(case["act"], case["ln"], case["dsd"], case["gw"], case["occ"], precision=precision)
    g = case["g"]
    _, gm, gs = oracle.trace_bwd(g["mus"], g["isg"], g["rays"], case["idx"], gl, ga, gd, precision=precision)
    return (ga, gl, gd), gm, gs


def fused_as_trace_case(case, slot_grads):
    """the fused case's lists and per-slot gradients in trace_case's layout (for trace_mu_terms)"""
    ga, gl, _ = slot_grads
    H, W, K = case["H"], case["W"], case["K"]
    sh = (1, H, W, K)
    return dict(B=1, N=case["P"], mus=case["g"]["mus"], isg=case["g"]["isg"], rays=case["g"]["rays"].reshape(1, H, W, 3),
                idx=np.maximum(case["idx"], 0).reshape(sh), live=(case["idx"] >= 0).reshape(sh), g_len=np.asarray(gl).reshape(sh),
                g_act=np.asarray(ga).reshape(sh))
