"""The fused backward's accumulation table on the CPU: how many iterations a wave's look-up loop takes per round under
several probe schemes, and how many distinct Gaussians a 4x3 group holds (what sizes the table's values).
Index lists: the fp32 oracle trace on row bands (default; no GPU), or --gpu: the renderer's own lists of the whole frame
(distinct counts of every group, the probe simulation on every `--every`-th group).  Groups, lanes and rounds are
fragment_bwd.hip's: 4x3 pixels, two slots per lane, pack_round's longest run of pixels whose lanes fit the wave.  A loop
iteration is one compare-and-swap per pending key (a lane's two keys go together); the wave iterates until its slowest lane
is done, at most 16 times.
usage: python tools/table_probe_sim.py [config] [--bands 252,120] [--gpu] [--every 16]"""
import argparse
import sys

import numpy as np

sys.path.insert(0, ".")
from voge_amd import scenes  # noqa: E402

GW, GH, PROBE = 4, 3, 16
MUL = 2654435761


def oracle_band(name, row):
    import oracle
    from oracle import camera_np
    N, (H, W), K, focal, pp, (dd, el, az) = scenes.CONFIGS[name]
    verts, sig, _ = scenes.random_gaussians(N, seed=0)
    R, T = camera_np.look_at_view_transform(dd, el, az)
    rays, origin = camera_np.pixel_rays(R, T, focal, pp, (H, W))
    rays = np.ascontiguousarray(rays[:, row:row + 4 * GH])
    mus = (verts[None] - origin[:, None].astype(np.float32)).astype(np.float32)
    isg = (2 * camera_np.expand_sigma(sig)).astype(np.float32)[None]
    return oracle.trace_fwd(mus, isg, rays, K, oracle.thr_act_of(0.01), precision="f32")[0][0]


def gpu_frame(name):
    import torch
    from voge_amd.Meshes import GaussianMeshes
    from voge_amd.Renderer import GaussianRenderer, GaussianRenderSettings
    from voge_amd.cameras import PerspectiveCameras, look_at_view_transform
    N, (H, W), K, focal, pp, (dd, el, az) = scenes.CONFIGS[name]
    dev = torch.device("cuda", 0)
    verts, sig, _ = scenes.random_gaussians(N, seed=0)
    gm = GaussianMeshes(torch.from_numpy(verts), torch.from_numpy(sig)).to(dev)
    R, T = look_at_view_transform(dist=dd, elev=el, azim=az, device=dev)
    cams = PerspectiveCameras(focal_length=focal, principal_point=(pp,), image_size=((H, W),), device=dev)
    renderer = GaussianRenderer(cams, GaussianRenderSettings(image_size=(H, W), max_assign=K, max_point_per_bin=-1)).to(dev)
    with torch.no_grad():
        frag = renderer(gm, R=R, T=T)
    idx = frag.vert_index[0].cpu().numpy()
    cnt = frag.valid_num[0].cpu().numpy()
    return np.where(np.arange(K)[None, None] < cnt[..., None], idx, -1)


def groups(idx):
    """[H, W, K] index lists (-1: empty) -> per group the list of its pixels' id arrays, in lane order"""
    H, W, _ = idx.shape
    for y0 in range(0, H, GH):
        for x0 in range(0, W, GW):
            px = [idx[y, x][idx[y, x] >= 0] for y in range(y0, min(y0 + GH, H)) for x in range(x0, min(x0 + GW, W))]
            if sum(len(p) for p in px):
                yield px


def rounds(px):
    """pack_round: consecutive pixels while their lanes (two slots each) fit 64; -> per round [(key0s, key1s)] of the lanes"""
    out, lanes, cur = [], 0, []
    for p in px:
        n = (len(p) + 1) // 2
        if lanes + n > 64:
            out.append(cur)
            lanes, cur = 0, []
        lanes += n
        if n:
            cur.append(p)
    if cur:
        out.append(cur)
    res = []
    for r in out:
        k0 = np.concatenate([p[0::2] for p in r])
        k1 = np.concatenate([np.concatenate([p[1::2], [-1] * (len(p) & 1)]) for p in r]).astype(np.int64)
        res.append((k0.astype(np.int64), k1))
    return res


class Open:
    """open addressing over nd slots; step: 0 = linear, 1 = an odd step from other bits of the same product"""
    def __init__(self, nd, double):
        self.nd, self.double, self.tab = nd, double, np.full(nd, -1, np.int64)
        self.bits = nd.bit_length() - 1

    def run(self, k0, k1):
        pend = [(int(k), which) for which, ks in ((0, k0), (1, k1)) for k in ks if k >= 0]
        prod = {k: (k * MUL) & 0xFFFFFFFF for k, _ in pend}
        pos = [prod[k] >> (32 - self.bits) for k, _ in pend]
        step = [(((prod[k] >> (32 - 2 * self.bits)) & (self.nd - 1)) | 1) if self.double else 1 for k, _ in pend]
        alive = list(range(len(pend)))
        it = fails = 0
        while alive and it < PROBE:
            it += 1
            nxt = []
            for i in alive:      # (key 0 of every lane, then key 1: the order of the two instructions)
                k, h = pend[i][0], pos[i]
                if self.tab[h] == -1:
                    self.tab[h] = k
                elif self.tab[h] != k:
                    pos[i] = (h + step[i]) & (self.nd - 1)
                    nxt.append(i)
            alive = nxt
        fails = len(alive)
        return it, fails


class Bucket:
    """nb buckets of 4 keys read with one 16-byte read; a hit costs no atomic; a miss claims the first empty way"""
    def __init__(self, nb):
        self.nb, self.tab, self.bits = nb, np.full((nb, 4), -1, np.int64), nb.bit_length() - 1

    def run(self, k0, k1):
        pend = [int(k) for ks in (k0, k1) for k in ks if k >= 0]
        pos = [((k * MUL) & 0xFFFFFFFF) >> (32 - self.bits) for k in pend]
        alive = list(range(len(pend)))
        it = 0
        while alive and it < PROBE:
            it += 1
            snap = self.tab.copy()       # every lane reads, then the claims go out
            nxt = []
            for i in alive:
                k, b = pend[i], pos[i]
                if k in snap[b]:
                    continue
                free = np.nonzero(snap[b] == -1)[0]
                if len(free) == 0:
                    pos[i] = (b + 1) & (self.nb - 1)
                    nxt.append(i)
                elif self.tab[b, free[0]] == -1:
                    self.tab[b, free[0]] = k
                elif self.tab[b, free[0]] != k:
                    nxt.append(i)       # lost the way to another key: read again
            alive = nxt
        return it, len(alive)


SCHEMES = {"linear 128 (today)": lambda: Open(128, False), "double hash 128": lambda: Open(128, True),
           "double hash 256": lambda: Open(256, True), "double hash 512": lambda: Open(512, True),
           "buckets 64 x 4": lambda: Bucket(64)}


def report(label, idx, every):
    gs = list(groups(idx))
    distinct = np.array([len(np.unique(np.concatenate(px))) for px in gs])
    live = np.array([sum(len(p) for p in px) for px in gs])
    print(f"{label}: {len(gs)} groups; live slots mean {live.mean():.0f}; distinct Gaussians mean {distinct.mean():.1f}, "
          f"p90 {np.percentile(distinct, 90):.0f}, p99 {np.percentile(distinct, 99):.0f}, max {distinct.max()}; "
          f"groups over 96 / 128 entries: {(distinct > 96).sum()} / {(distinct > 128).sum()}")
    sub = gs[::every]
    for name, make in SCHEMES.items():
        its, first, later, fails, nr = [], [], [], 0, 0
        for px in sub:
            t = make()
            for j, (k0, k1) in enumerate(rounds(px)):
                it, f = t.run(k0, k1)
                its.append(it)
                (first if j == 0 else later).append(it)
                fails += f
                nr += 1
        its = np.array(its)
        print(f"  {name:20s} iterations per round mean {its.mean():.2f} p90 {np.percentile(its, 90):.0f} max {its.max()} "
              f"(first round {np.mean(first):.2f}, later {np.mean(later) if later else 0:.2f}); per group {its.sum() / len(sub):.1f}; "
              f"keys out of probes {fails} in {nr} rounds")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="cfg3_50k_512")
    ap.add_argument("--bands", default="252,120")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--every", type=int, default=None)
    a = ap.parse_args()
    if a.gpu:
        report(f"{a.config} whole frame (renderer)", gpu_frame(a.config), a.every or 16)
    else:
        for row in (int(r) for r in a.bands.split(",")):
            report(f"{a.config} rows {row}..{row + 4 * GH - 1} (fp32 oracle)", oracle_band(a.config, row), a.every or 1)
