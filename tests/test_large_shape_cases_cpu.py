"""tests/large_shape_cases.py without a GPU: every case lies on the side of every restated gate it is meant for, with the smallest
(or the largest) tile count that does; none needs more than 48 GiB; the tiling rule puts base t mod 3 into tile t with the
Gaussians' index offset and keeps the empty slots at -1; a read displaced by 2^32 bytes never lands on the same base; and the
fp64 reference gradients of every base tile are far from degenerate."""
import numpy as np
import pytest

import large_shape_cases as ls

CASES = list(ls.CASES.values())
ids = [c.name for c in CASES]


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_case_lies_on_its_side_of_every_gate(c):
    g = c.gates()
    assert c.sides, c.name
    for gate, side in c.sides:
        assert g[gate] is side, (c.name, gate, g[gate])
    off = ls.byte_offsets(c.npix, c.K, c.C if c.shade_bg else 0)
    if dict(c.sides).get("fused backward narrow") is True:
        assert max(off.values()) <= ls.U32, (c.name, off)      # every offset the 32-bit form multiplies out fits
    if dict(c.sides).get("fused backward narrow") is False or dict(c.sides).get("composite from records narrow") is False:
        assert max(off.values()) > ls.U32 or c.slots >= ls.SLOT_GATE, (c.name, off)
    # the entries' own limits
    assert c.P < ls.P_LIMIT and c.P * max(c.C, 1) < ls.ATTR_LIMIT, (c.name, c.P)
    fused_attr = any(e in ("voge_fragment_shade_bwd_iso", "voge_frame_depth_bwd_iso") for e in c.entries)
    assert c.K <= (128 if fused_attr else 256)      # (the fused backward's shade / depth forms: a pixel's lanes in one wave at two slots each)
    if c.stack == "W":
        assert c.W0 % 8 == 0 and c.H0 == 8


@pytest.mark.parametrize("c", [c for c in CASES if c.smallest], ids=lambda c: c.name)
def test_the_tile_count_is_the_smallest_that_reaches_2_30_slots(c):
    assert c.slots >= ls.SLOT_GATE and (c.T - 1) * c.pix0 * c.K < ls.SLOT_GATE, (c.name, c.T)


@pytest.mark.parametrize("c", [c for c in CASES if c.short_of], ids=lambda c: c.name)
def test_the_largest_32_bit_cases_are_one_tile_short(c):
    wide = ls.CASES[c.short_of]
    assert (c.K, c.H0, c.W0, c.stack, c.form) == (wide.K, wide.H0, wide.W0, wide.stack, wide.form)
    if wide.smallest:
        assert c.T == wide.T - 1 and c.slots < ls.SLOT_GATE <= wide.slots
        assert c.slots * 4 < ls.U32 <= (c.slots + c.pix0 * c.K) * 4      # byte offsets just under 2^32
    else:      # the K = 1 gate case: the ray offsets decide -- the largest tile count whose last ray still fits
        assert c.npix * 12 <= ls.U32 < (c.npix + c.pix0) * 12 and wide.T == c.T + 2
        assert wide.npix - wide.pix0 > ls.PIX_GATE > wide.npix - 2 * wide.pix0      # the smallest multiple above 357 913 942, and one more
        assert wide.lit_tiles()[-4:-2] == c.lit_tiles()[-2:]      # the companion's last two tiles are lit too


def test_the_shade_gate_case_is_just_below_a_third_of_2_30():
    c = ls.CASES["gate_fb_shade_K3_C4"]
    assert c.npix * 3 < ls.SLOT_GATE <= (c.npix + c.pix0) * 3
    assert c.npix * 16 > ls.U32 and (c.lit_tiles()[-2]) * c.pix0 >= (1 << 28)      # both lit tiles at the end have wrapped rgb offsets


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_no_case_needs_more_than_48_GiB(c):
    need = c.need_bytes()
    if c.short_of:
        assert need == 0      # a view of the first tiles of its parent's arrays
        return
    by_hand = 0
    for name, kind, size in c.arrays:
        n = {"slot": c.npix * c.K, "pix": c.npix, "gauss": c.P, "once": 1}[kind]
        by_hand += n * size
    print(f"{c.name}: {need / 2**30:.2f} GiB in {len(c.arrays)} arrays ({c.slots} slots, {c.npix} pixels, {c.P} Gaussians)")
    assert need == by_hand and 0 < need <= ls.CAP_BYTES == 48 * 2**30, (c.name, need)


@pytest.mark.parametrize("offset", [None, 11])
def test_tiling_at_seven_tiles(offset):
    rng = np.random.default_rng(3)
    bases = [np.where(rng.uniform(size=(5, 4)) < 0.3, -1, rng.integers(0, 11, (5, 4))).astype(np.int32) for _ in range(3)]
    for b in bases:
        assert (b == -1).any() and (b >= 0).any()
    out = ls.fill_tiles(np.full((7, 5, 4), -7, np.int32), bases, offset)
    for t in range(7):
        want = bases[t % 3] if offset is None else np.where(bases[t % 3] >= 0, bases[t % 3] + t * offset, -1)
        assert np.array_equal(out[t], want), t
        assert ((out[t] == -1) == (bases[t % 3] == -1)).all()      # empty slots stay -1 whatever the offset
        if offset:
            live = out[t][out[t] >= 0]
            assert (live >= t * offset).all() and (live < (t + 1) * offset).all()      # tile t refers to its own Gaussians
    # only some tiles, through a strided view, chunked
    big = np.full((7, 5, 4), -7, np.int32)
    ls.fill_tiles(big, bases, offset, tiles=[0, 5, 6])
    assert (big[1:5] == -7).all() and np.array_equal(big[5], out[5]) and np.array_equal(big[0], out[0])
    old, ls.CHUNK = ls.CHUNK, 20
    try:
        assert np.array_equal(ls.fill_tiles(np.full((7, 5, 4), -7, np.int32), bases, offset), out)
    finally:
        ls.CHUNK = old


def test_tiles_view_is_a_view_in_every_stacking():
    c = ls.CASES["sweep_W262144"]
    big = np.zeros((c.H0, 5 * c.W0, 3), np.float32)
    v = ls.tiles_view(big, c, (3,))
    assert v.shape == (5, c.H0, c.W0, 3) and np.shares_memory(v, big)
    v[3] = 1.0
    assert big[:, 3 * c.W0:4 * c.W0].min() == 1.0 and big.sum() == c.H0 * c.W0 * 3
    r = ls.CASES["fb_weights_K256"]
    big = np.zeros((5 * r.pix0, r.K), np.float32)
    v = ls.tiles_view(big, r, (r.K,))
    assert v.shape == (5, r.pix0, r.K) and np.shares_memory(v, big)


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_a_read_displaced_by_2_32_bytes_lands_on_another_base(c):
    for name, nbytes in c.tile_bytes().items():
        # 2^32 / tile_bytes tiles: a multiple of 3 tiles would find the same base again
        assert ls.U32 % (ls.NBASE * nbytes) != 0, (c.name, name, nbytes)
    bases = ls.case_bases(c)
    for i in range(3):
        j = (i + 1) % 3
        assert not np.array_equal(bases[i]["rays"], bases[j]["rays"]) and not np.array_equal(bases[i]["mus"], bases[j]["mus"])


_ORACLE = {}


def _fwd(c, b):
    key = (c.K, c.H0, c.W0, c.form, b)
    if key not in _ORACLE:
        _ORACLE[key] = ls.oracle_forward(ls.case_bases(c)[b], c.K)
    return _ORACLE[key]


@pytest.mark.parametrize("c", [c for c in CASES if not c.short_of and c.stack != "W"], ids=lambda c: c.name)
def test_base_tiles_have_empty_partial_and_full_lists(c):
    counts = []
    for b in range(3):
        vn = _fwd(c, b)["vn"].numpy()
        assert (vn == 0).mean() > 0.05 and (vn == c.K).mean() > 0.05, (c.name, b)
        assert c.K == 1 or ((vn > 0) & (vn < c.K)).mean() > 0.01, (c.name, b)
        counts.append(vn)
    assert not np.array_equal(counts[0], counts[1]) and not np.array_equal(counts[1], counts[2])


@pytest.mark.parametrize("c", [c for c in CASES if c.gradients and not c.short_of], ids=lambda c: c.name)
def test_reference_gradients_are_not_degenerate(c):
    for b in range(3):
        r = ls.oracle_gradients(c, b)
        tile = r["tile"]
        for name, g in r["grads"].items():
            inputs = tile["mus"] if name == "mus" else tile["colors"] if name == "colors" else tile.get("a", tile.get("isigmas"))
            # (the upstream gradients are unit normals)
            print(c.name, b, name, np.abs(g).max(), np.abs(inputs).max())
            assert np.isfinite(g).all() and np.abs(g).max() > 1e-3 * np.abs(inputs).max(), (c.name, b, name, np.abs(g).max())
