"""The memos that outlive a call, on host tensors: Losses._checked_faces (a recycled address must not answer for a new tensor),
cameras._intrinsics (identity + version + B) and distributed._stripe_index (keys that share two of their three numbers).  The GPU
half is tests/test_gpu_call_sequences.py."""
import numpy as np
import pytest
import torch

from voge_amd import Losses, cameras
from voge_amd.distributed import Stripes, _stripe_index

V = 4
GOOD, BAD = [[0, 1, 2], [1, 2, 3]] * 50, [[0, 1, 2], [1, 2, 9]] * 50      # BAD names vertex 9 of 4
VERTS = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
POINTS = torch.tensor([[0.2, 0.2, 0.1], [0.9, 0.1, 0.3], [-0.5, 0.4, 0.2]])
CHECKS = {
    "_checked_faces": (3, lambda f: Losses._checked_faces(f, V, "t")),
    "point_mesh_face_distance": (3, lambda f: Losses.point_mesh_face_distance(VERTS, f, POINTS)),
    "point_mesh_edge_distance": (2, lambda f: Losses.point_mesh_edge_distance(VERTS, f, POINTS)),
    "closest_faces": (3, lambda f: Losses.closest_faces(POINTS, VERTS, f)),
}


def remade_at(ptr, make, tries=32):
    """A new tensor from make() at the address ptr that a tensor freed just now had, where the allocator gives it back within
    `tries` allocations of that size (the others are held meanwhile, so each try gets another block); else the last one made."""
    held = []
    for _ in range(tries):
        held.append(make())
        if held[-1].data_ptr() == ptr:
            break
    return held[-1]


def recycled_faces(check, width, device="cpu", rounds=8):
    """`rounds` times: a good table is checked and freed, and a bad one of its shape and dtype, made right after, must raise
    ValueError.  -> in how many rounds the bad table really had the good one's address (both at version 0).
    On the host the two tables wrap one numpy buffer in turn (at_the_same_address below), so the address is the same in every
    round whatever the heap looks like: whether malloc hands a freed 2 400-byte block back depends on where the pieces trimmed
    off its aligned allocation went, and came out anywhere between 0 and 8 rounds of 8 from one run of the suite to the next.  A device's
    caching allocator does hand the block back, and there the tables are made and freed as a caller's are."""
    reused = 0
    buf = np.zeros((len(GOOD), width), np.int64)
    for _ in range(rounds):
        if device == "cpu":
            f = at_the_same_address(buf, np.asarray(GOOD)[:, 3 - width:])
        else:
            f = torch.tensor([row[3 - width:] for row in GOOD], device=device)
        check(f)
        ptr = f.data_ptr()
        del f
        if device == "cpu":
            g = at_the_same_address(buf, np.asarray(BAD)[:, 3 - width:])
        else:
            g = remade_at(ptr, lambda: torch.tensor([row[3 - width:] for row in BAD], device=device))
        assert g._version == 0
        reused += int(g.data_ptr() == ptr)
        with pytest.raises(ValueError, match="indices must lie"):
            check(g)
        del g
    return reused


@pytest.mark.parametrize("name", list(CHECKS))
def test_a_new_faces_tensor_at_a_recycled_address_is_checked(name):
    width, check = CHECKS[name]
    reused = recycled_faces(check, width)
    print(f"[faces memo] {name}: the bad table had the freed table's address in {reused} of 8 rounds")
    assert reused >= 1, "the allocator never handed the address back: the test did not reach the case it is about"


def test_a_view_whose_base_is_edited_in_place_is_checked_again():
    base = torch.tensor(GOOD + GOOD)
    view = base[100:]
    Losses._checked_faces(view, V, "t")
    base[150, 1] = 9      # (the view and its base share one version counter)
    with pytest.raises(ValueError, match=r"got \[0, 9\]"):
        Losses._checked_faces(view, V, "t")
    with pytest.raises(ValueError):
        Losses.point_mesh_face_distance(VERTS, view, POINTS)
    base[150, 1] = 2
    Losses._checked_faces(view, V, "t")
    # the tensor itself edited in place, and the same tensor asked about a smaller mesh
    f = torch.tensor(GOOD)
    Losses._checked_faces(f, V, "t")
    with pytest.raises(ValueError):
        Losses._checked_faces(f, V - 1, "t")
    f[7, 0] = -1
    with pytest.raises(ValueError, match=r"got \[-1, 3\]"):
        Losses._checked_faces(f, V, "t")


def test_an_unmodified_tensor_is_read_once(monkeypatch):
    """No second check of the same tensor at the same version (the read-back of a device tensor is a synchronisation), through a
    spy on Tensor.min; an edit, another V or another tensor reads again."""
    reads = []
    real_min = torch.Tensor.min
    monkeypatch.setattr(torch.Tensor, "min", lambda self, *a, **k: (reads.append(id(self)), real_min(self, *a, **k))[1])
    f = torch.tensor(GOOD)
    for _ in range(3):
        Losses._checked_faces(f, V, "t")
        Losses.closest_faces(POINTS, VERTS, f)
    assert reads.count(id(f)) == 1
    Losses._checked_faces(f, V + 1, "t")
    assert reads.count(id(f)) == 2
    f[0, 0] = 1
    Losses._checked_faces(f, V + 1, "t")
    Losses._checked_faces(f, V + 1, "t")
    assert reads.count(id(f)) == 3
    # the memo stays small and holds no tensor alive
    import gc
    import weakref
    for _ in range(200):
        Losses._checked_faces(torch.tensor(GOOD), V, "t")
    assert len(Losses._FACES_CHECKED) <= 65
    w = weakref.ref(f)
    del f
    gc.collect()
    assert w() is None


# ---- cameras._intrinsics -------------------------------------------------------------------------------------------------------------
def intr(focal, pp, B=1):
    f, p = cameras._intrinsics(focal, pp, B, torch.device("cpu"))
    assert f.shape == (B, 2) and p.shape == (B, 2) and f.dtype == torch.float32 and f.is_contiguous() and p.is_contiguous()
    return f.numpy().copy(), p.numpy().copy()


NB = 3


def at_the_same_address(buf, value):
    """A NEW tensor (version 0) of another value at the address of one that was dropped: both wrap one numpy buffer in turn."""
    buf[...] = value
    return torch.from_numpy(buf)


def test_intrinsics_follow_every_change_torch_can_see():
    cameras._INTR.clear()
    fbuf, pbuf = np.zeros((NB,), np.float32), np.zeros((NB, 2), np.float64)      # one focal per camera; pp in another dtype
    focal, pp = at_the_same_address(fbuf, 30.0), at_the_same_address(pbuf, 3.5)
    f, p = intr(focal, pp, NB)
    assert (f == 30.0).all() and (p == 3.5).all()
    a = cameras._intrinsics(focal, pp, NB, torch.device("cpu"))
    b = cameras._intrinsics(focal, pp, NB, torch.device("cpu"))
    assert a[0] is b[0] and a[1] is b[1], "the same pair at the same versions is remembered"
    # step 4: an edit in place bumps the version
    focal.mul_(2.0)
    assert (intr(focal, pp, NB)[0] == 60.0).all()
    focal[1] = 45.0
    assert (intr(focal, pp, NB)[0][1] == 45.0).all() and (intr(focal, pp, NB)[0][2] == 60.0).all()
    # step 5: a new tensor of another value at the dropped one's very address, 8 times
    for i in range(8):
        ptr = focal.data_ptr()
        del focal
        focal = at_the_same_address(fbuf, 50.0 + i)
        assert focal._version == 0 and focal.data_ptr() == ptr and (intr(focal, pp, NB)[0] == 50.0 + i).all()
    # step 6: the principal point likewise
    pp[1, 0] = 4.5
    assert (intr(focal, pp, NB)[1][1] == [4.5, 3.5]).all() and (intr(focal, pp, NB)[1][2] == 3.5).all()
    for i in range(8):
        ptr = pp.data_ptr()
        del pp
        pp = at_the_same_address(pbuf, 1.0 + i)
        assert pp._version == 0 and pp.data_ptr() == ptr and (intr(focal, pp, NB)[1] == 1.0 + i).all()
    # one of the two replaced while the other stays
    pp = torch.full((NB, 2), 6.0, dtype=torch.float64)
    assert (intr(focal, pp, NB)[1] == 6.0).all() and (intr(focal, pp, NB)[0] == 57.0).all()


def test_intrinsics_follow_b_under_unchanged_tensors():
    cameras._INTR.clear()
    focal, pp = torch.tensor([57.0]), torch.tensor([[8.0, 2.0]])
    for B in (1, 2, 3, 2, 1, 1):
        f, p = intr(focal, pp, B)
        assert (f == 57.0).all() and (p == [[8.0, 2.0]] * B).all()
    # numbers, not tensors, are never remembered
    for v in (12.0, 13.0):
        assert (cameras._intrinsics(v, ((1.0, 2.0),), 1, torch.device("cpu"))[0] == v).all()
    assert (intr(focal, pp)[0] == 57.0).all()


# ---- distributed._stripe_index --------------------------------------------------------------------------------------------------------
def stripe_index_by_hand(H, world, stripe_h):
    sets = [Stripes(H, r, world, stripe_h) for r in range(world)]
    hmax = max(s.h for s in sets)
    idx = np.full(H, -1, np.int64)
    for r, s in enumerate(sets):
        for j, row in enumerate(s.image_rows().tolist()):
            idx[row] = r * hmax + j
    return hmax, idx


def test_stripe_index_keys_that_share_two_numbers():
    configs = [(10, 2, 2), (10, 2, 1), (10, 3, 2), (12, 2, 2), (10, 2, 2), (7, 2, 2), (7, 1, 2), (10, 2, 1)]
    seen = {}
    for H, world, stripe_h in configs:
        hmax, idx = _stripe_index(H, world, stripe_h, "cpu")
        want_h, want = stripe_index_by_hand(H, world, stripe_h)
        assert hmax == want_h and idx.dtype == torch.int64 and (idx.numpy() == want).all(), (H, world, stripe_h)
        assert sorted(set(want.tolist())) == sorted(want.tolist()) and want.min() >= 0      # (a permutation into the padded rows)
        if (H, world, stripe_h) in seen:
            assert seen[(H, world, stripe_h)] is idx, "the same key is remembered"
        seen[(H, world, stripe_h)] = idx
    assert not (seen[(10, 2, 2)].numpy() == seen[(10, 2, 1)].numpy()).all()
    assert not (seen[(10, 2, 2)].numpy() == seen[(10, 3, 2)].numpy()).all()
