"""CPU test of the nine geometry workspace-size entries: every value below was recorded from the library as it was BEFORE the layouts
moved onto voge_common.h's carving vocabulary (up16, Carve), and a refactor of a layout must return the same bytes -- the Python side
allocates what these entries say and the kernels index what the layouts say.  No GPU: a size entry makes no HIP call.

The item counts sit around the 256-item blocks, the 4 096-item scan tiles, at 10^6 and at the largest size the entries take.  Entries
of one or two arguments get every combination; those of three get every count for every single argument (the others at 4 097) and
every combination of (1, 4 097, 2^28 - 1); knn gets every count on five grids from 1 x 1 x 1 to 1024 x 1024 x 1 (a grid with more
cells than max(8 N, 2^15) is refused: 0)."""
import itertools
import os

import pytest

BIG = 2 ** 28 - 1
COUNTS = (1, 255, 256, 257, 4095, 4096, 4097, 10 ** 6, BIG)
MID, CORNERS = 4097, (1, 4097, BIG)
GRIDS = ((1, 1, 1), (2, 3, 5), (32, 32, 32), (1024, 32, 1), (1024, 1024, 1))


def _product(nargs):
    return list(itertools.product(COUNTS, repeat=nargs))


def _thinned(nargs):
    single = [tuple(c if i == pos else MID for i in range(nargs)) for pos in range(nargs) for c in COUNTS]
    return list(dict.fromkeys(single + list(itertools.product(CORNERS, repeat=nargs))))


# entry -> the argument tuples, in the order of EXPECTED's values
CASES = {
    "voge_knn_workspace_bytes": [(n,) + g for g in GRIDS for n in COUNTS],
    "voge_chamfer_workspace_bytes": _product(2),
    "voge_mesh_sample_workspace_bytes": _thinned(3),
    "voge_point_mesh_workspace_bytes": _thinned(3),
    "voge_point_mesh_grid_workspace_bytes": _thinned(3),
    "voge_vertex_normals_workspace_bytes": _product(1),
    "voge_mesh_simplify_workspace_bytes": _product(2),
    "voge_mesh_simplify_acc_bytes": [(n, q) for q in (0, 1) for n in COUNTS],
    "voge_mesh_simplify_attr_workspace_bytes": _product(1),
}

# entry -> (the arguments that are item counts, the smallest count it takes)
COUNT_ARGS = {
    "voge_knn_workspace_bytes": (1, 0),
    "voge_chamfer_workspace_bytes": (2, 1),
    "voge_mesh_sample_workspace_bytes": (3, 1),      # (S, the third, may be 0: see below)
    "voge_point_mesh_workspace_bytes": (3, 1),
    "voge_point_mesh_grid_workspace_bytes": (3, 1),
    "voge_vertex_normals_workspace_bytes": (1, 1),
    "voge_mesh_simplify_workspace_bytes": (2, 1),
    "voge_mesh_simplify_acc_bytes": (1, 1),
    "voge_mesh_simplify_attr_workspace_bytes": (1, 1),
}

EXPECTED = {
    "voge_knn_workspace_bytes": [
        80, 5152, 5168, 5200, 81952, 81968, 82000, 20000048, 5368709152, 304, 5376, 5392, 5424, 82176, 82192, 82224, 20000272,
        5368709376, 262256, 267328, 267344, 267376, 344128, 344144, 344176, 20262224, 5368971328, 262256, 267328, 267344, 267376,
        344128, 344144, 344176, 20262224, 5368971328, 0, 0, 0, 0, 0, 0, 0, 28390672, 5377099776],
    "voge_chamfer_workspace_bytes": [
        524672, 530752, 530768, 530816, 622976, 623024, 623232, 152054896, 40816869408, 530752, 536832, 536848, 536896, 629088,
        629104, 629312, 152060976, 40816875520, 530768, 536848, 536864, 536912, 629104, 629120, 629328, 152060992, 40816875536,
        530816, 536896, 536912, 536960, 629152, 629168, 629376, 152061040, 40816875584, 622976, 629088, 629104, 629152, 721280,
        721296, 721536, 152153232, 40816967712, 623024, 629104, 629120, 629168, 721296, 721312, 721584, 152153248, 40816967728,
        623232, 629312, 629328, 629376, 721536, 721584, 721632, 152153296, 40816967808, 152054896, 152060976, 152060992, 152061040,
        152153232, 152153248, 152153296, 176078272, 40840892816, 40816869408, 40816875520, 40816875536, 40816875584, 40816967712,
        40816967728, 40816967808, 40840892816, 47265611712],
    "voge_mesh_sample_workspace_bytes": [
        98368, 104464, 104496, 104512, 196624, 196656, 196672, 24098352, 6442549264, 98368, 104464, 104496, 104512, 196624, 196656,
        24098352, 6442549264, 196672, 196672, 196672, 196672, 196672, 196672, 196672, 196672, 64, 64, 64, 98368, 98368, 6442450960,
        6442450960, 6442450960, 98368, 98368, 6442549264, 6442549264, 6442450960, 6442450960, 6442450960, 6442549264, 6442549264,
        12884901856, 12884901856, 12884901856],
    "voge_point_mesh_workspace_bytes": [
        98352, 104448, 104472, 104496, 196608, 196632, 196656, 24098328, 6442549248, 196656, 196656, 196656, 196656, 196656, 196656,
        4028192, 1076904032, 98352, 104448, 104472, 104496, 196608, 196632, 24098328, 6442549248, 64, 98352, 6442450944, 16496,
        6442450944, 1076887600, 1076904032, 6442450944, 98352, 6442549248, 1076887600, 6442549248, 6442450944, 6442549248,
        12884901840, 6442450944, 12884901840, 6442450944, 6442549248, 12884901840],
    "voge_point_mesh_grid_workspace_bytes": [
        934672, 934672, 934672, 934672, 934688, 934720, 934720, 24098328, 6442549248, 623360, 642640, 642704, 642816, 934528,
        934592, 204145552, 54773514400, 836320, 842400, 842416, 842464, 934624, 934672, 152366384, 40817180896, 524752, 623312,
        40816869488, 836272, 40817180848, 54773415952, 54773514352, 61222158224, 524800, 40816869536, 54773416000, 61222158272,
        6442450944, 6442549248, 40820015216, 6442450944, 40820326576, 54776561648, 54776660048, 61225303952],
    "voge_vertex_normals_workspace_bytes": [
        48, 8176, 8208, 8240, 131056, 131088, 131120, 32000016, 8589934576],
    "voge_mesh_simplify_workspace_bytes": [
        136, 5968, 5984, 8064, 94352, 94368, 127168, 23404320, 6178209872, 3920, 7728, 7728, 9808, 96112, 96112, 128912, 23406064,
        6178211632, 3936, 7728, 7728, 9824, 96112, 96112, 128928, 23406064, 6178211632, 6016, 9808, 9824, 9856, 96144, 96160,
        128960, 23406128, 6178211664, 61584, 65392, 65392, 65424, 123040, 123040, 155856, 23433008, 6178238560, 61600, 65392, 65392,
        65440, 123040, 123040, 155872, 23433008, 6178238560, 94400, 98192, 98208, 98240, 155856, 155872, 155904, 23433056,
        6178238608, 15404320, 15408112, 15408112, 15408176, 15465776, 15465776, 15465824, 30419904, 6185225456, 4030726224,
        4030730032, 4030730032, 4030730064, 4030787680, 4030787680, 4030787728, 4045741808, 8061452320],
    "voge_mesh_simplify_acc_bytes": [
        32, 8160, 8192, 8224, 131040, 131072, 131104, 32000000, 8589934560, 112, 28560, 28672, 28784, 458640, 458752, 458864,
        112000000, 30064770960],
    "voge_mesh_simplify_attr_workspace_bytes": [
        88, 18376, 18448, 18520, 294856, 294928, 295000, 72000016, 19327352776],
}


@pytest.fixture(scope="module")
def lib():
    from voge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_the_tables_cover_what_they_say():
    assert sorted(CASES) == sorted(EXPECTED) == sorted(COUNT_ARGS) and len(CASES) == 9
    for name, cases in CASES.items():
        assert len(cases) == len(set(cases)) == len(EXPECTED[name]), name
        for pos in range(COUNT_ARGS[name][0]):      # every count for every single argument
            assert {c[pos] for c in cases} == set(COUNTS), (name, pos)
        n = COUNT_ARGS[name][0]
        assert {c[:n] for c in cases} >= set(itertools.product((1, BIG), repeat=n)), name      # the extremes in combination


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_size_is_the_recorded_one(lib, name):
    entry = getattr(lib, name)
    got = [entry(*args) for args in CASES[name]]
    wrong = [(args, g, e) for args, g, e in zip(CASES[name], got, EXPECTED[name]) if g != e]
    assert not wrong, f"{name}: {len(wrong)} of {len(got)} sizes differ from the recorded ones, the first (arguments, got, recorded): {wrong[0]}"
    assert any(got) and all(g % 8 == 0 for g in got), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_out_of_range_give_zero(lib, name):
    entry = getattr(lib, name)
    nargs, smallest = COUNT_ARGS[name]
    tail = {"voge_knn_workspace_bytes": (2, 3, 5), "voge_mesh_simplify_acc_bytes": (1,)}.get(name, ())
    assert entry(*((MID,) * nargs + tail)) > 0
    for pos in range(nargs):
        low = -1 if name == "voge_mesh_sample_workspace_bytes" and pos == 2 else smallest - 1      # (no samples: the areas alone)
        for bad in (low, -1, BIG + 1, 2 ** 31, 2 ** 40):
            args = tuple(bad if i == pos else MID for i in range(nargs)) + tail
            assert entry(*args) == 0, (name, args)
    if name == "voge_knn_workspace_bytes":
        for g in ((0, 1, 1), (1, 1025, 1), (1, 1, -1), (64, 64, 64)):      # (the last: 2^18 cells for 4 097 points)
            assert entry(MID, *g) == 0, g
