"""tests/dirty.py proven on host tensors: the wrapped allocators return filled memory, the wrappers are gone on exit (also after an
exception), and nothing outside the context is touched."""
import numpy as np
import pytest
import torch

import dirty as D

REAL = (torch.empty, torch.empty_like, torch.Tensor.new_empty)


def unpatched():
    return (torch.empty, torch.empty_like, torch.Tensor.new_empty) == REAL and "new_empty" not in torch.Tensor.__dict__


@pytest.mark.parametrize("pattern", [0x00, 0x7F, 0xFF], ids=D.pattern_id)
def test_the_wrapped_allocators_return_filled_memory(pattern):
    like = torch.zeros((3, 5, 2)).permute(2, 0, 1)      # (a dense layout that is not contiguous: empty_like preserves it)
    with D.dirty(pattern, devices=("cpu",), only=None) as d:
        made = [torch.empty((7, 3), dtype=torch.float32), torch.empty(5, dtype=torch.int32), torch.empty((2, 3), dtype=torch.int64),
                torch.empty((4,), dtype=torch.int16), torch.empty((9,), dtype=torch.uint8), torch.empty((), dtype=torch.float32),
                torch.empty((0, 3)), torch.empty_like(like), torch.empty_like(torch.zeros(6, dtype=torch.int32)),
                torch.zeros(3).new_empty((4, 2)), torch.zeros(3, dtype=torch.int32).new_empty(11)]
        assert d.filled == len(made)
    assert made[7].stride() == like.stride()
    for t_ in made:
        raw = t_.contiguous().reshape(-1).view(torch.uint8).numpy()
        assert (raw == pattern).all(), (t_.dtype, tuple(t_.shape))
    # what the patterns are, as the kernels see them
    f, i = made[0].numpy().ravel(), made[1].numpy().ravel()
    if pattern == 0x7F:
        assert (f == np.array([0x7F7F7F7F], np.uint32).view(np.float32)[0]).all() and 3.39e38 < f[0] < 3.40e38 and (i == 2139062143).all()
    elif pattern == 0xFF:
        assert np.isnan(f).all() and (i == -1).all() and (made[4].numpy() == 255).all()
    else:
        assert (f == 0).all() and (i == 0).all()


def test_only_the_named_devices_are_filled_and_values_elsewhere_stay():
    keep = torch.arange(12, dtype=torch.float32)
    copy = keep.clone()
    with D.dirty(0xFF) as d:      # devices=("cuda",): a host result passes through as it is
        entered = d.filled        # (with a device present the entry itself grows the cached scratch through ops._workspace: one fill)
        assert entered in (0, 1)
        a = torch.empty(4)
        a.fill_(2.0)
        b = torch.empty_like(keep)
        torch.zeros(3).new_empty(5)
        assert d.filled == entered
    assert (a == 2.0).all() and b.shape == keep.shape and torch.equal(keep, copy)
    with D.dirty(0x7F, devices=("cpu",), only=None):
        torch.empty(100)
        c = keep + 1      # (torch's own allocations are not the wrappers' business)
    assert torch.equal(keep, copy) and torch.equal(c, copy + 1)


def test_the_wrappers_are_undone_on_exit_and_after_an_exception():
    assert unpatched()
    with D.dirty(0x7F, devices=("cpu",), only=None):
        assert torch.empty is not REAL[0] and torch.empty_like is not REAL[1] and torch.Tensor.new_empty is not REAL[2]
    assert unpatched()
    with pytest.raises(RuntimeError, match="inside"):
        with D.dirty(0xFF, devices=("cpu",), only=None):
            assert torch.empty is not REAL[0]
            raise RuntimeError("inside")
    assert unpatched()
    # nested: the inner exit gives the outer's wrappers back, the outer exit the real functions
    with D.dirty(0x00, devices=("cpu",), only=None) as outer:
        mine = torch.empty
        with D.dirty(0xFF, devices=("cpu",), only=None):
            assert np.isnan(torch.empty(3).numpy()).all()
        assert torch.empty is mine and (torch.empty(3) == 0).all() and outer.filled > 0
    assert unpatched()
    assert torch.isfinite(torch.zeros(3).new_empty(0)).all()      # (and the real ones work)


def test_leftovers_fills_nothing_and_runs_the_other_entry_point():
    ran = []
    with D.dirty("leftovers", devices=("cpu",), only=None, before=lambda: ran.append(1)) as d:
        assert torch.empty is REAL[0] and torch.empty_like is REAL[1] and ran == [1]
        d.refill()
        assert ran == [1, 1] and d.filled == 0
    assert unpatched()


def test_an_unknown_pattern_is_refused():
    with pytest.raises(AssertionError):
        with D.dirty(0x55):
            pass
    assert unpatched()


def test_only_the_librarys_own_allocations_are_filled():
    """only=("voge_amd",), the default: torch.empty called from this module comes back as it is, the one inside
    voge_amd.distributed._stripe_index is filled -- and, being written completely, gives the same index."""
    from voge_amd import distributed
    want = distributed._stripe_index(11, 3, 2, "cpu")[1].clone()
    distributed._STRIPE_INDEX.clear()
    with D.dirty(0x7F, devices=("cpu",)) as d:
        mine = torch.empty(5)
        assert d.filled == 0
        got = distributed._stripe_index(11, 3, 2, "cpu")[1]
        assert d.filled == 1
    assert torch.equal(got, want) and unpatched() and mine.shape == (5,)
    distributed._STRIPE_INDEX.clear()
