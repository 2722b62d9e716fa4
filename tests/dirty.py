"""Dirty state between calls: what a library call finds in its scratch and in its freshly allocated outputs, made hostile on purpose.

A fit of hundreds of iterations hands every entry point of voge_amd/ops.py the scratch buffer the previous entry point left
(ops._WS, one per (device, stream)) and output tensors from torch.empty whose bytes are whatever the allocator's block held.  A
fresh test process hides both: new blocks tend to hold what an identical test left there.  `with dirty(pattern):` takes that luck
away for the library calls inside it:

  * the cached scratch buffer of the current (device, stream) is first grown to `grow` bytes (so that no call under test
    replaces it by a fresh allocation) and byte-filled with the pattern -- on entry, on refill(), and again every time an entry
    point takes it (ops._workspace is wrapped; an entry point owns the scratch from there to its return, so nothing is lost);
  * torch.empty, torch.empty_like and Tensor.new_empty are wrapped: the whole storage of every result on a device in `devices`
    is byte-filled with the pattern before the caller sees it.  ops.py binds them at call time, so the wrappers reach it.
    Only allocations made by the modules named in `only` (default: voge_amd's) are filled -- the patch is active around the
    library's own calls and never around a reference computed beside them -- and nothing is filled under stream capture (a
    fill would become part of the graph);
  * pattern "leftovers" fills nothing and wraps nothing: `before()` -- another entry point -- runs on entry and on refill(), and
    the call under test finds what it left.

Patterns: 0x00; 0x7F (every float 3.39e38, every int32 2139062143); 0xFF (every float a NaN, every int -1, every unsigned counter
full); "leftovers".  The wrappers are pytest's MonkeyPatch's, undone on exit whether or not the body raised.  This exposes a read-before-write as a wrong VALUE on a path DESIGN.md "State between
calls" has already traced to its writer; it is no tool for finding faults."""
import contextlib
import sys

import pytest
import torch

PATTERNS = ("leftovers", 0x00, 0x7F, 0xFF)
GROW = 1 << 22      # 4 MiB: above the scratch of every case of tests/test_gpu_dirty_scratch.py (asserted there: see `taken`)


def pattern_id(p):
    return p if isinstance(p, str) else f"0x{p:02X}"


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class _Dirty:
    def __init__(self, pattern, devices, grow, before, only):
        self.pattern, self.devices, self.grow, self.before = pattern, tuple(devices), int(grow), before
        self.only = None if only is None else tuple(only)      # prefixes of the module names whose allocations are filled
        self.filled = 0          # results of the wrapped allocators that were filled
        self.taken = []          # (bytes asked for, bytes of the buffer handed out) per ops._workspace call inside the context
        self._empty, self._workspace = torch.empty, None      # (the unwrapped functions)

    def fill(self, t, caller=""):
        """Byte-fill the whole storage behind a freshly allocated tensor (any dtype, layout or size) -> the tensor."""
        if t.device.type not in self.devices or (t.is_cuda and _capturing()):
            return t
        if self.only is not None and not any(caller == m or caller.startswith(m + ".") for m in self.only):
            return t
        st = t.untyped_storage()
        if st.nbytes():
            self._empty(0, dtype=torch.uint8, device=t.device).set_(st).fill_(self.pattern)
        self.filled += 1
        return t

    def refill(self):
        """Before a call under test: the scratch of the current (device, stream) holds the pattern again / `before()` ran again."""
        if self.pattern == "leftovers":
            if self.before is not None:
                self.before()
        elif self._workspace is not None and not _capturing():
            self._workspace(torch.device("cuda", torch.cuda.current_device()), self.grow).fill_(self.pattern)


@contextlib.contextmanager
def dirty(pattern, devices=("cuda",), grow=GROW, before=None, only=("voge_amd",)):
    """See the module's docstring.  -> the _Dirty in charge: refill(), filled, taken."""
    assert pattern in PATTERNS, pattern
    d = _Dirty(pattern, devices, grow, before, only)

    def who():
        return sys._getframe(2).f_globals.get("__name__", "")      # (the module that called the wrapper)
    with pytest.MonkeyPatch.context() as mp:
        if pattern != "leftovers":
            real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty
            d._empty = real_empty
            mp.setattr(torch, "empty", lambda *a, **k: d.fill(real_empty(*a, **k), who()))
            mp.setattr(torch, "empty_like", lambda *a, **k: d.fill(real_like(*a, **k), who()))
            mp.setattr(torch.Tensor, "new_empty", lambda self, *a, **k: d.fill(real_new(self, *a, **k), who()))
            if "cuda" in d.devices and torch.cuda.is_available():
                from voge_amd import ops
                real_ws = d._workspace = ops._workspace

                def workspace(dev, nbytes):
                    ws = real_ws(dev, max(int(nbytes), d.grow))
                    d.taken.append((int(nbytes), ws.numel()))
                    if not _capturing():
                        ws.fill_(pattern)
                    return ws

                mp.setattr(ops, "_workspace", workspace)
        d.refill()
        yield d
