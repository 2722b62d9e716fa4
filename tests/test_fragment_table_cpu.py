"""CPU checks of the fused backward's accumulation table: the resource envelope of the flagship instantiation read from the
gfx950 code object's metadata (its occupancy is what the kernel's time hangs on: 256 table entries once cost 17 us through
it), and the probe sequence's arithmetic."""
import os

import numpy as np
import pytest

from test_isa_cpu import HIPCC, _asm, _field, _kernel

LDS_PER_CU = 160 * 1024      # MI355X


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_flagship_backward_resource_envelope(tmp_path):
    text = _asm("fragment_bwd", tmp_path)
    # <SRC 0, C 3, NS 2, u32 offsets, ISO, NOAD>: the kernel of the frame bench.py times
    body, desc = _kernel(text, "fragment_bwd_kernelILi0ELi3ELi2EjLb1ELb1ELb0E")
    vgpr, lds = _field(desc, "amdhsa_next_free_vgpr"), _field(desc, "amdhsa_group_segment_fixed_size")
    print(f"flagship fused backward: {vgpr} VGPRs, {lds} bytes of LDS = {LDS_PER_CU // lds} workgroups per CU by LDS")
    assert vgpr <= 128
    assert _field(desc, "amdhsa_private_segment_fixed_size") == 0, "scratch"
    assert "SGPR spill" not in body and "v_writelane_b32" not in body
    assert LDS_PER_CU // lds >= 16, (lds, "fewer than 16 waves per CU fit by LDS")
    # every other two-slots-per-lane instantiation: no fewer workgroups per CU by LDS than with the 128-slot table it replaced
    # (6640 / 8688 / 10736 / 12784 bytes for 1 / 2 / 3 / 4 float4s per entry)
    before = {1: 6640, 2: 8688, 3: 10736, 4: 12784}
    for frag, nv4 in (("fragment_bwd_kernelILi1ELi0ELi2EjLb1ELb1ELb0E", 1), ("fragment_bwd_kernelILi2ELi0ELi2EjLb1ELb1ELb0E", 1),
                      ("fragment_bwd_kernelILi1ELi0ELi2EjLb0ELb1ELb1E", 2), ("fragment_bwd_kernelILi0ELi3ELi2EjLb0ELb1ELb1E", 3),
                      ("fragment_bwd_kernelILi1ELi0ELi2EjLb0ELb1ELb0E", 3), ("fragment_bwd_kernelILi0ELi3ELi2EjLb0ELb1ELb0E", 4)):
        _, d = _kernel(text, frag)
        assert LDS_PER_CU // _field(d, "amdhsa_group_segment_fixed_size") >= LDS_PER_CU // before[nv4], frag


@pytest.mark.parametrize("bits", [8, 9])
def test_double_hash_sequence_visits_every_directory_slot(bits):
    """wd_find2's sequence for 256 / 512 slots: start = the top bits of id * 2654435761, step = the next ones | 1 (odd)."""
    nd = 1 << bits
    ids = np.arange(0, 200000, 37, dtype=np.int64)
    prod = (ids * 2654435761) & 0xFFFFFFFF
    start, step = prod >> (32 - bits), ((prod >> (32 - 2 * bits)) & (nd - 1)) | 1
    assert (step % 2 == 1).all() and len(np.unique(step)) == nd // 2 and start.max() < nd
    seq = (start[:, None] + step[:, None] * np.arange(nd)[None]) & (nd - 1)
    assert (np.sort(seq, axis=1) == np.arange(nd)[None]).all()
