"""Registers and LDS of the pair expansion, from the kernel descriptor of the cross-compiled unit (no GPU needed).

Every workgroup of the C3 expansion launch must be resident at once: 1 594 workgroups on 256 CUs, seven four-wave workgroups per CU
(decision 14a: a launch whose last few workgroups run as a second round loses a third of the kernel).  Seven
waves per SIMD of 512 vector registers, allocated in blocks of 8, need at most 72; seven workgroups in a CU's 160 KB of LDS need at
most 23 405 bytes each, static plus the finished-tile rows of a later slab (1 088 bytes at 1920 x 1080).  Two empty asm
statements and a launch bound hold the kernel there: a compiler that stops honouring them fails here, not in a benchmark."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DONE_ROWS_1080P = 68 * 4 * 4   # grid_y tile rows x row_words x 4 bytes


def test_expand_kernel_fits_seven_workgroups_per_cu():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_isa_census as census
    finally:
        sys.path.pop(0)
    from autovfx_amd import build
    c = census.census(census.assembly(build.CSRC, "gsr_binning.hip"), "expand_kernel")
    print(c)
    assert c["vgpr"] <= 72, f"expand_kernel needs {c['vgpr']} vector registers: fewer than seven waves per SIMD"
    assert c["scratch"] == 0, f"expand_kernel spills {c['scratch']} bytes per lane"
    assert 7 * (c["lds_bytes"] + DONE_ROWS_1080P) <= 160 * 1024, f"expand_kernel's {c['lds_bytes']} bytes of LDS: fewer than seven workgroups per CU"
