"""The headline rollout kernel's step loop starts on an 8-byte boundary in the built library.

fdr_rollout_pair.hip pads the code ahead of the loop (FDR_STEP_LOOP_PLACED): the same 1,203 instructions measured
~0.9 % faster per FD step with the loop's first instruction on an 8-byte boundary than 4 bytes off one (DESIGN.md 3.0
p14).  The padding counts on the size of the loop set-up the compiler puts behind it; this pins the result.
"""
import os
import shutil

import pytest

import tools.isa_hazards as ih
import tools.prologue_mix as pm


@pytest.mark.skipif(not os.path.exists(ih.DEFAULT_SO) or not shutil.which(os.path.join(ih.LLVM, "llvm-objdump")),
                    reason="libfdr.so or llvm-objdump missing")
def test_pair_kernel_step_loop_starts_on_an_8_byte_boundary():
    head = pm.placement(ih.DEFAULT_SO, "rollout_pair_kernelILi17ELi6ELb0ELi0E")
    assert head % 8 == 0, hex(head)
