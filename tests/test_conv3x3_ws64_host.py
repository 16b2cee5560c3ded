"""Host check of the built library: every conv3x3_ws64 kernel is spill-free (zero scratch bytes in its code-object notes).  The kernel
is allocated max(producer, consumer) registers at 8 waves per block; a variant that spilled would not be offered."""
import os
import sys

import pytest


def test_ws64_kernels_carry_no_scratch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import codeobj_notes as cn
    so = os.path.join(root, "iea-gan_amd", "libieagan_hip.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    rows = [r for r in cn.kernels(so) if "conv3x3_ws64_kernel" in r["name"]]
    # (AFF, RELU) x RS forward forms, the masked and the BatchNorm-backward dgrad form, each FULL and partial-tile
    assert len(rows) == 20, len(rows)
    bad = [(r["name"], r["scratch"]) for r in rows if r["scratch"]]
    assert not bad, bad
