"""The constant-geometry envelope kernels run Q on accumulator 0's tap fragments (minimal-sdr_amd/csrc/msdr_chain_mfw.hiph, burst_geom and
mw_q_squares): per dense k-step one bh | bl fragment pair feeds both accumulators, the merged step's th | tl | index are read once.  What
that buys is LDS reads inside the FIR burst, so this test counts them in the PRODUCT binary, the way tests/test_mfw_geom_static.py counts
the burst's matrix instructions: in every stretch from `s_setprio 3` to the next `s_setprio 1` of the four chain_mfw_geom_kernel
instantiations at most 6 D + 11 `ds_read*` (D = dense steps per accumulator: 2 window reads each for I and Q and 2 fragment reads per
dense step; 8 window reads and 3 reads of the merged step) -- 53 at 256 taps, 101 at 512.  Two separate sequences need 8 D + 14 (70 and
134; the compiler merged one read away at 256 taps: 69 and 134 in the build before this one), which is over the bound: the test fails on a
burst that reads accumulator 1's fragments on their own.  The realignment and the tile
carry sit behind `s_setprio 1`: no lane permute and no read-lane inside the burst.  No GPU needed."""
import subprocess

import pytest

from test_chain_kernel_no_scratch import OBJDUMP, code_object, kernels_of
from test_mfw_geom_static import bursts, count, geometry_of, needs_tools


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("mfw_iq"))
    text = "\n".join(subprocess.run([OBJDUMP, "-d", co], check=True, stdout=subprocess.PIPE, text=True).stdout for co in code_object(tmp))
    return kernels_of(text, "chain_mfw_geom_kernel")


@needs_tools
def test_the_burst_reads_one_fragment_pair_per_dense_step_for_both_accumulators(kernels):
    assert len(kernels) == 4, sorted(kernels)
    seen = set()
    for name, ins in kernels.items():
        g = geometry_of(name)
        dense_per_acc = {cnt - 2 * mg for _, cnt, mg in g["runs"] if cnt}
        assert len(dense_per_acc) == 1, (name, g)
        d = dense_per_acc.pop()
        bound = 6 * d + 11
        bs = bursts(ins)
        assert len(bs) == 2, (name, len(bs))                                 # the hot and the cold tile
        for b in bs:
            reads = count(b, "ds_read")
            print(name[:60], "dense steps per accumulator", d, "ds_read in the burst", reads, "bound", bound, "of", len(b), "instructions")
            assert reads <= bound, (name, reads, bound)
            assert count(b, "v_permlane") == 0 and count(b, "v_readlane_b32") == 0, name
        seen.add((g["halo"], bound))
    assert seen == {(288, 53), (544, 101)}, seen


@needs_tools
def test_the_realignment_sits_behind_the_burst(kernels):
    # four v_permlane32_swap_b32 of mw_q_squares per tile body, beside the ones the cascade phase already had: more than in the burst (none)
    for name, ins in kernels.items():
        assert count(ins, "v_permlane32_swap") >= 2 * 4, (name, count(ins, "v_permlane32_swap"))
