"""The six-term product of the other forward kernels of the split family, bit for bit: rd_gconv_split and rd_gconv_split_pre at 3x3
and 1x1 (rd_gconv_split routes one-tap descriptors to gemm1_split: plan marker 1000), rd_gemm_taps_split on a k = 2 deconvolution
forward, rd_conv16_split -- each on the three integer-lattice classes of tests/wino_cases.py (A: the activation's three pieces, B: the
weight's three pieces, C: the cross term; the dropped products exactly zero), against desc_emulator.run_desc in float64.  Every
intermediate is an integer below 2^24 quanta (asserted with the data), so the stored output IS the float64 result: no tolerance.
tests/test_wino_host.py shows that removing any kept term changes the class meant for it.

Observed on an MI355X when the file was added: all six kernels hold all three classes bit for bit (the hardware premise -- the bf16 MFMA
loses no bits of sums that are exact in fp32 -- holds); a library built without the a2 b0 product fails class A on every kernel that
goes through RD_SPLIT_TERMS."""
import pytest

import wino_cases as WC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cls", sorted(WC.LATTICE))
@pytest.mark.parametrize("kernel", WC.FLAT_KERNELS)
def test_split_family_lattice_bit_for_bit(kernel, cls):
    marker, n_bad, first = WC.run_flat(kernel, cls)
    print("LATTICE %-26s class %s plan marker %s differing elements: %d %s" % (kernel, cls, marker, n_bad, first))
    if kernel == "gconv_split_1x1":
        assert marker == 1000, "the one-tap descriptor runs on gemm1_split"
    assert n_bad == 0, (kernel, cls, n_bad, first)
