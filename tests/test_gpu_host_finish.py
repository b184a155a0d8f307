"""GPU: whole fits (fit_resident with RIDGE, LSTSQ_PROBE and RIDGE_INV, and a fit_resident + solve_device(rhs) pair that
re-uses the factor) give the same bits with the fused host finish as with the separate steps (FSNAP_CHOL_VARIANT=3), on
shapes that read the upper-triangle mirror (4 096 x 128, masked), pad to a half chunk (1 303 x 142), run 96 columns, and
go through the packed mirror (3 000 x 200).  Inside each process the coefficients of fit_resident are byte-equal to the
host solve on the statistics the fit left on the device (asserted by the worker)."""
import pytest

from test_host_finish_cpu import compare, run_worker

pytestmark = pytest.mark.gpu


def test_fits_have_the_same_bits_with_fused_and_separate_host_finish():
    fused, legacy = run_worker("gpu", None), run_worker("gpu", "3")
    assert len(fused) == 3 * 4 * 2 + 3 + 1
    compare(fused, legacy)
