"""Runs tests/cpp/test_staging.cpp: the staging layer of include/rcflow_module.hpp on padded host images and on wrong views."""
import pytest

import _cpp


@pytest.mark.gpu
def test_cpp_staging_padded_rows_and_refusals(tmp_path):
    """Every class of the C++ mirror on a 37 x 23 pipeline, twice: with dense host images and with every host image on rows of
    row_bytes() + 5.  The program itself fails unless every output pixel and every record read back is equal between the two,
    the padding is untouched, and every wrong view of every host-image argument is refused with RC_EINVAL and changes nothing."""
    _cpp.run("test_staging", tmp_path)
