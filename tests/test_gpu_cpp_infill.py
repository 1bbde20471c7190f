"""rc::Infill (include/rcflow_module.hpp) against the C ABI it wraps, in the program tests/cpp/test_infill.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_infill_equals_the_entry_points_and_the_statement(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program pushes a field made from integers with the hole pattern p900
    and a NaN through the class, holds summary, cell sums and records to the figures tests/_infill_ref.py printed for the case
    (7 levels; then 2 levels, min_known 2, zero left), the pictures to what must be true of them, and gets the same source bytes,
    filled field, sums, records and summary from the entry points called directly"""
    _cpp.run("test_infill", tmp_path)
