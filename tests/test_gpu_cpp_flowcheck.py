"""rc::FlowCheck (include/rcflow_module.hpp) against the C ABI it wraps, in the program tests/cpp/test_flowcheck.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_flowcheck_equals_the_entry_points(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program pushes a moving integer pattern with a true field, a patch of
    wrong vectors, a NaN and a backward field through the class, holds flags, mask, checked field, picture, records and summary to
    what must be true of them, and gets the same flags, mask, sums, records and summary from the entry points called directly"""
    _cpp.run("test_flowcheck", tmp_path)
