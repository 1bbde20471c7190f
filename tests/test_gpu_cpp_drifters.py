"""rc::Drifters (include/rcflow_module.hpp) against the entry points called directly, in the program tests/cpp/test_drifters.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_drifters_census_of_a_column_jet(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program seeds a lattice into a field of columns that flow seaward in
    one band and shoreward elsewhere, holds the census, the records, the histograms and the pictures to what it computes itself,
    and runs the same session through the class and through the C ABI"""
    _cpp.run("test_drifters", tmp_path)
