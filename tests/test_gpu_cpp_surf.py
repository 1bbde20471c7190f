"""rc::Surf (include/rcflow_module.hpp) on a two-level picture with one gap, in the program tests/cpp/test_surf.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_surf_on_the_band_with_a_gap(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program alternates a band with a hole and plain water through the
    class and holds the six pictures, the line records, the channel and the summary to numbers it computes itself"""
    _cpp.run("test_surf", tmp_path)
