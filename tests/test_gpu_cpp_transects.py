"""rc::Transects (include/rcflow_module.hpp) against the C ABI, in the program tests/cpp/test_transects.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_transects_against_the_c_abi(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program pushes frames it makes itself through the class and through
    the C ABI on a second context, and compares every output byte for byte"""
    _cpp.run("test_transects", tmp_path, 9)
