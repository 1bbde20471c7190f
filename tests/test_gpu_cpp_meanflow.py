"""rc::MeanFlow (include/rcflow_module.hpp) on the scene the product is named for, in the program tests/cpp/test_meanflow.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_meanflow_names_the_jet(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program pushes 20 fields of waves, noise and a jet through the class
    and holds the mask, the mean, the steadiness, the picture, the records and the summary to numbers it computes itself"""
    _cpp.run("test_meanflow", tmp_path)
