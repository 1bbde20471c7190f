"""rc::Shoreline (include/rcflow_module.hpp) on a step picture, in the program tests/cpp/test_shoreline.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_shoreline_on_the_step_picture(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program pushes a sand / water step through the class and holds mask,
    plane, records, summary and ring to numbers it computes itself"""
    _cpp.run("test_shoreline", tmp_path)
