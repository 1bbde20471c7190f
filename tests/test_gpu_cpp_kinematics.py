"""rc::Kinematics (include/rcflow_module.hpp) on the rotation field, in the program tests/cpp/test_kinematics.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_kinematics_on_the_rotation_field(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program pushes the analytic rotation field through the class and
    holds planes, mask, picture, records, sums and summary to numbers it computes itself"""
    _cpp.run("test_kinematics", tmp_path)
