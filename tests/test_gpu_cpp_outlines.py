"""rc::Outlines (include/rcflow_module.hpp) against the C ABI it wraps, in the program tests/cpp/test_outlines.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_outlines_equals_the_entry_points_and_the_statement(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program traces 96 x 64 labels (a rectangle with a hole, a disc, a
    diagonal pair) through the class, holds the summary and every record to the figures of tests/_outlines_ref.py compiled in, every
    polygon to being closed, rectilinear and of the record's area, the mask path, the filter and a refused open, and gets the same
    records, vertices, summary and drawing from the entry points called directly"""
    _cpp.run("test_outlines", tmp_path)
