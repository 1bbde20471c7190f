"""rc::Offshore (include/rcflow_module.hpp) against the C ABI it wraps, in the program tests/cpp/test_offshore.cpp."""
import pytest

import _cpp

pytestmark = pytest.mark.gpu


def test_cpp_offshore_equals_the_entry_points_and_the_prototype(tmp_path):
    """compiled with the flags of tests/cpp's test_module: the program runs the prototype (96 x 64, a cuspate shore, a jet in columns
    48..59, one NaN) through the class, holds both summaries, the sums of near, r, cross and along, the mask and band counts, station
    4's bins and every station's reach to the figures compiled in, the planes to what must be true of them, and gets the same near
    plane, cross / along field, table, records and summaries from the entry points called directly"""
    _cpp.run("test_offshore", tmp_path)
