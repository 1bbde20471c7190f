"""Known answers for the numpy restatement of the time-exposure pipelines (tests/_timex_ref.py), which the GPU tests
compare the kernels against, and a compile check of the C++ host mirror's time-exposure methods.  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _timex_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def px(*rgb):
    return np.array([[rgb]], np.uint8)


@pytest.mark.parametrize("rgb, hsv", [
    ((255, 0, 0), (0, 255, 255)), ((0, 255, 0), (60, 255, 255)), ((0, 0, 255), (120, 255, 255)),
    ((255, 255, 0), (30, 255, 255)), ((0, 255, 255), (90, 255, 255)), ((255, 0, 255), (150, 255, 255)),
    ((0, 0, 0), (0, 0, 0)), ((77, 77, 77), (0, 0, 77)), ((255, 255, 255), (0, 0, 255)),
    ((128, 64, 64), (0, 128, 128)), ((255, 0, 64), (172, 255, 255)),    # (-64 * 482 + 2048) >> 12 = -8, shifted arithmetically
])
def test_rgb_to_hsv_known_answers(rgb, hsv):
    assert tuple(R.rgb_to_hsv_u8(px(*rgb))[0, 0]) == hsv


def test_hsv_tables():
    assert R.SDIV[0] == 0 and R.HDIV[0] == 0
    assert R.SDIV[255] == 4096 and R.SDIV[1] == 255 << 12
    assert R.HDIV[1] == 122880 and R.HDIV[255] == 482       # 481.88...


@pytest.mark.parametrize("hsv, rgb", [
    ((0, 255, 255), (255, 0, 0)), ((60, 255, 255), (0, 255, 0)), ((120, 255, 255), (0, 0, 255)),
    ((0, 0, 200), (200, 200, 200)), ((17, 0, 0), (0, 0, 0)),
    ((180, 255, 255), (255, 0, 0)), ((240, 255, 255), (0, 255, 0)),     # hue bytes past 179 wrap: h -= 6
])
def test_hsv_to_rgb_known_answers(hsv, rgb):
    assert tuple(R.hsv_to_rgb_u8(px(*hsv))[0, 0]) == rgb


def test_round_trip_within_one_code_value_where_hue_is_well_defined():
    g = np.arange(0, 256, 15, dtype=np.uint8)
    img = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3)
    hsv = R.rgb_to_hsv_u8(img)
    back = R.hsv_to_rgb_u8(hsv).astype(int)
    # the hue is stored in 2-degree steps: one step moves a channel by up to diff / 30 code values
    diff = img.max(-1).astype(int) - img.min(-1).astype(int)
    err = np.abs(back - img.astype(int)).max(-1)
    assert (err <= 1 + diff // 30 + 1).all()
    grey = diff == 0
    assert (err[grey] == 0).all()
    # value and (up to rounding) saturation survive exactly through a second forward conversion
    assert (np.abs(R.rgb_to_hsv_u8(back.astype(np.uint8))[..., 2].astype(int) - hsv[..., 2].astype(int)) <= 1).all()


def test_divide_ties_to_even():
    v = np.array([25, 75, 125, 24, 26, 255], np.uint8)
    assert R.divide_u8(v, 50).tolist() == [0, 2, 2, 0, 1, 5]    # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert R.divide_u8(np.array([255], np.uint8), 10).tolist() == [26]


def test_average_saturates_at_window_10():
    ref = R.TimexRef(1, 1, window=10)
    white_hsv = px(0, 0, 255)                       # grey 255: V = 255, q(255) = 26, ten of them = 260 -> 255
    frame = R.hsv_to_rgb_u8(white_hsv)
    assert tuple(frame[0, 0]) == (255, 255, 255)
    for n in range(1, 11):
        out = ref.push(frame, ("average",))["average"]
        assert out[0, 0, 0] == min(255, 26 * n)
    assert tuple(out[0, 0]) == (255, 255, 255)


def test_bright_slot0_enters_divided():
    # slot 0 holds the largest raw V (250 -> q = 62 at window 4) and loses to any slot above 62
    ref = R.TimexRef(1, 1, window=4)
    outs = [ref.push(px(v, v, v), ("bright", "dark")) for v in (250, 63, 10, 5)]
    assert outs[0]["bright"][0, 0, 0] == 62         # ring = [250, 0, 0, 0]: q(250) = 62 (62.5 ties to even) beats the zeros
    assert outs[1]["bright"][0, 0, 0] == 63         # 63 > 62
    assert outs[3]["bright"][0, 0, 0] == 63
    assert outs[0]["dark"][0, 0, 0] == 0 and outs[3]["dark"][0, 0, 0] == 5
    # a slot that only equals the divided seed does not replace it: the hue of slot 0 (divided) stays
    ref = R.TimexRef(1, 1, window=4)
    ref.push(px(250, 0, 0), ("bright",))            # hsv (0, 255, 250) -> divided (0, 64, 62)
    out = ref.push(px(0, 62, 0), ("bright",))["bright"]        # hsv (60, 255, 62): V ties with the seed
    assert tuple(out[0, 0]) == tuple(R.hsv_to_rgb_u8(px(0, 64, 62))[0, 0])


def test_bright_tie_goes_to_the_lower_slot():
    ref = R.TimexRef(1, 1, window=4)
    ref.push(px(0, 0, 0), ("bright",))
    ref.push(px(0, 200, 0), ("bright",))            # slot 1: green, V = 200
    out = ref.push(px(0, 0, 200), ("bright",))["bright"]       # slot 2: blue, V = 200: the walk keeps slot 1
    assert tuple(out[0, 0]) == (0, 200, 0)
    ref.push(px(0, 0, 0), ("bright",))
    ref.push(px(0, 0, 0), ("bright",))              # slot 0 again
    out = ref.push(px(1, 1, 1), ("bright",))["bright"]         # slot 1 overwritten: slot 2 is left
    assert tuple(out[0, 0]) == (0, 0, 200)


def test_mean_ties_to_even_through_the_reciprocal():
    # n = 2: the reciprocal is exact, the means 1.5, 3.5 and 254.5 are ties: to even
    ref = R.TimexRef(1, 1)
    assert ref.push(px(1, 3, 255), ("mean",))["mean"].tolist() == [[[1, 3, 255]]]
    assert ref.push(px(2, 4, 254), ("mean",))["mean"].tolist() == [[[2, 4, 254]]]
    # n = 3: what is rounded is the product with float(1.0 / 3) = 0.3333333433, not the quotient
    out = ref.push(px(3, 8, 255), ("mean",))["mean"]
    for c, total in enumerate((6, 15, 764)):
        assert out[0, 0, c] == int(np.rint(np.float32(total) * np.float32(1.0 / 3)))
    assert out.tolist() == [[[2, 5, 255]]]


def test_resize_bgr_identity_and_constant():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (9, 13, 3)).astype(np.uint8)
    assert np.array_equal(R.resize_bgr(img, 13, 9), img)
    flat = np.full((7, 5, 3), 91, np.uint8)
    assert (R.resize_bgr(flat, 11, 17) == 91).all() and (R.resize_bgr(flat, 3, 2) == 91).all()


def test_host_mirror_compiles(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = tmp_path / "timex_mirror.cpp"
    src.write_text('''
#include "rcflow_module.hpp"
int run(unsigned char* frame, unsigned char* mean, unsigned char* bright) {
    rc::Pipeline p(64, 48);
    p.timexOpen(50, RC_TIMEX_MEAN | RC_TIMEX_BRIGHT);
    rc::Mat f(48, 64, 3, 1, frame), m(48, 64, 3, 1, mean), none, b(48, 64, 3, 1, bright);
    p.timexPush(f, m, none, b, none);
    p.timexReset();
    p.timexClose();
    return 0;
}
''')
    subprocess.check_call([hipcc, "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), "-Wall", "-fsyntax-only", str(src)])
