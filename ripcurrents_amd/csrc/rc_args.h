// rc_args.h -- the argument rules of the device entry points, stated once (rc_args.cpp).  Host-only: no HIP header, so the
// unit also builds with a plain C++ compiler and is tested without a GPU (tests/test_args_host.py).  An entry point
// declares what it was handed and calls check(); the rules ("argument rules"):
//   form     an image's step is at least w * bytes per pixel; step and pointer are multiples of its alignment; its size
//            is not empty.  An array's pointer is a multiple of its alignment.  A required argument is not null; an
//            optional one that is null is skipped
//   range    [p, p + (h - 1) * step + w * bytes per pixel): the padding between rows counts as the image's
//   overlap  two ranges overlap when neither ends at or before the other's start.  Every output is compared with every
//            input and every other output, inputs never with each other; the one declared in-place pair is exempt when
//            pointer and step are both equal
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rcflow.h"

void rc_set_error(const char* fmt, ...);

// RC_ARG_ANY_BASE: the alignment is asked of the step alone (the flow field of rcflow_ripmap_push_dev and
// rcflow_tracers_push_dev: an open point of DESIGN.md, kept as it was found)
enum { RC_ARG_IN = 0, RC_ARG_OUT = 1, RC_ARG_OPTIONAL = 2, RC_ARG_ANY_BASE = 4 };
enum { RC_ARGS_MAX = 7 };   // RcArgs' own capacity (rcflow_tracks_push_dev, rcflow_motion_push_dev); a longer list: RcArgsN

class RcArgs {
  public:
    RcArgs(const char* who, int w, int h) : who_(who), w_(w), h_(h) {}
    // every declaration returns the argument's index.  align: of pointer and step in bytes, 1 for none
    int image(const char* name, const void* p, size_t step, int bpp, int align, int flags) { return image(name, p, step, bpp, align, flags, w_, h_); }
    int image(const char* name, const void* p, size_t step, int bpp, int align, int flags, int w, int h);   // of its own size
    int array(const char* name, const void* p, size_t bytes, int align, int flags);
    void in_place(int out, int in) { ip_out_ = out; ip_in_ = in; }   // `out` may be `in` itself: the same pointer and the same step
    int check() const;   // RC_OK, or RC_EINVAL with the text set

  protected:
    struct Arg { const char* name; uintptr_t p; size_t step, row_bytes; int w, h, align, flags; bool img; };
    RcArgs(const char* who, int w, int h, Arg* store, int cap) : who_(who), w_(w), h_(h), cap_(cap), a_(store) {}   // the caller's storage

  private:
    int add(const Arg& a);
    const char* who_;
    int w_, h_, n_ = 0, ip_out_ = -1, ip_in_ = -1, cap_ = RC_ARGS_MAX;
    Arg own_[RC_ARGS_MAX];
    Arg* a_ = own_;
};

// the same collector with room for N arguments (rcflow_ftle_push_dev declares 8)
template <int N>
class RcArgsN : public RcArgs {
  public:
    RcArgsN(const char* who, int w, int h) : RcArgs(who, w, h, more_, N) {}

  private:
    Arg more_[N];
};

// one image alone: its form.  Arguments declared one by one are not compared with each other
inline int rc_image_check(const char* who, const char* name, const void* p, size_t step, int w, int h, int bpp, int align, int flags) {
    RcArgs a(who, w, h);
    a.image(name, p, step, bpp, align, flags);
    return a.check();
}

// a pointer alone: not null unless optional, a multiple of its alignment.  Nothing is asked of what lies behind it
inline int rc_ptr_check(const char* who, const char* name, const void* p, int align = 1, int flags = RC_ARG_IN) {
    RcArgs a(who, 1, 1);
    a.array(name, p, 0, align, flags);
    return a.check();
}

// a flow field as the entry points older than this layer ask it: rows of float2, the step a multiple of 8, nothing asked of
// the base (an open point of DESIGN.md, kept as it was found)
inline int rc_flow_check(const char* who, const char* name, const void* p, size_t step, int w, int h, int flags) {
    return rc_image_check(who, name, p, step, w, h, 8, 8, flags | RC_ARG_ANY_BASE);
}

// a run of n images frame_stride bytes apart: the first frame's form, and for n > 1 a stride of at least one frame's range
// that is a multiple of the alignment (every later frame's rows are then aligned as the first frame's are).  The bounds on n
// stay with each caller
int rc_clip_check(const char* who, const char* name, const void* p, size_t frame_stride, size_t step, int n, int w, int h, int bpp, int align,
                  int flags);

// the first lines of every *_prims_dev: d_prims not null and 4-byte aligned, thickness 1..RC_DRAW_MAX_THICKNESS, disc_radius
// 0..RC_DRAW_COORD_MAX
int rc_prims_check(const char* who, const void* d_prims, int thickness, int disc_radius);
