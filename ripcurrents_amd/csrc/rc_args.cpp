// rc_args.cpp -- the argument rules of the device entry points (rc_args.h).  Host-only C++.
#include "rc_args.h"

int RcArgs::add(const Arg& a) {
    if (n_ < cap_) a_[n_] = a;
    return n_++;                                              // past the capacity: check() refuses
}

int RcArgs::image(const char* name, const void* p, size_t step, int bpp, int align, int flags, int w, int h) {
    return add({name, (uintptr_t)p, step, (size_t)(w > 0 ? w : 0) * bpp, w, h, align, flags, true});
}

int RcArgs::array(const char* name, const void* p, size_t bytes, int align, int flags) {
    return add({name, (uintptr_t)p, 0, bytes, 1, 1, align, flags, false});
}

int RcArgs::check() const {
    if (n_ > cap_) { rc_set_error("%s: %d arguments declared, the capacity is %d", who_, n_, cap_); return RC_EINVAL; }
    for (int i = 0; i < n_; i++) {
        const Arg& a = a_[i];
        const char* broke = nullptr;
        if (!a.p) { if (!(a.flags & RC_ARG_OPTIONAL)) broke = "a null pointer"; }
        else if (a.w <= 0 || a.h <= 0) broke = "an empty size";
        else if (a.img && a.step < a.row_bytes) broke = "a step below the bytes of a row";
        else if (a.step % a.align) broke = "a step that is no multiple of the alignment";
        else if (!(a.flags & RC_ARG_ANY_BASE) && a.p % a.align) broke = "a pointer that is not aligned";
        if (broke) {
            rc_set_error("%s: bad %s argument %s (%s; %d-byte alignment, %zu bytes a row)", who_, a.img ? "image" : "array", a.name, broke,
                         a.align, a.row_bytes);
            return RC_EINVAL;
        }
    }
    for (int i = 0; i < n_; i++)
        for (int j = i + 1; j < n_; j++) {
            const Arg &a = a_[i], &b = a_[j];
            if (!a.p || !b.p || !((a.flags | b.flags) & RC_ARG_OUT)) continue;
            const uintptr_t ae = a.p + (size_t)(a.h - 1) * a.step + a.row_bytes, be = b.p + (size_t)(b.h - 1) * b.step + b.row_bytes;
            if (ae <= b.p || be <= a.p) continue;
            const bool pair = (i == ip_in_ && j == ip_out_) || (i == ip_out_ && j == ip_in_);
            if (pair && a.p == b.p && a.step == b.step) continue;
            rc_set_error("%s: %s overlaps %s", who_, a.name, b.name);
            return RC_EINVAL;
        }
    return RC_OK;
}

int rc_clip_check(const char* who, const char* name, const void* p, size_t frame_stride, size_t step, int n, int w, int h, int bpp, int align,
                  int flags) {
    if (int rc = rc_image_check(who, name, p, step, w, h, bpp, align, flags)) return rc;
    const size_t frame = step * (size_t)(h - 1) + (size_t)w * bpp;   // the range of one frame
    if (!p || n <= 1) return RC_OK;
    if (frame_stride < frame) {
        rc_set_error("%s: bad clip argument %s (a frame stride of %zu bytes below the %zu of a frame)", who, name, frame_stride, frame);
        return RC_EINVAL;
    }
    // the rows of frames 1, 2, ... start at p + k * frame_stride: held to the alignment the step is held to
    if (frame_stride % align) {
        rc_set_error("%s: bad clip argument %s (a frame stride of %zu bytes that is no multiple of the alignment %d)", who, name, frame_stride, align);
        return RC_EINVAL;
    }
    return RC_OK;
}

int rc_prims_check(const char* who, const void* d_prims, int thickness, int disc_radius) {
    if (d_prims && !((uintptr_t)d_prims & 3) && thickness >= 1 && thickness <= RC_DRAW_MAX_THICKNESS && disc_radius >= 0 &&
        disc_radius <= RC_DRAW_COORD_MAX)
        return RC_OK;
    rc_set_error("%s: d_prims (4-byte aligned), thickness 1..%d, disc_radius 0..%d", who, RC_DRAW_MAX_THICKNESS, RC_DRAW_COORD_MAX);
    return RC_EINVAL;
}
