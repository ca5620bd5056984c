// The minimum of a Gaussian's quadratic form over an axis-aligned rectangle, in two steps: what depends on ONE
// interval of the rectangle (axis_terms), and what needs both (min_q_of_terms).  grid_walk.h's ellipse_min_q_rect is
// "x-terms, y-terms, combine"; the list build's product path (plan_lists.h) computes the terms of a block's 4 x- and
// 4 y-intervals once per survivor and combines them for its 16 group boxes -- the same helpers, every product an
// explicit FMA or a lone multiplication, so both form bit-identical minima for the same (ellipse, box).
// No HIP in here: a host compiler takes this header too (tests/ellipse_rect_main.cpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PIGS_ER_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PIGS_ER_FN inline
#endif

namespace pigs {

struct Ellipse {
    float x, y, a, b, c, nb_c, nb_a;      // centre, conic, -b/c, -b/a
};

// clamp(v, lo, hi) with lo <= hi is the median of the three (one v_med3_f32; like the min / max pair it returns a
// bound when v is NaN)
PIGS_ER_FN float med3f(float v, float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(v, lo, hi);
#else
    return fmaxf(fminf(v, lo), fminf(fmaxf(v, lo), hi));
#endif
}

// One interval [x0, x1] of one axis against an ellipse: the interval relative to the centre, the point `e` of it
// nearest to the centre, and of the edge through e the constant term p e^2, the linear coefficient 2b e and the
// unclamped vertex nb e of the parabola that q is along that edge.
struct AxisTerms {
    float lo, hi, pee, be2, v;
};
// centre: the centre's coordinate on this axis; p: the conic's coefficient of this axis (a for x, c for y); b2 = 2b;
// nb = -b / (the OTHER axis' coefficient): -b/c for x, -b/a for y
PIGS_ER_FN AxisTerms axis_terms(float centre, float p, float b2, float nb, float x0, float x1) {
    AxisTerms t;
    t.lo = x0 - centre;
    t.hi = x1 - centre;
    const float e = med3f(0.f, t.lo, t.hi);
    t.pee = (p * e) * e;
    t.be2 = b2 * e;
    t.v = nb * e;
    return t;
}
// the minimum of q along the edge of `s` that faces the centre, the other coordinate within `o`; po: the conic's
// coefficient of o's axis
PIGS_ER_FN float edge_min_q(const AxisTerms& s, const AxisTerms& o, float po) {
    const float w = med3f(s.v, o.lo, o.hi);
    return __builtin_fmaf(__builtin_fmaf(po, w, s.be2), w, s.pee);
}
// q is convex with its minimum at the centre, so its minimum over the rectangle lies on the edge(s) facing the
// centre (0 with the centre inside: both edges then pass through it); NaN for a degenerate conic
PIGS_ER_FN float min_q_of_terms(const AxisTerms& X, const AxisTerms& Y, float a, float c) {
    return fminf(edge_min_q(X, Y, c), edge_min_q(Y, X, a));
}
// the minimum of q over the rectangle (NaN for a degenerate conic: every comparison `!(qmin > q_max)` accepts)
PIGS_ER_FN float ellipse_min_q_rect(const Ellipse& e, float x0, float y0, float x1, float y1) {
    const float b2 = 2.f * e.b;
    const AxisTerms X = axis_terms(e.x, e.a, b2, e.nb_c, x0, x1);
    const AxisTerms Y = axis_terms(e.y, e.c, b2, e.nb_a, y0, y1);
    return min_q_of_terms(X, Y, e.a, e.c);
}

}  // namespace pigs
