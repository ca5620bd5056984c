// Stand-alone, host only: the list build's ellipse / rectangle arithmetic (pigs_amd/csrc/ellipse_rect.h: axis terms,
// then their combination) against a float64 statement of "the minimum of q over the rectangle" that shares no formula
// with it, on seeded (ellipse, rectangle) pairs.  tests/test_ellipse_rect.py compiles and runs it.
//
//   ellipse_rect_main <ellipses> <seed>   ->   one line: ellipses (each against a 4 x 4 product of boxes), boxes compared
//   and the worst relative error for |rho| <= 0.98, the same two for |rho| = 0.9999, ellipses with identical products
//
// Float64 statement: q is convex, so its minimum over the rectangle is 0 with the centre inside and otherwise lies on
// the boundary; each of the FOUR edges is minimised in float64 (the parabola's vertex clamped to the edge) -- the kernel's form looks at the two facing edges only and clamps with med3.
// "identical products": for a 4 x 4 product of intervals, combining shared axis terms (the product path) gives the
// very bits that ellipse_min_q_rect gives for each of the 16 boxes (the general path).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../pigs_amd/csrc/ellipse_rect.h"

static double edge64(double a, double b, double c, double fixed, double lo, double hi, bool vertical) {
    // vertical edge: x = fixed, y in [lo, hi]; horizontal: y = fixed, x in [lo, hi]
    const double p = vertical ? c : a;                     // coefficient of the free coordinate
    double w = -b * fixed / p;
    w = std::fmin(std::fmax(w, lo), hi);
    return vertical ? a * fixed * fixed + 2 * b * fixed * w + c * w * w : a * w * w + 2 * b * w * fixed + c * fixed * fixed;
}
static double min_q64(double a, double b, double c, double l, double r, double bt, double tp) {
    if (l <= 0 && r >= 0 && bt <= 0 && tp >= 0) return 0.0;
    return std::fmin(std::fmin(edge64(a, b, c, l, bt, tp, true), edge64(a, b, c, r, bt, tp, true)),
                     std::fmin(edge64(a, b, c, bt, l, r, false), edge64(a, b, c, tp, l, r, false)));
}

int main(int argc, char** argv) {
    const long pairs = argc > 1 ? atol(argv[1]) : 100000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    double worst[2] = {0.0, 0.0};
    long compared[2] = {0, 0}, same = 0, products = 0;
    for (long i = 0; i < pairs; ++i) {
        // an ellipse of the kinds the sampler meets: variances over four decades, correlations up to 0.9999
        const double sx = std::exp(std::log(1e-3) + U(rng) * std::log(1e2)), sy = std::exp(std::log(1e-3) + U(rng) * std::log(1e2));
        const double u = U(rng), rho = (u < 0.1 ? 0.9999 : u < 0.2 ? -0.9999 : 2 * U(rng) - 1) * (u < 0.2 ? 1.0 : 0.98);
        const double det = sx * sx * sy * sy * (1 - rho * rho);
        pigs::Ellipse e;
        e.a = (float)(sy * sy / det); e.c = (float)(sx * sx / det); e.b = (float)(-rho * sx * sy / det);
        e.x = (float)(2 * U(rng) - 1); e.y = (float)(2 * U(rng) - 1);
        e.nb_c = -e.b / e.c; e.nb_a = -e.b / e.a;
        // a 4 x 4 product of intervals within a few standard deviations of the centre
        float xs[5], ys[5];
        const double wx = sx * (0.2 + 3 * U(rng)), wy = sy * (0.2 + 3 * U(rng));
        xs[0] = (float)(e.x + sx * 8 * (U(rng) - 0.5)); ys[0] = (float)(e.y + sy * 8 * (U(rng) - 0.5));
        for (int k = 1; k < 5; ++k) { xs[k] = xs[k - 1] + (float)(wx * U(rng)); ys[k] = ys[k - 1] + (float)(wy * U(rng)); }
        const float b2 = 2.f * e.b;
        pigs::AxisTerms X[4], Y[4];
        for (int k = 0; k < 4; ++k) {
            X[k] = pigs::axis_terms(e.x, e.a, b2, e.nb_c, xs[k], xs[k + 1]);
            Y[k] = pigs::axis_terms(e.y, e.c, b2, e.nb_a, ys[k], ys[k + 1]);
        }
        bool all_same = true;
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 4; ++r) {
                const float qp = pigs::min_q_of_terms(X[c], Y[r], e.a, e.c);
                const float qg = pigs::ellipse_min_q_rect(e, xs[c], ys[r], xs[c + 1], ys[r + 1]);
                all_same = all_same && std::memcmp(&qp, &qg, 4) == 0;
                // against float64 on the float32 inputs, where q is of the size of a cut-off (0.5 .. 100)
                const double q64 = min_q64(e.a, e.b, e.c, (double)xs[c] - e.x, (double)xs[c + 1] - e.x, (double)ys[r] - e.y, (double)ys[r + 1] - e.y);
                if (q64 >= 0.5 && q64 <= 100.0) {
                    ++compared[u < 0.2];
                    worst[u < 0.2] = std::fmax(worst[u < 0.2], std::fabs((double)qg - q64) / q64);
                }
            }
        ++products;
        same += all_same;
    }
    printf("%ld %ld %.6e %ld %.6e %ld\n", products, compared[0], worst[0], compared[1], worst[1], same);
    return 0;
}
