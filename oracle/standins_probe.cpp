/*
 * standins_probe.cpp -- TEST INFRASTRUCTURE.  The stand-in headers of oracle/standins/ behind a C ABI, by themselves:
 * nothing of the reference is compiled into oracle/libstandins_probe.so, so it builds wherever this repository is.
 * tests/test_oracle_vs_ref_mi.py checks the stand-ins through it (digamma against scipy, the search against a numpy
 * brute force, the generator against the oracle's noise stream, and that a query replaces its output vectors).
 */
#include <cmath>
#include <cstddef>
#include <limits>
#include <stdexcept>
#include <vector>

#include <Utils/Random/Xorshift.hpp>
#include <Utils/SearchStructures/KdTreed.hpp>
#include <boost/math/special_functions/digamma.hpp>

extern "C" {

// digamma(n); NaN where the stand-in throws
double standin_digamma(int n) {
    try {
        return boost::math::digamma(n);
    } catch (const std::domain_error&) {
        return std::numeric_limits<double>::quiet_NaN();
    }
}

// u of the stand-in generator with the reference's seed constants (which = 0: reference vector, 1: query vector)
void standin_noise01(int which, int n, float* out) {
    sgl::XorshiftRandomGenerator gen(which == 0 ? 617406168ul : 864730169ul);
    for (int e = 0; e < n; e++) out[e] = gen.getRandomFloatBetween(0.0f, 1.0f);
}

// One query of the 2-D search over n points (px, py) around point `center`, asking for `count` neighbours.  The output
// vectors hold `prefill` stale entries before the call; returns how many entries they hold after it (at most capacity
// are copied out), -1 if the two overloads disagree about the distances.
int standin_knn(const double* px, const double* py, int n, int center, int count, int prefill, int capacity,
                double* outDist, double* outX, double* outY) {
    using Point = glm::vec<2, double>;
    std::vector<Point> points, copy;
    for (int e = 0; e < n; e++) points.emplace_back(px[e], py[e]);
    copy = points;
    sgl::KdTreed<double, 2, sgl::DistanceMeasure::CHEBYSHEV> tree;
    tree.buildInplace(copy);
    std::vector<Point> neighbors((size_t)prefill, Point(-1.0, -1.0));
    std::vector<double> distances((size_t)prefill, -1.0), only((size_t)prefill, -1.0);
    tree.findKNearestNeighbors(points.at(size_t(center)), count, neighbors, distances);
    tree.findKNearestNeighbors(points.at(size_t(center)), count, only);
    if (only != distances || neighbors.size() != distances.size()) return -1;
    for (size_t i = 0; i < distances.size() && i < size_t(capacity); i++) {
        outDist[i] = distances[i];
        outX[i] = neighbors[i].x;
        outY[i] = neighbors[i].y;
    }
    return int(distances.size());
}

}  // extern "C"
