/*
 * Stand-in for sgl's <Utils/SearchStructures/KdTreed.hpp> -- TEST INFRASTRUCTURE, this repository's own code, written
 * from the interface that the call sites in the reference's MutualInformation.{hpp,cpp} show.  It also declares the
 * little of glm::vec<1|2, Real> those call sites use.
 *
 * Behaviour this stand-in commits to:
 *   - findKNearestNeighbors is an EXACT brute-force search under the Chebyshev (maximum) norm over the points given to
 *     build / buildInplace, the query point included when it is one of them.  It returns min(k, #points) results in
 *     ascending order of distance, the farthest LAST (the reference reads `.back()` as the k-th distance); points at
 *     equal distance come in the order in which they were given to build.  Any exact search yields the same distances;
 *     only which of several equidistant points is returned could differ, and only KSG-2 reads the points.
 *   - Both overloads REPLACE the contents of their output vectors.  computeMutualInformationKraskov2 clears the distance
 *     vector before every query but never the neighbour vector, and then takes maxima over the WHOLE neighbour vector:
 *     were the query to append, the vector would grow with every point, the marginal distances would cover ever more
 *     points, and KSG-2 would collapse to 0 everywhere.  sgl's source is not available here, so "replaces" is an
 *     assumption -- the one the oracle and the kernels make too; tests/test_oracle_vs_ref_mi.py checks it by itself.
 *   - getNumPointsInSphere exists only so that the reference's `#else` branch (no USE_1D_BINARY_SEARCH) would parse; the
 *     reference's build never takes that branch.
 */
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace glm {

template <int L, class T>
struct vec;

template <class T>
struct vec<1, T> {
    T x;
    vec() : x(0) {}
    explicit vec(T x) : x(x) {}
    T operator[](int) const { return x; }
};

template <class T>
struct vec<2, T> {
    T x, y;
    vec() : x(0), y(0) {}
    vec(T x, T y) : x(x), y(y) {}
    T operator[](int i) const { return i == 0 ? x : y; }
};

}  // namespace glm

namespace sgl {

enum class DistanceMeasure { EUCLIDEAN, CHEBYSHEV };

template <class Real, int K, DistanceMeasure M>
class KdTreed {
    static_assert(M == DistanceMeasure::CHEBYSHEV, "stand-in KdTreed: Chebyshev distance only");

public:
    using Point = glm::vec<K, Real>;

    void clear() { points.clear(); }
    void build(const std::vector<Point>& pts) { points = pts; }
    void buildInplace(std::vector<Point>& pts) { points = pts; }

    void findKNearestNeighbors(const Point& center, int k, std::vector<Real>& distances) {
        search(center, k);
        distances.clear();
        for (const auto& c : found) distances.push_back(c.first);
    }

    void findKNearestNeighbors(const Point& center, int k, std::vector<Point>& neighbors, std::vector<Real>& distances) {
        search(center, k);
        neighbors.clear();
        distances.clear();
        for (const auto& c : found) {
            neighbors.push_back(points[c.second]);
            distances.push_back(c.first);
        }
    }

    size_t getNumPointsInSphere(const Point& center, Real radius) {
        size_t count = 0;
        for (const Point& p : points) count += distance(center, p) <= radius ? 1 : 0;
        return count;
    }

private:
    static Real distance(const Point& a, const Point& b) {
        Real d = std::abs(a[0] - b[0]);
        for (int i = 1; i < K; i++) d = std::max(d, std::abs(a[i] - b[i]));
        return d;
    }

    // the min(k, n) nearest points as (distance, index in build order), ascending, ties by index
    void search(const Point& center, int k) {
        found.resize(points.size());
        for (size_t j = 0; j < points.size(); j++) found[j] = {distance(center, points[j]), j};
        const size_t count = std::min(size_t(std::max(k, 0)), points.size());
        std::partial_sort(found.begin(), found.begin() + count, found.end());
        found.resize(count);
    }

    std::vector<Point> points;
    std::vector<std::pair<Real, size_t>> found;
};

}  // namespace sgl
