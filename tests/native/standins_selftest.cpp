// Host self-test of oracle/standins/ and, with -DWITH_REFERENCE, of oracle/ref_mi_driver.cpp linked with the
// reference's MutualInformation.cpp and DKL.cpp.  Built with -fsanitize=address,undefined by
// tests/test_oracle_vs_ref_mi.py: the point is that the sanitizers see every access of the stand-ins, of the driver's
// loops and of the reference's two files on a handful of vectors (ties, k beyond the member count, a NaN voxel, the
// digamma pole).  Prints "OK ..." and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <Math/Math.hpp>
#include <Utils/Random/Xorshift.hpp>
#include <Utils/SearchStructures/KdTreed.hpp>
#include <boost/math/special_functions/digamma.hpp>

#ifdef WITH_REFERENCE
extern "C" {
float ref_mi_binned(const float* x01, const float* y01, int numBins, int n);
float ref_mi_kraskov(const float* x, const float* y, int k, int n, int estimator);
float ref_kraskov_max(int k, int n);
float ref_dkl_binned(const float* values, int numBins, int n);
float ref_dkl_knn(const float* values, int k, int n);
int ref_mi_field(int measure, const float* const* fields, int cs, size_t voxelBegin, size_t voxelEnd,
                 const float* referenceValues, int k, int estimator, int numBins, float minRef, float maxRef,
                 float minQuery, float maxQuery, float* out);
int ref_mi_symmetric_field(int measure, const float* const* fieldsRef, const float* const* fieldsQuery, int cs,
                           size_t voxelBegin, size_t voxelEnd, int k, int numBins, float minRef, float maxRef,
                           float minQuery, float maxQuery, float* out);
int ref_mi_pair_requests(int measure, const float* const* fields, int cs, const size_t* idxI, const size_t* idxJ,
                         size_t numRequests, int k, int numBins, int useAbs, float* out);
int ref_dkl_field(int estimator, const float* const* fields, int cs, size_t numPoints, int numBins, int k, float* out);
}
#endif

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            failures++;                                                  \
        }                                                                \
    } while (0)

static void standins() {
    // digamma: psi(1) = -gamma, psi(n+1) - psi(n) = 1/n, the pole throws
    CHECK(std::abs(boost::math::digamma(1) + 0.5772156649015329) < 1e-15);
    for (int n = 1; n < 300; n++) CHECK(std::abs(boost::math::digamma(n + 1) - boost::math::digamma(n) - 1.0 / n) < 1e-15);
    bool thrown = false;
    try {
        boost::math::digamma(0);
    } catch (const std::domain_error&) {
        thrown = true;
    }
    CHECK(thrown);

    // generator: in [0, 1), same stream for the same seed, scaled by the bounds
    sgl::XorshiftRandomGenerator a(617406168ul), b(617406168ul);
    for (int i = 0; i < 1000; i++) {
        const float u = a.getRandomFloatBetween(0.0f, 1.0f);
        CHECK(u >= 0.0f && u < 1.0f);
        CHECK(b.getRandomFloatBetween(2.0f, 4.0f) == 2.0f + u * 2.0f);
    }

    // search: ascending distances, farthest last, at most n results, outputs replaced, empty tree after clear()
    using P2 = glm::vec<2, double>;
    std::vector<P2> pts;
    sgl::XorshiftRandomGenerator g(7ul);
    for (int i = 0; i < 37; i++) {  // ties in y
        const float px = g.getRandomFloatBetween(-1.0f, 1.0f);
        pts.emplace_back(px, std::floor(g.getRandomFloatBetween(0.0f, 4.0f)));
    }
    std::vector<P2> copy = pts;
    sgl::KdTreed<double, 2, sgl::DistanceMeasure::CHEBYSHEV> tree;
    tree.buildInplace(copy);
    std::vector<double> dist(5, -1.0);
    std::vector<P2> nbr(9, P2(-1.0, -1.0));
    for (int count : {1, 4, 37, 50}) {
        for (size_t e = 0; e < pts.size(); e++) {
            tree.findKNearestNeighbors(pts[e], count, nbr, dist);
            const size_t expect = size_t(count < 37 ? count : 37);
            CHECK(dist.size() == expect && nbr.size() == expect);
            CHECK(dist.front() == 0.0);
            for (size_t i = 0; i < dist.size(); i++) {
                CHECK(dist[i] == std::max(std::abs(pts[e].x - nbr[i].x), std::abs(pts[e].y - nbr[i].y)));
                if (i > 0) CHECK(dist[i - 1] <= dist[i]);
            }
            std::vector<double> only(3, -1.0);
            tree.findKNearestNeighbors(pts[e], count, only);
            CHECK(only == dist);
            CHECK(tree.getNumPointsInSphere(pts[e], dist.back()) >= dist.size());
        }
    }
    tree.clear();
    tree.findKNearestNeighbors(pts[0], 3, dist);
    CHECK(dist.empty());
    sgl::KdTreed<double, 1, sgl::DistanceMeasure::CHEBYSHEV> tree1;
    std::vector<glm::vec<1, double>> line;
    for (int i = 0; i < 5; i++) line.emplace_back(double(i));
    tree1.build(line);
    CHECK(tree1.getNumPointsInSphere(line[2], 1.0) == 3);

    CHECK(sgl::iceil(1, 2) == 1 && sgl::iceil(2, 2) == 1 && sgl::iceil(3, 2) == 2 && sgl::iceil(7, 2) == 4);
    CHECK(sgl::sqr(3.0) == 9.0 && sgl::TWO_PI == sgl::PI * 2.0f);
}

#ifdef WITH_REFERENCE
static void driver() {
    const int cs = 23, voxels = 11;
    sgl::XorshiftRandomGenerator g(99ul);
    std::vector<std::vector<float>> members((size_t)cs, std::vector<float>((size_t)voxels));
    for (auto& m : members)
        for (auto& v : m) v = g.getRandomFloatBetween(-2.0f, 2.0f);
    for (int c = 0; c < cs; c++) {
        members[size_t(c)][1] = std::round(members[size_t(c)][1]);      // ties
        members[size_t(c)][2] = 0.75f;                                  // constant voxel
    }
    members[4][3] = std::nanf("");                                      // NaN voxel
    std::vector<const float*> fields;
    for (auto& m : members) fields.push_back(m.data());
    std::vector<float> x((size_t)cs), y((size_t)cs), out((size_t)voxels);
    for (int c = 0; c < cs; c++) {
        x[size_t(c)] = members[size_t(c)][0];
        y[size_t(c)] = members[size_t(c)][1];
    }
    std::vector<float> x01(x), y01(y);
    for (auto& v : x01) v = (v + 2.0f) / 4.0f;
    for (auto& v : y01) v = (v + 2.0f) / 4.0f;
    y01[5] = INFINITY;                                                  // int() of an overflowing bin index
    for (int bins : {1, 4, 80, 255}) CHECK(std::isfinite(ref_mi_binned(x01.data(), y01.data(), bins, cs)));
    for (int k : {1, 3, cs - 1, cs, cs + 2}) {
        for (int est : {1, 2}) CHECK(ref_mi_kraskov(x.data(), y.data(), k, cs, est) >= 0.0f);
    }
    const float px[2] = {0.0f, 1099511627776.0f}, py[2] = {0.0f, 1.0f};  // KSG-2: digamma(0), thrown and caught
    CHECK(std::isnan(ref_mi_kraskov(px, py, 1, 2, 2)));
    CHECK(ref_mi_kraskov(px, py, 1, 2, 1) >= 0.0f);
    CHECK(ref_kraskov_max(3, cs) > 0.0f && std::isnan(ref_kraskov_max(0, cs)));
    for (int bins : {1, 10, 255}) CHECK(std::isfinite(ref_dkl_binned(x.data(), bins, cs)));
    for (int k : {1, 2, 3, 7, cs - 1}) CHECK(std::isfinite(ref_dkl_knn(x.data(), k, cs)));
    CHECK(std::isnan(ref_dkl_knn(y.data(), 1, cs)));                     // duplicates: log(0)
    for (int measure = 3; measure <= 6; measure++) {
        for (int est : {1, 2}) {
            CHECK(ref_mi_field(measure, fields.data(), cs, 0, size_t(voxels), x.data(), 3, est, 20, -2.0f, 2.0f, -2.0f, 2.0f,
                               out.data()) == 0);
            CHECK(std::isnan(out[3]) && !std::isnan(out[0]));
        }
        CHECK(ref_mi_symmetric_field(measure, fields.data(), fields.data(), cs, 2, size_t(voxels), 3, 20, -2.0f, 2.0f, -2.0f,
                                     2.0f, out.data()) == 0);
        CHECK(std::isnan(out[1]));
        const size_t ii[4] = {0, 1, 2, 3}, jj[4] = {5, 1, 6, 7};
        CHECK(ref_mi_pair_requests(measure, fields.data(), cs, ii, jj, 4, 3, 20, 1, out.data()) == 0);
        CHECK(std::isnan(out[3]) && out[0] >= 0.0f);
    }
    for (int est : {0, 1}) {
        CHECK(ref_dkl_field(est, fields.data(), cs, size_t(voxels), 16, 2, out.data()) == 0);
        CHECK(std::isnan(out[3]) && std::isfinite(out[0]));
    }
    CHECK(ref_dkl_field(1, fields.data(), cs, size_t(voxels), 16, cs, out.data()) == 1);   // k must be < cs
    CHECK(ref_dkl_field(0, fields.data(), 1, size_t(voxels), 16, 1, out.data()) == 0 && out[0] == 1.0f);
}
#endif

int main() {
    standins();
#ifdef WITH_REFERENCE
    driver();
    const char* what = "stand-ins and driver";
#else
    const char* what = "stand-ins";
#endif
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("OK %s\n", what);
    return 0;
}
