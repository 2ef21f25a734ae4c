/*
 * Stand-in for <boost/math/special_functions/digamma.hpp> -- TEST INFRASTRUCTURE, this repository's own code.
 *
 * The reference's MutualInformation.cpp and DKL.cpp call boost::math::digamma only with `int` arguments (neighbour
 * counts, k, the member count).  This header provides exactly that: the digamma function at an integer,
 *     psi(n) = -gamma + H_{n-1},   H_m = 1 + 1/2 + ... + 1/m,
 * accumulated in long double from the largest term down the harmonic series (1/1 first) and rounded to double once.
 * That is the correctly rounded value up to the last bit of a 64-bit-mantissa sum; tests/test_oracle_vs_ref_mi.py
 * holds it within 1 ulp of scipy.special.digamma for n = 1 ... 4096.
 * At n <= 0 (a pole) it throws std::domain_error, which is what boost's default error policy does there.
 * Non-integer arguments are not supported: the reference never passes one, and the stand-in refuses to compile for them.
 */
#pragma once

#include <stdexcept>
#include <type_traits>
#include <vector>

namespace boost { namespace math {

template <class T>
inline double digamma(T n) {
    static_assert(std::is_integral<T>::value, "stand-in digamma: integer arguments only");
    if (n <= 0) throw std::domain_error("digamma: pole at a non-positive integer");
    // psi(1 + i) for i = 0 ... size-1, extended on demand; one table per thread (the field loops are OpenMP-parallel)
    thread_local std::vector<double> table;
    thread_local long double harmonic = 0.0L;
    const long double gamma = 0.577215664901532860606512090082402431L;
    while (table.size() < size_t(n)) {
        table.push_back(double(harmonic - gamma));
        harmonic += 1.0L / (long double)(table.size());
    }
    return table[size_t(n) - 1];
}

}}  // namespace boost::math
