/*
 * Stand-in for sgl's <Math/Math.hpp> -- TEST INFRASTRUCTURE, this repository's own code.
 *
 * DKL.cpp takes four things from it: the constants PI and TWO_PI, sqr(x) and iceil(x, y).  sgl declares the
 * constants as `float` (so `std::log(sgl::TWO_PI)` is the float overload and `Real(sgl::PI)` is pi rounded to float);
 * the stand-in keeps that type, which corr_oracle.cpp assumes as well.  A build with double constants would move the
 * DKL results by less than 1e-7 absolute.
 */
#pragma once

namespace sgl {

const float PI = 3.14159265358979323846f;
const float TWO_PI = PI * 2.0f;

template <class T>
inline T sqr(T x) {
    return x * x;
}

// ceil(x / y) for positive integers
inline int iceil(int x, int y) {
    return (x + y - 1) / y;
}

}  // namespace sgl
