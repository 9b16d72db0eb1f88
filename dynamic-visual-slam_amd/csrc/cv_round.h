// cv_round.h — OpenCV's host rounding helpers (core/fast_math.hpp) as the two extractors' table builders use them
#pragma once
#include <math.h>

namespace dvs {

inline int cv_round_f(float v) { return (int)lrintf(v); }  // cvRound: round-half-even
inline int cv_round_d(double v) { return (int)lrint(v); }
inline int cv_floor_d(double v) { int i = (int)v; return i - (i > v); }
inline int cv_floor_f(float v) { int i = (int)v; return i - (i > v); }
inline int cv_ceil_f(float v) { int i = (int)v; return i + (i < v); }

}  // namespace dvs
