// f32round.h -- TEST INFRASTRUCTURE ONLY: a double that is always a float value.
//
// hs_oracle_f32.cpp compiles the oracle with every `double` replaced by f32r (the trick of
// flopcount.h), which gives the restatement's own answer in single precision: every + - * /, sqrt
// and trigonometric call is computed in float on the operands cast to float, and every value
// constructed is rounded through float. The member stays a double, so f32r has the size and layout
// of double and the C ABI's double* arrays stay valid: values written by this build are exactly
// representable in float; values it is handed are rounded at their first arithmetic use
// (oracle.py rounds them before the call, so comparisons and copies see float values too).
#pragma once
#include <cmath>
#include <istream>
#include <ostream>
#include <type_traits>

struct f32r {
  double v;
  f32r() = default;
  constexpr f32r(double x) : v((double)(float)x) {}
  template <class T, class = typename std::enable_if<std::is_arithmetic<T>::value>::type>
  explicit constexpr operator T() const { return (T)v; }
  f32r& operator+=(f32r o);
  f32r& operator-=(f32r o);
  f32r& operator*=(f32r o);
  f32r& operator/=(f32r o);
};
static_assert(sizeof(f32r) == sizeof(double) && alignof(f32r) == alignof(double), "f32r must lie as a double");

inline f32r hso_f32(float x) { return f32r((double)x); }
inline f32r operator+(f32r a, f32r b) { return hso_f32((float)a.v + (float)b.v); }
inline f32r operator-(f32r a, f32r b) { return hso_f32((float)a.v - (float)b.v); }
inline f32r operator*(f32r a, f32r b) { return hso_f32((float)a.v * (float)b.v); }
inline f32r operator/(f32r a, f32r b) { return hso_f32((float)a.v / (float)b.v); }
inline f32r operator-(f32r a) { return hso_f32(-(float)a.v); }
inline f32r operator+(f32r a) { return a; }
inline f32r& f32r::operator+=(f32r o) { return *this = *this + o; }
inline f32r& f32r::operator-=(f32r o) { return *this = *this - o; }
inline f32r& f32r::operator*=(f32r o) { return *this = *this * o; }
inline f32r& f32r::operator/=(f32r o) { return *this = *this / o; }
inline bool operator<(f32r a, f32r b) { return a.v < b.v; }
inline bool operator>(f32r a, f32r b) { return a.v > b.v; }
inline bool operator<=(f32r a, f32r b) { return a.v <= b.v; }
inline bool operator>=(f32r a, f32r b) { return a.v >= b.v; }
inline bool operator==(f32r a, f32r b) { return a.v == b.v; }
inline bool operator!=(f32r a, f32r b) { return a.v != b.v; }

inline f32r sqrt(f32r a) { return hso_f32(std::sqrt((float)a.v)); }
inline f32r fabs(f32r a) { return f32r(std::fabs(a.v)); }
inline f32r sin(f32r a) { return hso_f32(std::sin((float)a.v)); }
inline f32r cos(f32r a) { return hso_f32(std::cos((float)a.v)); }
inline f32r tan(f32r a) { return hso_f32(std::tan((float)a.v)); }
inline f32r asin(f32r a) { return hso_f32(std::asin((float)a.v)); }
inline f32r acos(f32r a) { return hso_f32(std::acos((float)a.v)); }
inline f32r atan(f32r a) { return hso_f32(std::atan((float)a.v)); }
inline f32r atan2(f32r a, f32r b) { return hso_f32(std::atan2((float)a.v, (float)b.v)); }
inline f32r fmax(f32r a, f32r b) { return f32r(std::fmax(a.v, b.v)); }
inline f32r fmin(f32r a, f32r b) { return f32r(std::fmin(a.v, b.v)); }
inline std::ostream& operator<<(std::ostream& o, f32r a) { return o << a.v; }
inline std::istream& operator>>(std::istream& i, f32r& a) {
  double x = 0;
  i >> x;
  a = f32r(x);
  return i;
}
namespace std {
inline bool isnan(f32r a) { return std::isnan(a.v); }
inline bool isfinite(f32r a) { return std::isfinite(a.v); }
inline f32r sqrt(f32r a) { return ::sqrt(a); }
inline f32r fabs(f32r a) { return ::fabs(a); }
inline f32r abs(f32r a) { return ::fabs(a); }
}  // namespace std
